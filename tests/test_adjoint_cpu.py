"""CPU (no GPU needed): the host half of reverse mode (aegolius_amd.autodiff.vjp / value_and_grad_sse) — argument checks
made before anything touches the GPU, the refusals, and the float64 chain rule from P̄ to the primals' gradients."""
import numpy as np
import pytest

import aegolius_amd.cores as ns
import autodiff_scenes
from aegolius_amd import autodiff as ad


def _circles(xs, ys):
    cs = []
    for x, y in zip(xs, ys):
        c = ns.Circle(0.3)
        c.move((x, y, 0))
        cs.append(c)
    return ns.CombineGeometry("UNION").combine(*cs)


def test_wrong_cotangent_or_target_length_raises_value_error(built):
    co = np.zeros((3, 10), dtype=np.float32)
    build = lambda r: ns.Circle(r)                      # noqa: E731
    with pytest.raises(ValueError, match="cotangent"):
        ad.vjp(build, co, (1.0,), np.ones(9))
    with pytest.raises(ValueError, match="cotangent"):
        ad.vjp(build, co, (1.0,), np.ones((2, 5)))
    with pytest.raises(ValueError, match="target"):
        ad.value_and_grad_sse(build, co, (1.0,), np.ones(11))

    class grid:                                         # a generate_grid array: N from its axis tables
        grid_axes = (np.zeros(4), np.zeros(5), np.zeros(1))
    with pytest.raises(ValueError, match="N = 20"):
        ad.value_and_grad_sse(build, grid, (1.0,), np.ones(19))


def test_grads_have_jax_grad_structure(built):
    primals = (1.0, np.arange(3.0), 2.0)
    pbar = np.array([1.0, 2.0, 4.0])
    rows_for = {0: [[1.0, 0, 0]], 1: [[0, 1.0, 0], [0, 0, 1.0], [1.0, 1.0, 0]], 2: [[0.5, 0, 0]]}

    def rows(argnums):
        nums = (argnums,) if isinstance(argnums, int) else argnums
        return np.array([r for a in nums for r in rows_for[a]])
    g = ad.chain_rule(rows(0), pbar, ad.channel_layout(primals, 0)[1], 0)
    assert isinstance(g, float) and g == 1.0
    g = ad.chain_rule(rows(1), pbar, ad.channel_layout(primals, 1)[1], 1)
    assert isinstance(g, np.ndarray) and g.dtype == np.float64 and g.shape == (3,)
    np.testing.assert_array_equal(g, [2.0, 4.0, 3.0])
    g = ad.chain_rule(rows((2, 1)), pbar, ad.channel_layout(primals, (2, 1))[1], (2, 1))
    assert isinstance(g, tuple) and len(g) == 2
    assert isinstance(g[0], float) and g[0] == 0.5
    np.testing.assert_array_equal(g[1], [2.0, 4.0, 3.0])
    g = ad.chain_rule(rows((1,)), pbar, ad.channel_layout(primals, (1,))[1], (1,))
    assert isinstance(g, tuple) and len(g) == 1 and g[0].shape == (3,)


def test_chain_rule_is_the_float64_contraction_of_the_parameter_tangents(built):
    """θ̄_k = Σ_j P̄_j dP_j/dθ_k with parameter_tangents' float64 rows (not rounded to fp32 as forward mode does)."""
    fn, primals, argnums = autodiff_scenes.SCENES["multi_position_optimization"]
    low, _origin, rows, chans, layout = ad.parameter_tangents(fn(ns), primals, argnums)
    pbar = np.random.default_rng(3).normal(size=low.params.size) * (1 + 1e-9)
    gx, gy = ad.chain_rule(rows, pbar, layout, argnums)
    want = np.zeros(len(chans))
    for k in range(len(chans)):
        for j in range(low.params.size):
            want[k] += pbar[j] * rows[k, j]
    np.testing.assert_allclose(np.concatenate([gx, gy]), want, rtol=1e-14, atol=1e-14)
    # a row that fp32 cannot hold: the contraction keeps it
    r = np.zeros((1, 2))
    r[0, 0] = 1.0 + 2.0 ** -40
    assert ad.chain_rule(r, np.array([1.0, 0.0]), [(0, 1, True)], 0) == 1.0 + 2.0 ** -40


def test_refusals(built):
    co = np.zeros((3, 8), dtype=np.float32)
    c = np.ones(8)

    def signed(r):
        o = ns.Circle(r)
        o.signed((32, 32, 1))
        return o
    with pytest.raises(ad.UnsupportedOpError, match="staged"):
        ad.vjp(signed, co, (0.5,), c)
    with pytest.raises(ad.UnsupportedOpError, match="has no dual rule"):
        ad.value_and_grad_sse(lambda r: ns.Braid(1.0, r, 0.1, 1.0), co, (0.3,), c)
    tape, _params = ad.adjoint_limits()
    with pytest.raises(ad.UnsupportedOpError, match="restore tape takes [0-9]+ floats per point, %d at most" % tape):
        ad.vjp(_circles, co, (np.zeros(60), np.zeros(60)), c, (0, 1))


def test_structure_change_raises_in_reverse_mode(built):
    with pytest.raises(ad.StructureError):
        ad.vjp(lambda n: ns.NGon(0.5, n), np.zeros((3, 4), np.float32), (5.0,), np.ones(4))


def test_largest_accepted_tape_is_the_limit(built):
    """The largest program the adjoint kernel takes: tape exactly at the limit, and one more push is refused."""
    tape, _params = ad.adjoint_limits()
    assert tape == 256
    build, extra = largest_program()
    low, origin = ad._lower(build(0.02), shortcuts=False)
    assert low.n_creg == 16
    ad._adjoint_program(low, origin)
    low, origin = ad._lower(extra(0.02), shortcuts=False)
    with pytest.raises(ad.UnsupportedOpError, match="restore tape takes %d floats" % (tape + 1)):
        ad._adjoint_program(low, origin)


def largest_program():
    """(builder at the tape limit with 16 coordinate registers, the same plus one value instruction). The builder's
    primal is the width of the last rounding."""
    from aegolius_amd import workloads
    import ctypes
    from aegolius_amd import _engine
    tape, _params = ad.adjoint_limits()

    def tape_of(geo):
        low, origin = ad._lower(geo, shortcuts=False)
        prog = ad._program(low, origin)
        t = ctypes.c_int64(0)
        _engine.lib().sdfk_program_vjp_check(prog.handle, None, ctypes.byref(t))
        return t.value

    def make(k):
        def build(r):
            tree = workloads.cfg2_tree(ns, count=16)
            for _ in range(k):
                tree.rounding(r)
            return tree
        return build
    k = tape - tape_of(make(0)(0.02))
    assert k >= 1
    return make(k), make(k + 1)
