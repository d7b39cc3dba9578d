"""aegolius_amd.render on the GPU (kernels: csrc/sdfk_rays.inc, csrc/sdfk_raydev.h) against the float64 oracle: soundness
of every ray, parity with the reference tracer, closed forms, interpreter = specialised kernel bit for bit, render = cast,
normals and the edge cases. Scenes, views and the derived bounds: tests/render_reference.py."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import aegolius_amd.cores as ns  # noqa: E402
import render_reference as ref  # noqa: E402
from aegolius_amd import _engine, render  # noqa: E402
from aegolius_amd._eval import config  # noqa: E402
from aegolius_amd._lower import lower_geometry  # noqa: E402
from test_render_cpu import CLOSED_FORM_STEPS, check_against_closed_form, closed_form_cases, sample_rays  # noqa: E402

pytestmark = pytest.mark.gpu

W, H = 160, 120
CAP = 0.005                      # share of a view's rays that may disagree (grazing rays are ill-conditioned for any tracer)


def views(name):
    cams = ref.cameras()
    # the twisted box's bound is derived for rays from the perspective eye only (render_reference.twisted_box_lipschitz)
    return {"perspective": cams["perspective"]} if name == "twisted" else cams


def setup(name):
    build, explicit, t_max, max_steps = ref.SCENES[name]
    geo = build()
    L = explicit if explicit is not None else lower_geometry(geo).lipschitz
    return geo, explicit, float(L), t_max, max_steps


def f32(x):
    return np.asarray(x, dtype=np.float32)


class mode:
    def __init__(self, m):
        self.m = m

    def __enter__(self):
        self.old, config.mode = config.mode, self.m

    def __exit__(self, *exc):
        config.mode = self.old


@pytest.mark.parametrize("name", list(ref.SCENES))
def test_soundness_every_ray(engine, name):
    """Hits lie within thr + slack of the surface and no ray passes through it (64 samples per traversed ray)."""
    geo, explicit, L, t_max, max_steps = setup(name)
    for vname, cam in views(name).items():
        o64, d64 = cam.rays(W, H)
        o, d = f32(o64), f32(d64)
        eps, cone = cam.footprint(W, H)
        hits = render.cast(geo, o, d, 0.0, t_max, eps, cone, max_steps, explicit)
        o64, d64, t = o.astype(np.float64), d.astype(np.float64), hits.t.astype(np.float64)
        hit = hits.status == render.HIT
        thr = ref.threshold(t, float(f32(eps)), float(f32(cone)))
        f, slack = ref.slack(geo, o64[:, hit] + t[hit] * d64[:, hit], L)
        over = f - (thr[hit] + slack)
        print("%s/%s: %d hits, %d misses, %d at the step limit; worst f - (thr + slack) at a hit %.3e" %
              (name, vname, hit.sum(), (hits.status == render.MISS).sum(), (hits.status == render.LIMIT).sum(),
               over.max() if over.size else float("nan")))
        assert np.all(over <= 0.0)
        end = np.where(hits.status == render.MISS, t_max, t)           # misses: the whole of [t_min, t_max]
        worst = np.inf
        for s in np.linspace(0.0, 1.0, 64):
            f, slack = ref.slack(geo, o64 + (s * end) * d64, L)
            worst = min(worst, float((f + slack).min()))
            assert np.all(f > -slack)
        print("%s/%s: smallest f + slack on the traversed segments %.3e" % (name, vname, worst))


def disagreement(t, status, t_ref, status_ref, eps, cone, L):
    both = (status == render.HIT) & (status_ref == ref.HIT)
    thr = ref.threshold(t_ref, eps, cone)
    dt = np.abs(t.astype(np.float64) - t_ref)
    bad = (status != status_ref) | (both & (dt > 2.0 * thr / L))
    worst = float((dt[both] * L / thr[both]).max()) if both.any() else 0.0     # |dt| in units of one threshold step
    return bad, worst


def parity(name, cam, w, h):
    geo, explicit, L, t_max, max_steps = setup(name)
    img = render.render(geo, cam, w, h, 0.0, t_max, max_steps, explicit, normals=False)
    o, d = cam.rays(w, h)
    eps, cone = (float(f32(x)) for x in cam.footprint(w, h))     # as the kernel sees them
    t_ref, s_ref, n_ref = ref.trace(ref.oracle_field(geo), o, d, 0.0, t_max, eps, cone, L, max_steps)
    bad, worst = disagreement(img.t.ravel(), img.status.ravel(), t_ref, s_ref, eps, cone, L)
    share = bad.mean()
    print("%s %dx%d: %.4f %% of the rays disagree (%d), largest |dt| L / thr %.3f, step-limit rays gpu %d / reference %d, "
          "most steps gpu %d / reference %d" % (name, w, h, 100 * share, bad.sum(), worst, (img.status == render.LIMIT).sum(),
                                                (s_ref == ref.LIMIT).sum(), img.steps.max(), n_ref.max()))
    return share


@pytest.mark.parametrize("name", list(ref.SCENES))
def test_parity_with_the_reference_tracer(engine, name):
    for vname, cam in views(name).items():
        assert parity(name, cam, W, H) <= CAP, vname


def test_parity_640x480(engine):
    assert parity("cfg2", ref.cameras()["perspective"], 640, 480) <= CAP


@pytest.mark.parametrize("name", ["sphere", "plane", "box"])
def test_closed_forms(engine, name):
    field, closed, build = closed_form_cases()[name]
    geo = build()
    o64, d64 = sample_rays()
    o, d = f32(o64), f32(d64)
    d = f32(d.astype(np.float64) / np.linalg.norm(d.astype(np.float64), axis=0))
    for eps, cone in ((1e-3, 0.0), (0.0, 2e-3), (1e-5, 1e-3)):
        hits = render.cast(geo, o, d, 0.0, 8.0, eps, cone, CLOSED_FORM_STEPS)
        o64, d64, t = o.astype(np.float64), d.astype(np.float64), hits.t.astype(np.float64)
        _, slack = ref.slack(geo, o64 + t * d64, 1.0)
        n_hit, n_graze = check_against_closed_form(field, closed, o64, d64, t, hits.status, 0.0, 8.0, float(f32(eps)),
                                                   float(f32(cone)), extra=slack)
        print("%s eps %g cone %g: %d exact hits, %d grazing hits, most steps %d" % (name, eps, cone, n_hit, n_graze,
                                                                                  hits.steps.max()))


def same_bits(a, b):
    assert np.array_equal(a.status, b.status)
    assert np.array_equal(a.steps, b.steps)
    assert np.array_equal(a.t.view(np.uint32), b.t.view(np.uint32))
    assert np.array_equal(np.asarray(a.normals).view(np.uint32), np.asarray(b.normals).view(np.uint32))


@pytest.mark.parametrize("name", list(ref.SCENES))
def test_interpreter_equals_specialised_bit_for_bit(engine, name):
    geo, explicit, L, t_max, max_steps = setup(name)
    assert lower_geometry(geo).fits_interpreter
    cams = ref.cameras()
    cam = cams["perspective"]
    o, d = (f32(x) for x in cam.rays(W, H))
    eps, cone = cam.footprint(W, H)
    out = {}
    for m in (_engine.MODE_INTERPRET, _engine.MODE_SPECIALIZED):
        with mode(m):
            # (both branches of the kernels' ray generation; the bits of a kernel must not depend on who compiled it, so
            #  the twisted box is rendered from the orthographic camera here too, although its bound is not derived for it)
            out[m] = (render.cast(geo, o, d, 0.0, t_max, eps, cone, max_steps, explicit, normals=True),
                      render.render(geo, cam, W + 3, H + 5, 0.0, t_max, max_steps, explicit, normals=True),
                      render.render(geo, cams["ortho_x"], W + 3, H + 5, 0.0, t_max, max_steps, explicit, normals=True))
    for a, b in zip(out[_engine.MODE_INTERPRET], out[_engine.MODE_SPECIALIZED]):
        same_bits(a, b)
    assert (out[_engine.MODE_INTERPRET][0].status == render.HIT).sum() > 100


def test_program_beyond_the_interpreter_runs_specialised_only(engine):
    from test_render_cpu import _beyond_interpreter
    geo = _beyond_interpreter()
    cam = ref.cameras()["perspective"]
    with mode(_engine.MODE_AUTO):
        img = render.render(geo, cam, 64, 48, 0.0, 8.0)
    assert (img.status == render.HIT).sum() > 50
    with mode(_engine.MODE_INTERPRET), pytest.raises(_engine.SdfkError, match="registers"):
        render.render(geo, cam, 64, 48, 0.0, 8.0)


def test_render_equals_cast_on_camera_rays_and_cast_is_permutation_invariant(engine):
    geo, explicit, L, t_max, max_steps = setup("cfg5")
    for vname, cam in ref.cameras().items():
        eps, cone = cam.footprint(W, H)
        img = render.render(geo, cam, W, H, 0.0, t_max, max_steps)
        o, d = (f32(x) for x in cam.rays(W, H))
        hits = render.cast(geo, o, d, 0.0, t_max, eps, cone, max_steps, normals=True)
        bad, worst = disagreement(img.t.ravel(), img.status.ravel(), hits.t.astype(np.float64), hits.status, eps, cone, L)
        print("render vs cast, %s: %d rays differ, largest |dt| L / thr %.3f" % (vname, bad.sum(), worst))
        assert np.array_equal(img.status.ravel(), hits.status)
        assert not bad.any()
        perm = np.random.default_rng(2).permutation(o.shape[1])
        shuffled = render.cast(geo, o[:, perm], d[:, perm], 0.0, t_max, eps, cone, max_steps, normals=True)
        assert np.array_equal(shuffled.status, hits.status[perm]) and np.array_equal(shuffled.steps, hits.steps[perm])
        assert np.array_equal(shuffled.t.view(np.uint32), hits.t[perm].view(np.uint32))
        assert np.array_equal(shuffled.normals.view(np.uint32), hits.normals[:, perm].view(np.uint32))


def angle(a, b):
    """Angle between unit vectors (3, n), from the chord (accurate for small angles)."""
    return 2.0 * np.arcsin(np.minimum(0.5 * np.linalg.norm(a - b, axis=0), 1.0))


@pytest.mark.parametrize("name", list(ref.SCENES))
def test_stencil_normals_against_the_oracle_stencil(engine, name):
    """The same tetrahedron stencil, same fp32 stencil points and width, evaluated by the oracle in float64. Four fp32
    field values, each within tau of the oracle's, enter g = sum k_i f_i / 4h with |k_i| = sqrt 3: |dg| <= sqrt(3) tau / h,
    an angle of at most |dg| / |g| — asserted with the factor 4 instead of sqrt 3. Rays whose stencil straddles a crease of
    a min / max may differ by any angle: at most CAP of the hits."""
    geo, explicit, L, t_max, max_steps = setup(name)
    cam = ref.cameras()["perspective"]
    o, d = (f32(x) for x in cam.rays(W, H))
    eps, cone = cam.footprint(W, H)
    hits = render.cast(geo, o, d, 0.0, t_max, eps, cone, max_steps, explicit, normals=True)
    hit = hits.status == render.HIT
    assert np.all(hits.normals[:, ~hit] == 0.0)
    p32 = hits.points()
    h = render.stencil_width(hits.t[hit], p32, eps, cone)
    field = ref.oracle_field(geo)

    def rounded(co):                                            # the kernel's stencil points: fp32 p + (+-h), one rounding
        k = np.sign(co - p32.astype(np.float64))
        return (p32 + f32(k) * h).astype(np.float64)
    g = ref.stencil_gradient(lambda co: field(rounded(co)), p32.astype(np.float64), h.astype(np.float64))
    gn = np.linalg.norm(g, axis=0)
    _, mag = ref.sdf_oracle.evaluate_with_magnitude(geo, p32.astype(np.float64))
    tau = 1e-6 * np.maximum(1.0, mag)
    bound = 4.0 * tau / (h * gn)
    ang = angle(hits.normals[:, hit].astype(np.float64), g / gn)
    bad = ~(ang <= bound)
    print("%s: %d hits, %d normals beyond 4 tau / (h |g|) (%.3f %%), largest angle / bound among the rest %.3f" %
          (name, hit.sum(), bad.sum(), 100 * bad.mean(), (ang[~bad] / bound[~bad]).max() if not bad.all() else float("nan")))
    assert np.allclose(np.linalg.norm(hits.normals[:, hit].astype(np.float64), axis=0), 1.0, rtol=0, atol=1e-6)
    assert bad.mean() <= CAP


def test_sphere_normals_against_the_analytic_normal(engine):
    """f = |x - c| - r at p, rho = |p - c|, n = (p - c) / rho, stencil offsets delta_i = h k_i (|k_i| = sqrt 3):
        f(p + delta) = rho + n.delta + (|delta|^2 - (n.delta)^2) / (2 rho) + R3,  |R3| <= 0.385 |delta|^3 / (2 rho^2) (1 + ...)
    Summed with the weights k_i / 4h: the first-order terms give n exactly (sum k_i k_i^T = 4 I); |delta|^2 drops out
    (sum k_i = 0); the (n.delta)^2 terms leave -(h / rho) (n_y n_z, n_z n_x, n_x n_y), because the tetrahedron's third
    moment sum_i k_ia k_ib k_ic is 4 for (a, b, c) a permutation of (x, y, z) and 0 otherwise: the four-point stencil is not
    centred, so its truncation error is of FIRST order, of length at most (h / rho) / sqrt 3 (at n = (1, 1, 1) / sqrt 3).
    R3: max u (1 - u^2) = 0.385, so each |R3| <= 1.0 h^3 / rho^2 and the weighted sum is at most sqrt(3) h^2 / rho^2; the
    orders beyond form a geometric series in sqrt(3) h / rho < 0.1, bounded by doubling that term. The angle to n is at
    most the length of the error: (h / rho) / sqrt 3 + 2 sqrt(3) (h / rho)^2, plus the rounding term sqrt(3) tau / h of the
    stencil test (|g| >= 1 - error)."""
    c = np.array([0.2, -0.1, 0.15])
    geo = ns.Sphere(0.5)
    geo.move(c)
    for vname, cam in ref.cameras().items():
        o, d = (f32(x) for x in cam.rays(W, H))
        eps, cone = cam.footprint(W, H)
        hits = render.cast(geo, o, d, 0.0, 8.0, eps, cone, 256, normals=True)
        hit = hits.status == render.HIT
        p = hits.points().astype(np.float64)
        h = render.stencil_width(hits.t[hit], f32(p), eps, cone).astype(np.float64)
        rho = np.linalg.norm(p - c[:, None], axis=0)
        n = (p - c[:, None]) / rho
        _, mag = ref.sdf_oracle.evaluate_with_magnitude(geo, p)
        tau = 1e-6 * np.maximum(1.0, mag) + 4.0 * 2.0 ** -24 * np.abs(p).max(axis=0)     # + the stencil points' rounding
        trunc = (h / rho) / np.sqrt(3.0) + 2.0 * np.sqrt(3.0) * (h / rho) ** 2
        bound = (trunc + np.sqrt(3.0) * tau / h) / (1.0 - trunc - np.sqrt(3.0) * tau / h)
        ang = angle(hits.normals[:, hit].astype(np.float64), n)
        print("sphere/%s: %d hits, largest angle %.3e, largest angle / bound %.3f" % (vname, hit.sum(), ang.max(), (ang / bound).max()))
        assert hit.sum() > 1000 and np.all(ang <= bound)


def test_exact_normals_are_the_gradients_mesh_uses(engine):
    from aegolius_amd.autodiff import value_and_grad_points
    geo, explicit, L, t_max, max_steps = setup("cfg2")
    cam = ref.cameras()["perspective"]
    img = render.render(geo, cam, W, H, 0.0, t_max, max_steps)
    stencil = img.normals.copy()
    exact = img.exact_normals(geo)
    _, grad = value_and_grad_points(geo, np.ascontiguousarray(img.points(), dtype=np.float32))
    g = np.asarray(grad, dtype=np.float64).reshape(3, -1).T
    norm = np.linalg.norm(g, axis=1, keepdims=True)
    want = np.ascontiguousarray(np.divide(g, norm, out=np.zeros_like(g), where=norm > 0), dtype=np.float32)
    hit = img.status == render.HIT
    assert np.array_equal(exact[hit].view(np.uint32), want.view(np.uint32)) and np.all(exact[~hit] == 0.0)
    ang = angle(exact[hit].T.astype(np.float64), stencil[hit].T.astype(np.float64))
    print("cfg2: median angle between stencil and exact normals %.3e" % np.median(ang))
    from aegolius_amd.autodiff import UnsupportedOpError
    cloud = ref.cloud()
    with pytest.raises(UnsupportedOpError):
        render.render(cloud, cam, 32, 24, 0.0, 8.0).exact_normals(cloud)


def test_edge_cases(engine):
    geo = ns.Sphere(0.5)
    empty = render.cast(geo, np.zeros((3, 0)), np.zeros((3, 0)), normals=True)
    assert empty.t.shape == (0,) and empty.status.shape == (0,) and empty.steps.shape == (0,) and empty.normals.shape == (3, 0)
    one = render.cast(geo, [[2.0], [0.0], [0.0]], [[-1.0], [0.0], [0.0]], eps=1e-4)
    assert one.status[0] == render.HIT and 0.0 <= 1.5 - one.t[0] <= 1.01e-4 and one.steps[0] >= 1
    inside = render.cast(geo, [[0.1], [0.0], [0.0]], [[1.0], [0.0], [0.0]], t_min=0.0)
    assert inside.status[0] == render.HIT and inside.t[0] == 0.0 and inside.steps[0] == 0
    away = render.cast(geo, [[2.0], [0.0], [0.0]], [[1.0], [0.0], [0.0]], t_max=10.0)
    assert away.status[0] == render.MISS and away.t[0] > 10.0
    once = render.cast(geo, [[2.0, 2.25, 0.0], [0.0] * 3, [0.0] * 3], [[-1.0, 1.0, 1.0], [0.0] * 3, [0.0] * 3], t_max=1.6, max_steps=1)
    assert list(once.status) == [render.LIMIT, render.MISS, render.HIT] and list(once.steps) == [1, 1, 0]
    assert once.t[0] == np.float32(1.5)
    # N not a multiple of 64, against the same rays one at a time being independent of their wave: a prefix is a prefix
    cam = ref.cameras()["perspective"]
    o, d = (f32(x) for x in cam.rays(37, 29))
    eps, cone = cam.footprint(37, 29)
    full = render.cast(geo, o, d, 0.0, 8.0, eps, cone, normals=True)
    part = render.cast(geo, o[:, :131], d[:, :131], 0.0, 8.0, eps, cone, normals=True)
    assert np.array_equal(part.t.view(np.uint32), full.t[:131].view(np.uint32)) and np.array_equal(part.status, full.status[:131])
    assert np.array_equal(part.normals.view(np.uint32), full.normals[:, :131].view(np.uint32))
    # image sizes that are not multiples of 8: every pixel written, and the same rays as cast up to the ray generation
    img = render.render(geo, cam, 37, 29, 0.0, 8.0)
    assert img.status.shape == (29, 37) and img.depth.shape == (29, 37) and img.normals.shape == (29, 37, 3)
    assert np.all(np.isinf(img.depth[img.status != render.HIT])) and np.all(np.isfinite(img.depth[img.status == render.HIT]))
    assert (img.status.ravel() != full.status).mean() <= CAP and (img.status == render.HIT).sum() > 20
    # resident in / resident out = host in / host out
    dev_o, dev_d = _engine.DeviceVectorField.from_host(o, config.device), _engine.DeviceVectorField.from_host(d, config.device)
    res = render.cast(geo, dev_o, dev_d, 0.0, 8.0, eps, cone, normals=True, resident=True)
    assert isinstance(res.t, _engine.DeviceField) and isinstance(res.normals, _engine.DeviceVectorField)
    assert np.array_equal(res.t.numpy().view(np.uint32), full.t.view(np.uint32)) and np.array_equal(res.status, full.status)
    assert np.array_equal(res.steps, full.steps) and np.array_equal(res.normals.numpy().view(np.uint32), full.normals.view(np.uint32))
    assert np.array_equal(res.points().view(np.uint32), full.points().view(np.uint32))
