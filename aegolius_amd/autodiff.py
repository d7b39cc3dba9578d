"""Forward-mode derivatives of SDF fields on the GPU.

The reference differentiates its fields with a JAX twin of its cores. Here the derivative is that of the field this
package computes, evaluated where the field is evaluated: one pass of a dual-number kernel (csrc/sdfk_dual.inc) carries
the value plus K <= 4 tangents per point; more channels run as several passes.

The "function" being differentiated is a BUILDER: a Python callable that takes the primals and returns a geometry
(a GenericGeometry or a CombineGeometry result), as the reference's autodiff examples write `geometry(r, a, w, s)`.

    value, jac  = value_and_jacfwd(builder, co, primals, argnums=0)        # jac: (N,) for a scalar primal, (m, N) for a 1-D one
    value, jacs = value_and_jacfwd(builder, co, primals, argnums=(0, 2))   # a tuple of the above
    value, tan  = jvp(builder, co, primals, tangents)                      # directional derivative, (N,)
    value, g    = value_and_grad_points(geometry, co)                      # spatial gradient, (3, N)
    out, out_t  = post_jvp(name, field, field_tangent, *params)            # chain rule through a post-processing map
    value, g    = vjp(builder, co, primals, cotangent, argnums=0)          # Σ_i c_i ∂f_i/∂θ, one adjoint pass
    loss, g     = value_and_grad_sse(builder, co, primals, target)         # Σ (f - t)² and its gradient, one pass

Layout: Jacobians are (m, N) — derivative first, points second, the package's (D, N) convention. That is the TRANSPOSE
of JAX's jacfwd layout, which puts the output dimension (N) first.

How parameter tangents are obtained: every geometry turns its arguments into the program's parameter table on the host,
in float64 (aegolius_amd._lower). The builder's geometry is lowered at p, p + h e_k and p - h e_k with the lowering's
shortcut-free mode (no instruction form is chosen from a parameter's value) and dP_k = (P+ - P-) / 2h is taken in
float64, rounded once to fp32. The program must be the same at all three points (else StructureError), and the two
one-sided differences must agree (else a jump in the host arithmetic: StructureError).

Reverse mode (vjp, value_and_grad_sse): one pass of the adjoint kernel (csrc/sdfk_adjoint.inc) evaluates the program with
a restore tape, back-propagates a cotangent per point and reduces P̄ = Σ_i c_i ∂f_i/∂P on the device in float64; the host
applies θ̄ = dP/dθ · P̄ with the float64 rows of parameter_tangents (not rounded). Gradients have JAX's grad structure.
"""
import contextlib
import ctypes
import inspect

import numpy as np

from . import _engine, _ops
from ._eval import config, device_coords
from ._ir import CombineSDF, ModSDF, NodeSDF, PrimSDF, UnsupportedSDF
from ._lower import OWNED, Lowerer, NeedsStage, _deep

GROUP = 4                 # tangent channels per kernel launch (sdfk_jvp_kernel<K>, K = 1..4)


class StructureError(ValueError):
    """The program's code or tables change when the differentiated argument moves (or its parameters jump)."""


class UnsupportedOpError(NotImplementedError):
    """The tree holds an operation without a dual rule, or needs a staged evaluation."""


# ---------------------------------------------------------------------------------------------------
# lowering with provenance
# ---------------------------------------------------------------------------------------------------
def _describe(expr):
    if isinstance(expr, PrimSDF):
        return expr.name
    if isinstance(expr, ModSDF):
        return ".%s()" % expr.name
    if isinstance(expr, CombineSDF):
        return "CombineGeometry(%r)" % getattr(expr.owner, "operation_type", "?")
    if isinstance(expr, UnsupportedSDF):
        return "a Python callable"
    if isinstance(expr, NodeSDF):
        return type(expr.obj).__name__
    return type(expr).__name__


class _TracingLowerer(Lowerer):
    """A Lowerer that remembers which cores object emitted each instruction (for the error messages).
    Also the base of aegolius_amd.render's lowerer (`origin`, `emit`): keep both when this class changes."""

    def __init__(self, shortcuts):
        Lowerer.__init__(self, shortcuts)
        self.origin = []
        self._where = []

    def lower_node(self, node, creg, mode):
        self._where.append(("node", type(node).__name__))
        try:
            return Lowerer.lower_node(self, node, creg, mode)
        finally:
            self._where.pop()

    def lower_expr(self, expr, creg, mode, params):
        self._where.append(("expr", _describe(expr)))
        try:
            return Lowerer.lower_expr(self, expr, creg, mode, params)
        finally:
            self._where.pop()

    def emit(self, opname, a, b=0, c=0, params=(), _fold=True):
        Lowerer.emit(self, opname, a, b, c, params, _fold)
        # the innermost expression and the geometry class it belongs to: "sdf_braid of Braid", ".twist() of Box"
        nodes = [label for kind, label in self._where if kind == "node"]
        inner = self._where[-1][1] if self._where and self._where[-1][0] == "expr" else None
        where = " of ".join([x for x in (inner, nodes[-1] if nodes else None) if x]) or "the geometry"
        del self.origin[len(self.code):]
        while len(self.origin) < len(self.code):
            self.origin.append(where)


def _lower(geometry, shortcuts):
    """-> (LoweredProgram, origin of each instruction)."""
    L = _TracingLowerer(shortcuts)
    try:
        v = _deep(lambda: L.lower_node(geometry, 0, OWNED))
    except NeedsStage as exc:
        raise UnsupportedOpError("%r needs a staged evaluation (signed / conv_* / custom_* / Python callables have no "
                                 "forward-mode derivative)" % (exc.expr.name,)) from None
    return L.finish(v), list(L.origin)


def _program(low, origin):
    """The native program of a lowering, checked for dual rules."""
    prog = _engine.Program(low.code, low.params, low.tables, low.result_reg)
    bad = ctypes.c_int(-1)
    rc = _engine.lib().sdfk_program_jvp_check(prog.handle, ctypes.byref(bad))
    if rc == 1:
        i = bad.value
        name = _ops.OPS[int(low.code[i, 0]) & 255].name
        raise UnsupportedOpError("opcode %s (from %s) has no dual rule" % (name, origin[i] if i < len(origin) else "?"))
    if rc == 2:
        raise UnsupportedOpError("program too large for the dual kernel (%d coordinate / %d value registers; 16 / 8 at most)"
                                 % (low.n_creg, low.n_vreg))
    _engine.check(rc, "sdfk_program_jvp_check")
    return prog


def dual_opcodes():
    """Names of the opcodes with a dual rule (the table in csrc/sdfk_dualdev.h)."""
    lib = _engine.lib()
    return [o.name for o in _ops.OPS if lib.sdfk_dual_has_rule(o.code)]


# ---------------------------------------------------------------------------------------------------
# channels and parameter tangents
# ---------------------------------------------------------------------------------------------------
def channel_layout(primals, argnums=0):
    """-> (channels, layout): channels = [(argnum, index or None)], one per tangent channel; layout = [(first channel,
    count, scalar)] per entry of argnums. A scalar primal is one channel, a 1-D primal one per element."""
    primals = tuple(primals)
    nums = (argnums,) if isinstance(argnums, (int, np.integer)) else tuple(argnums)
    chans, layout = [], []
    for a in nums:
        arr = np.asarray(primals[a], dtype=np.float64)
        if arr.ndim == 0:
            layout.append((len(chans), 1, True))
            chans.append((int(a), None))
        elif arr.ndim == 1:
            layout.append((len(chans), arr.size, False))
            chans.extend((int(a), i) for i in range(arr.size))
        else:
            raise ValueError("primal %d must be a float or a 1-D array; got shape %r" % (a, arr.shape))
    return chans, layout


def _step(p):
    """A power of two near 1e-5 max(1, |p|)."""
    return float(2.0 ** np.round(np.log2(1e-5 * max(1.0, abs(p)))))


def _moved(primals, argnum, index, delta):
    out = list(primals)
    if index is None:
        out[argnum] = float(primals[argnum]) + delta
    else:
        arr = np.array(primals[argnum], dtype=np.float64)
        arr[index] += delta
        out[argnum] = arr
    return tuple(out)


def _same_structure(a, b):
    return (a.code.shape == b.code.shape and np.array_equal(a.code, b.code) and a.result_reg == b.result_reg
            and a.n_creg == b.n_creg and a.n_vreg == b.n_vreg and a.params.size == b.params.size
            and a.tables.shape == b.tables.shape and np.array_equal(a.tables.view(np.uint32), b.tables.view(np.uint32)))


def _param_tangent(builder, primals, low0, argnum, index):
    """dP / dθ (float64, one entry per parameter) for primal `argnum` (element `index`)."""
    p = float(np.asarray(primals[argnum], dtype=np.float64).ravel()[0 if index is None else index])
    h = _step(p)
    what = "argnum %d" % argnum + ("" if index is None else " element %d" % index)
    lows = []
    for sgn in (1.0, -1.0):
        low, _ = _lower(builder(*_moved(primals, argnum, index, sgn * h)), shortcuts=False)
        if not _same_structure(low0, low):
            raise StructureError("the program's code or tables change when %s moves from %r by %s%g" %
                                 (what, p, "+" if sgn > 0 else "-", h))
        lows.append(low)
    hp, hm = (p + h) - p, p - (p - h)
    P0, Pp, Pm = low0.params64, lows[0].params64, lows[1].params64
    with np.errstate(all="ignore"):
        d = (Pp - Pm) / (hp + hm)
        dp, dm = (Pp - P0) / hp, (P0 - Pm) / hm
    ok = np.isfinite(P0)
    if not np.all(np.isfinite(d[ok])):
        raise StructureError("the parameters are not differentiable in %s at %r" % (what, p))
    tol = 1e-2 * np.maximum(1.0, np.abs(d)) + 1e-12 * np.maximum(1.0, np.abs(P0)) / h
    jump = ok & ~(np.abs(dp - dm) <= tol)
    if np.any(jump):
        j = int(np.flatnonzero(jump)[0])
        raise StructureError("parameter %d of the program jumps at %s = %r (one-sided differences %g and %g)" %
                             (j, what, p, dp[j], dm[j]))
    d[~ok] = 0.0
    return d


def parameter_tangents(builder, primals, argnums=0):
    """-> (LoweredProgram at the primals, origin, dP (channels, n_params) float64, channels, layout). Host only."""
    primals = tuple(primals)
    chans, layout = channel_layout(primals, argnums)
    low0, origin = _lower(builder(*primals), shortcuts=False)
    rows = np.zeros((len(chans), low0.params.size))
    for c, (a, i) in enumerate(chans):
        rows[c] = _param_tangent(builder, primals, low0, a, i)
    return low0, origin, rows, chans, layout


# ---------------------------------------------------------------------------------------------------
# device plumbing
# ---------------------------------------------------------------------------------------------------
def _run(prog, coords, rows, seed_points=False):
    """rows: (K <= 4, n_params) fp32 parameter tangents -> (value DeviceField, [K tangent DeviceFields])."""
    L = _engine.lib()
    vp = _engine._vp
    n, K = coords.n, rows.shape[0]
    dP = np.ascontiguousarray(rows, dtype=np.float32)
    with contextlib.ExitStack() as on_error, _engine.DeviceBuffer(dP.size * 4, what="autodiff") as d_dp, \
            _engine.DeviceRows(K, n, what="autodiff") as d_t:
        d_dp.upload(dP)
        value = on_error.enter_context(_engine.DeviceField(n, config.device))
        _engine.check(L.sdfk_eval_jvp_device(prog.handle, vp(coords.ptr), n, coords.stride, d_dp.at(), K,
                                             1 if seed_points else 0, vp(value.ptr), d_t.at(), d_t.stride, None),
                      "sdfk_eval_jvp_device")
        tangents = [on_error.enter_context(_engine.DeviceField.from_device(d_t.row_ptr(k), n, config.device))
                    for k in range(K)]
        _engine.check(L.sdfk_sync(None), "sdfk_sync")
        on_error.pop_all()
        return value, tangents


def _host(field):
    out = field.numpy()
    field.free()
    return out


def _evaluate_channels(prog, co, rows, resident):
    """All channels of `rows` (m, n_params), in groups of GROUP per launch -> (value, [m tangents])."""
    _engine.require_gpu()
    _engine.check(_engine.lib().sdfk_set_device(config.device), "sdfk_set_device")
    with device_coords(co, "autodiff") as coords:
        value, tangents = None, []
        groups = [rows[i:i + GROUP] for i in range(0, rows.shape[0], GROUP)] or [np.zeros((1, rows.shape[1]), np.float32)]
        for block in groups:
            v, ts = _run(prog, coords, block)
            if value is None:
                value = v                                      # the value comes from the first group
            else:
                v.free()
            tangents.extend(ts)
        tangents = tangents[:rows.shape[0]]
    if resident:
        return value, tangents
    return _host(value), [_host(t) for t in tangents]


# ---------------------------------------------------------------------------------------------------
# public API
# ---------------------------------------------------------------------------------------------------
def value_and_jacfwd(builder, co, primals, argnums=0, resident=False):
    """Field of `builder(*primals)` on `co` and its derivative with respect to the primals named by `argnums`.

    `primals`: a tuple of floats or 1-D float arrays (each float, each array element is one tangent channel).
    `co`: what create() accepts — a (3, N) host array (generate_grid output included) — or a DeviceVectorField.
    Returns (value (N,), jac): jac is (N,) for a scalar primal and (m, N) for a 1-D primal of m elements (the transpose of
    JAX's layout); with a tuple `argnums`, a tuple of those. Host float32 arrays, or with resident=True DeviceFields
    (a list of m DeviceFields for a 1-D primal)."""
    low, origin, rows, chans, layout = parameter_tangents(builder, primals, argnums)
    prog = _program(low, origin)
    value, tangents = _evaluate_channels(prog, co, rows.astype(np.float32), resident)
    jacs = []
    for first, count, scalar in layout:
        part = tangents[first:first + count]
        if scalar:
            jacs.append(part[0])
        else:
            jacs.append(list(part) if resident else (np.stack(part) if part else np.zeros((0, value.size), np.float32)))
    if isinstance(argnums, (int, np.integer)):
        return value, jacs[0]
    return value, tuple(jacs)


def jvp(builder, co, primals, tangents, resident=False):
    """(value, directional derivative) of the field along `tangents` (same structure as `primals`), both (N,)."""
    primals, tangents = tuple(primals), tuple(tangents)
    if len(tangents) != len(primals):
        raise ValueError("one tangent per primal: %d primals, %d tangents" % (len(primals), len(tangents)))
    chans, _ = channel_layout(primals, tuple(range(len(primals))))
    low0, origin = _lower(builder(*primals), shortcuts=False)
    prog = _program(low0, origin)
    row = np.zeros(low0.params.size)
    for a, i in chans:
        t = np.asarray(tangents[a], dtype=np.float64)
        if t.shape != np.shape(np.asarray(primals[a], dtype=np.float64)):
            raise ValueError("tangent %d has shape %r, its primal %r" % (a, t.shape, np.shape(primals[a])))
        w = float(t if i is None else t[i])
        if w != 0.0:
            row += w * _param_tangent(builder, primals, low0, a, i)
    value, tans = _evaluate_channels(prog, co, row[None].astype(np.float32), resident)
    return value, tans[0]


def value_and_grad_points(geometry, co, resident=False):
    """(field, ∇_x field) of `geometry` on `co`: the exact spatial gradient at arbitrary points, (N,) and (3, N).
    The program is create()'s own, so the value equals create()'s bit for bit."""
    low, origin = _lower(geometry, shortcuts=True)
    prog = _program(low, origin)
    _engine.require_gpu()
    _engine.check(_engine.lib().sdfk_set_device(config.device), "sdfk_set_device")
    with device_coords(co, "autodiff") as coords:
        value, grads = _run(prog, coords, np.zeros((3, low.params.size), dtype=np.float32), seed_points=True)
    if resident:
        return value, grads
    host = [_host(g) for g in grads]
    return _host(value), np.stack(host) if coords.n else np.zeros((3, 0), np.float32)


# the array-level functions of cores/post_processing.py that have a value op with a dual rule
POST_MAPS = ("sigmoid_falloff", "positive_sigmoid_falloff", "capped_exponential", "hard_binarization", "linear_falloff",
             "relu", "smooth_relu", "slowstart", "gaussian_boundary", "gaussian_falloff")


def post_jvp(name, field, field_tangent, *params):
    """Chain rule through the post-processing map `name` of cores.post_processing, called as name(field, *params):
    -> (map(field), map'(field) * field_tangent). The parameters' tangents are zero. `field` and `field_tangent` are
    arrays of one shape (results: that shape, float32) or both DeviceFields (results: DeviceFields)."""
    from ._mods import VALUE_OPS
    from .cores import post_processing
    if name not in POST_MAPS:
        raise UnsupportedOpError("post_jvp: %r is not one of %s" % (name, ", ".join(POST_MAPS)))
    fn = getattr(post_processing, name)
    bound = inspect.signature(fn).bind(field, *params)
    bound.apply_defaults()
    args = dict(list(bound.arguments.items())[1:])
    opname, prm_fn = VALUE_OPS[name]
    P = np.ascontiguousarray(np.asarray(prm_fn(args), dtype=np.float64).astype(np.float32).ravel())
    _engine.require_gpu()
    L = _engine.lib()
    vp = _engine._vp
    resident = isinstance(field, _engine.DeviceField)
    if resident != isinstance(field_tangent, _engine.DeviceField):
        raise TypeError("post_jvp: field and tangent must both be arrays or both DeviceFields")
    if resident:
        if field.n != field_tangent.n:
            raise ValueError("post_jvp: field and tangent differ in size")
        dv, dt, n, shape = field, field_tangent, field.n, None
    else:
        v = np.asarray(field)
        t = np.asarray(field_tangent)
        if v.shape != t.shape:
            raise ValueError("post_jvp: field %r and tangent %r differ in shape" % (v.shape, t.shape))
        shape = v.shape
        dv = _engine.DeviceField.from_host(v, config.device)
        dt = _engine.DeviceField.from_host(t, config.device)
        n = dv.n
    out_v, out_t = _engine.DeviceField(n, config.device), _engine.DeviceField(n, config.device)
    _engine.check(L.sdfk_value_jvp_device(_ops.BY_NAME[opname].code, _engine._ptr(P), vp(dv.ptr), vp(dt.ptr), n,
                                          vp(out_v.ptr), vp(out_t.ptr), None), "sdfk_value_jvp_device")
    _engine.check(L.sdfk_sync(None), "sdfk_sync")
    if resident:
        return out_v, out_t
    dv.free()
    dt.free()
    return _host(out_v).reshape(shape), _host(out_t).reshape(shape)


# ---------------------------------------------------------------------------------------------------
# reverse mode
# ---------------------------------------------------------------------------------------------------
def adjoint_limits():
    """(restore-tape floats per point, parameters per program) the adjoint kernel accepts."""
    tape, params = ctypes.c_int(0), ctypes.c_int(0)
    _engine.lib().sdfk_vjp_limits(ctypes.byref(tape), ctypes.byref(params))
    return tape.value, params.value


def _adjoint_program(low, origin):
    """The native program of a lowering, checked for dual rules and the adjoint kernel's tape and parameter limits."""
    prog = _program(low, origin)
    tape = ctypes.c_int64(0)
    rc = _engine.lib().sdfk_program_vjp_check(prog.handle, None, ctypes.byref(tape))
    if rc == 3:
        raise UnsupportedOpError("program too large for the adjoint kernel: its restore tape takes %d floats per point, "
                                 "%d at most" % (tape.value, adjoint_limits()[0]))
    if rc == 4:
        raise UnsupportedOpError("program too large for the adjoint kernel: %d parameters, %d at most"
                                 % (low.params.size, adjoint_limits()[1]))
    _engine.check(rc, "sdfk_program_vjp_check")
    return prog


def _point_count(co):
    """N of what _eval.device_coords accepts, on the host (nothing touches the GPU)."""
    if isinstance(co, _engine.DeviceVectorField):
        return int(co.n)
    axes = getattr(co, "grid_axes", None) if config.grid_fast_path else None
    if axes is not None:
        return int(np.prod([np.asarray(a).size for a in axes]))
    return _engine.coords_n(np.shape(co))


def _check_size(x, n, what):
    size = x.n if isinstance(x, _engine.DeviceField) else np.asarray(x).size
    if size != n or (not isinstance(x, _engine.DeviceField) and np.ndim(x) != 1):
        raise ValueError("%s must be an (N,) array or a DeviceField of N = %d points; got %s" %
                         (what, n, size if isinstance(x, _engine.DeviceField) else np.shape(x)))


def chain_rule(rows, pbar, layout, argnums):
    """θ̄_k = Σ_j P̄_j dP_j/dθ_k in float64, shaped like JAX's grad: a float for a scalar primal, an (m,) array for a 1-D
    one, a tuple of those for a tuple `argnums`. rows: (channels, n_params) float64 (parameter_tangents)."""
    theta = np.asarray(rows, dtype=np.float64).dot(np.asarray(pbar, dtype=np.float64)) if len(rows) else np.zeros(0)
    grads = [float(theta[first]) if scalar else theta[first:first + count].copy() for first, count, scalar in layout]
    return grads[0] if isinstance(argnums, (int, np.integer)) else tuple(grads)


def _reverse(prog, co, d_in, mode, generic, n_params):
    """One adjoint launch -> (value DeviceField, P̄ (n_params,) float64, loss)."""
    _engine.require_gpu()
    L = _engine.lib()
    vp = _engine._vp
    _engine.check(L.sdfk_set_device(config.device), "sdfk_set_device")
    with contextlib.ExitStack() as on_error, contextlib.ExitStack() as stack:
        coords = stack.enter_context(device_coords(co, "autodiff"))
        if not isinstance(d_in, _engine.DeviceField):
            d_in = stack.enter_context(_engine.DeviceField.from_host(np.asarray(d_in, dtype=np.float32), config.device))
        value = on_error.enter_context(_engine.DeviceField(coords.n, config.device))
        pbar = np.zeros(n_params, dtype=np.float64)
        loss = ctypes.c_double(0.0)
        _engine.check(L.sdfk_eval_vjp_device(prog.handle, vp(coords.ptr), coords.n, coords.stride, vp(d_in.ptr), mode,
                                             1 if generic else 0, vp(value.ptr), _engine._ptr(pbar), ctypes.byref(loss),
                                             None), "sdfk_eval_vjp_device")
        on_error.pop_all()
        return value, pbar, loss.value


def _grad(builder, co, primals, d_in, argnums, mode, generic, what):
    n = _point_count(co)
    _check_size(d_in, n, what)
    low, origin, rows, _chans, layout = parameter_tangents(builder, primals, argnums)
    prog = _adjoint_program(low, origin)
    value, pbar, loss = _reverse(prog, co, d_in, mode, generic, low.params.size)
    return value, chain_rule(rows, pbar, layout, argnums), loss


def vjp(builder, co, primals, cotangent, argnums=0, resident=False, generic_rules=False):
    """(field, Σ_i c_i ∂f_i/∂θ) for the primals named by `argnums`, from ONE pass of the adjoint kernel whatever their
    number. `builder`, `co`, `primals`, `argnums` as in value_and_jacfwd; `cotangent` c: an (N,) host array or a
    DeviceField. Returns (value, grads): value (N,) host float32, or a DeviceField with resident=True; grads in JAX's
    grad structure — a float per scalar primal, a float64 (m,) array per 1-D primal, a tuple for a tuple `argnums`.
    generic_rules=True derives every instruction's product from its dual rule (no hand-written adjoints): a check."""
    value, grads, _loss = _grad(builder, co, primals, cotangent, argnums, 0, generic_rules, "the cotangent")
    return (value if resident else _host(value)), grads


def value_and_grad_sse(builder, co, primals, target, argnums=0, generic_rules=False):
    """(L, ∂L/∂θ) of L = Σ_i (f_i - t_i)² in one adjoint pass: the field, the cotangent 2 (f_i - t_i) (in registers) and
    the loss (float64) come from the same launch. `target`: an (N,) host array (rounded to float32) or a DeviceField;
    the rest as in vjp. This is the `value_and_grad(worker)` of the reference's optimisation examples."""
    value, grads, loss = _grad(builder, co, primals, target, argnums, 1, generic_rules, "the target")
    value.free()
    return loss, grads
