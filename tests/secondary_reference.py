"""Float64 reference of aegolius_amd.render.visibility / ambient_occlusion: both rules over a field (the rules of the
module text of render.py and of csrc/sdfk_raydev.h, operation by operation but in float64), a copy of the visibility rule
in numpy float32 (what the accumulation of t in fp32 alone does to vis), closed forms, and the conditioning of the scene
views that the CPU and the GPU tests share. Test infrastructure — never on a product code path."""
import numpy as np

import aegolius_amd.cores as ns
import render_reference as ref
import spans_reference as sref

MISS, HIT, LIMIT = ref.MISS, ref.HIT, ref.LIMIT


def trace_visibility(field, origins, directions, t_min, t_max, eps, cone, lipschitz, max_steps, softness, limits=None,
                     dtype=np.float64):
    """The visibility rule, vectorised over the rays that still march. field: (3, n) float64 -> (n,).
    dtype = float64: the reference. dtype = float32: every number of the rule is a float32 as in the kernel — the field's
    value rounded to float32, 1 / L rounded once, p = fmaf(t, d, o) and t = fmaf(f, 1 / L, t) rounded once (computed in
    float64, where the product of two float32 is exact). -> (vis, status uint8, steps int32, final t)."""
    f32 = np.dtype(dtype) == np.float32
    T = np.float32 if f32 else np.float64
    o = np.asarray(origins, dtype=np.float64)
    d = np.asarray(directions, dtype=np.float64)
    n = o.shape[1]
    inv = np.float64(np.float32(1.0 / lipschitz)) if f32 else 1.0 / float(lipschitz)
    k = np.float64(T(softness))
    eps, cone = np.float64(T(eps)), np.float64(T(cone))
    t_end = np.full(n, np.float64(T(t_max)))
    if limits is not None:
        t_end = np.minimum(t_end, np.asarray(limits, dtype=T).astype(np.float64))
    t = np.full(n, np.float64(T(t_min)))
    vis = np.ones(n)
    status = np.full(n, LIMIT, dtype=np.uint8)
    steps = np.zeros(n, dtype=np.int32)
    active = np.arange(n)

    def rnd(x):                                                 # one rounding to the rule's precision
        return x.astype(np.float32).astype(np.float64) if f32 else x
    for _ in range(int(max_steps)):
        if active.size == 0:
            break
        ta = t[active]
        f = rnd(field(rnd(o[:, active] + ta * d[:, active])))
        thr = np.maximum(eps, rnd(cone * ta))
        hit = f <= thr
        vis[active[hit]] = 0.0
        status[active[hit]] = HIT
        go = active[~hit]
        fg, tg = f[~hit], ta[~hit]
        if k > 0.0:
            with np.errstate(divide="ignore", invalid="ignore"):
                est = rnd(rnd(k * rnd(fg * inv)) / tg)          # t = 0: +inf (f > 0)
            vis[go] = np.fmin(vis[go], est)
        t[go] = rnd(fg * inv + tg)
        steps[go] += 1
        miss = t[go] > t_end[go]
        status[go[miss]] = MISS
        active = go[~miss]
    return vis, status, steps, t


def occlusion(field, points, normals, radius, samples, strength, lipschitz):
    """The ambient-occlusion rule in float64. -> ao (n,)."""
    p = np.asarray(points, dtype=np.float64)
    nrm = np.asarray(normals, dtype=np.float64)
    occ = np.zeros(p.shape[1])
    for i in range(1, int(samples) + 1):
        h = radius * i / samples
        occ += 2.0 ** -i * np.maximum(0.0, h - field(p + h * nrm) / lipschitz)
    return np.minimum(1.0, np.maximum(0.0, 1.0 - strength * occ / radius))


def occlusion_tolerance(geometry, points, normals, radius, samples, strength, lipschitz):
    """What an fp32 evaluation of the rule may differ from `occlusion` by: every sample's field is off by at most its slack
    (render_reference.slack), which enters occ as 2^-i slack_i / L, and occ enters ao as strength / radius; the rule's own
    roundings — h (two), the sample point (in the slack), f / L, the difference, one fmaf per sample, the last three
    operations: each below 2^-24 of a number that is at most 1 in units of ao when ao is not clamped — are covered by 16 2^-24.
    -> (n,)."""
    p = np.asarray(points, dtype=np.float64)
    nrm = np.asarray(normals, dtype=np.float64)
    tol = np.zeros(p.shape[1])
    for i in range(1, int(samples) + 1):
        h = radius * i / samples
        tol += 2.0 ** -i * ref.slack(geometry, p + h * nrm, lipschitz)[1] / lipschitz
    return strength / radius * tol + 16.0 * 2.0 ** -24


# ---- closed forms ---------------------------------------------------------------------------------------------------------------
def sphere_clearance(o, d, centre, radius, t_min, t_end):
    """The smallest distance of the segment o + t d, t in [t_min, t_end], from the sphere's surface (negative: inside)."""
    oc = o - np.asarray(centre, dtype=np.float64)[:, None]
    t = np.clip(-(oc * d).sum(axis=0), t_min, t_end)
    return np.linalg.norm(oc + t * d, axis=0) - radius


def sphere_visibility(o, d, centre, radius, t_min, t_max, thr):
    """Hard visibility past a sphere by render_reference.sphere_hit: 0 where the segment meets the sphere, 1 where it does
    not. -> (vis, band): the march blocks a ray at f <= thr, so a ray that misses the sphere but comes within thr of it may
    be blocked or clear; `band` marks those."""
    t_hit, _ = ref.sphere_hit(o, d, centre, radius, t_min, t_max)
    vis = np.where(np.isfinite(t_hit), 0.0, 1.0)
    clear = sphere_clearance(o, d, centre, radius, t_min, t_max)
    return vis, (vis == 1.0) & (clear <= thr)


def floor_and_wall(a):
    """The floor z <= 0 and the wall x >= a: the field min(z, a - x)."""
    return ns.CombineGeometry("UNION").combine(ns.OrientedPlane((0.0, 0.0, 1.0), 0.0), ns.OrientedPlane((-1.0, 0.0, 0.0), -a))


def floor_and_wall_ao(a, radius, samples, strength):
    """AO of the floor point at distance a from the wall, normal +z: the samples see min(h_i, a)."""
    h = radius * np.arange(1, samples + 1) / samples
    occ = np.sum(2.0 ** -np.arange(1, samples + 1) * np.maximum(0.0, h - np.minimum(h, a)))
    return 1.0 - strength / radius * occ


# ---- the scene views: reference, conditioning, tolerance ------------------------------------------------------------------------
SCENE_EPS, SCENE_SOFTNESS, SCENE_W, SCENE_H = 2e-3, 8.0, 160, 120
TOL_CAP = 0.05                 # a ray whose derived tolerance is larger than this counts as ill-conditioned
# The absolute floor of the visibility tolerance: 4 x the largest amount by which the float32 copy of the rule
# (trace_visibility(dtype=float32): oracle values rounded to float32, t accumulated in float32) differs from the float64
# reference beyond the shift term, over the well-conditioned rays of all scene views. Measured on the CPU: 2.4364e-7
# (cloud / perspective; every other view is below 2e-7) — tests/test_secondary_cpu.py checks every view against it.
A = 9.75e-7


def conditioned_visibility(geometry, lipschitz, o, d, t_min, t_max, eps, cone, max_steps, softness, limits=None, floor=0.0):
    """-> ((vis, status, steps, t) of the reference over the oracle, ill (n,) bool, tolerance of vis (n,)).
    A ray is ILL-CONDITIONED, by the reference alone, when its status changes with the oracle shifted by +slack or by -slack
    (spans_reference.shifted_field: what an fp32 evaluation may differ by) or when it reaches the step limit. The tolerance
    of the others is 2 max(|vis+ - vis|, |vis- - vis|) + floor — twice what the uniform shifts do to vis, because the
    kernel's error is not a uniform shift, plus an absolute floor for the fp32 accumulation of t, which no shift models."""
    base = trace_visibility(ref.oracle_field(geometry), o, d, t_min, t_max, eps, cone, lipschitz, max_steps, softness, limits)
    ill = base[1] == LIMIT
    shift = np.zeros(base[0].shape)
    for sign in (-1.0, 1.0):
        other = trace_visibility(sref.shifted_field(geometry, lipschitz, sign), o, d, t_min, t_max, eps, cone, lipschitz,
                                 max_steps, softness, limits)
        ill |= other[1] != base[1]
        shift = np.maximum(shift, np.abs(other[0] - base[0]))
    return base, ill, 2.0 * shift + floor


def scene_views():
    """(scene, view) of every scene view of the GPU tests (the twisted box: perspective only, as in the render tests)."""
    return [(n, v) for n in ref.SCENES for v in (("perspective",) if n == "twisted" else ("perspective", "ortho_x"))]


def view_rays(vname, w=SCENE_W, h=SCENE_H):
    """The camera's rays rounded to float32 (directions as they are: unit to 1e-7), and the same numbers in float64."""
    o, d = (np.asarray(x, dtype=np.float32) for x in ref.cameras()[vname].rays(w, h))
    return o, d, o.astype(np.float64), d.astype(np.float64)
