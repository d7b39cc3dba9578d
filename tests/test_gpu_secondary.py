"""aegolius_amd.render.visibility / ambient_occlusion / illuminate on the GPU (kernels: csrc/sdfk_rays.inc,
sdfk_trace_visibility and sdfk_trace_occlusion in csrc/sdfk_raydev.h): the same march as cast bit for bit, interpreter =
specialised and culled = not culled bit for bit, the launch sizes, closed forms, the lower bound of vis, parity of ao and vis
with the float64 reference, per-ray ends, and illuminate. Scenes, views and slack: tests/render_reference.py; the reference
rules, closed forms and the conditioning: tests/secondary_reference.py.

Ill-conditioned share of each view by the reference alone (secondary_reference.conditioned_visibility, 160 x 120, eps 2e-3,
softness 8; tests/test_secondary_cpu.py checks them), which must stay within CAP = 0.005: cloud / perspective 0.00005, every
other view of cfg1, cfg2, cfg5, union200, cloud, onion_scaled, extruded, sheared (perspective / ortho_x) and twisted
(perspective) 0. No view exceeds the cap, so none needs other options.

The absolute floor A of the visibility tolerance (test 7) is 9.75e-7 = 4 x 2.4364e-7, the largest excess of the numpy-float32
copy of the rule over the shift term across these views (cloud / perspective), measured on the CPU
(secondary_reference.A; the other views: cfg2 1.96e-7 / 9.6e-8, cfg5 1.35e-7 / 1.13e-7, union200 1.64e-7 / 1.54e-7, cloud
ortho_x 8.7e-8, all others 0)."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import aegolius_amd.cores as ns  # noqa: E402
import render_reference as ref  # noqa: E402
import secondary_reference as sec  # noqa: E402
import spans_reference as sref  # noqa: E402
from aegolius_amd import _engine, render  # noqa: E402
from aegolius_amd._eval import config, program_for  # noqa: E402
from aegolius_amd._lower import lower_geometry  # noqa: E402
from test_gpu_render import CAP, f32, mode, setup, views  # noqa: E402

pytestmark = pytest.mark.gpu

W, H = sec.SCENE_W, sec.SCENE_H
EPS, SOFT = sec.SCENE_EPS, sec.SCENE_SOFTNESS
THR = float(np.float32(EPS))                                   # cone = 0: the threshold of every scene test, as the kernel sees it
SCENE_VIEWS = sec.scene_views()
AO_RADIUS, AO_SAMPLES = 0.2, 5
CENTRE, RADIUS = np.array([0.2, -0.1, 0.15]), 0.5              # the sphere of the closed-form tests (test_render_cpu)

_SCENE = {}


def scene(name, vname):
    """One scene view, computed once: the geometry, its bound, the camera's float32 rays (and the same numbers in float64),
    and render.visibility along them with softness 0 and SOFT."""
    if (name, vname) not in _SCENE:
        geo, explicit, L, t_max, steps = setup(name)
        o, d, o64, d64 = sec.view_rays(vname)
        vis = {k: render.visibility(geo, o, d, 0.0, t_max, EPS, 0.0, steps, explicit, k) for k in (0.0, SOFT)}
        _SCENE[name, vname] = dict(geo=geo, explicit=explicit, L=L, t_max=t_max, steps=steps, o=o, d=d, o64=o64, d64=d64, vis=vis)
    return _SCENE[name, vname]


_HITS = {}


def hit_points(name, vname):
    """The hit points and stencil normals of render() of one scene view (its default thresholds), computed once; pixels
    whose stencil is degenerate (the zero vector) are left out."""
    if (name, vname) not in _HITS:
        geo, explicit, L, t_max, steps = setup(name)
        img = render.render(geo, views(name)[vname], W, H, 0.0, t_max, steps, explicit)
        p = img.points()
        n = np.ascontiguousarray(img.normals[img.status == render.HIT].T)
        unit = np.abs((n.astype(np.float64) ** 2).sum(axis=0) - 1.0) <= 1e-5
        _HITS[name, vname] = (geo, explicit, L, np.ascontiguousarray(p[:, unit]), np.ascontiguousarray(n[:, unit]))
    return _HITS[name, vname]


def bits(x):
    return np.asarray(x, dtype=np.float32).view(np.uint32)


# ---- 1. the same march as cast ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,vname", SCENE_VIEWS)
def test_same_march_as_cast(engine, name, vname):
    s = scene(name, vname)
    hits = render.cast(s["geo"], s["o"], s["d"], 0.0, s["t_max"], EPS, 0.0, s["steps"], s["explicit"])
    for k, got in s["vis"].items():
        assert np.array_equal(got.status, hits.status) and np.array_equal(got.steps, hits.steps)
        assert np.array_equal(got.vis == 0.0, hits.status == render.HIT)
        assert np.all((got.vis >= 0.0) & (got.vis <= 1.0))
    hard, soft = s["vis"][0.0], s["vis"][SOFT]
    assert np.all(hard.vis[hits.status == render.MISS] == 1.0) and np.all((hard.vis == 0.0) | (hard.vis == 1.0))
    assert np.all(soft.vis <= hard.vis)
    print("%s/%s: %d blocked, %d clear, %d at the step limit; %d rays in a penumbra" % (
        name, vname, (hits.status == render.HIT).sum(), (hits.status == render.MISS).sum(), (hits.status == render.LIMIT).sum(),
        ((soft.vis > 0.0) & (soft.vis < 1.0)).sum()))
    assert (hits.status == render.HIT).sum() > 500 and ((soft.vis > 0.0) & (soft.vis < 1.0)).sum() > 500


# ---- 2. interpreter = specialised, culled = not culled, bit for bit -----------------------------------------------------------
def secondary(s, pts, nrm, o=None, d=None):
    o, d = (s["o"], s["d"]) if o is None else (o, d)
    out = [render.visibility(s["geo"], o, d, 0.0, s["t_max"], EPS, 0.0, s["steps"], s["explicit"], k) for k in (0.0, SOFT)]
    ao = [render.ambient_occlusion(s["geo"], pts, nrm, AO_RADIUS, m, 1.5, s["explicit"]) for m in (AO_SAMPLES, 16)]
    return out, ao


def same_bits(a, b):
    for x, y in zip(a[0], b[0]):
        assert np.array_equal(x.status, y.status) and np.array_equal(x.steps, y.steps) and np.array_equal(bits(x.vis), bits(y.vis))
    for x, y in zip(a[1], b[1]):
        assert np.array_equal(bits(x), bits(y))


@pytest.mark.parametrize("name", list(ref.SCENES))
def test_interpreter_equals_specialised_bit_for_bit(engine, name):
    s = scene(name, "perspective")
    assert lower_geometry(s["geo"]).fits_interpreter
    _, _, _, pts, nrm = hit_points(name, "perspective")
    out = {}
    for m in (_engine.MODE_INTERPRET, _engine.MODE_SPECIALIZED):
        with mode(m):
            out[m] = secondary(s, pts, nrm)
    same_bits(out[_engine.MODE_INTERPRET], out[_engine.MODE_SPECIALIZED])
    ao = out[_engine.MODE_SPECIALIZED][1][0]
    assert pts.shape[1] > 500 and np.all((ao >= 0.0) & (ao <= 1.0))


def test_culled_equals_nocull_bit_for_bit_in_any_ray_order(engine):
    s = scene("union200", "perspective")
    assert _engine.Program.from_lowered(lower_geometry(s["geo"])).chain_members == 200
    _, _, _, pts, nrm = hit_points("union200", "perspective")
    out = {}
    for m in (_engine.MODE_SPECIALIZED, _engine.MODE_NOCULL):
        with mode(m):
            out[m] = secondary(s, pts, nrm)
    same_bits(out[_engine.MODE_SPECIALIZED], out[_engine.MODE_NOCULL])
    (hard, soft), (ao5, ao16) = out[_engine.MODE_SPECIALIZED]
    perm = np.random.default_rng(2).permutation(s["o"].shape[1])
    pp = np.random.default_rng(3).permutation(pts.shape[1])
    with mode(_engine.MODE_SPECIALIZED):
        (hard_p, soft_p), (ao5_p, ao16_p) = secondary(s, np.ascontiguousarray(pts[:, pp]), np.ascontiguousarray(nrm[:, pp]),
                                                      np.ascontiguousarray(s["o"][:, perm]), np.ascontiguousarray(s["d"][:, perm]))
    for a, b in ((hard, hard_p), (soft, soft_p)):
        assert np.array_equal(b.status, a.status[perm]) and np.array_equal(b.steps, a.steps[perm])
        assert np.array_equal(bits(b.vis), bits(a.vis[perm]))
    assert np.array_equal(bits(ao5_p), bits(ao5[pp])) and np.array_equal(bits(ao16_p), bits(ao16[pp]))


# ---- 3. sizes at which the launch can go wrong --------------------------------------------------------------------------------
GUARD_N = 320                                                  # the outputs are this long; a call writes its first n entries


@pytest.mark.parametrize("name,m", [("cfg2", _engine.MODE_INTERPRET), ("cfg2", _engine.MODE_SPECIALIZED),
                                    ("union200", _engine.MODE_SPECIALIZED)])
def test_launch_sizes_write_their_rays_only(engine, name, m):
    """n = 0, 1, 63, 64, 65, 257 rays through the C entry points into outputs of 320 entries filled with guard values: the
    first n entries are those of the 320-ray call, the others keep the guard. With and without limits; samples 1 and 16."""
    s = scene(name, "perspective")
    lib = _engine.lib()
    prog = program_for(render.lower(s["geo"])[0])
    inv = float(np.float32(1.0 / s["L"]))
    pick = np.random.default_rng(7).choice(s["o"].shape[1], GUARD_N, replace=False)
    o, d = np.ascontiguousarray(s["o"][:, pick]), np.ascontiguousarray(s["d"][:, pick])
    _, _, _, pts, nrm = hit_points(name, "perspective")
    pts, nrm = np.ascontiguousarray(pts[:, :GUARD_N]), np.ascontiguousarray(nrm[:, :GUARD_N])
    lim = np.random.default_rng(8).uniform(1.0, 6.0, GUARD_N).astype(np.float32)
    dev = config.device
    bufs = [_engine.DeviceVectorField.from_host(x, dev) for x in (o, d, pts, nrm)]
    d_o, d_d, d_p, d_n = bufs
    g_f, g_b, g_i = np.full(GUARD_N, -7.25, dtype=np.float32), np.full(GUARD_N, 0xAB, dtype=np.uint8), np.full(GUARD_N, -99, dtype=np.int32)
    with _engine.DeviceField.from_host(lim, dev) as d_lim, _engine.DeviceField(GUARD_N, dev) as d_vis, \
            _engine.DeviceBuffer(GUARD_N) as d_status, _engine.DeviceBuffer(GUARD_N * 4) as d_steps:
        def vis_call(n, limits):
            d_vis.upload(g_f), d_status.upload(g_b), d_steps.upload(g_i)
            rc = lib.sdfk_visibility_rays_device(prog.handle, _engine._vp(d_o.ptr), d_o.stride, _engine._vp(d_d.ptr), d_d.stride, n,
                                                 0.0, s["t_max"], EPS, 0.0, inv, s["steps"], SOFT, d_lim.at() if limits else None,
                                                 d_vis.at(), d_status.at(), d_steps.at(), None, m)
            _engine.check(rc, "sdfk_visibility_rays_device")
            _engine.check(lib.sdfk_sync(None), "sdfk_sync")
            return d_vis.numpy(), d_status.download(np.empty(GUARD_N, dtype=np.uint8)), d_steps.download(np.empty(GUARD_N, dtype=np.int32))

        def ao_call(n, samples):
            d_vis.upload(g_f)
            rc = lib.sdfk_occlusion_rays_device(prog.handle, _engine._vp(d_p.ptr), d_p.stride, _engine._vp(d_n.ptr), d_n.stride, n,
                                                AO_RADIUS, samples, 1.0, inv, d_vis.at(), None, m)
            _engine.check(rc, "sdfk_occlusion_rays_device")
            _engine.check(lib.sdfk_sync(None), "sdfk_sync")
            return (d_vis.numpy(),)
        for call, variants, guards in ((vis_call, (False, True), (g_f, g_b, g_i)), (ao_call, (1, 16), (g_f,))):
            for variant in variants:
                full = call(GUARD_N, variant)
                assert all(not np.any(x == g[0]) for x, g in zip(full, guards))
                for n in (0, 1, 63, 64, 65, 257):
                    for x, want, g in zip(call(n, variant), full, guards):
                        assert np.array_equal(x[:n], want[:n]) and np.array_equal(x[n:], g[n:]), (n, variant)
        with_l, without = vis_call(GUARD_N, True), vis_call(GUARD_N, False)
        assert (with_l[1] != without[1]).sum() > 10            # the ends do end rays
    for b in bufs:
        b.free()


# ---- 4. closed forms on the device ---------------------------------------------------------------------------------------------
def closed_form_sphere():
    o = ns.Sphere(RADIUS)
    o.move(CENTRE)
    return o


def test_hard_visibility_past_a_sphere(engine):
    """render.visibility with softness 0 against render_reference.sphere_hit on 20,000 rays. The kernel's field differs from
    the exact one by at most slack, so a ray is left out when its closest approach is within thr + slack outside the sphere
    or within slack inside it; their share is known before anything runs on the GPU and capped."""
    geo = closed_form_sphere()
    o64, d64 = sref.sample_rays()
    o, d = f32(o64), f32(d64)
    d = f32(d.astype(np.float64) / np.linalg.norm(d.astype(np.float64), axis=0))
    o64, d64 = o.astype(np.float64), d.astype(np.float64)
    for eps in (1e-2, 1e-3, 1e-4):
        thr = float(np.float32(eps))
        clear = sec.sphere_clearance(o64, d64, CENTRE, RADIUS, sref.T_MIN, sref.T_MAX)
        t_close = np.clip(-((o64 - CENTRE[:, None]) * d64).sum(axis=0), sref.T_MIN, sref.T_MAX)
        slack = ref.slack(geo, o64 + t_close * d64, 1.0)[1]
        band = (clear <= thr + slack) & (clear >= -slack)
        assert band.mean() <= sref.THIN_CAP                     # a condition on the sample, checked on the CPU
        want = np.where(clear < 0.0, 0.0, 1.0)
        got = render.visibility(geo, o, d, sref.T_MIN, sref.T_MAX, eps, 0.0, 200000)
        assert not np.any(got.status == render.LIMIT)
        assert np.array_equal(got.vis[~band], want[~band].astype(np.float32))
        exact, _ = ref.sphere_hit(o64, d64, CENTRE, RADIUS, sref.T_MIN, sref.T_MAX)
        assert np.array_equal(np.isfinite(exact)[~band], want[~band] == 0.0)    # (the clearance says what sphere_hit says)
        print("sphere, eps %g: %.3f %% of the rays in the band, %d blocked, most steps %d" % (
            eps, 100 * band.mean(), (got.vis == 0).sum(), got.steps.max()))


def test_occlusion_closed_forms(engine):
    """A half-space: ao = 1; the floor at distance a from a wall: 1 - s / r sum 2^-i max(0, h_i - min(h_i, a)). Tolerance:
    secondary_reference.occlusion_tolerance, the one of the parity test."""
    rng = np.random.default_rng(4)
    n_pts = 130
    p = f32(np.concatenate([rng.uniform(-2, 2, (2, n_pts)), np.zeros((1, n_pts))]))
    nrm = f32(np.repeat(np.array([[0.0], [0.0], [1.0]]), n_pts, axis=1))
    plane = ns.OrientedPlane((0.0, 0.0, 1.0), 0.0)
    for samples in (1, 5, 16):
        ao = render.ambient_occlusion(plane, p, nrm, 0.3, samples)
        tol = sec.occlusion_tolerance(plane, p, nrm, 0.3, samples, 1.0, 1.0)
        assert np.all(np.abs(ao.astype(np.float64) - 1.0) <= tol) and np.all(ao <= 1.0)
    for a, radius, samples, strength in ((0.05, 0.2, 5, 1.0), (0.1, 0.4, 16, 2.0), (0.3, 0.2, 5, 1.0), (0.01, 0.5, 1, 1.0)):
        geo = sec.floor_and_wall(a)
        q = f32(np.stack([np.zeros(n_pts), p[1], np.zeros(n_pts)]))        # floor points at distance a from the wall
        ao = render.ambient_occlusion(geo, q, nrm, radius, samples, strength)
        want = sec.floor_and_wall_ao(a, radius, samples, strength)
        tol = sec.occlusion_tolerance(geo, q, nrm, radius, samples, strength, 1.0)
        print("floor and wall a = %g, r = %g, m = %d: ao %.7f, closed form %.7f, tolerance %.2e" % (a, radius, samples, ao[0], want,
                                                                                                  tol.max()))
        assert np.all(np.abs(ao.astype(np.float64) - want) <= tol)


# ---- 5. the lower bound of vis ---------------------------------------------------------------------------------------------------
DENSE, COARSE = 4096, 256


def cell_bounds(s, o, d, mid, w):
    """Lower bounds of k (f - slack) / (L t) over the cells of width w around the parameters `mid` (n,) of the rays (o, d)
    (3, n): f >= f(mid) - L w / 2 and t <= mid + w / 2 inside a cell (the Lipschitz bound itself, no tolerance). -> (n,)."""
    f, slack = ref.slack(s["geo"], o + mid * d, s["L"])
    return SOFT * (f - slack - 0.5 * s["L"] * w) / (s["L"] * (mid + 0.5 * w))


def dense_infimum_bound(s, o, d, t_max):
    """min over the DENSE = 4096 cells of every ray of cell_bounds, computed by branch and bound: a pass over COARSE = 256
    cells first; the 16 dense cells inside a coarse cell have bounds that are at least the coarse cell's (the same
    inequalities with the larger width; slack varies by far less than L w), so a coarse cell whose bound is not below the
    smallest dense bound found so far cannot hold the minimum and is not sampled further. -> (n,)."""
    n, per = o.shape[1], DENSE // COARSE
    wc, w = t_max / COARSE, t_max / DENSE
    ray, cell = np.repeat(np.arange(n), COARSE), np.tile(np.arange(COARSE), n)
    coarse = cell_bounds(s, o[:, ray], d[:, ray], (cell + 0.5) * wc, wc).reshape(n, COARSE)
    best = np.full(n, np.inf)
    todo = coarse <= coarse.min(axis=1, keepdims=True)             # the most promising coarse cell of every ray first
    done = np.zeros_like(todo)
    while todo.any():
        ray, cell = np.nonzero(todo)
        ray, fine = np.repeat(ray, per), (cell[:, None] * per + np.arange(per)[None, :]).ravel()
        np.minimum.at(best, ray, cell_bounds(s, o[:, ray], d[:, ray], (fine + 0.5) * w, w))
        done |= todo
        todo = ~done & (coarse < best[:, None] + 1e-9)
    return best


@pytest.mark.parametrize("name", list(ref.SCENES))
def test_visibility_is_never_below_the_infimum_along_the_ray(engine, name):
    """vis >= min(1, k inf_t (f(t) - slack(t)) / (L t)) on every ray that is not blocked (a blocked ray has vis = 0 by the hit
    rule, not by the estimate): the marched samples are points of the ray, and the kernel's field is at least f - slack.
    The infimum over [0, t_max] is bounded from below cell by cell on 4096 cells per ray of a 2,000-ray subsample
    (dense_infimum_bound). The estimate is three fp32 operations, k (f / L) / t: the bound is lowered by 4 2^-24 of itself."""
    s = scene(name, "perspective")
    got = s["vis"][SOFT]
    pick = np.random.default_rng(12).choice(s["o"].shape[1], 2000, replace=False)
    bound = dense_infimum_bound(s, s["o64"][:, pick], s["d64"][:, pick], float(np.float32(s["t_max"])))
    bound = np.minimum(1.0, bound - np.abs(bound) * 4.0 * 2.0 ** -24)
    open_ = got.status[pick] != render.HIT
    vis = got.vis[pick].astype(np.float64)
    dim = open_ & (vis < 1.0)
    print("%s: %d rays not blocked, %d of them in a penumbra, where vis - bound is at least %.3e (median %.3e); %d bounds above 0" % (
        name, open_.sum(), dim.sum(), (vis - bound)[dim].min(), np.median((vis - bound)[dim]), (open_ & (bound > 0.0)).sum()))
    assert open_.sum() > 200 and (open_ & (bound > 0.0)).sum() > 100 and np.all(vis[open_] >= bound[open_])


# ---- 6. ambient occlusion: parity with the reference ---------------------------------------------------------------------------
@pytest.mark.parametrize("name,vname", SCENE_VIEWS)
def test_occlusion_parity_with_the_reference(engine, name, vname):
    """|ao - ao_ref| <= strength / radius sum 2^-i slack_i / L + 16 2^-24 at the hit points of the view."""
    geo, explicit, L, pts, nrm = hit_points(name, vname)
    ao = render.ambient_occlusion(geo, pts, nrm, AO_RADIUS, AO_SAMPLES, 1.0, explicit)
    p64, n64 = pts.astype(np.float64), nrm.astype(np.float64)
    want = sec.occlusion(ref.oracle_field(geo), p64, n64, AO_RADIUS, AO_SAMPLES, 1.0, L)
    tol = sec.occlusion_tolerance(geo, p64, n64, AO_RADIUS, AO_SAMPLES, 1.0, L)
    err = np.abs(ao.astype(np.float64) - want)
    print("%s/%s: %d points, ao from %.3f to %.3f, largest |ao - reference| %.3e, largest error / tolerance %.3f" % (
        name, vname, pts.shape[1], ao.min(), ao.max(), err.max(), (err / tol).max()))
    assert pts.shape[1] > 500 and np.all(err <= tol)


# ---- 7. visibility: parity with the reference -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name,vname", SCENE_VIEWS)
def test_visibility_parity_with_the_reference(engine, name, vname):
    """On the well-conditioned rays: the reference's status, and |vis - vis_ref| <= 2 max(|vis+ - vis_ref|, |vis- - vis_ref|)
    + A. Ill-conditioned rays, and those whose tolerance exceeds 0.05, are at most CAP of the view."""
    s = scene(name, vname)
    got = s["vis"][SOFT]
    base, ill, tol = sec.conditioned_visibility(s["geo"], s["L"], s["o64"], s["d64"], 0.0, float(np.float32(s["t_max"])), THR, 0.0,
                                                s["steps"], SOFT, floor=sec.A)
    ill = ill | (tol > sec.TOL_CAP)
    ok = ~ill
    err = np.abs(got.vis.astype(np.float64) - base[0])
    print("%s/%s: %.5f of the rays ill-conditioned; on the others %d statuses differ, largest |vis - reference| %.3e, largest "
          "error / tolerance %.3f (tolerances from %.2e to %.2e), steps gpu %d / reference %d at most" % (
              name, vname, ill.mean(), (got.status != base[1])[ok].sum(), err[ok].max(), (err / tol)[ok].max(), tol[ok].min(),
              tol[ok].max(), got.steps.max(), base[2].max()))
    assert ill.mean() <= CAP
    assert np.array_equal(got.status[ok], base[1][ok])
    assert np.all(err[ok] <= tol[ok])


# ---- 8. limits -------------------------------------------------------------------------------------------------------------------
def test_limits_end_the_rays_at_the_light(engine):
    """A sphere (centre (0, 0, 1), radius 0.3) between a point light at (0, 0, 2) and the plane z = 0.
    Rays from above the light, aimed at it: with limits = the distance to the light they end before the sphere and are clear;
    the same rays without limits and t_max = 8 go on into the sphere and are blocked.
    Rays from points of the plane toward the light, limits = the distance: blocked under the sphere, clear outside its shadow."""
    sphere = ns.Sphere(0.3)
    sphere.move((0.0, 0.0, 1.0))
    geo = ns.CombineGeometry("UNION").combine(ns.OrientedPlane((0.0, 0.0, 1.0), 0.0), sphere)
    light = render.Light.point((0.0, 0.0, 2.0))
    rng = np.random.default_rng(21)
    n = 300
    above = np.stack([rng.uniform(-0.15, 0.15, n), rng.uniform(-0.15, 0.15, n), rng.uniform(3.0, 4.0, n)])
    d64, dist = light.rays(above)
    o, d = f32(above), f32(d64)
    d = f32(d.astype(np.float64) / np.linalg.norm(d.astype(np.float64), axis=0))
    assert np.all(np.isfinite(ref.sphere_hit(o.astype(np.float64), d.astype(np.float64), (0, 0, 1.0), 0.3, 0.0, 8.0)[0]))
    ended = render.visibility(geo, o, d, 0.0, 8.0, 1e-3, limits=f32(dist))
    assert np.all(ended.vis == 1.0) and np.all(ended.status == render.MISS)
    longer = render.visibility(geo, o, d, 0.0, 8.0, 1e-3, limits=None)
    assert np.all(longer.vis == 0.0) and np.all(longer.status == render.HIT)
    # from the plane: which points lie in the sphere's shadow is decided by the clearance of their segment, in closed form
    floor = np.stack([rng.uniform(-1.5, 1.5, 2000), rng.uniform(-1.5, 1.5, 2000), np.full(2000, 0.01)])
    d64, dist = light.rays(floor)
    o, d = f32(floor), f32(d64)
    d = f32(d.astype(np.float64) / np.linalg.norm(d.astype(np.float64), axis=0))
    o64, d64 = o.astype(np.float64), d.astype(np.float64)
    t_end = float(f32(dist).max())
    clear = sec.sphere_clearance(o64, d64, (0, 0, 1.0), 0.3, 0.0, f32(dist).astype(np.float64))
    band = (clear <= 1e-3 + 1e-5) & (clear >= -1e-5)           # (thr + slack; the slack of these points is below 1e-5)
    got = render.visibility(geo, o, d, 0.0, t_end, 1e-3, limits=f32(dist))
    assert band.mean() <= sref.THIN_CAP and (clear < 0).sum() > 50 and (clear > 1e-2).sum() > 500
    assert np.array_equal(got.vis[~band] == 0.0, clear[~band] < 0.0) and np.all((got.vis == 0.0) | (got.vis == 1.0))
    # a DeviceField of limits gives the same bytes
    with _engine.DeviceField.from_host(f32(dist), config.device) as dev:
        again = render.visibility(geo, o, d, 0.0, t_end, 1e-3, limits=dev, resident=True)
        assert isinstance(again.vis, _engine.DeviceField)
        assert np.array_equal(bits(again.vis.numpy()), bits(got.vis)) and np.array_equal(again.steps, got.steps)
        again.vis.free()


# ---- 9. illuminate ---------------------------------------------------------------------------------------------------------------
def test_illuminate_a_lone_sphere(engine):
    """A convex body does not shadow itself: from o = p + bias n on a sphere, f(o + t l) >= bias + t (n . l), so the estimate
    k f / t never drops below k (n . l): shadow = 1 wherever k (n . l) >= 1 + 1e-3 — with the exact normals, which are the n
    of this argument — and 0 where the pixel faces away. Ambient occlusion of a sphere is 1 up to its tolerance."""
    geo = ns.Sphere(0.5)
    cam = ref.cameras()["perspective"]
    img = render.render(geo, cam, W, H, 0.0, 8.0)
    img.exact_normals(geo)
    toward = np.array([-0.5, 1.0, -0.3])            # nearly at right angles to the viewing direction
    out = render.illuminate(geo, img, render.Light.directional(toward), softness=SOFT, ao_radius=AO_RADIUS)
    assert out is img and img.shadow.shape == (H, W) and img.shadow.dtype == np.float32 and img.ao.shape == (H, W)
    hit = img.status == render.HIT
    nl = img.normals.astype(np.float64).dot(toward / np.linalg.norm(toward))
    lit, away = hit & (SOFT * nl >= 1.0 + 1e-3), hit & (nl <= 0.0)
    print("lone sphere: %d hit pixels, %d lit, %d facing away, %d in between (shadow from %.3f to %.3f there)" % (
        hit.sum(), lit.sum(), away.sum(), (hit & ~lit & ~away).sum(), img.shadow[hit & ~lit & ~away].min(),
        img.shadow[hit & ~lit & ~away].max()))
    assert lit.sum() > 500 and away.sum() > 500
    assert np.all(img.shadow[lit] == 1.0) and np.all(img.shadow[away] == 0.0) and np.all(img.shadow[~hit] == 1.0)
    assert np.all((img.shadow >= 0.0) & (img.shadow <= 1.0))
    assert np.all(img.ao[~hit] == 1.0) and np.all(img.ao[hit] >= 1.0 - 1e-4) and np.all(img.ao <= 1.0)
    shaded = img.shade(light=toward, shadow=img.shadow, occlusion=img.ao, dtype=np.float32)
    assert np.all(shaded[away] <= 0.15 + 1e-6) and shaded[lit].max() > 0.9
    # without ao_radius the occlusion image is not made
    img2 = render.render(geo, cam, 64, 48, 0.0, 8.0)
    render.illuminate(geo, img2, render.Light.point((3.0, 1.0, 1.0)))
    assert img2.ao is None and img2.shadow.shape == (48, 64)
    nl2 = (img2.normals[img2.status == render.HIT].astype(np.float64).T *
           render.Light.point((3.0, 1.0, 1.0)).rays(img2.points().astype(np.float64))[0]).sum(axis=0)
    assert np.all(img2.shadow[img2.status == render.HIT][nl2 < -0.05] == 0.0) and (img2.shadow[img2.status == render.HIT] == 1.0).sum() > 100


def test_illuminate_hard_shadow_of_a_sphere_on_a_plane(engine):
    """A sphere over the half-space z <= 0, directional light, softness 0: a plane pixel is in shadow exactly when its shadow
    ray — from p + bias n toward the light, bias = 4 stencil widths, as illuminate documents — meets the sphere by
    sphere_hit. Pixels whose ray passes within the march's threshold (half the smallest bias) + slack of the sphere are
    left out; their share is capped."""
    c, r = np.array([0.0, 0.0, 0.6]), 0.35
    sphere = ns.Sphere(r)
    sphere.move(c)
    geo = ns.CombineGeometry("UNION").combine(ns.OrientedPlane((0.0, 0.0, 1.0), 0.0), sphere)
    cam = ref.cameras()["perspective"]
    img = render.render(geo, cam, W, H, 0.0, 8.0)
    toward = np.array([0.3, -0.2, 1.0])
    light = render.Light.directional(toward)
    render.illuminate(geo, img, light, softness=0.0)
    hit = img.status == render.HIT
    p32 = img.points()
    pts, nrm = p32.astype(np.float64), img.normals[hit].astype(np.float64).T
    lift = render.BIAS_WIDTHS * render.stencil_width(img.t[hit], p32, img.eps, img.cone).astype(np.float64)
    o64 = f32(pts + lift * nrm).astype(np.float64)
    d64 = f32(np.repeat(light.toward[:, None], pts.shape[1], axis=1)).astype(np.float64)
    d64 = f32(d64 / np.linalg.norm(d64, axis=0)).astype(np.float64)
    t_far = float(np.float32(img.t.max()))
    plane = (np.abs(pts[2]) < 0.05) & ((nrm * d64).sum(axis=0) > 0.0)
    thr2 = float(np.float32(0.5 * lift[(nrm * d64).sum(axis=0) > 0.0].min()))
    clear = sec.sphere_clearance(o64, d64, c, r, 0.0, t_far)
    band = (clear <= thr2 + 1e-5) & (clear >= -1e-5)
    want = np.isfinite(ref.sphere_hit(o64, d64, c, r, 0.0, t_far)[0])
    shadow = img.shadow[hit]
    use = plane & ~band
    print("sphere on a plane: %d plane pixels, %d in shadow, %.3f %% in the boundary band" % (
        plane.sum(), (plane & want).sum(), 100 * band[plane].mean()))
    assert plane.sum() > 3000 and (use & want).sum() > 100 and band[plane].mean() <= sref.THIN_CAP
    assert np.array_equal(shadow[use] == 0.0, want[use]) and np.all((shadow[use] == 0.0) | (shadow[use] == 1.0))
