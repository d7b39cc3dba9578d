"""The culled ray kernels of long hard unions (per-wave survivor lists: csrc/sdfk_raycull.h SdfkCullField) on
the GPU: the same bits as the plain kernel (MODE_NOCULL) over scenes, views and the edge cases of cast; the lists exist and
are used (statistics build); soundness and parity of the 1000-member union against the float64 tracer."""
import ctypes
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import aegolius_amd.cores as ns  # noqa: E402
import render_reference as ref  # noqa: E402
from aegolius_amd import _engine, render, workloads  # noqa: E402
from aegolius_amd._eval import config  # noqa: E402
from aegolius_amd._lower import lower_geometry  # noqa: E402

pytestmark = pytest.mark.gpu

W, H = 320, 240
T_MAX, MAX_STEPS = 8.0, 256
CAP = 0.005                      # as test_gpu_render.py: share of a view's rays that may disagree with the float64 tracer
FAR = np.array([1000.0, 0.0, 0.0])


def f32(x):
    return np.asarray(x, dtype=np.float32)


class mode:
    def __init__(self, m):
        self.m = m

    def __enter__(self):
        self.old, config.mode = config.mode, self.m

    def __exit__(self, *exc):
        config.mode = self.old


def _spheres(count, seed, radius=0.05, extent=0.9):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        o = ns.Sphere(float(radius * rng.uniform(0.5, 1.5)))
        o.move(rng.uniform(-extent, extent, 3))
        out.append(o)
    return out


def box_minus_spheres():
    return ns.CombineGeometry("SUBTRACT2").combine(ns.Box(1.6, 1.6, 1.6), ns.CombineGeometry("UNION").combine(*_spheres(500, 5, 0.08)))


def spheres_in_sphere():
    return ns.CombineGeometry("INTERSECT2").combine(ns.CombineGeometry("UNION").combine(*_spheres(500, 6, 0.08)), ns.Sphere(0.8))


def polytope(count=80):
    rng = np.random.default_rng(9)
    planes = []
    for _ in range(count):
        n = rng.normal(size=3)
        planes.append(ns.OrientedPlane(n / np.linalg.norm(n), float(rng.uniform(0.5, 0.7))))
    return ns.CombineGeometry("INTERSECT").combine(*planes)


def far_union():
    geo = workloads.sphere_union(ns, count=1000)
    geo.move(FAR)
    return geo


SCENES = {
    "union100": lambda: workloads.sphere_union(ns, count=100),
    "union300": lambda: workloads.sphere_union(ns, count=300),
    "union1000": lambda: workloads.sphere_union(ns, count=1000),
    "union16384": lambda: workloads.sphere_union(ns, count=16384, radius=0.02),
    "clustered": lambda: workloads.clustered_union(ns),
    "box_minus_500": box_minus_spheres,
    "500_in_sphere": spheres_in_sphere,
    "polytope80": polytope,
    "union1000_far": far_union,
}


def cameras(name):
    cams = ref.cameras()
    if name != "union1000_far":
        return cams
    return {"perspective": render.Camera(np.array(ref.EYE) + FAR, FAR, (0, 0, 1), 40.0),
            "ortho_x": render.Camera.orthographic(np.array([3.0, 0.0, 0.0]) + FAR, FAR, (0, 0, 1), 2.4)}


def same(a, b):
    np.testing.assert_array_equal(a.status, b.status)
    np.testing.assert_array_equal(a.steps, b.steps)
    np.testing.assert_array_equal(np.asarray(a.t).view(np.uint32), np.asarray(b.t).view(np.uint32))
    if a.normals is not None or b.normals is not None:
        np.testing.assert_array_equal(np.asarray(a.normals).view(np.uint32), np.asarray(b.normals).view(np.uint32))


def both(call):
    out = []
    for m in (_engine.MODE_NOCULL, _engine.MODE_SPECIALIZED):
        with mode(m):
            out.append(call())
    return out


@pytest.mark.parametrize("name", list(SCENES))
def test_culled_kernel_has_the_plain_kernels_bits(engine, name):
    geo = SCENES[name]()
    assert _engine.Program.from_lowered(lower_geometry(geo)).chain_members >= 64
    w, h = (160, 120) if name == "union16384" else (W, H)
    for vname, cam in cameras(name).items():
        plain, culled = both(lambda: render.render(geo, cam, w, h, 0.0, T_MAX, MAX_STEPS))
        same(plain, culled)
        hits = int((plain.status == render.HIT).sum())
        print("%s/%s %dx%d: %d hits, %d at the step limit" % (name, vname, w, h, hits, (plain.status == render.LIMIT).sum()))
        assert hits > 100, vname


def test_tiles_cut_by_the_image_edge(engine):
    geo = SCENES["union1000"]()
    for cam in ref.cameras().values():
        same(*both(lambda: render.render(geo, cam, 163, 117, 0.0, T_MAX, MAX_STEPS)))


def _camera_rays(w=W, h=H):
    cam = ref.cameras()["perspective"]
    o, d = (f32(x) for x in cam.rays(w, h))
    eps, cone = cam.footprint(w, h)
    return o, d, eps, cone


def test_cast_permuted_rays(engine):
    """Incoherent waves: the overflow, split and plain paths. The result is the unpermuted one, re-indexed."""
    geo = SCENES["union1000"]()
    o, d, eps, cone = _camera_rays()
    perm = np.random.default_rng(3).permutation(o.shape[1])
    plain, culled = both(lambda: render.cast(geo, o[:, perm], d[:, perm], 0.0, T_MAX, eps, cone, MAX_STEPS, normals=True))
    same(plain, culled)
    with mode(_engine.MODE_SPECIALIZED):
        straight = render.cast(geo, o, d, 0.0, T_MAX, eps, cone, MAX_STEPS, normals=True)
    np.testing.assert_array_equal(culled.status, straight.status[perm])
    np.testing.assert_array_equal(culled.steps, straight.steps[perm])
    np.testing.assert_array_equal(culled.t.view(np.uint32), straight.t[perm].view(np.uint32))
    np.testing.assert_array_equal(culled.normals.view(np.uint32), straight.normals[:, perm].view(np.uint32))
    assert (straight.status == render.HIT).sum() > 1000


@pytest.mark.parametrize("case", ["ragged", "one_step", "t_min_inside", "t_max_short", "no_normals"])
def test_cast_edge_cases(engine, case):
    geo = SCENES["union1000"]()
    o, d, eps, cone = _camera_rays(160, 120)
    if case == "ragged":                                         # not a multiple of 64
        o, d = o[:, :64 * 40 + 37], d[:, :64 * 40 + 37]
        call = lambda: render.cast(geo, o, d, 0.0, T_MAX, eps, cone, MAX_STEPS, normals=True)   # noqa: E731
    elif case == "one_step":
        call = lambda: render.cast(geo, o, d, 2.0, T_MAX, eps, cone, 1, normals=True)          # noqa: E731
    elif case == "t_min_inside":
        # every ray is at the centre of a member at t = t_min = 0.25 (the draws of workloads.sphere_union): hit, no step
        rng, pts = np.random.default_rng(31), []
        for _ in range(1000):
            rng.uniform(0.5, 1.5)
            pts.append(rng.uniform(-0.9, 0.9, 3))
        pts = np.stack(pts, axis=1)
        o = f32(np.tile(pts, (1, 20))[:, :o.shape[1]] - 0.25 * d.astype(np.float64))
        call = lambda: render.cast(geo, o, d, 0.25, T_MAX, eps, cone, MAX_STEPS, normals=True)  # noqa: E731
    elif case == "t_max_short":
        call = lambda: render.cast(geo, o, d, 0.0, 1.5, eps, cone, MAX_STEPS, normals=True)    # noqa: E731
    else:
        call = lambda: render.cast(geo, o, d, 0.0, T_MAX, eps, cone, MAX_STEPS, normals=False)  # noqa: E731
    plain, culled = both(call)
    same(plain, culled)
    counts = {s: int((plain.status == s).sum()) for s in (render.MISS, render.HIT, render.LIMIT)}
    print(case, counts)
    if case == "one_step":
        assert counts[render.LIMIT] > 0 and plain.steps.max() == 1
    if case == "t_min_inside":
        started = (plain.status == render.HIT) & (plain.steps == 0)
        assert started.sum() > 0.9 * plain.status.size and np.all(plain.t[started] == np.float32(0.25))
    if case == "t_max_short":
        assert counts[render.HIT] == 0 and counts[render.MISS] == plain.status.size
    if case == "no_normals":
        assert culled.normals is None and counts[render.HIT] > 1000


STAT_NAMES = ("builds", "build_evaluations", "survivor_evaluations", "plain_evaluations", "splits", "point_evaluations")


class statistics:
    """The statistics build of the ray flavour for the calls inside; .read() returns and clears the counters."""

    def __enter__(self):
        L = _engine.lib()
        assert hasattr(L, "sdfk_debug_rays_stats")
        L.sdfk_debug_set_rtc_defs(b"-DSDFK_DEBUG_RAYSTATS=1")
        self.out = (ctypes.c_longlong * 8)()
        L.sdfk_debug_rays_stats(1, self.out)
        return self

    def read(self):
        _engine.lib().sdfk_debug_rays_stats(1, self.out)
        return dict(zip(STAT_NAMES, (int(v) for v in self.out)))

    def __exit__(self, *exc):
        _engine.lib().sdfk_debug_rays_stats(0, None)
        _engine.lib().sdfk_debug_set_rtc_defs(b"")


def members_per_evaluation(c, members):
    return (c["build_evaluations"] + c["survivor_evaluations"] + members * c["plain_evaluations"]) / 64.0 / c["point_evaluations"]


def test_lists_exist_and_are_used(engine):
    """1000 spheres, perspective, 320 x 240, counted by the kernels themselves. The quarter is a condition, not a
    measurement: tools/ray_cull_model.py, the same rule in float64, meets it (tests/test_render_cull_cpu.py)."""
    geo = SCENES["union1000"]()
    cam = ref.cameras()["perspective"]
    with mode(_engine.MODE_NOCULL):
        want = render.render(geo, cam, W, H, 0.0, T_MAX, MAX_STEPS)
    with statistics() as st, mode(_engine.MODE_SPECIALIZED):
        got = render.render(geo, cam, W, H, 0.0, T_MAX, MAX_STEPS)
        image = st.read()
        o, d, eps, cone = _camera_rays()
        perm = np.random.default_rng(3).permutation(o.shape[1])
        render.cast(geo, o[:, perm], d[:, perm], 0.0, T_MAX, eps, cone, MAX_STEPS, normals=True)
        permuted = st.read()
        # one 8 x 8 tile from the centre of that image: the same pixel size, 8 pixels across
        narrow = render.Camera(ref.EYE, (0, 0, 0), (0, 0, 1), float(np.degrees(2.0 * np.arctan(np.tan(np.radians(20.0)) * 8 / H))))
        render.render(geo, narrow, 8, 8, 0.0, T_MAX, MAX_STEPS)
        tile = st.read()
    same(want, got)                                              # (the statistics build computes the same image)
    ratio = members_per_evaluation(image, 1000)
    print("image:", image, "members per evaluation %.1f of 1000" % ratio)
    print("permuted cast:", permuted, "members per evaluation %.1f" % members_per_evaluation(permuted, 1000))
    print("one tile:", tile)
    assert image["builds"] > 0
    assert image["splits"] > 0
    assert permuted["plain_evaluations"] > 0 and tile["plain_evaluations"] == 0 and tile["builds"] > 0
    assert ratio < 250.0


@pytest.mark.parametrize("members", [300, 16384])
def test_members_per_evaluation_is_reported(engine, members):
    """The measured ratios DESIGN §4.14 records (no bound of their own beyond: fewer than every member)."""
    geo = SCENES["union%d" % members]()
    w, h = (160, 120) if members == 16384 else (W, H)
    with statistics() as st, mode(_engine.MODE_SPECIALIZED):
        render.render(geo, ref.cameras()["perspective"], w, h, 0.0, T_MAX, MAX_STEPS)
        c = st.read()
    print("%d members %dx%d:" % (members, w, h), c, "members per evaluation %.1f" % members_per_evaluation(c, members))
    assert c["builds"] > 0 and members_per_evaluation(c, members) < members


def test_soundness_and_parity_against_the_float64_tracer(engine):
    from test_gpu_render import disagreement
    geo = SCENES["union1000"]()
    L = float(lower_geometry(geo).lipschitz)
    w, h = 160, 120
    for vname, cam in ref.cameras().items():
        with mode(_engine.MODE_SPECIALIZED):
            img = render.render(geo, cam, w, h, 0.0, T_MAX, MAX_STEPS, normals=False)
        o, d = cam.rays(w, h)
        eps, cone = (float(f32(x)) for x in cam.footprint(w, h))
        t_ref, s_ref, _ = ref.trace(ref.oracle_field(geo), o, d, 0.0, T_MAX, eps, cone, L, MAX_STEPS)
        bad, worst = disagreement(img.t.ravel(), img.status.ravel(), t_ref, s_ref, eps, cone, L)
        print("union1000/%s: %.4f %% of the rays disagree (%d), largest |dt| L / thr %.3f" % (vname, 100 * bad.mean(), bad.sum(), worst))
        assert bad.mean() <= CAP, vname
        # soundness as test_gpu_render.py checks it, on the same rays as fp32 arrays: hits within thr + slack of the surface,
        # and no ray passes through it (16 samples per traversed ray)
        o32, d32 = f32(o), f32(d)
        with mode(_engine.MODE_SPECIALIZED):
            hits = render.cast(geo, o32, d32, 0.0, T_MAX, eps, cone, MAX_STEPS)
        o64, d64, t = o32.astype(np.float64), d32.astype(np.float64), hits.t.astype(np.float64)
        hit = hits.status == render.HIT
        thr = ref.threshold(t, eps, cone)
        f, slack = ref.slack(geo, o64[:, hit] + t[hit] * d64[:, hit], L)
        assert hit.sum() > 1000 and np.all(f - (thr[hit] + slack) <= 0.0), vname
        end = np.where(hits.status == render.MISS, T_MAX, t)
        for s in np.linspace(0.0, 1.0, 16):
            f, slack = ref.slack(geo, o64 + (s * end) * d64, L)
            assert np.all(f > -slack), vname
