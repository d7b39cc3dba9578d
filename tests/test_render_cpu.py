"""aegolius_amd.render without a GPU: the reference tracer against closed forms, camera rays, Lipschitz bounds of the
lowering, refusals, the ray flavour's build, shading and the image writers."""
import numpy as np
import pytest

import aegolius_amd.cores as ns
import render_reference as ref
from aegolius_amd import render, workloads
from aegolius_amd._lower import lower_geometry
from aegolius_amd.autodiff import UnsupportedOpError


def _rot(angle, axis):
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K.dot(K)


def closed_form_cases():
    """name -> (float64 field, closed form (o, d, t_min, t_max) -> (t_exact, cos), geometry builder)."""
    c = np.array([0.2, -0.1, 0.15])
    R = _rot(0.7, (1, 2, 0.5))
    bc = np.array([-0.1, 0.2, 0.05])
    size = np.array([0.9, 0.6, 0.5])
    n = np.array([0.3, -0.2, 1.0])
    n = n / np.linalg.norm(n)

    def box_field(p):
        q = np.abs(R.T.dot(p - bc[:, None])) - 0.5 * size[:, None]
        return np.linalg.norm(np.maximum(q, 0.0), axis=0) + np.minimum(q.max(axis=0), 0.0)

    def sphere():
        o = ns.Sphere(0.5)
        o.move(c)
        return o

    def plane():
        return ns.OrientedPlane(n, -0.4)

    def box():
        o = ns.Box(*size)
        o.rotate(0.7, (1, 2, 0.5))
        o.move(bc)
        return o
    return {
        "sphere": (lambda p: np.linalg.norm(p - c[:, None], axis=0) - 0.5,
                   lambda o, d, a, b: ref.sphere_hit(o, d, c, 0.5, a, b), sphere),
        "plane": (lambda p: n.dot(p) + 0.4, lambda o, d, a, b: ref.halfspace_hit(o, d, n, -0.4, a, b), plane),
        "box": (box_field, lambda o, d, a, b: ref.box_hit(o, d, size, R, bc, a, b), box),
    }


def check_against_closed_form(field, closed, o, d, t, status, t_min, t_max, eps, cone, extra=0.0):
    """The bound of CPU test 1 for EVERY ray (`extra`: per-ray slack of an fp32 tracer, 0 for the reference)."""
    t_exact, cos = closed(o, d, t_min, t_max)
    thr = ref.threshold(t, eps, cone)
    exact_hit = np.isfinite(t_exact)
    assert not np.any(status == ref.LIMIT)
    # where the closed form hits: the tracer hits, before the surface and within thr / cos of it
    assert np.all(status[exact_hit] == ref.HIT)
    gap = (t_exact - t)[exact_hit]
    assert np.all(gap >= -np.broadcast_to(extra, t.shape)[exact_hit] / cos[exact_hit])
    assert np.all(gap <= (thr + extra)[exact_hit] / cos[exact_hit])
    # where it misses: a miss, or a hit within thr of the body (a grazing ray is a hit by the rule)
    grazing = ~exact_hit & (status == ref.HIT)
    assert np.all(field(o + t * d)[grazing] <= (thr + extra)[grazing])
    assert np.all((status == ref.MISS) | (status == ref.HIT))
    return int(exact_hit.sum()), int(grazing.sum())


# a ray that meets a plane at incidence cosine c closes the gap by the factor (1 - c) per step: the random rays below go
# down to c = 5e-4, about 2e4 steps; the limit is set far above so that no ray of these tests is cut short
CLOSED_FORM_STEPS = 200000


def sample_rays():
    """Camera rays plus rays that start inside, point away and graze."""
    rng = np.random.default_rng(11)
    cams = ref.cameras()
    o1, d1 = cams["perspective"].rays(64, 48)
    o2, d2 = cams["ortho_x"].rays(64, 48)
    d3 = rng.normal(size=(3, 2000))
    d3 /= np.linalg.norm(d3, axis=0)
    o3 = rng.uniform(-1.2, 1.2, (3, 2000))
    return np.concatenate([o1, o2, o3], axis=1), np.concatenate([d1, d2, d3], axis=1)


@pytest.mark.parametrize("name", ["sphere", "plane", "box"])
def test_reference_tracer_against_closed_forms(name):
    field, closed, _ = closed_form_cases()[name]
    o, d = sample_rays()
    for eps, cone in ((1e-3, 0.0), (0.0, 2e-3), (1e-5, 1e-3)):
        t, status, _ = ref.trace(field, o, d, 0.0, 8.0, eps, cone, 1.0, CLOSED_FORM_STEPS)
        hits, _ = check_against_closed_form(field, closed, o, d, t, status, 0.0, 8.0, eps, cone)
        assert hits > 500


@pytest.mark.parametrize("name", ["sphere", "plane", "box"])
def test_closed_form_fields_are_the_oracles(name):
    field, _, build = closed_form_cases()[name]
    p = np.random.default_rng(3).uniform(-2, 2, (3, 500))
    assert np.allclose(field(p), ref.oracle_field(build())(p), rtol=0, atol=1e-12)


def test_camera_rays():
    cam = render.Camera(ref.EYE, (0, 0, 0), (0, 0, 1), 40.0)
    W, H = 161, 121
    o, d = cam.rays(W, H)
    assert o.shape == d.shape == (3, W * H) and o.dtype == d.dtype == np.float64
    assert np.allclose(np.linalg.norm(d, axis=0), 1.0, rtol=0, atol=1e-15)
    assert np.all(o == np.asarray(ref.EYE)[:, None])
    fwd = -np.asarray(ref.EYE) / np.linalg.norm(ref.EYE)
    centre = (H // 2) * W + W // 2
    assert np.allclose(d[:, centre], fwd, rtol=0, atol=1e-15)
    # corners: tan of the half angles, reduced by half a pixel
    th = np.tan(np.radians(20.0))
    a, b = (1 - 1 / W) * th * W / H, (1 - 1 / H) * th
    right = np.cross(fwd, (0, 0, 1))
    right /= np.linalg.norm(right)
    up = np.cross(right, fwd)
    for idx, sa, sb in ((0, -1, 1), (W - 1, 1, 1), ((H - 1) * W, -1, -1), (H * W - 1, 1, -1)):
        want = fwd + sa * a * right + sb * b * up
        assert np.allclose(d[:, idx], want / np.linalg.norm(want), rtol=0, atol=1e-15)
    assert cam.footprint(W, H) == (0.0, th / H)
    rec = cam.record(W, H)
    assert rec.dtype == np.float32 and rec.shape == (12,)
    oc = render.Camera.orthographic((3, 0, 0), (0, 0, 0), (0, 0, 1), 2.4)
    o, d = oc.rays(160, 120)
    assert np.all(d == np.array([-1.0, 0, 0])[:, None])
    grid = o.reshape(3, 120, 160)
    assert np.allclose(np.diff(grid[2], axis=0), -2.4 / 120, rtol=0, atol=1e-15)      # rows go down
    assert np.allclose(np.linalg.norm(np.diff(grid, axis=2), axis=0), 2.4 / 120, rtol=0, atol=1e-15)
    assert oc.footprint(160, 120) == (0.5 * 2.4 / 120, 0.0)
    with pytest.raises(ValueError):
        render.Camera((0, 0, 1), (0, 0, 0), (0, 0, 1))


def test_lowered_lipschitz():
    L = lambda g: lower_geometry(g).lipschitz                # noqa: E731
    assert L(workloads.cfg1_sphere(ns)) == 1.0
    assert L(workloads.sphere_union(ns, count=200)) == 1.0
    assert abs(L(workloads.cfg2_tree(ns)) - 1.0) <= 1e-12
    assert abs(L(workloads.cfg5_tree(ns)) - 1.0) <= 1e-12
    assert abs(L(ref.onion_scaled()) - 1.0) <= 1e-12
    assert L(ns.CombineGeometry("SUM").combine(ns.Sphere(0.3), ns.Box(0.5, 0.4, 0.3))) == 2.0
    assert abs(L(ref.extruded()) - np.sqrt(2.0)) <= 1e-12
    s = np.tan(0.4)
    assert abs(L(ref.sheared()) - (s + np.sqrt(s * s + 4.0)) / 2.0) <= 1e-9
    assert abs(L(ref.sheared()) - 1.2335) <= 5e-5
    assert L(workloads.cfg3_chain(ns)) == np.inf
    assert L(ref.twisted()) == np.inf
    assert abs(ref.twisted_box_lipschitz() - 5.854) <= 5e-4


def test_lipschitz_is_not_part_of_the_program_key():
    low = lower_geometry(workloads.cfg2_tree(ns))
    key = low.key()
    low.lipschitz = 3.0
    assert low.key() == key


def test_refusals_need_no_gpu(built):
    o = np.zeros((3, 4))
    d = np.tile(np.array([[1.0], [0.0], [0.0]]), (1, 4))
    cam = ref.cameras()["perspective"]
    chain = workloads.cfg3_chain(ns)
    with pytest.raises(ValueError, match=r"instruction \d+ \(\w+, from .*\).*lipschitz="):
        render.cast(chain, o, d)
    with pytest.raises(ValueError, match=r"instruction \d+ \(\w+, from .*\).*lipschitz="):
        render.render(chain, cam, 16, 12)

    signed = ns.Circle(0.5)
    signed.signed((32, 32, 1))
    with pytest.raises(UnsupportedOpError, match="staged"):
        render.cast(signed, o, d)
    custom = ns.Sphere(0.5)
    custom.custom_post_process(lambda u, k: u * k, (2.0,))
    with pytest.raises(UnsupportedOpError, match="staged"):
        render.render(custom, cam, 16, 12)

    sphere = ns.Sphere(0.5)
    with pytest.raises(ValueError, match="t_max"):
        render.cast(sphere, o, d, t_min=1.0, t_max=0.5)
    with pytest.raises(ValueError, match="max_steps"):
        render.cast(sphere, o, d, max_steps=0)
    with pytest.raises(ValueError, match="unit vectors"):
        render.cast(sphere, o, 1.01 * d)
    with pytest.raises(ValueError, match="lipschitz"):
        render.cast(sphere, o, d, lipschitz=0.0)
    with pytest.raises(ValueError, match="shape"):
        render.cast(sphere, o[:2], d)
    with pytest.raises(ValueError, match="t_max"):
        render.render(sphere, cam, 16, 12, t_min=2.0, t_max=1.0)
    with pytest.raises(ValueError, match="max_steps"):
        render.render(sphere, cam, 16, 12, max_steps=0)


def test_native_argument_checks(built):
    """The C entries validate on the host and launch nothing (no GPU is touched before the checks)."""
    from aegolius_amd import _engine
    low = lower_geometry(ns.Sphere(0.5))
    prog = _engine.Program.from_lowered(low)
    L = built.lib()
    one = 4096                                                   # (never dereferenced: the calls fail first)
    def rays(t_min=0.0, t_max=1.0, inv=1.0, steps=8, eps=1e-3):
        return L.sdfk_trace_rays_device(prog.handle, one, 64, one, 64, 1, t_min, t_max, eps, 0.0, inv, steps, one, one, one,
                                        None, 0, None, built.MODE_INTERPRET)
    assert rays(t_min=1.0, t_max=0.5) == -1 and "t_max" in built.last_error()
    assert rays(steps=0) == -1 and "max_steps" in built.last_error()
    assert rays(inv=0.0) == -1 and "Lipschitz" in built.last_error()
    assert rays(inv=float("inf")) == -1
    assert rays(inv=float("nan")) == -1
    assert rays(eps=-1.0) == -1
    rec = np.zeros(12, dtype=np.float32)
    assert L.sdfk_trace_camera_device(prog.handle, built._ptr(rec), 8, 8, 0, 0.0, 1.0, 0.0, 0.0, 0.0, 8, one, one, one, None,
                                      0, None, built.MODE_INTERPRET) == -1
    assert L.sdfk_program_rays_check(prog.handle, None) == 0


def test_ray_flavour_builds_for_gfx950(built):
    from aegolius_amd import _engine
    fits = []
    for tree in (workloads.cfg2_tree(ns), _beyond_interpreter()):
        low = lower_geometry(tree)
        fits.append(low.fits_interpreter)
        prog = _engine.Program.from_lowered(low)
        size, _ = prog.compile_flavour(_engine.FLAVOUR_RAYS)
        assert size > 5000
        builds = _engine.jit_stats()[0]
        again, _ = prog.compile_flavour(_engine.FLAVOUR_RAYS)
        assert again == size and _engine.jit_stats()[0] == builds      # served from the cache: no hiprtc build ran
    assert fits == [True, False]
    with pytest.raises(_engine.SdfkError):
        prog.compile_flavour(_engine.FLAVOUR_RAYS | _engine.FLAVOUR_FLAGS)


def _beyond_interpreter():
    """A balanced tree of smooth unions deep enough to need more value registers than the interpreter has."""
    def level(depth, k):
        if depth == 0:
            o = ns.Sphere(0.2 + 0.01 * k)
            o.move((0.1 * k, -0.05 * k, 0.02 * k))
            return o
        return ns.CombineGeometry("SMOOTH_UNION2").combine_parametric(level(depth - 1, 2 * k), level(depth - 1, 2 * k + 1),
                                                                      parameters=0.1)
    return level(9, 0)


def synthetic_image():
    H, W = 6, 9
    status = np.zeros((H, W), dtype=np.uint8)
    status[1:5, 2:7] = render.HIT
    status[0, 0] = render.LIMIT
    normals = np.zeros((H, W, 3), dtype=np.float32)
    normals[status == render.HIT] = (0.0, 0.0, 1.0)
    normals[2, 3] = (1.0, 0.0, 0.0)
    depth = np.where(status == render.HIT, np.float32(2.0), np.float32(np.inf)).astype(np.float32)
    return render.Image(depth, status, np.zeros((H, W), dtype=np.int32), normals)


def _read_pnm(path):
    raw = open(path, "rb").read()
    magic, dims, maxval, body = raw.split(b"\n", 3)
    w, h = (int(x) for x in dims.split())
    return magic, w, h, int(maxval), np.frombuffer(body, dtype=np.uint8)


def test_shade_and_writers(tmp_path):
    img = synthetic_image()
    g = img.shade(light=(0, 0, 1), ambient=0.2)
    assert g.dtype == np.uint8 and g.shape == (6, 9)
    assert g[3, 4] == 255 and g[2, 3] == 51 and g[0, 0] == 0 and g[5, 8] == 0       # lit, grazing = ambient, not hit
    f = img.shade(light=(0, 0, 1), ambient=0.2, dtype=np.float32)
    assert f.dtype == np.float32 and f.min() >= 0.0 and f.max() <= 1.0 and abs(f[2, 3] - 0.2) < 1e-7
    rgb = img.shade(light=(0, 0, 2), ambient=0.0, color=(1.0, 0.5, 0.0))
    assert rgb.shape == (6, 9, 3) and tuple(rgb[3, 4]) == (255, 128, 0) and tuple(rgb[0, 0]) == (0, 0, 0)
    img.save_pgm(tmp_path / "a.pgm", g)
    magic, w, h, maxval, body = _read_pnm(tmp_path / "a.pgm")
    assert (magic, w, h, maxval) == (b"P5", 9, 6, 255) and np.array_equal(body.reshape(6, 9), g)
    img.save_ppm(tmp_path / "a.ppm", rgb)
    magic, w, h, maxval, body = _read_pnm(tmp_path / "a.ppm")
    assert (magic, w, h, maxval) == (b"P6", 9, 6, 255) and np.array_equal(body.reshape(6, 9, 3), rgb)
    img.save_pgm(tmp_path / "b.pgm")                           # defaults: shade()
    assert _read_pnm(tmp_path / "b.pgm")[4].size == 54
    img.save_npz(tmp_path / "a.npz")
    back = np.load(tmp_path / "a.npz")
    assert np.array_equal(back["status"], img.status) and np.array_equal(back["depth"], img.depth)
    with pytest.raises(ValueError):
        img.save_ppm(tmp_path / "c.ppm", g)
    with pytest.raises(ValueError):
        render.Image(img.depth, img.status, img.steps, None).shade()


def test_stencil_width_is_the_kernels_arithmetic():
    t = np.array([0.5, 1.0, 3.0], dtype=np.float32)
    p = np.array([[0.1, -70.0, 0.0], [0.2, 3.0, 0.0], [-0.3, 1.0, 0.0]], dtype=np.float32)
    h = render.stencil_width(t, p, 1e-4, 1e-3)
    assert h.dtype == np.float32
    want = [np.float32(1e-3) * np.float32(0.5), np.float32(2.0 ** -16) * np.float32(70.0), np.float32(1e-3) * np.float32(3.0)]
    assert np.array_equal(h, np.array(want, dtype=np.float32))
