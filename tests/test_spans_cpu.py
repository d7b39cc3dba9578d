"""aegolius_amd.render.spans / thickness without a GPU: the float64 span march against closed forms, option validation and
refusals, intervals / truncated / volume / the writers on synthetic arrays, the C entries' argument checks and the span
flavour's build."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import aegolius_amd.cores as ns
import render_reference as ref
import spans_reference as sref
from aegolius_amd import render, workloads
from aegolius_amd._lower import lower_geometry
from aegolius_amd.autodiff import UnsupportedOpError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. the reference against closed forms ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sphere", "shell", "box"])
def test_reference_spans_against_closed_forms(name):
    field, roots_of, _ = sref.bodies()[name]
    o, d = sref.sample_rays()
    assert o.shape == (3, 20000)
    roots, n_exact, chord_exact = sref.exact(field, roots_of, o, d, sref.T_MIN, sref.T_MAX)
    assert np.nanmax(roots) < 7.0 and (n_exact > 0).sum() > 3000
    if name == "shell":
        assert (n_exact == 4).sum() > 1000 and (n_exact == 3).sum() + (n_exact == 1).sum() > 100      # (starts inside too)
    for eps, cone in sref.OPTIONS:
        got = sref.trace_spans(field, o, d, sref.T_MIN, sref.T_MAX, eps, cone, 1.0, 200000, 8)
        assert np.all(got.status == sref.COMPLETE)
        thin, worst = sref.check_closed_form(got, roots, n_exact, chord_exact, eps, cone)
        print("%s eps %g cone %g: %.3f %% thin rays, largest crossing error / thr %.3f, evaluations per ray %.1f, at most %d"
              % (name, eps, cone, 100 * thin, worst, got.steps.mean(), got.steps.max()))
        assert thin <= sref.THIN_CAP
        # parity of a ray that was followed to the end: inside at t_max = inside0 xor (count odd)
        end = field(o + sref.T_MAX * d) <= 0.0
        assert np.array_equal(end, got.inside0 ^ (got.count % 2 == 1))


@pytest.mark.parametrize("name", ["sphere", "shell", "box"])
def test_closed_form_fields_are_the_oracles(name):
    field, _, build = sref.bodies()[name]
    p = np.random.default_rng(3).uniform(-2, 2, (3, 500))
    assert np.allclose(field(p), ref.oracle_field(build())(p), rtol=0, atol=1e-12)


def test_reference_limit_and_truncation():
    field, roots_of, _ = sref.bodies()["shell"]
    o = np.array([[3.0, 3.0, 0.7], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]])
    d = np.array([[-1.0, 1.0, -1.0], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]])
    got = sref.trace_spans(field, o, d, 0.0, 8.0, 1e-3, 0.0, 1.0, 4096, 2)
    assert list(got.count) == [4, 0, 3] and list(got.inside0) == [False, False, True]
    assert abs(got.chord[0] - 0.5) <= 4e-3 and got.chord[1] == 0.0 and abs(got.chord[2] - (0.075 + 0.25)) <= 3e-3
    assert np.all(np.isfinite(got.crossings[:, 0])) and np.all(np.isnan(got.crossings[:, 1]))
    assert abs(got.crossings[0, 0] - 2.125) <= 1e-3 and abs(got.crossings[1, 0] - 2.375) <= 1e-3
    one = sref.trace_spans(field, o, d, 0.0, 8.0, 1e-3, 0.0, 1.0, 1, 2)
    assert np.all(one.status == sref.LIMIT) and list(one.steps) == [1, 1, 1] and list(one.count) == [0, 0, 0]
    assert one.chord[2] == 0.0 and np.all(one.t_last == 0.0)
    stuck = sref.trace_spans(lambda p: np.zeros(p.shape[1]) + 1.0, o, d, 1e20, 2e20, 1e-3, 0.0, 1.0, 16, 0)
    assert np.all(stuck.status == sref.LIMIT) and list(stuck.steps) == [1, 1, 1]             # no progress: never loops


# ---- 2. Python behaviour ------------------------------------------------------------------------------------------------------
def test_option_validation(built):
    o = np.zeros((3, 4))
    d = np.tile(np.array([[1.0], [0.0], [0.0]]), (1, 4))
    cam = ref.cameras()["perspective"]
    sphere = ns.Sphere(0.5)
    with pytest.raises(ValueError, match="t_max"):
        render.spans(sphere, o, d, t_min=1.0, t_max=0.5)
    with pytest.raises(ValueError, match="max_steps"):
        render.spans(sphere, o, d, max_steps=0)
    with pytest.raises(ValueError, match="not negative"):
        render.spans(sphere, o, d, cone=-1.0)
    with pytest.raises(ValueError, match="advances t in float32"):
        render.spans(sphere, o, d, eps=0.0)
    with pytest.raises(ValueError, match="advances t in float32"):
        render.spans(sphere, o, d, t_max=100.0, eps=0.99 * 100.0 * 2.0 ** -20)
    with pytest.raises(ValueError, match="advances t in float32"):
        render.spans(sphere, o, d, t_min=-200.0, t_max=100.0, eps=1e-4)
    with pytest.raises(ValueError, match="advances t in float32"):
        render.thickness(sphere, cam, 16, 12, eps=0.0)
    with pytest.raises(ValueError, match="max_crossings"):
        render.spans(sphere, o, d, max_crossings=33)
    with pytest.raises(ValueError, match="max_crossings"):
        render.thickness(sphere, cam, 16, 12, max_crossings=-1)
    with pytest.raises(ValueError, match="t_max"):
        render.thickness(sphere, cam, 16, 12, t_min=2.0, t_max=1.0)
    with pytest.raises(ValueError, match="image sizes"):
        render.thickness(sphere, cam, 0, 12)
    assert render._span_options(0.0, 100.0, 100.0 * 2.0 ** -20, 0.0, 5, 32)[2:] == (100.0 * 2.0 ** -20, 0.0, 5, 32)
    assert (render.COMPLETE, render.LIMIT, render.MAX_CROSSINGS) == (0, 2, 32)


def test_refusals_need_no_gpu(built):
    o = np.zeros((3, 4))
    d = np.tile(np.array([[1.0], [0.0], [0.0]]), (1, 4))
    cam = ref.cameras()["perspective"]
    chain = workloads.cfg3_chain(ns)
    with pytest.raises(ValueError, match=r"instruction \d+ \(\w+, from .*\).*lipschitz="):
        render.spans(chain, o, d)
    with pytest.raises(ValueError, match=r"instruction \d+ \(\w+, from .*\).*lipschitz="):
        render.thickness(chain, cam, 16, 12)
    signed = ns.Circle(0.5)
    signed.signed((32, 32, 1))
    with pytest.raises(UnsupportedOpError, match="staged"):
        render.spans(signed, o, d)
    custom = ns.Sphere(0.5)
    custom.custom_post_process(lambda u, k: u * k, (2.0,))
    with pytest.raises(UnsupportedOpError, match="staged"):
        render.thickness(custom, cam, 16, 12)
    sphere = ns.Sphere(0.5)
    with pytest.raises(ValueError, match="unit vectors"):
        render.spans(sphere, o, 1.01 * d)
    with pytest.raises(ValueError, match="lipschitz"):
        render.spans(sphere, o, d, lipschitz=0.0)
    with pytest.raises(ValueError, match="lipschitz"):
        render.thickness(sphere, cam, 16, 12, lipschitz=float("inf"))
    with pytest.raises(ValueError, match="shape"):
        render.spans(sphere, o[:2], d)
    with pytest.raises(ValueError, match="shape"):
        render.spans(sphere, o, d.T)
    with pytest.raises(ValueError, match="origins for"):
        render.spans(sphere, o, d[:, :3])


def synthetic_spans():
    """Four rays, K = 2: outside-in-out; starts inside and leaves; truncated (4 crossings); inside at a LIMIT end."""
    nan = np.nan
    crossings = np.array([[1.0, 0.5, 1.0, 2.0], [1.5, nan, 1.25, nan]], dtype=np.float32)
    count = np.array([2, 1, 4, 1], dtype=np.int32)
    status = np.array([0, 0 | 4, 0, 2], dtype=np.uint8)
    chord = np.array([0.5, 0.25, 0.75, 1.5], dtype=np.float32)
    return render.RaySpans(chord, count, status, np.array([9, 8, 30, 5], dtype=np.int32), crossings, 0.25, 8.0, 2)


def test_intervals_and_truncated():
    s = synthetic_spans()
    assert list(s.status) == [0, 0, 0, 2] and list(s.inside0) == [False, True, False, False]
    assert list(s.truncated) == [False, False, True, False]
    assert s.intervals(0) == [(1.0, 1.5)]
    assert s.intervals(1) == [(0.25, 0.5)]                       # opens at t_min
    with pytest.raises(ValueError, match="max_crossings"):
        s.intervals(2)
    assert s.intervals(3) == [(2.0, 3.5)]                        # LIMIT: closes at the last evaluated t = t_enter + chord
    # a ray that is still inside at t_max closes there; K = 0 keeps no crossings at all
    t = render.RaySpans(np.array([7.0], dtype=np.float32), np.array([1], dtype=np.int32), np.array([0], dtype=np.uint8),
                        np.array([40], dtype=np.int32), np.array([[1.0]], dtype=np.float32), 0.0, 8.0, 1)
    assert t.intervals(0) == [(1.0, 8.0)]
    z = render.RaySpans(np.array([8.0], dtype=np.float32), np.array([0], dtype=np.int32), np.array([4], dtype=np.uint8),
                        np.array([40], dtype=np.int32), np.empty((0, 1), dtype=np.float32), 0.0, 8.0, 0)
    assert z.intervals(0) == [(0.0, 8.0)] and not z.truncated[0]
    assert "4 rays" in repr(s)
    # the reference's own intervals agree with its chord
    field, _, _ = sref.bodies()["shell"]
    o, d = sref.sample_rays(300)
    got = sref.trace_spans(field, o, d, 0.0, 8.0, 1e-3, 0.0, 1.0, 60, 8)      # (some rays reach the limit of 60)
    assert (got.status == sref.LIMIT).sum() > 5 and (got.status == sref.COMPLETE).sum() > 100
    for i in range(300):
        iv = sref.intervals(got.crossings[:, i], got.count[i], got.inside0[i], got.status[i], 0.0, 8.0, got.t_last[i])
        assert abs(sum(b - a for a, b in iv) - got.chord[i]) <= 1e-12
        mine = render._intervals(got.crossings[:, i], got.count[i], got.inside0[i], got.status[i], got.chord[i], 0.0, 8.0)
        assert len(mine) == len(iv) and np.allclose(np.asarray(mine), np.asarray(iv), rtol=0, atol=1e-12)


def _read_pnm(path):
    raw = open(path, "rb").read()
    magic, dims, maxval, body = raw.split(b"\n", 3)
    w, h = (int(x) for x in dims.split())
    return magic, w, h, int(maxval), np.frombuffer(body, dtype=np.uint8)


def test_volume_and_writers(tmp_path):
    H, W = 6, 9
    chord = np.zeros((H, W), dtype=np.float32)
    chord[1:5, 2:7] = 0.5
    chord[2, 3] = 1.0
    count = np.where(chord > 0, 2, 0).astype(np.int32)
    status = np.zeros((H, W), dtype=np.uint8)
    status[0, 0] = 2 | 4
    cam = render.Camera.orthographic((3, 0, 0), (0, 0, 0), (0, 0, 1), height=1.2)
    cross = np.full((2, H, W), np.nan, dtype=np.float32)
    img = render.ThicknessImage(chord, count, status, np.ones((H, W), dtype=np.int32), cross, camera=cam, eps=0.1)
    assert img.status[0, 0] == render.LIMIT and img.inside0[0, 0] and not img.inside0[1, 1]
    assert abs(img.volume() - (19 * 0.5 + 1.0) * 0.2 * 0.2) <= 1e-12              # pixels of 1.2 / 6 = 0.2 a side
    with pytest.raises(ValueError, match="orthographic"):
        render.ThicknessImage(chord, count, status, count, None, camera=ref.cameras()["perspective"]).volume()
    with pytest.raises(ValueError, match="orthographic"):
        render.ThicknessImage(chord, count, status, count, None).volume()
    img.save_pgm(tmp_path / "x.pgm")
    magic, w, h, maxval, body = _read_pnm(tmp_path / "x.pgm")
    px = body.reshape(H, W)
    assert (magic, w, h, maxval) == (b"P5", W, H, 255) and px[2, 3] == 255 and px[1, 2] == 128 and px[0, 0] == 0
    img.save_pgm(tmp_path / "y.pgm", scale=2.0)
    assert _read_pnm(tmp_path / "y.pgm")[4].reshape(H, W)[2, 3] == 128
    img.save_npz(tmp_path / "x.npz")
    back = np.load(tmp_path / "x.npz")
    assert np.array_equal(back["chord"], chord) and np.array_equal(back["count"], count)
    assert np.array_equal(back["status"], img.status) and np.array_equal(back["inside0"], img.inside0)
    assert back["crossings"].shape == (2, H, W)
    render.ThicknessImage(chord * 0, count, status, count, None, camera=cam).save_pgm(tmp_path / "z.pgm")
    assert not _read_pnm(tmp_path / "z.pgm")[4].any()
    assert "9 x 6" in repr(img)


# ---- 3. native -----------------------------------------------------------------------------------------------------------------
def test_native_argument_checks(built):
    """The C entries validate on the host and launch nothing (no GPU is touched before the checks)."""
    with open(os.path.join(ROOT, "include", "sdfk.h")) as f:
        header = f.read()
    assert "#define SDFK_FLAVOUR_SPANS 12" in header and built.FLAVOUR_SPANS == 12
    assert "int sdfk_span_rays_device(" in header and "int sdfk_span_camera_device(" in header
    prog = built.Program.from_lowered(lower_geometry(ns.Sphere(0.5)))
    L = built.lib()
    one = 4096                                                   # (never dereferenced: the calls fail first)

    def rays(n=1, t_min=0.0, t_max=1.0, inv=1.0, steps=8, eps=1e-3, chord=one, count=one, status=one, nsteps=one, cross=one,
             stride=64, k=4):
        return L.sdfk_span_rays_device(prog.handle, one, 64, one, 64, n, t_min, t_max, eps, 0.0, inv, steps, chord, count, status,
                                       nsteps, cross, stride, k, None, built.MODE_INTERPRET)
    for kw in (dict(chord=None), dict(count=None), dict(status=None), dict(nsteps=None)):
        assert rays(**kw) == -1 and "null output" in built.last_error()
    assert rays(k=-1) == -1 and "max_crossings" in built.last_error()
    assert rays(k=33) == -1 and "max_crossings" in built.last_error()
    assert rays(steps=0) == -1 and "max_steps" in built.last_error()
    assert rays(n=-1) == -1 and "negative" in built.last_error()
    assert rays(n=3, stride=2) == -1 and "stride" in built.last_error()
    assert rays(t_min=1.0, t_max=0.5) == -1 and "t_max" in built.last_error()
    assert rays(inv=0.0) == -1 and rays(inv=float("nan")) == -1 and rays(eps=-1.0) == -1
    assert rays(n=0) == 0                                        # nothing to do is not an error, and launches nothing
    rec = np.zeros(12, dtype=np.float32)

    def cam(w=8, h=8, steps=8, k=4, stride=64, chord=one, record=rec):
        return L.sdfk_span_camera_device(prog.handle, None if record is None else built._ptr(record), w, h, 0, 0.0, 1.0, 1e-3,
                                         0.0, 1.0, steps, chord, one, one, one, one, stride, k, None, built.MODE_INTERPRET)
    assert cam(chord=None) == -1 and "null output" in built.last_error()
    assert cam(k=40) == -1 and cam(steps=0) == -1 and cam(stride=63) == -1 and cam(w=-1) == -1 and cam(record=None) == -1
    assert cam(record=np.full(12, np.nan, dtype=np.float32)) == -1 and "finite" in built.last_error()
    assert cam(w=0) == 0


_SCRIPT = """
import json, sys
sys.path.insert(0, {root!r})
import aegolius_amd.cores as ns
from aegolius_amd import _engine, workloads
from aegolius_amd._lower import lower_geometry
geo = workloads.sphere_union(ns, count=64) if {chain} else workloads.cfg2_tree(ns)
prog = _engine.Program.from_lowered(lower_geometry(geo))
size, seconds = prog.compile_flavour(_engine.FLAVOUR_SPANS)
builds = _engine.jit_stats()[0]
again, _ = prog.compile_flavour(_engine.FLAVOUR_SPANS)
assert again == size and _engine.jit_stats()[0] == builds
try:
    prog.compile_flavour(_engine.FLAVOUR_SPANS | _engine.FLAVOUR_FLAGS)
    refused = False
except _engine.SdfkError:
    refused = True
print(json.dumps(dict(size=size, chain_members=prog.chain_members, refused=refused)))
"""
KERNELS = [b"sdfk_spec_spans", b"sdfk_spec_spancam", b"sdfk_spec_spans_cull", b"sdfk_spec_spancam_cull"]


@pytest.mark.parametrize("chain", [False, True])
def test_span_flavour_builds_for_gfx950(built, tmp_path, chain):
    """cfg2 exports the plain pair; a 64-member sphere union (chain mode, the culling threshold) the `_cull` pair as well.
    The names are read from the code object compile_flavour leaves in the on-disk cache, as the ray flavour's test does."""
    import json
    env = dict(os.environ, SDFK_CACHE_DIR=str(tmp_path))
    res = subprocess.run([sys.executable, "-c", _SCRIPT.format(root=ROOT, chain=chain)], env=env, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    info = json.loads(res.stdout.strip().splitlines()[-1])
    assert info["size"] > 5000 and info["refused"]
    assert info["chain_members"] == (64 if chain else 0)
    files = list(tmp_path.iterdir())
    assert len(files) == 1
    blob = files[0].read_bytes()
    names = [k for k in KERNELS if k + b"\0" in blob]
    assert names == (KERNELS if chain else KERNELS[:2])
    # the ray kernels are not in this module, nor the span kernels in the ray flavour's
    assert b"sdfk_spec_rays\0" not in blob and b"sdfk_spec_raycam\0" not in blob

