"""aegolius_amd.render.visibility / ambient_occlusion / illuminate without a GPU: the float64 reference against closed
forms, the argument checks, shading with shadow and occlusion on the host, the secondary flavour's build, and the
conditioning of the scene views of tests/test_gpu_secondary.py by the reference alone."""
import os
import subprocess
import sys

import numpy as np
import pytest

import aegolius_amd.cores as ns
import render_reference as ref
import secondary_reference as sec
import spans_reference as sref
from aegolius_amd import render
from aegolius_amd._lower import lower_geometry
from test_render_cpu import CLOSED_FORM_STEPS, synthetic_image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAP = 0.005                    # the cap of tests/test_gpu_render.py (a GPU module: restated, not imported)
CENTRE, RADIUS = np.array([0.2, -0.1, 0.15]), 0.5


# ---- 1. the reference against closed forms ------------------------------------------------------------------------------------
def test_hard_visibility_past_a_sphere_is_sphere_hit():
    """20,000 rays, three thresholds: blocked exactly where the segment meets the sphere, clear where it stays more than thr
    away; the rays that miss the sphere by less than thr are blocked or clear, and few."""
    o, d = sref.sample_rays()

    def field(p):
        return np.linalg.norm(p - CENTRE[:, None], axis=0) - RADIUS
    for eps in (1e-2, 1e-3, 1e-4):
        vis, status, steps, _ = sec.trace_visibility(field, o, d, sref.T_MIN, sref.T_MAX, eps, 0.0, 1.0, CLOSED_FORM_STEPS, 0.0)
        want, band = sec.sphere_visibility(o, d, CENTRE, RADIUS, sref.T_MIN, sref.T_MAX, eps)
        assert band.mean() <= sref.THIN_CAP
        assert not np.any(status == sec.LIMIT) and np.all((vis == 0.0) | (vis == 1.0))
        assert np.array_equal(vis[~band], want[~band])
        assert np.array_equal(vis == 0.0, status == sec.HIT)
        assert (want == 0.0).sum() > 4000 and (want == 1.0).sum() > 4000
        # the same march as the first-hit reference
        t, s, n = ref.trace(field, o, d, sref.T_MIN, sref.T_MAX, eps, 0.0, 1.0, CLOSED_FORM_STEPS)
        assert np.array_equal(s, status) and np.array_equal(n, steps)
        # a soft march takes the same steps, is blocked on the same rays and never sees more
        soft, s8, n8, _ = sec.trace_visibility(field, o, d, sref.T_MIN, sref.T_MAX, eps, 0.0, 1.0, CLOSED_FORM_STEPS, 8.0)
        assert np.array_equal(s8, status) and np.array_equal(n8, steps) and np.all(soft <= vis) and np.all(soft >= 0.0)
        assert ((soft > 0.0) & (soft < 1.0)).sum() > 500


def test_limits_end_the_ray():
    def field(p):
        return np.linalg.norm(p - CENTRE[:, None], axis=0) - RADIUS
    o, d = sref.sample_rays(3000)
    t_hit, _ = ref.sphere_hit(o, d, CENTRE, RADIUS, 0.0, 8.0)
    far = np.isfinite(t_hit) & (t_hit > 0.5)
    limits = np.where(far, t_hit - 0.25, 8.0)
    vis, status, _, _ = sec.trace_visibility(field, o, d, 0.0, 8.0, 1e-3, 0.0, 1.0, CLOSED_FORM_STEPS, 0.0, limits)
    assert far.sum() > 500 and np.all(vis[far] == 1.0) and np.all(status[far] == sec.MISS)
    vis, _, _, _ = sec.trace_visibility(field, o, d, 0.0, 8.0, 1e-3, 0.0, 1.0, CLOSED_FORM_STEPS, 0.0)
    assert np.all(vis[far] == 0.0)


def test_occlusion_closed_forms():
    rng = np.random.default_rng(4)
    p = np.concatenate([rng.uniform(-2, 2, (2, 100)), np.zeros((1, 100))])
    n = np.repeat(np.array([[0.0], [0.0], [1.0]]), 100, axis=1)
    for samples in (1, 5, 16):
        ao = sec.occlusion(lambda q: q[2], p, n, 0.3, samples, 1.0, 1.0)
        assert np.all(ao == 1.0)                               # a half-space: f = h at every sample, exactly
    for a, radius, samples, strength in ((0.05, 0.2, 5, 1.0), (0.1, 0.4, 16, 2.0), (0.3, 0.2, 5, 1.0), (0.01, 0.5, 1, 1.0)):
        ao = sec.occlusion(lambda q: np.minimum(q[2], a - q[0]), np.zeros((3, 1)), n[:, :1], radius, samples, strength, 1.0)
        want = sec.floor_and_wall_ao(a, radius, samples, strength)
        assert abs(ao[0] - want) <= 1e-15 and (want < 1.0) == (a < radius)
    # the closed-form fields are the oracle's
    q = rng.uniform(-1, 1, (3, 500))
    assert np.allclose(ref.oracle_field(sec.floor_and_wall(0.05))(q), np.minimum(q[2], 0.05 - q[0]), rtol=0, atol=1e-12)
    assert np.allclose(ref.oracle_field(ns.OrientedPlane((0.0, 0.0, 1.0), 0.0))(q), q[2], rtol=0, atol=1e-12)


# ---- 2. argument checks, before anything asks for the GPU ------------------------------------------------------------------------
def test_argument_checks_need_no_gpu(built):
    sphere = ns.Sphere(0.5)
    o = np.zeros((3, 4))
    d = np.tile(np.array([[1.0], [0.0], [0.0]]), (1, 4))
    with pytest.raises(ValueError, match="t_min"):
        render.visibility(sphere, o, d, t_min=-0.1)
    with pytest.raises(ValueError, match="unit vectors"):
        render.visibility(sphere, o, 1.01 * d)
    with pytest.raises(ValueError, match="limits"):
        render.visibility(sphere, o, d, limits=np.ones(3))
    with pytest.raises(ValueError, match="limits"):
        render.visibility(sphere, o, d, limits=np.ones((4, 1)))
    with pytest.raises(ValueError, match="softness"):
        render.visibility(sphere, o, d, softness=-1.0)
    with pytest.raises(ValueError, match="t_max"):
        render.visibility(sphere, o, d, t_min=1.0, t_max=0.5)
    with pytest.raises(ValueError, match="lipschitz"):
        render.visibility(sphere, o, d, lipschitz=0.0)
    for bad in (0, 17):
        with pytest.raises(ValueError, match="samples"):
            render.ambient_occlusion(sphere, o, d, 0.2, samples=bad)
    with pytest.raises(ValueError, match="unit vectors"):
        render.ambient_occlusion(sphere, o, 0.9 * d, 0.2)
    with pytest.raises(ValueError, match="radius"):
        render.ambient_occlusion(sphere, o, d, 0.0)
    with pytest.raises(ValueError, match="strength"):
        render.ambient_occlusion(sphere, o, d, 0.2, strength=-1.0)
    with pytest.raises(ValueError, match="normals"):
        render.illuminate(sphere, render.Image(None, np.zeros((2, 2), dtype=np.uint8), None, None), render.Light.point((0, 0, 3)))
    with pytest.raises(TypeError, match="Light"):
        render.illuminate(sphere, synthetic_image(), (0, 0, 1))
    with pytest.raises(ValueError):
        render.Light.directional((0, 0, 0))
    with pytest.raises(ValueError):
        render.Light()
    d_, dist = render.Light.point((0.0, 0.0, 2.0)).rays(np.array([[0.0, 0.0], [0.0, 0.0], [0.0, 2.0]]))
    assert np.array_equal(d_, [[0.0, 0.0], [0.0, 0.0], [1.0, 0.0]]) and np.array_equal(dist, [2.0, 0.0])
    d_, dist = render.Light.directional((0, 0, 2)).rays(np.zeros((3, 2)))
    assert dist is None and np.array_equal(d_, [[0.0, 0.0], [0.0, 0.0], [1.0, 1.0]])


def test_native_argument_checks(built):
    """The C entries are declared, bound and exported, validate on the host and launch nothing."""
    with open(os.path.join(ROOT, "include", "sdfk.h")) as f:
        header = f.read()
    assert "#define SDFK_FLAVOUR_SECONDARY 13" in header and built.FLAVOUR_SECONDARY == 13
    for name in ("sdfk_visibility_rays_device", "sdfk_occlusion_rays_device"):
        assert "int %s(" % name in header and name in built.SIGNATURES and hasattr(built.lib(), name)
    prog = built.Program.from_lowered(lower_geometry(ns.Sphere(0.5)))
    L = built.lib()
    one = 4096                                                   # (never dereferenced: the calls fail first)

    def vis(n=1, t_min=0.0, t_max=1.0, inv=1.0, steps=8, eps=1e-3, k=0.0, out=one, stride=64):
        return L.sdfk_visibility_rays_device(prog.handle, one, stride, one, 64, n, t_min, t_max, eps, 0.0, inv, steps, k, None, out,
                                             one, one, None, built.MODE_INTERPRET)
    assert vis(t_min=-1.0) == -1 and "sdfk_visibility_rays_device: t_min" in built.last_error()
    assert vis(k=-1.0) == -1 and "sdfk_visibility_rays_device: softness" in built.last_error()
    assert vis(k=float("inf")) == -1 and vis(k=float("nan")) == -1
    assert vis(out=None) == -1 and "null output" in built.last_error()
    assert vis(steps=0) == -1 and vis(inv=0.0) == -1 and vis(eps=-1.0) == -1 and vis(t_min=1.0, t_max=0.5) == -1
    assert vis(n=-1) == -1 and vis(n=65, stride=64) == -1 and "stride" in built.last_error()
    assert vis(n=0) == 0                                         # nothing to do is not an error, and launches nothing

    def occ(n=1, radius=0.2, samples=5, strength=1.0, inv=1.0, out=one):
        return L.sdfk_occlusion_rays_device(prog.handle, one, 64, one, 64, n, radius, samples, strength, inv, out, None,
                                            built.MODE_INTERPRET)
    assert occ(radius=0.0) == -1 and "sdfk_occlusion_rays_device: radius" in built.last_error()
    assert occ(radius=float("inf")) == -1 and occ(radius=-1.0) == -1
    assert occ(samples=0) == -1 and "sdfk_occlusion_rays_device: samples" in built.last_error()
    assert occ(samples=17) == -1 and "samples" in built.last_error()
    assert occ(strength=-0.5) == -1 and "strength" in built.last_error()
    assert occ(strength=float("nan")) == -1 and occ(inv=0.0) == -1
    assert occ(out=None) == -1 and "null output" in built.last_error()
    assert occ(n=-1) == -1 and occ(n=0) == 0


_SCRIPT = """
import json, sys
sys.path.insert(0, {root!r})
import aegolius_amd.cores as ns
from aegolius_amd import _engine, workloads
from aegolius_amd._lower import lower_geometry
geo = workloads.sphere_union(ns, count=64) if {chain} else workloads.cfg2_tree(ns)
prog = _engine.Program.from_lowered(lower_geometry(geo))
size, seconds = prog.compile_flavour(_engine.FLAVOUR_SECONDARY)
try:
    prog.compile_flavour(_engine.FLAVOUR_SECONDARY | _engine.FLAVOUR_FLAGS)
    refused = False
except _engine.SdfkError:
    refused = True
print(json.dumps(dict(size=size, chain_members=prog.chain_members, refused=refused)))
"""
KERNELS = [b"sdfk_spec_visibility", b"sdfk_spec_occlusion", b"sdfk_spec_visibility_cull", b"sdfk_spec_occlusion_cull"]


@pytest.mark.parametrize("chain", [False, True])
def test_secondary_flavour_builds_for_gfx950(built, tmp_path, chain):
    """cfg2 exports the plain pair; a 64-member sphere union (chain mode, the culling threshold) the `_cull` pair as well.
    The names are read from the code object that compile_flavour leaves in the on-disk cache, as the span flavour's test does."""
    import json
    env = dict(os.environ, SDFK_CACHE_DIR=str(tmp_path))
    res = subprocess.run([sys.executable, "-c", _SCRIPT.format(root=ROOT, chain=chain)], env=env, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    info = json.loads(res.stdout.strip().splitlines()[-1])
    assert info["size"] > 5000 and info["refused"] and info["chain_members"] == (64 if chain else 0)
    files = list(tmp_path.iterdir())
    assert len(files) == 1
    blob = files[0].read_bytes()
    assert [k for k in KERNELS if k + b"\0" in blob] == (KERNELS if chain else KERNELS[:2])
    assert b"sdfk_spec_rays\0" not in blob and b"sdfk_spec_spans\0" not in blob


# ---- 3. shading on the host ------------------------------------------------------------------------------------------------------
def test_shade_with_shadow_and_occlusion(tmp_path):
    img = synthetic_image()
    hit = img.status == render.HIT
    for light, ambient in (((0, 0, 1), 0.2), ((1.0, 1.0, 2.0), 0.15), ((1, 0, 0.3), 0.0)):
        l = np.asarray(light, dtype=np.float64)
        lam = np.clip(np.asarray(img.normals, dtype=np.float64).dot(l / np.linalg.norm(l)), 0.0, 1.0)
        old = np.clip(np.where(hit, float(ambient) + (1.0 - float(ambient)) * lam, 0.0), 0.0, 1.0)     # the formula as it was
        assert np.array_equal(img.shade(light=light, ambient=ambient, shadow=None, occlusion=None),
                              np.rint(old * 255.0).astype(np.uint8))
        got = img.shade(light=light, ambient=ambient, dtype=np.float32)
        assert got.tobytes() == old.astype(np.float32).tobytes()
        rng = np.random.default_rng(9)
        shadow, ao = rng.uniform(0, 1, hit.shape).astype(np.float32), rng.uniform(0, 1, hit.shape).astype(np.float32)
        want = np.clip(np.where(hit, ambient * ao.astype(np.float64) + (1.0 - ambient) * lam * shadow.astype(np.float64), 0.0), 0, 1)
        got = img.shade(light=light, ambient=ambient, dtype=np.float32, shadow=shadow, occlusion=ao)
        assert np.array_equal(got, want.astype(np.float32))
        only = img.shade(light=light, ambient=ambient, dtype=np.float32, shadow=shadow)
        assert np.array_equal(only, np.clip(np.where(hit, ambient + (1.0 - ambient) * lam * shadow.astype(np.float64), 0.0), 0, 1)
                              .astype(np.float32))
        rgb = img.shade(light=light, ambient=ambient, color=(1.0, 0.5, 0.0), shadow=shadow, occlusion=ao)
        assert rgb.shape == hit.shape + (3,) and np.array_equal(rgb[..., 0], np.rint(want * 255.0).astype(np.uint8))
    with pytest.raises(ValueError, match="shape"):
        img.shade(shadow=np.ones((2, 2)))
    assert img.shadow is None and img.ao is None
    img.save_npz(tmp_path / "a.npz")
    assert "shadow" not in np.load(tmp_path / "a.npz") and "ao" not in np.load(tmp_path / "a.npz")
    img.shadow, img.ao = shadow, ao
    img.save_npz(tmp_path / "b.npz")
    back = np.load(tmp_path / "b.npz")
    assert np.array_equal(back["shadow"], shadow) and np.array_equal(back["ao"], ao) and np.array_equal(back["status"], img.status)


# ---- 4. the scene views of the GPU tests are well-conditioned --------------------------------------------------------------------
@pytest.mark.parametrize("name,vname", sec.scene_views())
def test_ill_conditioned_share_and_accumulation_floor(name, vname):
    """By the reference alone: the rays whose status changes under a shift of the oracle by its fp32 slack, that reach the
    step limit or whose derived tolerance of vis exceeds 0.05 are at most CAP of the view; and the float32 copy of the
    rule stays within the shift term plus a quarter of the floor A that the GPU test adds."""
    build, explicit, t_max, max_steps = ref.SCENES[name]
    geo = build()
    L = float(explicit if explicit is not None else lower_geometry(geo).lipschitz)
    _, _, o, d = sec.view_rays(vname)
    eps, t_max = float(np.float32(sec.SCENE_EPS)), float(np.float32(t_max))
    base, ill, tol = sec.conditioned_visibility(geo, L, o, d, 0.0, t_max, eps, 0.0, max_steps, sec.SCENE_SOFTNESS, floor=sec.A)
    share = float((ill | (tol > sec.TOL_CAP)).mean())
    low = sec.trace_visibility(ref.oracle_field(geo), o, d, 0.0, t_max, eps, 0.0, L, max_steps, sec.SCENE_SOFTNESS, dtype=np.float32)
    ok = ~ill & (low[1] == base[1])
    excess = float(max(0.0, (np.abs(low[0] - base[0]) - (tol - sec.A))[ok].max()))
    print("%s/%s: ill-conditioned share %.5f; %d rays in a penumbra, largest tolerance %.3e; float32 copy: %d statuses differ, "
          "largest excess over the shift term %.3e" % (name, vname, share, ((base[0] > 0) & (base[0] < 1)).sum(), tol[~ill].max(),
                                                        (low[1] != base[1]).sum(), excess))
    assert share <= CAP
    assert 4.0 * excess <= sec.A
    assert ((base[0] > 0) & (base[0] < 1)).sum() > 1000          # the views do have penumbrae to compare
