"""The culled ray kernels without a GPU: what the ray flavour of a long union and of a small tree exports, the statistics
entry of the C-ABI, and the survivor rule itself in float64 (tools/ray_cull_model.py): it never drops the minimiser, and
on the 1000-sphere scene it meets the condition tests/test_gpu_render_cull.py sets for the kernels' own counters."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = [b"sdfk_spec_rays", b"sdfk_spec_raycam", b"sdfk_spec_rays_cull", b"sdfk_spec_raycam_cull"]

_SCRIPT = """
import json, sys
sys.path.insert(0, {root!r})
import aegolius_amd.cores as ns
from aegolius_amd import _engine, workloads
from aegolius_amd._lower import lower_geometry
geo = workloads.sphere_union(ns, count=300) if {chain} else workloads.cfg2_tree(ns)
prog = _engine.Program.from_lowered(lower_geometry(geo))
size, seconds = prog.compile_flavour(_engine.FLAVOUR_RAYS)
print(json.dumps(dict(size=size, chain_members=prog.chain_members)))
"""


def model():
    spec = importlib.util.spec_from_file_location("ray_cull_model", os.path.join(ROOT, "tools", "ray_cull_model.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def exported(tmp_path, chain):
    """Kernel names in the code object that compile_flavour leaves in the on-disk cache (an ELF: the names are in its
    symbol table and in the metadata note)."""
    env = dict(os.environ, SDFK_CACHE_DIR=str(tmp_path))
    res = subprocess.run([sys.executable, "-c", _SCRIPT.format(root=ROOT, chain=chain)], env=env, capture_output=True,
                         text=True, check=True)
    info = json.loads(res.stdout.strip().splitlines()[-1])
    files = list(tmp_path.iterdir())
    assert len(files) == 1 and files[0].stat().st_size == info["size"] + 24
    blob = files[0].read_bytes()
    return info, [k for k in KERNELS if k + b"\0" in blob]


def test_ray_flavour_of_a_long_union_exports_the_plain_and_the_culled_pair(built, tmp_path):
    info, names = exported(tmp_path, True)
    assert info["chain_members"] == 300 and names == KERNELS


def test_ray_flavour_of_a_small_tree_is_the_two_kernels_it_was(built, tmp_path):
    info, names = exported(tmp_path, False)
    assert info["chain_members"] == 0 and names == KERNELS[:2]


def test_statistics_entry_is_declared_listed_and_exported(built):
    with open(os.path.join(ROOT, "include", "sdfk.h")) as f:
        header = f.read()
    assert "void sdfk_debug_rays_stats(int enable, long long* out8);" in header
    assert "#define SDFK_ABI_VERSION 1" in header
    assert "sdfk_debug_rays_stats" in built.SIGNATURES and hasattr(built.lib(), "sdfk_debug_rays_stats")


def test_model_scene_is_the_workload(built):
    import aegolius_amd.cores as ns
    from aegolius_amd import workloads
    from oracle import sdf_oracle
    m = model()
    centres, radii = m.spheres(200)
    pts = np.random.default_rng(0).uniform(-1.2, 1.2, (3, 500))
    want = sdf_oracle.evaluate(workloads.sphere_union(ns, count=200), pts)
    np.testing.assert_allclose(m.members_at(centres, radii, pts.T).min(axis=1), want, rtol=0, atol=1e-12)


def test_model_meets_the_quarter_at_320x240():
    """The condition of the GPU test — fewer than a quarter of the 1000 members per lane and evaluation — is one the rule
    itself meets: every tile of the 320 x 240 image, the kernels' cap, depth and policy."""
    c = model().model(members=1000, width=320, height=240, cap=192, depth=3, look=0.0, tiles=0)
    print(c)
    assert c["tiles"] == 1200 and c["builds"] > 0 and c["splits"] > 0
    assert c["members_per_evaluation"] < 250.0


def test_survivor_rule_never_drops_the_minimiser():
    """Random spheres, random bounding spheres; at 10,000 points of those balls (float64) the minimiser over all members is
    on the list, so the minimum over the list is the minimum."""
    m = model()
    rng = np.random.default_rng(11)
    checked = dropped = 0
    for trial in range(100):
        n = int(rng.integers(22, 400))
        centres = rng.uniform(-1.0, 1.0, (n, 3))
        radii = rng.uniform(0.01, 0.2, n)
        c = rng.uniform(-1.2, 1.2, 3)
        rho = float(10.0 ** rng.uniform(-3, 0))
        keep, R = m.survivors(centres, radii, c, rho, look=float(rng.choice([0.0, 0.5])))
        assert R >= rho and keep.size >= 1 and np.all(np.diff(keep) > 0)
        dropped += n - keep.size
        v = rng.normal(size=(100, 3))
        v *= (R * rng.uniform(0.0, 1.0, 100) ** (1.0 / 3.0) / np.linalg.norm(v, axis=1))[:, None]
        v[:10] *= (R / np.linalg.norm(v[:10], axis=1))[:, None]              # (ten of them on the sphere itself)
        pts = c[None] + v * (1.0 - 1e-12)
        e = m.members_at(centres, radii, pts)
        assert np.all(np.isin(e.argmin(axis=1), keep))
        assert np.array_equal(e[:, keep].min(axis=1), e.min(axis=1))
        checked += pts.shape[0]
    assert checked == 10000 and dropped > 1000
