"""Developer tool (GPU): the liquid-crystal waveguide kernels on resident fields at 257^3 and 513^3, in one process.

Inputs: uu / ww = the example's waveguide SDF and vertical distance (tests/lcwg_scenes.py), created on the device.
Timed (best of 5, HIP events, kernels already loaded): the crossings pass (sdfk_field_crossings_2d on pp), the fused
LCWG3Dm1 / LCWG3Dp1 / LCWG2D kernel (sdfk_lcwg_eval, automatic sign plane precomputed) and, as the in-process
yardstick, from_sdf's normalised gradient (sdfk_field_gradient) on the same grid. Algorithmic bytes per point:
LCWG3D 20 (uu, ww in, 3 rows out), LCWG2D 16, gradient 16. With --isa the VALU count of the fused kernel's gfx950 code
(compiled here from aegolius_amd/csrc/sdfk.hip) is added, to name the bound.

    python tools/lcwg_bench.py [--isa] [--out profiles/lcwg_bench.json]
"""
import argparse
import collections
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
HBM_GBS = 8000.0


def isa_counts():
    """VALU / fp64 / memory instruction counts of every sdfk_lcwg_kernel instantiation (static, whole kernel body)."""
    src = os.path.join(ROOT, "aegolius_amd", "csrc", "sdfk.hip")
    with tempfile.TemporaryDirectory() as tmp:
        asm = os.path.join(tmp, "sdfk.s")
        subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-fno-honor-nans",
                        "-mno-amdgpu-ieee", "-std=c++17", "-S", "--cuda-device-only", "-Wno-unused-command-line-argument",
                        src, "-o", asm], check=True, cwd=os.path.dirname(src), capture_output=True)
        text = open(asm).read()
    out = {}
    for m in re.finditer(r"^(_Z\d+sdfk_lcwg_kernelILi(\d)EEv\S*):[^\n]*\n(.*?)\n\s*s_endpgm", text, re.S | re.M):
        body = m.group(3)
        ops = collections.Counter(re.findall(r"^\s+(v_\w+|s_\w+|global_\w+|buffer_\w+)", body, re.M))
        valu = sum(c for k, c in ops.items() if k.startswith("v_"))
        f64 = sum(c for k, c in ops.items() if k.startswith("v_") and "f64" in k)
        vgpr = re.search(r"; NumVgprs:\s+(\d+)", text[m.end():])
        out["variant%s" % m.group(2)] = {"valu_static": valu, "valu_f64_static": f64,
                                         "global_ops": sum(c for k, c in ops.items() if k.startswith("global_")),
                                         "vgpr": int(vgpr.group(1)) if vgpr else None}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--isa", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--sizes", default="257,513")
    args = ap.parse_args()
    import __graft_entry__
    __graft_entry__.build()
    import lcwg_scenes as ls
    import aegolius_amd.cores as ns
    from aegolius_amd import _engine
    vp = _engine._vp
    lib = _engine.lib()
    _engine.require_gpu()
    rec = {"hbm_roof_GB/s": HBM_GBS, "sizes": {}}

    def best_ms(fn, reps=5):
        fn()
        best = 1e9
        for _ in range(reps):
            e0, e1 = _engine.Event(), _engine.Event()
            e0.record(None)
            fn()
            e1.record(None)
            best = min(best, e0.elapsed_ms(e1))
        return best

    for r in [int(s) for s in args.sizes.split(",")]:
        res = (r, r, r)
        grid, _ = ns.generate_grid(ls.co_size(), res)
        wg, vertical = ls.quarter_circle(ns)
        uu, ww = wg.create_resident(grid), vertical.create_resident(grid)
        n = uu.n
        out = _engine.DeviceVectorField(n)
        plane = lib.sdfk_malloc(r * r)
        entry = {"points": n}

        def crossings():
            _engine.check(lib.sdfk_field_crossings_2d(vp(uu.ptr), vp(ww.ptr), r, r, r, float(ls.W), float(ls.D), 0.06,
                                                      vp(plane), None), "crossings")

        def fused(variant):
            return lambda: _engine.check(lib.sdfk_lcwg_eval(variant, vp(uu.ptr), vp(ww.ptr), r, r, r, float(ls.W), float(ls.D),
                                                            1, 0.0, vp(plane), vp(out.ptr), out.stride, None), "lcwg")

        def gradient():
            _engine.check(lib.sdfk_field_gradient(vp(uu.ptr), r, r, r, 3, 1, vp(out.ptr), out.stride, None), "gradient")

        entry["crossings_ms"] = round(best_ms(crossings), 4)
        for label, fn, nbytes in (("LCWG3Dm1", fused(2), 20), ("LCWG3Dp1", fused(1), 20), ("LCWG2D", fused(0), 16),
                                  ("from_sdf_gradient", gradient, 16)):
            ms = best_ms(fn)
            gbs = nbytes * n / ms / 1e6
            entry[label] = {"ms": round(ms, 4), "B/point": nbytes, "GB/s": round(gbs, 1), "frac_of_hbm": round(gbs / HBM_GBS, 3)}
        entry["LCWG3Dm1_over_gradient"] = round(entry["LCWG3Dm1"]["ms"] / entry["from_sdf_gradient"]["ms"], 2)
        rec["sizes"][str(r)] = entry
        lib.sdfk_free(vp(plane))
        for f in (uu, ww):
            f.free()
        out.free()
    if args.isa:
        rec["isa"] = isa_counts()
    print(json.dumps(rec, indent=1))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
