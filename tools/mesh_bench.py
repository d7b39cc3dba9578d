"""Isosurface extraction on one MI355X: the cfg 2 tree's resident field at 513^3 and 1025^3 (and 257^3, where the output
is also compared with the numpy definition in tests/mesh_reference.py). Device events around the counting call (bits,
count and scans) and the emit call, the copy of the mesh to the host, and the whole host call; warm-up, median of 5.
Writes profiles/mesh_bench.json. Per-kernel times come from a rocprofv3 --kernel-trace --stats run of this script.

    python tools/mesh_bench.py [--sizes 257,513,1025] [--reps 5] [--out profiles/mesh_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="257,513,1025")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_bench.json"))
    args = ap.parse_args()
    import __graft_entry__
    __graft_entry__.build()
    import aegolius_amd.cores as ns
    from aegolius_amd import _engine, mesh, workloads
    _engine.require_gpu()
    out = {"workload": "cfg2_tree resident field, isosurface at level 0", "reps": args.reps, "sizes": {}}
    for r in [int(s) for s in args.sizes.split(",")]:
        co, _ = ns.generate_grid((2, 2, 2), (r, r, r))
        dev = workloads.cfg2_tree(ns).create_resident(co)
        try:
            mesh.isosurface(dev, co)                            # warm-up (code objects, allocator)
            runs = []
            for _ in range(args.reps):
                t = {}
                t0 = time.perf_counter()
                m = mesh.isosurface(dev, co, timings=t)
                t["host_call"] = (time.perf_counter() - t0) * 1e3
                runs.append(t)
            med = {k: float(np.median([x[k] for x in runs])) for k in runs[0]}
            n = r ** 3
            dev_ms = med["count"] + med["emit"]
            rec = {"points": n, "vertices": int(len(m.vertices)), "faces": int(len(m.faces)), "median_ms": med,
                   "device_ms": dev_ms, "runs_ms": runs,
                   "field_read_GBps": 4.0 * n / (med["count"] * 1e-3) / 1e9,
                   "mesh_bytes": int(m.vertices.nbytes + len(m.faces) * 12)}
            if r <= 257:
                import mesh_reference as R
                f = dev.numpy()
                t0 = time.perf_counter()
                want = R.extract(f, co.grid_axes)
                rec["numpy_reference_ms"] = (time.perf_counter() - t0) * 1e3
                rec["equal_to_reference"] = bool(np.array_equal(m.vertices, want[0]) and np.array_equal(m.faces, want[1]))
            out["sizes"][str(r)] = rec
            print(r, json.dumps({k: v for k, v in rec.items() if k != "runs_ms"}), flush=True)
        finally:
            dev.free()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
