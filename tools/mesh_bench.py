"""Isosurface extraction on one MI355X: the cfg 2 tree's resident field at 513^3 and 1025^3 (and 257^3, where the output
is also compared with the numpy definition in tests/mesh_reference.py). Device events around the counting call (bits,
count and scans) and the emit call, the copy of the mesh to the host, and the whole host call; warm-up, median of 5.
Writes profiles/mesh_bench.json. Per-kernel times come from a rocprofv3 --kernel-trace --stats run of this script.

--geometry: the geometry path (mesh.isosurface(geometry, axes): no field, no coordinate array) against the field path
(the field evaluated from the axis tables into HBM, then mesh.isosurface(field)), the cfg 2 tree at level 0, the two
paths alternately in one process at each size, device events, median of 5 after a warm-up; per-phase times and scratch
bytes of each. --solo sizes run the geometry path alone (4097^3: the field path does not fit). Also the wall time of
from_geometry at 513^3 against the old composition (generate_grid, create_resident, isosurface). Writes
profiles/mesh_geometry_bench.json.

    python tools/mesh_bench.py [--sizes 257,513,1025] [--reps 5] [--out profiles/mesh_bench.json]
    python tools/mesh_bench.py --geometry [--sizes 257,513,1025,2049] [--solo 4097] [--out profiles/mesh_geometry_bench.json]
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
    ap.add_argument("--out", default=None)
    ap.add_argument("--geometry", action="store_true")
    ap.add_argument("--solo", default="")
    ap.add_argument("--wall", type=int, default=513, help="from_geometry wall-time size (0: skip)")
    args = ap.parse_args()
    import __graft_entry__
    __graft_entry__.build()
    if args.geometry:
        return geometry_leg(args)
    args.out = args.out or os.path.join(ROOT, "profiles", "mesh_bench.json")
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


def _median(runs):
    return {k: float(np.median([x[k] for x in runs])) for k in runs[0]}


def geometry_leg(args):
    import aegolius_amd.cores as ns
    from aegolius_amd import _engine, mesh, workloads
    from aegolius_amd._eval import config, program_for
    from aegolius_amd._lower import lower_geometry
    _engine.require_gpu()
    L = _engine.lib()
    geo = workloads.cfg2_tree(ns)
    prog = program_for(lower_geometry(geo))
    out = {"workload": "cfg2_tree, isosurface at level 0: geometry path vs field path (field from the axis tables)",
           "reps": args.reps, "sizes": {}}

    def field_run(axes, n):
        t = {}
        e0, e1 = _engine.Event(), _engine.Event()
        t0 = time.perf_counter()
        e0.record()
        dev = _engine.DeviceField(n, config.device)
        try:
            prog.eval_grid(axes, 0, n, dev.ptr, mode=config.mode)
            e1.record()
            m = mesh.isosurface(dev, axes, timings=t)
        finally:
            dev.free()
        t["evaluate"] = e0.elapsed_ms(e1)
        t["device_ms"] = t["evaluate"] + t["count"] + t["emit"]
        t["host_call"] = (time.perf_counter() - t0) * 1e3
        return t, m

    def geo_run(axes):
        t = {}
        t0 = time.perf_counter()
        m = mesh.isosurface(geo, axes, timings=t)
        t["device_ms"] = t["count"] + t["emit"]
        t["host_call"] = (time.perf_counter() - t0) * 1e3
        return t, m

    sizes = [int(s) for s in args.sizes.split(",") if s]
    solo = [int(s) for s in args.solo.split(",") if s]
    for r in sizes + solo:
        axes = [np.linspace(-1.0, 1.0, r)] * 3
        n = r ** 3
        both = r not in solo
        geo_run(axes)                                           # warm-up (code objects, allocator)
        if both:
            field_run(axes, n)
        runs_f, runs_g = [], []
        for _ in range(args.reps):                              # alternately, in one process
            if both:
                t, mf = field_run(axes, n)
                runs_f.append(t)
            t, mg = geo_run(axes)
            runs_g.append(t)
        rec = {"points": n, "vertices": int(len(mg.vertices)), "faces": int(len(mg.faces)),
               "geometry": {"median_ms": _median(runs_g), "runs_ms": runs_g,
                            "scratch_bytes": int(L.sdfk_eval_grid_isosurface_scratch(r, r, r)),
                            "scratch_bytes_per_point": L.sdfk_eval_grid_isosurface_scratch(r, r, r) / n,
                            "edge_end_bytes": 32 * int(len(mg.vertices))}}
        if both:
            rec["field"] = {"median_ms": _median(runs_f), "runs_ms": runs_f,
                            "scratch_bytes": int(4 * n + L.sdfk_field_isosurface_scratch(r, r, r)),
                            "scratch_bytes_per_point": (4 * n + L.sdfk_field_isosurface_scratch(r, r, r)) / n}
            rec["equal_output"] = bool(np.array_equal(mf.vertices.view(np.uint32), mg.vertices.view(np.uint32)) and
                                       np.array_equal(mf.faces, mg.faces))
            rec["device_ratio_geometry_over_field"] = (rec["geometry"]["median_ms"]["device_ms"] /
                                                       rec["field"]["median_ms"]["device_ms"])
        out["sizes"][str(r)] = rec
        print(r, json.dumps({k: ({kk: vv for kk, vv in v.items() if kk != "runs_ms"} if isinstance(v, dict) else v)
                             for k, v in rec.items()}), flush=True)
    if args.wall:
        r = args.wall
        old, new = [], []
        for rep in range(args.reps + 1):
            t0 = time.perf_counter()
            co, _ = ns.generate_grid((2, 2, 2), (r, r, r))
            dev = geo.create_resident(co)
            try:
                mesh.isosurface(dev, co)
            finally:
                dev.free()
            del co
            t1 = time.perf_counter()
            mesh.from_geometry(geo, (2, 2, 2), (r, r, r))
            t2 = time.perf_counter()
            if rep:                                             # rep 0: warm-up
                old.append((t1 - t0) * 1e3)
                new.append((t2 - t1) * 1e3)
        out["from_geometry_wall_ms"] = {"size": r, "old_composition_with_host_grid": float(np.median(old)),
                                        "geometry_path": float(np.median(new)), "old_runs": old, "new_runs": new}
        print("from_geometry", json.dumps(out["from_geometry_wall_ms"]), flush=True)
    path = args.out or os.path.join(ROOT, "profiles", "mesh_geometry_bench.json")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
