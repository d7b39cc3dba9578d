"""Redistancing benchmark and accuracy table (aegolius_amd.redistance). One step per call, so that a job can
give every step a time limit of its own; every call appends its lines to --out (default profiles/redistance_bench.txt).
    python tools/bench_redistance.py time cfg2 [--size 513 --band-steps 8 --reps 5 --warmup 1 --cpu]
    python tools/bench_redistance.py accuracy [--size 65]
time: the scene's BASELINE box with `size` points per axis; the field is evaluated into HBM from the axis tables
  (Program.eval_grid, timed as field_ms: the plain field kernel's time for the same grid) and redistanced `reps` times,
  resident in and out. Reported: device-event milliseconds per pass and in total (medians), the seeds, and with --cpu, if
  scipy imports, scipy.ndimage.distance_transform_edt of the inside mask and of its complement on the host (wall clock).
  --band-steps 0 is band=None.
accuracy: |out - true| in units of the grid step — max and mean over the first ring (the ends of crossing edges), the
  second ring (their 6-neighbours) and the points beyond — with near="seeds" and near="gradient", for a sphere given as
  3 (|p| - r) and as |p|^2 - r^2 (true = |p| - r) and for a twisted box (true = the result, near="gradient", on the grid
  refined 4 times per axis, read at the coarse points: an estimate itself, good to a fraction of the fine step)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def emit(out, record):
    line = json.dumps(record)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "a") as f:
        f.write(line + "\n")


def run_time(args):
    import aegolius_amd.cores as ns
    from aegolius_amd import _engine, redistance, workloads
    from aegolius_amd._eval import config, program_for
    from aegolius_amd._lower import lower_geometry
    from aegolius_amd.cores.helper_functions import grid_axes
    tree, box, _ = workloads.build(args.scene, ns)
    n = args.size
    axes, _ = grid_axes(box, (n, n, n))
    tabs = [np.asarray(a, dtype=np.float32) for a in axes]
    step = float(tabs[0][1] - tabs[0][0])
    band = args.band_steps * step if args.band_steps > 0 else None
    prog = program_for(lower_geometry(tree))
    total = n ** 3
    record = {"what": "time", "scene": args.scene, "size": n, "points": total, "band_steps": args.band_steps or None,
              "near": args.near, "device": "MI355X (gfx950), 1 GPU"}
    with _engine.DeviceField(total, config.device) as field:
        ms = []
        for i in range(args.warmup + args.reps):
            a, b = _engine.Event(), _engine.Event()
            a.record()
            prog.eval_grid(tabs, 0, total, field.ptr, mode=_engine.MODE_SPECIALIZED)
            b.record()
            _engine.check(_engine.lib().sdfk_sync(None), "sdfk_sync")
            if i >= args.warmup:
                ms.append(a.elapsed_ms(b))
        record["field_ms"] = float(np.median(ms))
        runs = []
        for i in range(args.warmup + args.reps):
            stats = {}
            out = redistance.redistance(field, tabs, band=band, near=args.near, resident=True, stats=stats)
            out.free()
            if i >= args.warmup:
                runs.append(stats)
        record["seeds"] = runs[0]["seeds"]
        record["pass_ms"] = {k: float(np.median([r["ms"][k] for r in runs])) for k in runs[0]["ms"]}
        record["total_ms"] = float(np.median([sum(r["ms"].values()) for r in runs]))
        record["slowest_pass"] = max(record["pass_ms"], key=record["pass_ms"].get)
        if args.cpu:
            try:
                from scipy import ndimage
            except ImportError:
                record["cpu_edt_s"] = None
            else:
                inside = (field.numpy() <= 0).reshape(n, n, n)
                t0 = time.time()
                ndimage.distance_transform_edt(inside, sampling=step)
                ndimage.distance_transform_edt(~inside, sampling=step)
                record["cpu_edt_s"] = time.time() - t0
    emit(args.out, record)


def rings(inside):
    """(first, second, beyond) masks: ends of crossing edges, their 6-neighbours, the rest."""
    first = np.zeros(inside.shape, dtype=bool)
    for a in range(inside.ndim):
        lo = tuple(slice(0, -1) if o == a else slice(None) for o in range(inside.ndim))
        hi = tuple(slice(1, None) if o == a else slice(None) for o in range(inside.ndim))
        cross = inside[lo] != inside[hi]
        first[lo] |= cross
        first[hi] |= cross
    grown = first.copy()
    for a in range(inside.ndim):
        lo = tuple(slice(0, -1) if o == a else slice(None) for o in range(inside.ndim))
        hi = tuple(slice(1, None) if o == a else slice(None) for o in range(inside.ndim))
        grown[lo] |= first[hi]
        grown[hi] |= first[lo]
    return first, grown & ~first, ~grown


def run_accuracy(args):
    import aegolius_amd.cores as ns
    from aegolius_amd import redistance
    n = args.size
    fine_n = 4 * (n - 1) + 1
    ax = [np.linspace(-1.0, 1.0, n)] * 3
    fine_ax = [np.linspace(-1.0, 1.0, fine_n)] * 3
    h = 2.0 / (n - 1)
    g = np.meshgrid(*[a.astype(np.float32) for a in ax], indexing="ij")
    r = np.sqrt(g[0] * g[0] + g[1] * g[1] + g[2] * g[2]).astype(np.float32)
    R = np.float32(0.6)

    def twisted():
        b = ns.Box(0.9, 0.6, 0.4)
        b.twist(np.pi / 2)
        return b
    fine = redistance.redistance(twisted(), fine_ax, near="gradient").reshape(fine_n, fine_n, fine_n)[::4, ::4, ::4]
    co = np.stack([x.ravel() for x in np.meshgrid(*ax, indexing="ij")])
    cases = {"sphere 3(|p|-r)": ((np.float32(3) * (r - R)).ravel(), (r - R).ravel()),
             "sphere |p|^2-r^2": ((r * r - R * R).ravel(), (r - R).ravel()),
             "twisted box": (np.asarray(twisted().create(co), dtype=np.float32), fine.ravel())}
    for name, (field, true) in cases.items():
        first, second, beyond = (m.ravel() for m in rings((field <= 0).reshape(n, n, n)))
        for near in redistance.NEAR:
            out = redistance.redistance(field, ax, near=near)
            err = np.abs(out.astype(np.float64) - true.astype(np.float64)) / h
            record = {"what": "accuracy", "field": name, "size": n, "near": near}
            for ring, mask in (("first", first), ("second", second), ("beyond", beyond)):
                record[ring] = {"points": int(mask.sum()), "max": float(err[mask].max()), "mean": float(err[mask].mean())}
            emit(args.out, record)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["time", "accuracy"])
    ap.add_argument("scene", nargs="?", default="cfg2")
    ap.add_argument("--size", type=int, default=None)
    ap.add_argument("--band-steps", type=float, default=8)
    ap.add_argument("--near", default="gradient")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--cpu", action="store_true", help="also time scipy's distance_transform_edt on the host")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "redistance_bench.txt"))
    args = ap.parse_args()
    import __graft_entry__
    __graft_entry__.build()
    from aegolius_amd import _engine
    _engine.require_gpu()
    if args.what == "time":
        args.size = args.size or 513
        run_time(args)
    else:
        args.size = args.size or 65
        run_accuracy(args)


if __name__ == "__main__":
    main()
