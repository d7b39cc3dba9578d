"""Occupancy benchmark (aegolius_amd.occupancy): one scene and one size per call, so that a job can give every
step a time limit of its own.
    python tools/bench_occupancy.py cfg2 --size 513 [--samples 4 --reps 7 --warmup 2 --nocull --compare --no-field]
scenes: cfg2, cfg5, union<N>. The grid is the scene's BASELINE box with `size` points per axis. Device events, the median
of `reps` calls after `warmup`:
  * total_ms: occupancy.fractions(resident=True), the whole public call (lowering, tables, allocation, the three passes, the
    volume's row sums);
  * per pass (centre / classify / sample / volume) from the call's own `timings`, near_cells, and the sub-samples the sample
    pass evaluated per second;
  * unless --no-field the yardstick — the plain field kernel of the same program (MODE_NOCULL) on a (3, M) array of
    M = min(that many, 2^26) random points — and the ratio of the two rates;
  * --nocull: the same call under MODE_NOCULL (every cell sampled);
  * --compare: Program.eval_grid of the fine grid the sub-sample tables span ((size k)^3 points into a resident field): the
    only route to the same counts without this module, timed the same way in the same process.
Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def scene(name):
    import aegolius_amd.cores as ns
    from aegolius_amd import workloads
    if name.startswith("union") and name[5:].isdigit():
        return workloads.sphere_union(ns, count=int(name[5:])), (2, 2, 2)
    tree, size, _ = workloads.build(name, ns)
    return tree, size


def timed(call, reps, warmup):
    """-> (median ms, min ms, the last result) of call(), device events around the whole call."""
    from aegolius_amd import _engine
    out, result = [], None
    for i in range(warmup + reps):
        if result is not None and hasattr(result, "free"):
            result.free()
        a, b = _engine.Event(), _engine.Event()
        a.record()
        result = call()
        b.record()
        _engine.check(_engine.lib().sdfk_sync(None), "sdfk_sync")
        if i >= warmup:
            out.append(a.elapsed_ms(b))
    return float(np.median(out)), float(min(out)), result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("scene")
    ap.add_argument("--size", type=int, default=257)
    ap.add_argument("--samples", type=int, default=4)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--nocull", action="store_true", help="also time MODE_NOCULL (every cell sampled)")
    ap.add_argument("--compare", action="store_true", help="also time Program.eval_grid of the fine grid")
    ap.add_argument("--no-field", action="store_true", help="skip the field-kernel yardstick")
    args = ap.parse_args()
    import __graft_entry__
    __graft_entry__.build()
    from aegolius_amd import _engine, occupancy, render
    from aegolius_amd._eval import config, program_for
    from aegolius_amd.cores.helper_functions import grid_axes
    _engine.require_gpu()
    geo, box = scene(args.scene)
    low, _ = render.lower(geo)
    prog = program_for(low)
    k, n = args.samples, args.size
    axes, _ = grid_axes(box, (n, n, n))
    K = k ** 3
    result = {"scene": args.scene, "size": n, "samples": k, "cells": n ** 3, "instructions": int(low.code.shape[0]),
              "lipschitz": low.lipschitz, "chain_members": prog.chain_members, "device": "MI355X (gfx950), 1 GPU"}
    config.mode = _engine.MODE_SPECIALIZED                      # the builds are waited for in the warm-up, not timed
    passes = []

    def call():
        passes.append({})
        return occupancy.fractions(geo, axes, k, resident=True, timings=passes[-1])
    ms, ms_min, occ = timed(call, args.reps, args.warmup)
    result.update(total_ms=ms, total_ms_min=ms_min, near_cells=occ.near_cells, near_share=occ.near_cells / n ** 3,
                  inside_samples=occ.inside_samples, volume=occ.volume)
    occ.free()
    for name in ("centre", "classify", "sample", "volume"):
        result[name + "_ms"] = float(np.median([p[name] for p in passes[args.warmup:]]))
    evals = occ.near_cells * K
    result["sub_samples"] = evals
    result["sub_samples_per_s"] = evals / (result["sample_ms"] * 1e-3) if result["sample_ms"] > 0 else None
    if not args.no_field and evals:
        m = min(evals, 1 << 26)
        co = _engine.DeviceVectorField.from_host(np.random.default_rng(1).uniform(-1.0, 1.0, (3, m)).astype(np.float32), config.device)
        field = _engine.DeviceField(m, config.device)
        try:
            result["field_ms"], _, _ = timed(lambda: prog.eval_device(co.row_ptr(0), m, co.stride, field.ptr,
                                                                      mode=_engine.MODE_NOCULL), args.reps, args.warmup)
        finally:
            co.free()
            field.free()
        result["field_points"] = m
        result["field_points_per_s"] = m / (result["field_ms"] * 1e-3)
        result["ratio_to_field_kernel"] = result["sub_samples_per_s"] / result["field_points_per_s"]
    if args.nocull:
        config.mode = _engine.MODE_NOCULL
        passes_nc = []

        def call_nc():
            passes_nc.append({})
            return occupancy.fractions(geo, axes, k, resident=True, timings=passes_nc[-1])
        ms, ms_min, occ_nc = timed(call_nc, args.reps, args.warmup)
        result["nocull"] = {"total_ms": ms, "total_ms_min": ms_min, "near_cells": occ_nc.near_cells,
                            "sample_ms": float(np.median([p["sample"] for p in passes_nc[args.warmup:]])),
                            "same_inside_samples": occ_nc.inside_samples == result["inside_samples"]}
        occ_nc.free()
        config.mode = _engine.MODE_SPECIALIZED
    if args.compare:
        tabs, _ = occupancy.sample_tables(axes, k)
        fine = int(np.prod([t.size for t in tabs], dtype=np.int64))
        field = _engine.DeviceField(fine, config.device)
        try:
            ms, ms_min, _ = timed(lambda: prog.eval_grid(tabs, 0, fine, field.ptr, mode=_engine.MODE_SPECIALIZED), args.reps,
                                  args.warmup)
        finally:
            field.free()
        result["fine_grid"] = {"points": fine, "bytes": 4 * fine, "eval_grid_ms": ms, "eval_grid_ms_min": ms_min,
                               "points_per_s": fine / (ms * 1e-3), "ratio_fine_over_occupancy": ms / result["total_ms"],
                               "occupancy_not_slower": bool(result["total_ms"] <= ms)}
    print(json.dumps(result))


if __name__ == "__main__":
    t0 = time.time()
    main()
    print("# %.1f s" % (time.time() - t0), file=sys.stderr)
