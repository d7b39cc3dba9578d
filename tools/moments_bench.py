"""Mass-properties benchmark (aegolius_amd.moments): the moments call against the route users had before it.
    python tools/moments_bench.py [cfg2:513 cfg5:513 union1000:257] [--samples 4 --reps 5 --warmup 2 --out profiles/moments_bench.txt]
scenes: cfg2, cfg5, union<N>, each with the points per axis of its BASELINE box. Per scene, in one process, the median of
`reps` calls after `warmup` (MODE_SPECIALIZED: the builds are waited for in the warm-up):
  * moments_ms: moments.moments(...), the whole public call, wall clock with the device idle at both ends; its passes
    (centre / far / sample) in device-event milliseconds from the call's own `timings`;
  * the route without this module: occupancy.fractions(...) with its host result (fractions_ms, wall clock; its passes too),
    then the numpy weighting of the downloaded field for volume, first and second moments (numpy_ms): three plane sums in
    float64 and the products with the cell centres — first-order at the surface, which is all that route can give;
  * ratio = moments_ms / (fractions_ms + numpy_ms), and how far the two centroids are apart.
Writes a header and one JSON line per scene to --out and prints them."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HEADER = """# tools/moments_bench.py, one MI355X (gfx950), k = %d, median of %d after %d warm-up(s), all scenes in one process
# moments_ms: moments.moments, the whole public call (wall clock); centre / far / sample: its passes (device events)
# fractions_ms: occupancy.fractions with its host result (wall clock); numpy_ms: volume, first and second moments of the
# downloaded field with numpy; route_ms = fractions_ms + numpy_ms; ratio = moments_ms / route_ms (below 1: moments is faster)
"""


def scene(name):
    import aegolius_amd.cores as ns
    from aegolius_amd import workloads
    if name.startswith("union") and name[5:].isdigit():
        return workloads.sphere_union(ns, count=int(name[5:])), (2, 2, 2)
    tree, size, _ = workloads.build(name, ns)
    return tree, size


def wall(call, reps, warmup):
    """-> (median ms, the results) of call(), wall clock, the device idle before and after."""
    from aegolius_amd import _engine
    out, results = [], []
    for i in range(warmup + reps):
        _engine.check(_engine.lib().sdfk_sync(None), "sdfk_sync")
        t0 = time.perf_counter()
        result = call()
        _engine.check(_engine.lib().sdfk_sync(None), "sdfk_sync")
        if i >= warmup:
            out.append((time.perf_counter() - t0) * 1e3)
            results.append(result)
    return float(np.median(out)), results


def numpy_moments(fraction, axes):
    """What a user computes from the fraction field: (volume, centroid (3,), central second moments (3, 3)), cell centres
    as the sample points."""
    n = [a.size for a in axes]
    step = [(a[-1] - a[0]) / (a.size - 1) for a in axes]
    f = fraction.reshape(n)
    planes = {(0, 1): f.sum(axis=2, dtype=np.float64), (0, 2): f.sum(axis=1, dtype=np.float64), (1, 2): f.sum(axis=0, dtype=np.float64)}
    lines = [planes[(0, 1)].sum(axis=1), planes[(0, 1)].sum(axis=0), planes[(0, 2)].sum(axis=0)]
    total = lines[0].sum()
    dV = step[0] * step[1] * step[2]
    centroid = np.array([lines[a] @ axes[a] for a in range(3)]) / total
    S = np.zeros((3, 3))
    for a in range(3):
        S[a, a] = lines[a] @ (axes[a] - centroid[a]) ** 2
        for b in range(a + 1, 3):
            S[a, b] = S[b, a] = (axes[a] - centroid[a]) @ planes[(a, b)] @ (axes[b] - centroid[b])
    return total * dV, centroid, S * dV


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("scenes", nargs="*", default=["cfg2:513", "cfg5:513", "union1000:257"])
    ap.add_argument("--samples", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "moments_bench.txt"))
    args = ap.parse_args()
    import __graft_entry__
    __graft_entry__.build()
    from aegolius_amd import _engine, moments, occupancy
    from aegolius_amd._eval import config
    from aegolius_amd.cores.helper_functions import grid_axes
    _engine.require_gpu()
    config.mode = _engine.MODE_SPECIALIZED
    k = args.samples
    lines = [HEADER % (k, args.reps, args.warmup)]
    for spec in args.scenes:
        name, n = spec.split(":")
        n = int(n)
        geo, box = scene(name)
        axes, _ = grid_axes(box, (n, n, n))
        axes = [np.asarray(a, dtype=np.float64) for a in axes]
        mom_passes, occ_passes = [], []

        def call_moments():
            mom_passes.append({})
            return moments.moments(geo, axes, k, timings=mom_passes[-1])

        def call_fractions():
            occ_passes.append({})
            return occupancy.fractions(geo, axes, k, timings=occ_passes[-1])
        moments_ms, got = wall(call_moments, args.reps, args.warmup)
        mp = got[-1]
        fractions_ms, got = wall(call_fractions, args.reps, args.warmup)
        occ = got[-1]
        numpy_out = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            volume, centroid, second = numpy_moments(occ.fraction, axes)
            numpy_out.append((time.perf_counter() - t0) * 1e3)
        numpy_ms = float(np.median(numpy_out))
        route_ms = fractions_ms + numpy_ms
        result = {"scene": name, "size": n, "samples": k, "cells": n ** 3, "near_cells": mp.near_cells,
                  "inside_samples": mp.inside_samples, "same_inside_samples": mp.inside_samples == occ.inside_samples,
                  "same_near_cells": mp.near_cells == occ.near_cells, "moments_ms": moments_ms}
        for key in ("centre", "far", "sample"):
            result[key + "_ms"] = float(np.median([p[key] for p in mom_passes[args.warmup:]]))
        result.update(fractions_ms=fractions_ms, numpy_ms=numpy_ms, route_ms=route_ms, ratio=moments_ms / route_ms,
                      moments_not_slower=bool(moments_ms <= route_ms))
        for key in ("centre", "classify", "sample", "volume"):
            result["fractions_" + key + "_ms"] = float(np.median([p[key] for p in occ_passes[args.warmup:]]))
        result.update(volume=mp.volume, volume_route=volume, centroid=[float(v) for v in mp.centroid],
                      centroid_distance_to_route=float(np.linalg.norm(mp.centroid - centroid)),
                      inertia_trace=float(np.trace(mp.inertia)), inertia_trace_route=float(2.0 * np.trace(second)))
        lines.append(json.dumps(result) + "\n")
        print(lines[-1], end="", flush=True)
        with open(args.out, "w") as f:                         # (after every scene: a time limit leaves the finished ones)
            f.writelines(lines)


if __name__ == "__main__":
    main()
