"""Plane-stack benchmark (aegolius_amd.slices): stack and measures against the route users had before them.
    python tools/slices_bench.py [cfg2 cfg5] [--sizes 257 1025 --loop-layers 33 --reps 5 --warmup 1 --out profiles/slices_bench.txt]
Per scene and size n, in one process (MODE_SPECIALIZED: the builds are waited for in the warm-up), z-sections on the
tables of generate_grid(box, (n, n, n)): n layers of n x n points. The median of `reps` calls after `warmup`, in
device-event milliseconds around the whole public call (the events bracket the host work between the launches too) and
in wall-clock milliseconds with the device idle at both ends:
  * stack_ms: slices.stack(...) with its host result; count / emit / copy: its passes from the call's own `timings`;
  * measures_ms: slices.measures(...);
  * the route without this module: one mesh.contour(moved copy, (x, y)) per layer, the copy moved by -h along z — run
    for `loop-layers` evenly spaced layers of the same stack (the copies are made before the clock starts); loop_ms is the
    whole loop, loop_ms_per_layer its share per layer;
  * ratio_per_layer = (stack_ms / n) / loop_ms_per_layer, measures_over_stack = measures_ms / stack_ms (stack_ms holds the
    download of the stack).
Writes a header and one JSON line per scene and size to --out and prints them."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HEADER = """# tools/slices_bench.py, one MI355X (gfx950), median of %d after %d warm-up(s), all cases in one process, MODE_SPECIALIZED
# z-sections of the scene on generate_grid(box, (n, n, n)): n layers of n x n points. *_ms: device events around the whole
# public call; *_wall_ms: wall clock, device idle at both ends. stack: slices.stack with its host result (count / emit / copy:
# its passes); measures: slices.measures; loop: mesh.contour of a copy moved by -h, per layer, over %d layers of the same stack
# ratio_per_layer = (stack_ms / n) / loop_ms_per_layer (below 1: the stack is faster per layer)
# measures_over_stack = measures_ms / stack_ms (below 1: the measures cost less than the stack with its download)
"""


def timed(call, reps, warmup):
    """-> (median device-event ms, median wall ms, last result) of call(), the device idle before and after."""
    from aegolius_amd import _engine
    sync = lambda: _engine.check(_engine.lib().sdfk_sync(None), "sdfk_sync")  # noqa: E731
    ev, wall, result = [], [], None
    for i in range(warmup + reps):
        e0, e1 = _engine.Event(), _engine.Event()
        sync()
        t0 = time.perf_counter()
        e0.record()
        result = call()
        e1.record()
        sync()
        if i >= warmup:
            wall.append((time.perf_counter() - t0) * 1e3)
            ev.append(e0.elapsed_ms(e1))
    return float(np.median(ev)), float(np.median(wall)), result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("scenes", nargs="*", default=["cfg2", "cfg5"])
    ap.add_argument("--sizes", type=int, nargs="*", default=[257, 1025])
    ap.add_argument("--loop-layers", type=int, default=33)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "slices_bench.txt"))
    args = ap.parse_args()
    import __graft_entry__
    __graft_entry__.build()
    import aegolius_amd.cores as ns
    from aegolius_amd import _engine, mesh, slices, workloads
    from aegolius_amd._eval import config
    from aegolius_amd.cores.helper_functions import grid_axes
    _engine.require_gpu()
    config.mode = _engine.MODE_SPECIALIZED
    lines = [HEADER % (args.reps, args.warmup, args.loop_layers)]
    for name in args.scenes:
        for n in args.sizes:
            geo, box, _ = workloads.build(name, ns)
            axes, _ = grid_axes(box, (n, n, n))
            x, y, z = (np.asarray(a, dtype=np.float64) for a in axes)
            passes = []

            def call_stack():
                passes.append({})
                return slices.stack(geo, (x, y), z, normal=2, timings=passes[-1])
            stack_ms, stack_wall, st = timed(call_stack, args.reps, args.warmup)
            measures_ms, measures_wall, sm = timed(lambda: slices.measures(geo, (x, y), z, normal=2), args.reps, args.warmup)
            picked = np.unique(np.linspace(0, n - 1, args.loop_layers).round().astype(int))
            copies = []
            for l in picked:
                copy, _, _ = workloads.build(name, ns)
                copy.move((0.0, 0.0, -float(np.float32(z[l]))))
                copies.append(copy)
            loop_ms, loop_wall, contours = timed(lambda: [mesh.contour(c, (x, y)) for c in copies], args.reps, args.warmup)
            same = sum(int(len(c.segments) == len(st.layer(int(l)).segments)) for c, l in zip(contours, picked))
            host = st.measures()
            ok = sm.closed & host.closed
            result = {"scene": name, "layers": n, "plane": [n, n], "vertices": int(len(st.vertices)),
                      "segments": int(len(st.segments)), "stack_ms": stack_ms, "stack_wall_ms": stack_wall}
            for key in ("count", "emit", "copy"):
                result[key + "_ms"] = float(np.median([p[key] for p in passes[args.warmup:]]))
            result.update(measures_ms=measures_ms, measures_wall_ms=measures_wall, loop_layers=int(len(picked)), loop_ms=loop_ms,
                          loop_wall_ms=loop_wall, loop_ms_per_layer=loop_ms / len(picked), stack_ms_per_layer=stack_ms / n,
                          ratio_per_layer=(stack_ms / n) / (loop_ms / len(picked)), measures_over_stack=measures_ms / stack_ms,
                          stack_faster_per_layer=bool(stack_ms / n < loop_ms / len(picked)),
                          measures_cheaper_than_stack=bool(measures_ms < stack_ms),
                          loop_layers_with_the_same_segment_count=same, open_layers=int(np.count_nonzero(~sm.closed)),
                          volume=sm.volume(), area_device_minus_host_max=float(np.abs(sm.area[ok] - host.area[ok]).max(initial=0.0)))
            lines.append(json.dumps(result) + "\n")
            print(lines[-1], end="", flush=True)
            with open(args.out, "w") as f:                     # (after every case: a time limit leaves the finished ones)
                f.writelines(lines)


if __name__ == "__main__":
    main()
