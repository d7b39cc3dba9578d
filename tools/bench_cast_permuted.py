"""Incoherent rays through the culled ray kernels: `render.cast` of the bench camera's rays in a seeded
random permutation, MODE_NOCULL and MODE_SPECIALIZED alternately, and the same rays in camera order for comparison.
    python tools/bench_cast_permuted.py [union1000 --width 640 --height 480 --reps 7]
Wall time of the whole call (upload of the rays, kernel, download of the results: the copies are the same for both
modes), median; the outputs of the two modes are compared bit for bit. Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("scene", nargs="?", default="union1000")
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    import __graft_entry__
    __graft_entry__.build()
    import bench_render
    from aegolius_amd import _engine, render
    from aegolius_amd._eval import config
    _engine.require_gpu()
    geo = bench_render.scene(args.scene)
    cam = render.Camera(bench_render.EYE, (0, 0, 0), (0, 0, 1), 40.0)
    W, H = args.width, args.height
    o, d = (np.ascontiguousarray(a, dtype=np.float32) for a in cam.rays(W, H))
    eps, cone = (float(np.float32(x)) for x in cam.footprint(W, H))
    perm = np.random.default_rng(3).permutation(o.shape[1])
    orders = {"camera_order": (o, d), "permuted": (np.ascontiguousarray(o[:, perm]), np.ascontiguousarray(d[:, perm]))}
    modes = {"nocull": _engine.MODE_NOCULL, "specialised": _engine.MODE_SPECIALIZED}
    result = {"scene": args.scene, "rays": int(o.shape[1]), "device": "MI355X (gfx950), 1 GPU", "ms": {}}
    old = config.mode
    try:
        for oname, (oo, dd) in orders.items():
            times = {m: [] for m in modes}
            outs = {}
            for rep in range(args.reps + 2):                     # (two warm-up rounds: the first builds the kernels)
                for m, value in modes.items():
                    config.mode = value
                    t0 = time.perf_counter()
                    outs[m] = render.cast(geo, oo, dd, 0.0, 8.0, eps, cone, 256, normals=True)
                    if rep >= 2:
                        times[m].append(1e3 * (time.perf_counter() - t0))
            a, b = outs["nocull"], outs["specialised"]
            same = all(np.array_equal(np.asarray(x).view(np.uint8), np.asarray(y).view(np.uint8))
                       for x, y in ((a.t, b.t), (a.status, b.status), (a.steps, b.steps), (a.normals, b.normals)))
            result["ms"][oname] = {m: float(np.median(v)) for m, v in times.items()}
            result["ms"][oname]["same_bits"] = bool(same)
    finally:
        config.mode = old
    print(json.dumps(result))


if __name__ == "__main__":
    main()
