"""Developer tool (GPU): Points.to_image on one MI355X, split into its phases, against numpy's histogramdd path.

Clouds: the 1.7 M-point image cloud owl_interior (tests/golden/image_clouds.npz, z = 0) in a (9, 16, 2) box, and 10^7
normal random 3-D points in a (2, 2, 2) box. Grids 257^3, 513^3, 1025^3, each without and with ("-Z", "+Z", "-X").
Timed with HIP events (median of --reps; the host-returning calls and numpy at 1025^3 once, they allocate 8.6 GB):
  resident      to_image_resident, split into bin (memset + scatter), extent (flags pass + read-back), fill, and
                transfer (the float32 widening into the DeviceField);
  host_bytes    to_image with 1 B/voxel over PCIe, widened to float64 on the host (wall time, its transfer phase split);
  host_f64      to_image widened on the device, 8 B/voxel over PCIe;
  numpy         the reference's path: histogramdd > 0, astype(float), the extend fills (wall time, one CPU core).

    python tools/points_bench.py [--out profiles/points_bench.json] [--sizes 257,513,1025] [--reps 5]
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
EXTEND = ("-Z", "+Z", "-X")


def numpy_path(cloud, size, res, extend):
    import points_scenes
    return points_scenes.to_image_restated(cloud, size, res, extend)


def timed(fn, reps):
    phases, walls = [], []
    for _ in range(reps):
        t = {}
        t0 = time.perf_counter()
        out = fn(t)
        walls.append((time.perf_counter() - t0) * 1e3)
        phases.append(t)
        if hasattr(out, "free"):
            out.free()
        del out
    rec = {"wall_ms": float(np.median(walls)), "reps": reps}
    for k in phases[0]:
        rec[k + "_ms"] = float(np.median([p[k] for p in phases]))
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--sizes", default="257,513,1025")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-numpy", action="store_true")
    args = ap.parse_args()
    import __graft_entry__
    __graft_entry__.build()
    from aegolius_amd import _points
    owl = np.load(os.path.join(ROOT, "tests", "golden", "image_clouds.npz"))["owl_interior"]
    clouds = {"owl_interior_1.7M": (np.concatenate([owl, np.zeros((1, owl.shape[1]))]), (9, 16, 2)),
              "random_1e7": (np.random.default_rng(5).normal(0.0, 0.4, (3, 10 ** 7)), (2, 2, 2))}
    _points.to_image(clouds["random_1e7"][0][:, :1000], (2, 2, 2), (33, 33, 33), EXTEND)          # load the kernels
    results = []
    for cname, (cloud, size) in clouds.items():
        for r in [int(s) for s in args.sizes.split(",")]:
            res = (r, r, r)
            big = r > 600
            for extend in ((), EXTEND):
                rec = {"cloud": cname, "points": int(cloud.shape[1]), "res": r, "extend": list(extend)}
                rec["resident"] = timed(lambda t: _points.to_image(cloud, size, res, extend, resident=True, timings=t),
                                        args.reps)
                host_reps = 1 if big else args.reps
                rec["host_bytes"] = timed(lambda t: _points.to_image(cloud, size, res, extend, transfer="bytes",
                                                                     timings=t), host_reps)
                rec["host_f64"] = timed(lambda t: _points.to_image(cloud, size, res, extend, transfer="f64", timings=t),
                                        host_reps)
                if not args.no_numpy:
                    rec["numpy"] = timed(lambda t: numpy_path(cloud, size, res, extend), 1 if big else 3)
                if r <= 257:
                    assert np.array_equal(_points.to_image(cloud, size, res, extend), numpy_path(cloud, size, res, extend))
                print(json.dumps(rec), flush=True)
                results.append(rec)
    out = {"device": "MI355X", "timing": "HIP events per phase, wall clock for whole calls; medians",
           "default_transfer": _points.DEFAULT_TRANSFER, "results": results}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
