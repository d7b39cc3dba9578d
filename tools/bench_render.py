"""Sphere-tracing benchmark (aegolius_amd.render): one scene per call, so that a job can give every scene a
time limit of its own.
    python tools/bench_render.py cfg2 [--width 1920 --height 1080 --reps 7 --warmup 2 --modes interpret,nocull,specialised]
scenes: cfg2, cfg5, clustered, union<N> (union200, union1000, union4096, ...). Per kernel — interpreter / nocull (the
specialised kernel without the per-wave survivor lists: every member at every step) / specialised —: median ms per frame
from device events around the launch alone (outputs pre-allocated, kernel already built), the kernels timed ALTERNATELY
in one process after the warm-up of all of them; rays/s, point evaluations (sum of steps + 1 per ray + 4 per shaded hit)
and evaluations/s; unless --no-field the yardstick — the plain field kernel of the same program (MODE_INTERPRET /
MODE_NOCULL) on a (3, M) array of M = that many random points — and the ratio of the two rates; the wave efficiency of the
8 x 8 tile mapping against a row-major one, from the steps image. --stats adds the counters of the culled kernel's
statistics build (a build of its own, not the one that is timed) and the members a lane paid for per evaluation;
--rtc-defs passes -D switches to the kernel build (experiments). Prints one JSON line."""
import argparse
import contextlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

EYE = (2.2, 1.6, 1.9)


def scene(name):
    import aegolius_amd.cores as ns
    from aegolius_amd import workloads
    if name.startswith("union") and name[5:].isdigit():
        return workloads.sphere_union(ns, count=int(name[5:]))
    return {"cfg2": lambda: workloads.cfg2_tree(ns), "cfg5": lambda: workloads.cfg5_tree(ns),
            "clustered": lambda: workloads.clustered_union(ns)}[name]()


def wave_efficiency(steps):
    """sum(steps) / sum over waves of 64 max(steps in the wave): 8 x 8 tiles, and 64 consecutive pixels of the row-major
    order (the lanes a wave would get without the tile mapping). Pixels beyond the image count as idle lanes."""
    h, w = steps.shape
    total = float(steps.sum())
    padded = np.zeros(((h + 7) // 8 * 8, (w + 7) // 8 * 8), dtype=np.int64)
    padded[:h, :w] = steps
    tiles = padded.reshape(padded.shape[0] // 8, 8, padded.shape[1] // 8, 8).max(axis=(1, 3))
    flat = np.zeros((h * w + 63) // 64 * 64, dtype=np.int64)
    flat[:h * w] = steps.ravel()
    rows = flat.reshape(-1, 64).max(axis=1)
    return total / (64.0 * tiles.sum()), total / (64.0 * rows.sum())


def alternating_ms(launches, reps, warmup):
    """{name: launch} -> {name: (median ms, min ms)}: every kernel warmed up, then one timed launch of each in turn."""
    from aegolius_amd import _engine
    for launch in launches.values():
        for _ in range(warmup):
            launch()
    _engine.check(_engine.lib().sdfk_sync(None), "sdfk_sync")
    out = {name: [] for name in launches}
    for _ in range(reps):
        for name, launch in launches.items():
            a, b = _engine.Event(), _engine.Event()
            a.record()
            launch()
            b.record()
            _engine.check(_engine.lib().sdfk_sync(None), "sdfk_sync")
            out[name].append(a.elapsed_ms(b))
    return {name: (float(np.median(v)), float(min(v))) for name, v in out.items()}


def median_ms(launch, reps, warmup):
    return alternating_ms({"": launch}, reps, warmup)[""]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("scene")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--t-max", type=float, default=8.0)
    ap.add_argument("--max-steps", type=int, default=256)
    ap.add_argument("--modes", default="interpret,nocull,specialised")
    ap.add_argument("--no-field", action="store_true", help="skip the field-kernel yardstick")
    ap.add_argument("--stats", action="store_true", help="counters of the culled kernel (statistics build)")
    ap.add_argument("--rtc-defs", default="", help="-D switches for the kernel build")
    args = ap.parse_args()
    import __graft_entry__
    __graft_entry__.build()
    from aegolius_amd import _engine, render
    from aegolius_amd._eval import config, program_for
    _engine.require_gpu()
    L = _engine.lib()
    vp = _engine._vp
    if args.rtc_defs:
        L.sdfk_debug_set_rtc_defs(args.rtc_defs.encode())
    geo = scene(args.scene)
    low, _ = render.lower(geo)
    prog = program_for(low)
    cam = render.Camera(EYE, (0, 0, 0), (0, 0, 1), 40.0)
    W, H = args.width, args.height
    n = W * H
    eps, cone = cam.footprint(W, H)
    rec = cam.record(W, H)
    inv = float(np.float32(1.0 / low.lipschitz))
    result = {"scene": args.scene, "width": W, "height": H, "instructions": int(low.code.shape[0]), "lipschitz": low.lipschitz,
              "chain_members": prog.chain_members, "device": "MI355X (gfx950), 1 GPU", "rtc_defs": args.rtc_defs, "kernels": {}}
    ray_modes = {"interpret": _engine.MODE_INTERPRET, "nocull": _engine.MODE_NOCULL, "specialised": _engine.MODE_SPECIALIZED}
    field_modes = {"interpret": _engine.MODE_INTERPRET, "nocull": _engine.MODE_NOCULL, "specialised": _engine.MODE_NOCULL}
    names = args.modes.split(",")
    with contextlib.ExitStack() as stack:
        t, normals, d_status, d_steps = render._outputs(stack, stack, n, True)

        def launcher(ray_mode):
            def launch():
                _engine.check(L.sdfk_trace_camera_device(prog.handle, _engine._ptr(rec), W, H, 0, 0.0, float(np.float32(args.t_max)),
                                                         float(np.float32(eps)), float(np.float32(cone)), inv, args.max_steps,
                                                         vp(t.ptr), d_status.at(), d_steps.at(), vp(normals.ptr),
                                                         normals.stride, None, ray_mode), "sdfk_trace_camera_device")
            return launch
        build = prog.compile_flavour(_engine.FLAVOUR_RAYS) if set(names) & {"nocull", "specialised"} else None
        times = alternating_ms({name: launcher(ray_modes[name]) for name in names}, args.reps, args.warmup)
        for name in names:
            k = {}
            if build and name != "interpret":
                k["build_bytes"], k["build_seconds"] = build
            k["ms"], k["ms_min"] = times[name]
            launcher(ray_modes[name])()
            status, steps = render._small(n, d_status, d_steps)
            evals = int(steps.sum()) + n + 4 * int(np.count_nonzero(status == render.HIT))
            k.update(rays_per_s=n / (k["ms"] * 1e-3), evaluations=evals, evaluations_per_s=evals / (k["ms"] * 1e-3),
                     hits=int(np.count_nonzero(status == render.HIT)), step_limit=int(np.count_nonzero(status == render.LIMIT)),
                     mean_steps=float(steps.mean()), max_steps=int(steps.max()))
            k["wave_efficiency_tiles"], k["wave_efficiency_rows"] = wave_efficiency(steps.reshape(H, W))
            if not args.no_field:
                # yardstick: the plain field kernel of the same program on as many points
                rng = np.random.default_rng(1)
                co = _engine.DeviceVectorField.from_host(rng.uniform(-1.0, 1.0, (3, evals)).astype(np.float32), config.device)
                field = _engine.DeviceField(evals, config.device)
                try:
                    def plain():
                        prog.eval_device(co.row_ptr(0), evals, co.stride, field.ptr, mode=field_modes[name])
                    k["field_ms"], _ = median_ms(plain, args.reps, args.warmup)
                finally:
                    co.free()
                    field.free()
                k["field_points_per_s"] = evals / (k["field_ms"] * 1e-3)
                k["ratio_to_field_kernel"] = k["evaluations_per_s"] / k["field_points_per_s"]
            result["kernels"][name] = k
        if args.stats and prog.chain_members:
            import ctypes
            L.sdfk_debug_set_rtc_defs((args.rtc_defs + " -DSDFK_DEBUG_RAYSTATS=1").strip().encode())
            out8 = (ctypes.c_longlong * 8)()
            L.sdfk_debug_rays_stats(1, out8)
            launcher(_engine.MODE_SPECIALIZED)()
            L.sdfk_debug_rays_stats(0, out8)
            L.sdfk_debug_set_rtc_defs(args.rtc_defs.encode())
            c = dict(zip(("builds", "build_evaluations", "survivor_evaluations", "plain_evaluations", "splits",
                          "point_evaluations"), (int(v) for v in out8)))
            if c["point_evaluations"]:
                c["members_per_evaluation"] = ((c["build_evaluations"] + c["survivor_evaluations"] +
                                                prog.chain_members * c["plain_evaluations"]) / 64.0 / c["point_evaluations"])
            result["cull_stats"] = c
    print(json.dumps(result))


if __name__ == "__main__":
    t0 = time.time()
    main()
    print("# %.1f s" % (time.time() - t0), file=sys.stderr)
