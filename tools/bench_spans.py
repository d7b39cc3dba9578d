"""Span-march benchmark (aegolius_amd.render.thickness): one scene per call.
    python tools/bench_spans.py cfg2 [--width 1920 --height 1080 --reps 7 --warmup 2]
scenes: cfg2, cfg5, union<N>. The perspective camera of tools/bench_render.py. Two kernels of the same build in the same
process, timed ALTERNATELY after the warm-up of both, device events around the launch alone (outputs pre-allocated, kernels
already built): `first_hit`, the camera kernel of render(normals=False), and `thickness`, the span kernel with K = 0 — both
with the pixel's footprint as the threshold (the span march's eps raised to its floor, as thickness() does). A chain-mode
scene (the unions) is timed culled (MODE_SPECIALIZED) and without the survivor lists (MODE_NOCULL). Per kernel: median and
smallest ms per frame, the sum of steps + 1 over the image, the evaluations (first hit: steps + 1 for a hit, steps otherwise;
spans: steps), the WAVE evaluations — the sum over the 8 x 8 tiles of the most evaluations of a ray in the tile, which is the
trip count of that wave's loop — and ns per wave evaluation = frame time / wave evaluations. Prints one JSON line."""
import argparse
import contextlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def wave_evaluations(evals):
    h, w = evals.shape
    padded = np.zeros(((h + 7) // 8 * 8, (w + 7) // 8 * 8), dtype=np.int64)
    padded[:h, :w] = evals
    return int(padded.reshape(padded.shape[0] // 8, 8, padded.shape[1] // 8, 8).max(axis=(1, 3)).sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("scene")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--t-max", type=float, default=8.0)
    ap.add_argument("--max-steps", type=int, default=1024)
    args = ap.parse_args()
    import __graft_entry__
    __graft_entry__.build()
    import bench_render
    from aegolius_amd import _engine, render
    from aegolius_amd._eval import program_for
    _engine.require_gpu()
    L = _engine.lib()
    vp = _engine._vp
    geo = bench_render.scene(args.scene)
    low, _ = render.lower(geo)
    prog = program_for(low)
    cam = render.Camera(bench_render.EYE, (0, 0, 0), (0, 0, 1), 40.0)
    W, H = args.width, args.height
    n = W * H
    fe, cone = cam.footprint(W, H)
    t_min, t_max, eps, cone, max_steps, _ = render._span_options(
        0.0, args.t_max, max(fe, float(np.nextafter(np.float32(render.SPAN_EPS_FLOOR * args.t_max), np.float32(np.inf)))), cone,
        args.max_steps, 0)
    rec = cam.record(W, H)
    inv = float(np.float32(1.0 / low.lipschitz))
    result = {"scene": args.scene, "width": W, "height": H, "instructions": int(low.code.shape[0]), "chain_members": prog.chain_members,
              "max_steps": max_steps, "eps": eps, "cone": cone, "device": "MI355X (gfx950), 1 GPU", "kernels": {}}
    modes = {"specialised": _engine.MODE_SPECIALIZED}
    if prog.chain_members:
        modes["nocull"] = _engine.MODE_NOCULL
    result["build_first_hit"] = prog.compile_flavour(_engine.FLAVOUR_RAYS)
    result["build_thickness"] = prog.compile_flavour(_engine.FLAVOUR_SPANS)
    with contextlib.ExitStack() as stack:
        t, _, d_status, d_steps = render._outputs(stack, stack, n, False)
        chord, _, d_count, s_status, s_steps = render._span_outputs(stack, stack, n, 0)

        def first_hit(m):
            def launch():
                _engine.check(L.sdfk_trace_camera_device(prog.handle, _engine._ptr(rec), W, H, 0, t_min, t_max, float(np.float32(fe)),
                                                         cone, inv, max_steps, vp(t.ptr), d_status.at(), d_steps.at(), None, 0, None,
                                                         m), "sdfk_trace_camera_device")
            return launch

        def thickness(m):
            def launch():
                _engine.check(L.sdfk_span_camera_device(prog.handle, _engine._ptr(rec), W, H, 0, t_min, t_max, eps, cone, inv,
                                                        max_steps, vp(chord.ptr), d_count.at(), s_status.at(), s_steps.at(), None, 0,
                                                        0, None, m), "sdfk_span_camera_device")
            return launch
        launches = {}
        for name, m in modes.items():
            launches["first_hit/" + name] = first_hit(m)
            launches["thickness/" + name] = thickness(m)
        times = bench_render.alternating_ms(launches, args.reps, args.warmup)
        for name, launch in launches.items():
            launch()
            _engine.check(L.sdfk_sync(None), "sdfk_sync")
            k = {"ms": times[name][0], "ms_min": times[name][1]}
            if name.startswith("first_hit"):
                status, steps = render._small(n, d_status, d_steps)
                evals = steps.astype(np.int64) + (status == render.HIT)
                k["hits"] = int(np.count_nonzero(status == render.HIT))
            else:
                status, steps = render._small(n, s_status, s_steps)
                evals = steps.astype(np.int64)
                k["crossings"] = int(d_count.download(np.empty(n, dtype=np.int32)).sum(dtype=np.int64))
                k["chord_sum"] = float(chord.numpy().sum(dtype=np.float64))
            k["step_limit"] = int(np.count_nonzero((status & 3) == render.LIMIT))
            k["sum_steps_plus_1"] = int(steps.sum(dtype=np.int64)) + n
            k["evaluations"] = int(evals.sum())
            k["wave_evaluations"] = wave_evaluations(evals.reshape(H, W))
            k["ns_per_wave_evaluation"] = k["ms"] * 1e6 / k["wave_evaluations"]
            k["max_evaluations"] = int(evals.max())
            result["kernels"][name] = k
        for name in modes:
            a, b = result["kernels"]["thickness/" + name], result["kernels"]["first_hit/" + name]
            result["cost_per_wave_evaluation_ratio/" + name] = a["ns_per_wave_evaluation"] / b["ns_per_wave_evaluation"]
    print(json.dumps(result))


if __name__ == "__main__":
    main()
