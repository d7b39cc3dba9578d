"""Times of the reverse-mode (adjoint) kernel against the forward-mode launches the same gradient needs, on BASELINE cfg 2
(10-member SMOOTH_UNION2 chain) with its 31 natural primals: the 10 centres (x, y, z) and the smoothing width.

    python tools/adjoint_bench.py [--sizes 513,1025] [--reps 5] [--out profiles/adjoint_bench.json]

Per grid size, coordinates resident (filled on the device from the axis tables), device events around the kernel calls
only, warm-up first, median of the repetitions (the methods of tools/autodiff_bench.py):
  * vjp with respect to m = 1, 4, 8 and 31 primals (one adjoint launch each; the cotangent is 1 at every point) against
    the ceil(m / 4) forward launches (K <= 4) of the same channels — the crossover in m;
  * value_and_grad_sse for all 31 primals (cotangent 2 (f - t) and the float64 loss formed in the same launch).
At the first size the 31-primal gradient is checked in the tool: c = 1 against the float64 sums of the forward tangents,
one channel at a time. Host time (the 2m + 1 lowerings of parameter_tangents and the chain rule) is reported apart.
Writes one JSON file.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="513,1025")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adjoint_bench.json"))
    args = ap.parse_args()

    import __graft_entry__
    __graft_entry__.build()
    import aegolius_amd.cores as ns
    from aegolius_amd.cores.helper_functions import grid_axes
    from aegolius_amd import _engine, _eval, autodiff as ad, workloads

    _engine.require_gpu()
    L = _engine.lib()
    vp = _engine._vp

    def cfg2(width, centres):
        prims = workloads._cfg2_prims(ns, np.random.default_rng(1234), 10)
        for k, o in enumerate(prims):
            o.set_location(np.asarray(centres[3 * k:3 * k + 3], dtype=np.float64))
        acc = prims[0]
        for o in prims[1:]:
            acc = ns.CombineGeometry("SMOOTH_UNION2").combine_parametric(acc, o, parameters=width)
        return acc

    centres = np.concatenate([np.asarray(o.center, dtype=np.float64).ravel()
                              for o in workloads._cfg2_prims(ns, np.random.default_rng(1234), 10)])
    primals = (0.1, centres)
    # m channels: the width, then the centre coordinates in order
    cases = {1: 0, 4: (0, 1), 8: (0, 1), 31: (0, 1)}

    def rows_for(m):
        t0 = time.perf_counter()
        low, origin, rows, _chans, layout = ad.parameter_tangents(cfg2, primals, cases[m])
        host = time.perf_counter() - t0
        return low, origin, rows[:m], host

    def timed(fn, reps):
        for _ in range(2):
            fn()
        fn()
        _engine.check(L.sdfk_sync(None), "sync")
        ts = []
        for _ in range(reps):
            a, b = _engine.Event(), _engine.Event()
            a.record()
            fn()
            b.record()
            ts.append(a.elapsed_ms(b))
        return float(np.median(ts)), [round(t, 3) for t in ts]

    results = {"workload": "BASELINE cfg 2 (10-member SMOOTH_UNION2 chain), grid over [-1, 1]^3, primals: width + 10 "
                           "centres (31)", "runs": []}
    prepared = {m: rows_for(m) for m in cases}
    low, origin, rows31, host31 = prepared[31]
    prog = ad._adjoint_program(low, origin)
    ns_ = low.params.size
    for size in [int(s) for s in args.sizes.split(",")]:
        axes, _res = grid_axes((2, 2, 2), (size - 1,) * 3)

        class co:                                              # what autodiff takes for a generate_grid array
            grid_axes = axes
        n = int(np.prod([a.size for a in axes]))
        run = {"size": size, "points": n, "n_params": ns_, "tape_floats_per_point": None}
        coords = _eval.device_coords(co)
        d_c = _engine.DeviceField.from_host(np.ones(n, dtype=np.float32))
        d_v = L.sdfk_malloc(n * 4)
        d_t = L.sdfk_malloc(4 * coords.stride * 4)
        pbar = np.zeros(ns_)
        loss = __import__("ctypes").c_double(0.0)
        try:
            tape = __import__("ctypes").c_int64(0)
            L.sdfk_program_vjp_check(prog.handle, None, __import__("ctypes").byref(tape))
            run["tape_floats_per_point"] = tape.value

            def reverse(mode):
                _engine.check(L.sdfk_eval_vjp_device(prog.handle, vp(coords.ptr), n, coords.stride, vp(d_c.ptr), mode, 0,
                                                     vp(d_v), _engine._ptr(pbar), __import__("ctypes").byref(loss), None),
                              "vjp")
            run["vjp_ms"], run["vjp_all"] = timed(lambda: reverse(0), args.reps)
            run["sse_ms"], run["sse_all"] = timed(lambda: reverse(1), args.reps)
            for m in (1, 4, 8, 31):
                lw, og, rw, host = prepared[m]
                pr = ad._program(lw, og)
                dP = np.ascontiguousarray(rw, dtype=np.float32)
                d_dp = L.sdfk_malloc(max(dP.size, 1) * 4)
                _engine.check(L.sdfk_memcpy_h2d(vp(d_dp), _engine._ptr(dP), dP.size * 4), "h2d")

                def forward():
                    for g in range(0, m, 4):
                        k = min(4, m - g)
                        _engine.check(L.sdfk_eval_jvp_device(pr.handle, vp(coords.ptr), n, coords.stride,
                                                             vp(d_dp + 4 * g * ns_), k, 0, vp(d_v), vp(d_t),
                                                             coords.stride, None), "jvp")
                ms, allt = timed(forward, args.reps)
                run["forward_m%d_ms" % m] = ms
                run["forward_m%d_all" % m] = allt
                run["forward_m%d_launches" % m] = (m + 3) // 4
                run["reverse_over_forward_m%d" % m] = round(run["vjp_ms"] / ms, 3)
                run["host_parameter_tangents_m%d_s" % m] = round(host, 4)
                if m == 31 and size == int(args.sizes.split(",")[0]):
                    # in-tool check: c = 1 -> θ̄_k = Σ_i ∂f_i/∂θ_k, against the float64 sums of the forward tangents
                    reverse(0)
                    t0 = time.perf_counter()
                    g = rows31.dot(pbar)
                    run["host_chain_rule_s"] = round(time.perf_counter() - t0, 6)
                    want = np.zeros(31)
                    scale = np.zeros(31)
                    t = np.empty(n, dtype=np.float32)
                    for ch in range(31):
                        grp, k = divmod(ch, 4)
                        kk = min(4, 31 - 4 * grp)
                        _engine.check(L.sdfk_eval_jvp_device(pr.handle, vp(coords.ptr), n, coords.stride,
                                                             vp(d_dp + 4 * 4 * grp * ns_), kk, 0, vp(d_v), vp(d_t),
                                                             coords.stride, None), "jvp")
                        _engine.check(L.sdfk_memcpy_d2h(_engine._ptr(t), vp(d_t + 4 * k * coords.stride), n * 4), "d2h")
                        want[ch] = np.sum(t, dtype=np.float64)
                        scale[ch] = np.sum(np.abs(t), dtype=np.float64)
                    err = np.abs(g - want) / (scale + 1e-30)
                    run["check_max_err_over_sum_abs"] = float(err.max())
                    run["check_passed"] = bool(np.all(np.abs(g - want) <= 1e-5 * scale + 1e-7))
                L.sdfk_free(vp(d_dp))
            print(json.dumps(run))
            results["runs"].append(run)
        finally:
            coords.free()
            d_c.free()
            L.sdfk_free(vp(d_v))
            L.sdfk_free(vp(d_t))
    results["host_parameter_tangents_m31_s"] = round(host31, 4)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(results, f, indent=1)
    print("wrote", args.out)
    if not all(r.get("check_passed", True) for r in results["runs"]):
        sys.exit(1)


if __name__ == "__main__":
    main()
