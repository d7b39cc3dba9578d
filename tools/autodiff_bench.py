"""Times of the forward-mode derivative kernel next to create() on BASELINE cfg 2 (10-member SMOOTH_UNION2 chain).

    python tools/autodiff_bench.py [--sizes 513,1025] [--reps 5] [--out profiles/autodiff_bench.json]

Per grid size: create() (the culled, specialised evaluation into a resident field), the dual kernel with K = 1 (d/d
smoothing width), K = 4 (width + the first primitive's offset x, y, z) and point mode (K = 3, spatial gradient). Device
events around the kernel calls only (coordinates already resident, filled on the device from the axis tables); warm-up
first, median of the repetitions. A sample of the K = 1 tangents is checked against a float64 central difference of the
oracle. Writes one JSON file.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="513,1025")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "autodiff_bench.json"))
    args = ap.parse_args()

    import __graft_entry__
    __graft_entry__.build()
    import aegolius_amd.cores as ns
    from aegolius_amd.cores.helper_functions import grid_axes
    from aegolius_amd import _engine, _eval, autodiff as ad, workloads
    from aegolius_amd._lower import lower_geometry
    from oracle import sdf_oracle

    _engine.require_gpu()
    L = _engine.lib()
    vp = _engine._vp

    def cfg2(w, x0=None):
        tree = workloads.cfg2_tree(ns, width=w)
        if x0 is not None:                                # the first primitive's offset as parameters
            first = tree
            while hasattr(first.modified_object, "children"):
                first = first.modified_object.children[0]
            first.set_location(np.asarray(x0, dtype=np.float64))
        return tree

    def first_centre():
        tree = workloads.cfg2_tree(ns)
        first = tree
        while hasattr(first.modified_object, "children"):
            first = first.modified_object.children[0]
        return np.asarray(first.center, dtype=np.float64).ravel()

    c0 = first_centre()
    width = 0.1
    results = {"workload": "BASELINE cfg 2 (10-member SMOOTH_UNION2 chain), grid over [-1, 1]^3", "runs": []}

    def timed(fn, reps):
        for _ in range(2):
            fn()
        L.sdfk_jit_drain()
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

    for size in [int(s) for s in args.sizes.split(",")]:
        axes, _res = grid_axes((2, 2, 2), (size - 1,) * 3)     # the tables of generate_grid, without its (3, N) array

        class co:                                              # what autodiff takes for a generate_grid array
            grid_axes = axes
        n = int(np.prod([a.size for a in axes]))
        run = {"size": size, "points": n}
        # create(): the evaluation the package runs for this tree, field left in HBM
        tree = cfg2(width)
        prog = _eval.program_for(lower_geometry(tree))
        field = _engine.DeviceField(n)
        run["create_ms"], run["create_all"] = timed(lambda: prog.eval_grid(axes, 0, n, field.ptr), args.reps)
        field.free()
        coords = _eval.device_coords(co)
        stride = coords.stride
        d_v = L.sdfk_malloc(n * 4)
        d_t = L.sdfk_malloc(4 * stride * 4)
        try:
            cases = []
            low, origin, rows, _c, _l = ad.parameter_tangents(lambda w: cfg2(w), (width,), 0)
            cases.append(("jvp_k1_width", low, origin, rows, False))
            low4, origin4, rows4, _c, _l = ad.parameter_tangents(lambda w, x: cfg2(w, x), (width, c0), (0, 1))
            cases.append(("jvp_k4_width_offset", low4, origin4, rows4, False))
            lowp, originp = ad._lower(tree, shortcuts=True)
            cases.append(("grad_points_k3", lowp, originp, np.zeros((3, lowp.params.size)), True))
            for name, lw, og, rw, seed in cases:
                pr = ad._program(lw, og)
                dP = np.ascontiguousarray(rw, dtype=np.float32)
                d_dp = L.sdfk_malloc(max(dP.size, 1) * 4)
                _engine.check(L.sdfk_memcpy_h2d(vp(d_dp), _engine._ptr(dP), dP.size * 4), "h2d")

                def launch():
                    _engine.check(L.sdfk_eval_jvp_device(pr.handle, vp(coords.ptr), n, coords.stride, vp(d_dp), dP.shape[0],
                                                         1 if seed else 0, vp(d_v), vp(d_t), stride, None), "jvp")
                ms, allt = timed(launch, args.reps)
                L.sdfk_free(vp(d_dp))
                k = dP.shape[0]
                run[name + "_ms"] = ms
                run[name + "_all"] = allt
                run[name + "_GBps"] = round(n * (12 + 4 * (1 + k)) / ms / 1e6, 1)
                run[name + "_vs_create"] = round(ms / run["create_ms"], 2)
                if name == "jvp_k1_width":
                    # oracle check on a sample: float64 central difference in the width
                    launch()
                    t = np.empty(n, dtype=np.float32)
                    _engine.check(L.sdfk_memcpy_d2h(_engine._ptr(t), vp(d_t), n * 4), "d2h")
                    idx = np.random.default_rng(0).choice(n, 2000, replace=False)
                    ix, iy, iz = np.unravel_index(idx, tuple(a.size for a in axes))
                    pts = np.stack([np.asarray(axes[0], np.float32)[ix], np.asarray(axes[1], np.float32)[iy],
                                    np.asarray(axes[2], np.float32)[iz]]).astype(np.float64)
                    h = 1e-6
                    D = (sdf_oracle.evaluate(cfg2(width + h), pts) - sdf_oracle.evaluate(cfg2(width - h), pts)) / (2 * h)
                    err = np.abs(t[idx] - D) / np.maximum(1.0, np.abs(D))
                    run["k1_sample_max_err"] = float(np.max(err))
                    run["k1_sample_p99_err"] = float(np.percentile(err, 99))
            print(json.dumps(run))
            results["runs"].append(run)
        finally:
            coords.free()
            L.sdfk_free(vp(d_v))
            L.sdfk_free(vp(d_t))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(results, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
