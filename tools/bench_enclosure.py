"""Enclosure benchmark (aegolius_amd.enclosure). No number in it is a pass criterion.
    python tools/bench_enclosure.py [--boxes 1048576 --reps 7 --warmup 2 --inner 1024 --out profiles/enclosure_bench.txt]
For cfg2, cfg3 and cfg5 (their BASELINE boxes), device events, the median of `reps` timed windows after `warmup` untimed ones,
for every row alike:
  * boxes per second of sdfk_enclose_boxes_device on `boxes` random boxes of the domain with half widths of 1/128 of it (the
    launch alone: boxes and factor table resident). One launch takes tens of microseconds, so a window holds `inner`
    back-to-back launches and the row states the window and the time per launch;
  * time and bracket width of volume_bounds at depths 6 .. 9 (the whole public call: lowering, allocation, one launch and one
    read-back of the counters per level), one call per window;
  * of the 64^3 bricks of 8^3 grid intervals of a 513^3 grid, the share classify() leaves mixed, next to the share the
    Lipschitz rule |f(c)| <= L rho leaves undecided (rho the brick's half diagonal; 1.0 by construction where L is infinite).
Writes the table to --out and prints it."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(call, reps, warmup):
    from aegolius_amd import _engine
    out, result = [], None
    for i in range(warmup + reps):
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
    ap.add_argument("--boxes", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--inner", type=int, default=1024, help="launches per timed window of the kernel rows")
    ap.add_argument("--depths", type=int, nargs="*", default=[6, 7, 8, 9])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "enclosure_bench.txt"))
    args = ap.parse_args()
    import __graft_entry__
    __graft_entry__.build()
    import aegolius_amd.cores as ns
    from aegolius_amd import _engine, enclosure, workloads
    _engine.require_gpu()
    lines = ["enclosure benchmark: MI355X (gfx950), 1 GPU; device events, every row the median of %d windows after %d warm-up "
             "windows (enclose: %d launches per window; volume_bounds: one call per window)" % (args.reps, args.warmup, args.inner)]
    for name in ("cfg2", "cfg3", "cfg5"):
        geo, size, desc = workloads.build(name, ns)
        half = np.array(size) / 2.0
        rng = np.random.default_rng(11)
        n = args.boxes
        c = rng.uniform(-half[:, None], half[:, None], (3, n))
        h = half[:, None] / 128.0
        lo32, hi32 = enclosure._boxes(c - h, c + h)
        with enclosure._Enclosed(geo) as enc, _engine.DeviceRows(3, n) as d_lo, _engine.DeviceRows(3, n) as d_hi, \
                _engine.DeviceBuffer(8 * n) as d_out:
            d_lo.upload_rows(lo32)
            d_hi.upload_rows(hi32)

            def launch():
                for _ in range(args.inner):
                    _engine.check(_engine.lib().sdfk_enclose_boxes_device(enc.prog.handle, d_lo.at(), d_hi.at(), n, d_lo.stride,
                                                                          enc.d_factors.at(), d_out.at(0, 4 * n),
                                                                          d_out.at(4 * n, 4 * n), None), "sdfk_enclose_boxes_device")
            window, window_min, _ = timed(launch, args.reps, args.warmup)
            ms, ms_min = window / args.inner, window_min / args.inner
            instr = len(enc.low.code)
            L = float(enc.low.lipschitz)
        lines.append("")
        lines.append("%s  (%d instructions, Lipschitz bound %g)" % (desc, instr, L))
        lines.append("  enclose: %d boxes in %.4f ms per launch (min %.4f; window of %d launches %.3f ms) = %.3e boxes/s"
                     % (n, ms, ms_min, args.inner, window, n / (ms * 1e-3)))
        for depth in args.depths:
            try:
                ms, ms_min, v = timed(lambda: enclosure.volume_bounds(geo, size, depth=depth), args.reps, args.warmup)
                lines.append("  volume_bounds depth %d: %.2f ms (min %.2f), [%.9g, %.9g], width %.4g, %d mixed leaves"
                             % (depth, ms, ms_min, v.lower, v.upper, v.width, v.mixed[-1]))
            except ValueError as exc:
                lines.append("  volume_bounds depth %d: %s" % (depth, exc))
        # bricks of 8^3 intervals of a 513^3 grid
        status = enclosure.classify(geo, size, (64, 64, 64))
        mixed = float(np.mean(status == 0))
        if np.isfinite(L):
            blo, bhi, _ = enclosure.subdivision(size, (64, 64, 64))
            centre = (np.float32(0.5) * blo + np.float32(0.5) * bhi).astype(np.float64)
            rho = np.sqrt(np.sum(np.maximum(bhi - centre, centre - blo) ** 2, axis=0))
            fc = np.asarray(workloads.build(name, ns)[0].create(centre), dtype=np.float64)
            undecided = float(np.mean(np.abs(fc) <= L * rho))
        else:
            undecided = 1.0
        lines.append("  513^3 grid, 64^3 bricks of 8^3 intervals: classify leaves %.4f mixed; the Lipschitz rule leaves %.4f undecided"
                     % (mixed, undecided))
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
