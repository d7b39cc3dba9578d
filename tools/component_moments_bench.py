"""Component-moments benchmark (aegolius_amd.topology, Components.moments): the pass over the labels against
the records pass of the same labelling and against the route users had before it.
    python tools/component_moments_bench.py [cfg2:513 cfg5:513 union1000:513 noise0.31:513] [--reps 5 --warmup 1
                                             --host-reps 1 --out profiles/component_moments_bench.txt]
Per case `scene:n` (the scenes of tools/bench_topology.py), in one process, MODE_SPECIALIZED, on the tables of
generate_grid(box, (n, n, n)); noise is a host field of +-1 at the given inside density, uploaded once. One labelling
(inside, faces), then medians of `reps` calls after `warmup`, device events around each call:
  * moments_ms: sdfk_label_moments — the pass over the labels with the allocation and the download of the K rows;
    rows_io_ms: an allocation of the rows' bytes and their download into a fresh host array alone — the part of
    moments_ms that is not the pass (the rows of 7 M components are 578 MB);
  * records_ms: sdfk_label_finish on the same labels — the records pass with ITS allocation and download;
    moments_over_records is their ratio;
  * the route before: labels_host() (4 bytes per point over the bus; download_ms, device events) and
    tests/component_moments_reference.py on the host (host_sums_ms, wall clock, median of --host-reps); old_over_new =
    (download_ms + host_sums_ms) / moments_ms. `same` says that the host's rows equal the device's bit for bit.
Writes a header and one JSON line per case to --out and prints them."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

HEADER = """# tools/component_moments_bench.py, one MI355X (gfx950), median of %d after %d warm-up(s), all cases in one process
# scene:n = the scene on generate_grid(box, (n, n, n)); noise: a resident field of +-1; one labelling (inside, faces). Milliseconds,
# device events around each call. moments_ms: sdfk_label_moments with the rows' allocation and download (rows_io_ms: an
# allocation and a download of that size alone, into a fresh host array); records_ms:
# sdfk_label_finish of the same labelling with the records' allocation and download; moments_over_records their ratio
# route before: download_ms = labels_host(), host_sums_ms = tests/component_moments_reference.py (wall clock, median of %d)
# old_over_new = (download_ms + host_sums_ms) / moments_ms; same: the host's rows equal the device's bit for bit
"""


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("cases", nargs="*", default=["cfg2:513", "cfg5:513", "union1000:513", "noise0.31:513"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--host-reps", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "component_moments_bench.txt"))
    args = ap.parse_args()
    import __graft_entry__
    __graft_entry__.build()
    import aegolius_amd.cores as ns
    import component_moments_reference
    from aegolius_amd import _engine, topology, workloads
    from aegolius_amd._eval import config, program_for
    from aegolius_amd._lower import lower_geometry
    from aegolius_amd.cores.helper_functions import grid_axes
    from bench_topology import timed
    _engine.require_gpu()
    config.mode = _engine.MODE_SPECIALIZED
    lines = [HEADER % (args.reps, args.warmup, args.host_reps)]
    for case in args.cases:
        name, n = case.split(":")
        n = int(n)
        if name.startswith("noise"):
            rng = np.random.default_rng(31)
            field = np.where(rng.random((n, n, n)) < float(name[5:]), np.float32(-1), np.float32(1)).astype(np.float32)
            source, box = _engine.DeviceField.from_host(field.ravel(), config.device), (2, 2, 2)
            del field
        else:
            geo, box = (workloads.sphere_union(ns, count=int(name[5:])), (2, 2, 2)) if name.startswith("union") \
                else workloads.build(name, ns)[:2]
            geo._sdf = geo.modified_object
            source = program_for(lower_geometry(geo))
        tables = topology._axes(grid_axes(box, (n, n, n))[0])
        shape = tuple(t.size for t in tables)
        result = {"case": case, "points": int(np.prod(shape, dtype=np.int64))}
        with _engine.LabelScratch(tables, config.device) as scratch, scratch.labels() as labels:
            count = scratch.label(source, 0.0, _engine.CONNECT_FACES, _engine.REGION_INSIDE, labels, config.mode)
            records_ms, _, records = timed(lambda: scratch.records(count, labels), args.reps, args.warmup)
            moments_ms, _, sums = timed(lambda: _engine.label_moments(labels, shape, count), args.reps, args.warmup)

            def rows_io():                                     # what the call does besides the pass over the labels
                with _engine.DeviceBuffer(max(sums.nbytes, 8), config.device, "rows") as rows:
                    return rows.download(np.zeros_like(sums))
            rows_io_ms, _, _ = timed(rows_io, args.reps, args.warmup)
            host = np.empty(shape, dtype=np.int32)
            download_ms, _, _ = timed(lambda: labels.download(host), max(1, args.reps // 2), 1)
        walls = []
        for _ in range(args.host_reps):
            t0 = time.perf_counter()
            want = component_moments_reference.sums(host, count)
            walls.append((time.perf_counter() - t0) * 1e3)
        result.update(components=count, largest=int(records[1].max(initial=0)), row_bytes=int(sums.nbytes),
                      moments_ms=moments_ms, rows_io_ms=rows_io_ms, records_ms=records_ms,
                      moments_over_records=moments_ms / records_ms,
                      download_ms=download_ms, host_sums_ms=float(np.median(walls)),
                      old_over_new=(download_ms + float(np.median(walls))) / moments_ms,
                      same=bool(sums.dtype == want.dtype and np.array_equal(sums, want)),
                      sizes_agree=bool(np.array_equal(records[1], sums[:, 0].astype(np.int64))))
        if isinstance(source, _engine.DeviceField):
            source.free()
        del host, want, sums
        lines.append(json.dumps(result) + "\n")
        print(lines[-1], end="", flush=True)
        with open(args.out, "w") as f:                         # (after every case: a time limit leaves the finished ones)
            f.writelines(lines)


if __name__ == "__main__":
    main()
