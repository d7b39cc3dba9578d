"""Topology benchmark (aegolius_amd.topology): labelling by phase, betti and cell_counts, against the bits pass
alone (the floor) and against the route users had before the module.
    python tools/bench_topology.py [cfg2:513 cfg5:513 union1000:257 union1000:513 noise0.31:513] [--reps 5 --warmup 1
                                    --host-limit 513 --out profiles/topology_bench.txt]
Per case `scene:n`, in one process (MODE_SPECIALIZED: the builds are waited for in the warm-up), on the tables of
generate_grid(box, (n, n, n)); noise is a host field of +-1 at the given inside density, uploaded once. Medians of `reps`
calls after `warmup`:
  * bits / init / merge / compress / number: the passes of one labelling call (inside, faces), device events inside the
    library; reduce: the finishing call with the download of the records, device events around it; label_ms their sum;
    label_over_bits = label_ms / bits (the bits pass alone is the floor: it is all a field-free consumer must do);
  * label_full_ms: the same labelling under full connectivity (passes added up, with reduce);
  * betti_ms, cells_ms: topology.betti / topology.cell_counts, device events around the whole public call;
  * the route without this module: create_resident + download of the field (field_ms, device events around both) and a
    host labelling of the downloaded field (host_label_ms, wall clock; scipy.ndimage.label when scipy is there, else
    tests/topology_reference.py — `host_labeller` says which), for n <= --host-limit; old_over_new = (field_ms +
    host_label_ms) / label_ms. The host's component count is compared with the device's.
Writes a header and one JSON line per case to --out and prints them."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HEADER = """# tools/bench_topology.py, one MI355X (gfx950), median of %d after %d warm-up(s), all cases in one process, MODE_SPECIALIZED
# scene:n = the scene on generate_grid(box, (n, n, n)); noise: a resident field of +-1. Milliseconds. bits .. number: device
# events inside the labelling call (inside, faces); reduce: the finishing call with the records' download; label_ms: their sum
# label_over_bits = label_ms / bits; label_full_ms: full connectivity; betti_ms / cells_ms: the whole public call
# old route: field_ms = create_resident + download, host_label_ms = %s on the host (wall clock)
# old_over_new = (field_ms + host_label_ms) / label_ms; bytes per point: 4 (labels) + scratch_bytes_per_point
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


def host_labeller():
    """-> (name, f(mask) -> component count) of the host labelling of the old route (faces connectivity)."""
    try:
        from scipy import ndimage
        return "scipy.ndimage.label", lambda mask: int(ndimage.label(mask)[1])
    except ImportError:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import topology_reference
        return "tests/topology_reference.py", lambda mask: int(topology_reference.label(mask, "faces").count)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("cases", nargs="*", default=["cfg2:513", "cfg5:513", "union1000:257", "union1000:513", "noise0.31:513"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--host-limit", type=int, default=513)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "topology_bench.txt"))
    args = ap.parse_args()
    import __graft_entry__
    __graft_entry__.build()
    import aegolius_amd.cores as ns
    from aegolius_amd import _engine, topology, workloads
    from aegolius_amd._eval import config, program_for
    from aegolius_amd._lower import lower_geometry
    from aegolius_amd.cores.helper_functions import grid_axes
    _engine.require_gpu()
    config.mode = _engine.MODE_SPECIALIZED
    labeller_name, labeller = host_labeller()
    lines = [HEADER % (args.reps, args.warmup, labeller_name)]
    for case in args.cases:
        name, n = case.split(":")
        n = int(n)
        geo, field = None, None
        if name.startswith("noise"):
            box = (2, 2, 2)
            rng = np.random.default_rng(31)
            field = np.where(rng.random((n, n, n)) < float(name[5:]), np.float32(-1), np.float32(1)).astype(np.float32)
        elif name.startswith("union"):
            geo, box = workloads.sphere_union(ns, count=int(name[5:])), (2, 2, 2)
        else:
            geo, box, _ = workloads.build(name, ns)
        axes, _ = grid_axes(box, (n, n, n))
        tables = topology._axes(axes)
        points = int(np.prod([t.size for t in tables], dtype=np.int64))
        if geo is not None:
            geo._sdf = geo.modified_object
            source, public = program_for(lower_geometry(geo)), geo
        else:
            source = public = _engine.DeviceField.from_host(field.ravel(), config.device)
        result = {"case": case, "points": points}
        with _engine.LabelScratch(tables, config.device) as scratch, scratch.labels() as labels:
            result["scratch_bytes_per_point"] = scratch.nbytes / points
            for conn, key in ((_engine.CONNECT_FACES, "label"), (_engine.CONNECT_FULL, "label_full")):
                passes, reduce_ms, count = [], [], 0
                for i in range(args.warmup + args.reps):
                    t = {}
                    count = scratch.label(source, 0.0, conn, _engine.REGION_INSIDE, labels, config.mode, t)
                    ms, _, rec = timed(lambda: scratch.records(count, labels), 1, 0)
                    if i >= args.warmup:
                        passes.append(t)
                        reduce_ms.append(ms)
                med = {p: float(np.median([t[p] for t in passes])) for p in _engine.LABEL_PASSES}
                med["reduce"] = float(np.median(reduce_ms))
                total = float(sum(med.values()))
                if key == "label":
                    result.update({p + "_ms": v for p, v in med.items()})
                    result.update(components=count, largest=int(rec[1].max(initial=0)), label_ms=total,
                                  label_over_bits=total / med["bits"])
                else:
                    result.update(components_full=count, label_full_ms=total, merge_full_ms=med["merge"])
        betti_ms, _, t = timed(lambda: topology.betti(public, tables), args.reps, args.warmup)
        cells_ms, _, cells = timed(lambda: topology.cell_counts(public, tables), args.reps, args.warmup)
        result.update(betti_ms=betti_ms, cells_ms=cells_ms, betti=[t.components, t.tunnels, t.cavities], euler=t.euler)
        if n <= args.host_limit:
            if geo is not None:
                from aegolius_amd import mesh
                grid = mesh._grid_array([np.asarray(a, dtype=np.float64) for a in axes])

                def old_field():
                    dev = geo.create_resident(grid)
                    try:
                        return dev.numpy()
                    finally:
                        dev.free()
            else:
                old_field = public.numpy
            field_ms, _, host = timed(old_field, max(1, args.reps // 2), 1)
            mask = host.reshape([t.size for t in tables]) <= 0
            walls = []
            for _ in range(max(1, args.reps // 2)):
                t0 = time.perf_counter()
                host_count = labeller(mask)
                walls.append((time.perf_counter() - t0) * 1e3)
            result.update(field_ms=field_ms, host_label_ms=float(np.median(walls)), host_labeller=labeller_name,
                          host_components=host_count, same_count=bool(host_count == result["components"]),
                          old_over_new=(field_ms + float(np.median(walls))) / result["label_ms"])
        if field is not None:
            public.free()
        lines.append(json.dumps(result) + "\n")
        print(lines[-1], end="", flush=True)
        with open(args.out, "w") as f:                         # (after every case: a time limit leaves the finished ones)
            f.writelines(lines)


if __name__ == "__main__":
    main()
