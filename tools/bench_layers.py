"""Layer-graph benchmark (aegolius_amd.layers): graph() by phase, the candidate count against the final
number of links, against the 3-D labelling of the same source and against the route users had before the module.
    python tools/bench_layers.py [cfg2:513 cfg5:513 union1000:513 noise0.31:513] [--reps 5 --warmup 1 --old-layers 9
                                  --out profiles/layers_bench.txt]
Per case `scene:n`, in one process (MODE_SPECIALIZED: the builds are waited for in the warm-up), on the tables of
generate_grid(box, (n, n, n)) with the layers along z (normal = 2); noise is a host field of +-1 at the given inside
density, uploaded once. Medians of `reps` calls after `warmup`:
  * graph_wall_ms: layers.graph(..., labels=False) as a user calls it, wall clock around the public call (scratch and label
    allocation, labelling, records, links, the host's combine); its phases from `timings`: prepare_ms (host: the checks and
    the lowering of the tree) and allocate_ms (host: scratch and labels), bits .. number (device events inside the labelling
    call), records_ms, links_ms (count, scan, supported) and candidates_ms (emit) (device events around each call, downloads
    included), combine_ms (host); label_ms = bits + init + merge + compress + number, label_wall_ms the wall clock around
    that call; unaccounted_ms = graph_wall_ms minus all of these (label_wall_ms in place of label_ms): the frees of labels
    and scratch and the result's arrays; candidates against links.
  * (a) topology_label_ms: the same five passes of topology's 3-D labelling (inside, faces) of the same source, same scratch,
    the two labellings taking turns call by call; layer_over_topology = label_ms / topology_label_ms. The in-plane merge
    does a subset of the 3-D merge's unions. label_in_turn_wall_ms / topology_label_wall_ms: wall clock around the same
    calls (the program object is made once here; graph() lowers the tree and makes one per call).
  * (b) the only route before: per layer one evaluation to a resident 2-D field, one topology.label(field, (U, V)) with its
    own scratch, labels_host(), then the reference's numpy link reduction between consecutive layers (np.unique over the
    stacked label pairs). Timed on `--old-layers` consecutive layers in the middle of the stack, wall clock;
    old_route_ms_extrapolated = per-layer time x L. SUBSAMPLED: the whole stack is never run this way.
Writes a header and one JSON line per case to --out and prints them."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HEADER = """# tools/bench_layers.py, one run on one MI355X (gfx950) box, median of %d after %d warm-up(s), all cases in one process, MODE_SPECIALIZED
# scene:n = the scene on generate_grid(box, (n, n, n)), layers along z; noise: a resident field of +-1. Milliseconds.
# graph_wall_ms: layers.graph(labels=False), wall clock around the public call; bits .. number: device events inside the
# labelling call; records_ms / links_ms (count, scan, supported) / candidates_ms (emit): device events around the call with its
# download; prepare_ms (checks, lowering) / allocate_ms (scratch, labels) / combine_ms (link reduction): the host, wall clock
# label_wall_ms: wall clock around the labelling call; unaccounted_ms: graph_wall_ms minus every phase (frees, result arrays)
# label_ms = bits + init + merge + compress + number; topology_label_ms: the same passes of the 3-D labelling (inside, faces),
# same process and scratch, taking turns; layer_over_topology = label_ms / topology_label_ms
# old route (SUBSAMPLED: %d consecutive layers, extrapolated to L): per layer a resident 2-D field, topology.label, labels_host,
# numpy link reduction; old_over_new = old_route_ms_extrapolated / graph_wall_ms
"""


HOST = ("prepare", "allocate", "combine")                      # the host's phases of graph(), wall clock


def median(values):
    return float(np.median(values))


def old_route(geo, field, tables, lo, count):
    """The route before the module on layers lo .. lo + count - 1 -> (wall ms, links found)."""
    from aegolius_amd import _engine, mesh, slices, topology
    from aegolius_amd._eval import config
    H, U, V = tables
    t0 = time.perf_counter()
    below, links = None, 0
    for l in range(lo, lo + count):
        if geo is not None:
            co = mesh._grid_array([H[l:l + 1].astype(np.float64), U.astype(np.float64), V.astype(np.float64)])
            dev = slices.Frame.axis(2).apply(geo).create_resident(co)
        else:
            dev = _engine.DeviceField.from_host(field[l], config.device)
        try:
            c = topology.label(dev, (U, V))
            labels = c.labels_host().astype(np.int64)
            c.free()
        finally:
            dev.free()
        if below is not None:
            both = (labels >= 0) & (below >= 0)
            pairs = np.unique(np.stack([labels[both], below[both]], axis=1), axis=0, return_counts=True)[0]
            links += len(pairs)
        below = labels
    return (time.perf_counter() - t0) * 1e3, links


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("cases", nargs="*", default=["cfg2:513", "cfg5:513", "union1000:513", "noise0.31:513"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--old-layers", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "layers_bench.txt"))
    args = ap.parse_args()
    import __graft_entry__
    __graft_entry__.build()
    import aegolius_amd.cores as ns
    from aegolius_amd import _engine, layers, slices, workloads
    from aegolius_amd._eval import config, program_for
    from aegolius_amd._lower import lower_geometry
    from aegolius_amd.cores.helper_functions import grid_axes
    _engine.require_gpu()
    config.mode = _engine.MODE_SPECIALIZED
    lines = [HEADER % (args.reps, args.warmup, args.old_layers)]
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
        heights, plane = axes[2], (axes[0], axes[1])
        source = geo if geo is not None else _engine.DeviceField.from_host(field.ravel(), config.device)
        result = {"case": case}
        walls, phases, g = [], [], None
        for i in range(args.warmup + args.reps):
            t = {}
            t0 = time.perf_counter()
            g = layers.graph(source, plane, heights, normal=2, labels=False, timings=t)
            if i >= args.warmup:
                walls.append((time.perf_counter() - t0) * 1e3)
                phases.append(t)
        med = {p: median([t[p] for t in phases]) for p in _engine.LABEL_PASSES + HOST + ("records", "links", "candidates")}
        label_ms = float(sum(med[p] for p in _engine.LABEL_PASSES))
        result.update({"shape": list(g.shape), "points": int(np.prod(g.shape)), "components": g.count, "links": int(g.child.size),
                       "candidates": phases[-1]["candidate_count"], "islands": int(g.islands().size),
                       "overhang_points": int(g.per_layer().overhang[1:].sum()), "graph_wall_ms": median(walls), "label_ms": label_ms,
                       "records_ms": med["records"], "links_ms": med["links"], "candidates_ms": med["candidates"]})
        result.update({p + "_ms": med[p] for p in HOST})
        result["label_wall_ms"] = median([t["label_wall"] for t in phases])
        # what is left: the frees of labels and scratch, the result's arrays
        result["unaccounted_ms"] = result["graph_wall_ms"] - float(sum(med.values())) - (result["label_wall_ms"] - label_ms)
        result.update({p + "_ms": med[p] for p in _engine.LABEL_PASSES})
        result["candidates_over_links"] = result["candidates"] / max(1, result["links"])
        # (a) the 3-D labelling of the same source on the same scratch, the two taking turns
        tables = g.axes
        if geo is not None:
            prog = program_for(lower_geometry(slices.Frame.axis(2).apply(geo)))
        else:
            prog = source
        layer_t, topo_t, layer_wall, topo_wall = [], [], [], []
        with _engine.LabelScratch(tables, config.device) as scratch, scratch.labels() as labels:
            for i in range(args.warmup + args.reps):
                a, b = {}, {}
                t0 = time.perf_counter()
                scratch.layer_label(prog, 0.0, _engine.CONNECT_FACES, labels, config.mode, a)
                t1 = time.perf_counter()
                k3 = scratch.label(prog, 0.0, _engine.CONNECT_FACES, _engine.REGION_INSIDE, labels, config.mode, b)
                t2 = time.perf_counter()
                if i >= args.warmup:
                    layer_t.append(a)
                    topo_t.append(b)
                    layer_wall.append((t1 - t0) * 1e3)
                    topo_wall.append((t2 - t1) * 1e3)
        turn = {p: median([t[p] for t in layer_t]) for p in _engine.LABEL_PASSES}
        topo = {p: median([t[p] for t in topo_t]) for p in _engine.LABEL_PASSES}
        result.update(label_in_turn_ms=float(sum(turn.values())), topology_label_ms=float(sum(topo.values())),
                      merge_in_turn_ms=turn["merge"], topology_merge_ms=topo["merge"], topology_components=k3,
                      label_in_turn_wall_ms=median(layer_wall), topology_label_wall_ms=median(topo_wall))
        result["layer_over_topology"] = result["label_in_turn_ms"] / result["topology_label_ms"]
        lines.append(json.dumps(result) + "\n")
        with open(args.out, "w") as f:                         # (after every step: a time limit leaves the finished ones)
            f.writelines(lines)
        # (b) the route before, on a few consecutive layers
        L = g.shape[0]
        count = min(args.old_layers, L)
        try:
            old_route(geo, field, tables, (L - count) // 2, min(2, count))           # (warm-up: builds, allocations)
            ms, found = old_route(geo, field, tables, (L - count) // 2, count)
            result.update(old_layers=count, old_route_ms=ms, old_route_links=found, old_route_ms_extrapolated=ms / count * L,
                          old_over_new=ms / count * L / result["graph_wall_ms"])
        except Exception as exc:                               # (the comparison is an extra: the case's own numbers stay)
            result["old_route_error"] = "%s: %s" % (type(exc).__name__, exc)
        if field is not None:
            source.free()
        lines[-1] = json.dumps(result) + "\n"
        print(lines[-1], end="", flush=True)
        with open(args.out, "w") as f:
            f.writelines(lines)


if __name__ == "__main__":
    main()
