"""Projection benchmark (aegolius_amd.surface). No number in it is a pass criterion.
    python tools/project_bench.py [--points 4194304 --mesh 513 --reps 5 --warmup 2 --out profiles/project_bench.txt]
Workloads: `points` uniform points in the BASELINE box of cfg2 and of cfg5, and the vertices of the cfg2 isosurface on a
`mesh`^3 grid. tol 1e-5, 32 steps at most. For each:
  (a) one sdfk_project_points_device launch, device events, the median of `reps` launches after `warmup`; the mean and
      maximum steps per point; the program evaluations the waves ran (one counter per workgroup, summed here);
  (b) the route without the kernel: a host loop of autodiff.value_and_grad_points and a numpy update, to the same cap of
      steps per point, by the wall clock, once with the points resident between the evaluation and the update's upload
      (resident=True) and once through host arrays;
  (c) the time per wave evaluation of (a) against that of one sdfk_jvp_kernel<3, ...> launch (point mode) on the same
      points and program: (t_project / evaluations) / (t_jvp / waves); and the launch with max_iter = 0, in which every
      wave evaluates once, against the jvp launch: the kernel's cost per evaluation without the uneven trip counts.
Writes the table to --out and prints it."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TOL, MAX_ITER = 1e-5, 32


def timed(call, reps, warmup):
    from aegolius_amd import _engine
    out = []
    for i in range(warmup + reps):
        a, b = _engine.Event(), _engine.Event()
        a.record()
        call()
        b.record()
        _engine.check(_engine.lib().sdfk_sync(None), "sdfk_sync")
        if i >= warmup:
            out.append(a.elapsed_ms(b))
    return float(np.median(out)), float(min(out))


def host_loop(geo, p, resident):
    """The parent route: evaluate, update with numpy, again — the kernel's arithmetic and statuses. -> (seconds, evaluations,
    points (3, n), status)"""
    from aegolius_amd import _engine, autodiff
    from aegolius_amd._eval import config
    t0 = time.perf_counter()
    q = np.array(p, dtype=np.float32)
    n = q.shape[1]
    status = np.full(n, -1, dtype=np.int64)
    tol, evaluations = np.float32(TOL), 0
    for trip in range(MAX_ITER + 1):
        if resident:
            d_q = _engine.DeviceVectorField.from_host(q, config.device)
            v, g = autodiff.value_and_grad_points(geo, d_q, resident=True)
            f, grad = v.numpy(), np.stack([x.numpy() for x in g])
            for x in [d_q, v] + list(g):
                x.free()
        else:
            f, grad = autodiff.value_and_grad_points(geo, q)
        evaluations += 1
        with np.errstate(all="ignore"):
            act = status < 0
            g2 = (grad[0] * grad[0] + grad[1] * grad[1]) + grad[2] * grad[2]
            status[act & ~(np.abs(f) <= np.finfo(np.float32).max)] = 3
            status[(status < 0) & (np.abs(f) <= tol)] = 0
            if trip == MAX_ITER:
                status[status < 0] = 1
            status[(status < 0) & ~(g2 >= np.float32(1e-24))] = 2
            go = status < 0
            if not go.any():
                break
            s = np.where(go, f / g2, np.float32(0.0)).astype(np.float32)
            q = np.where(go, q - s * grad, q).astype(np.float32)
    return time.perf_counter() - t0, evaluations, q, status


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1 << 22)
    ap.add_argument("--mesh", type=int, default=513)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "project_bench.txt"))
    args = ap.parse_args()
    import __graft_entry__
    __graft_entry__.build()
    import aegolius_amd.cores as ns
    from aegolius_amd import _engine, autodiff, mesh, workloads
    from aegolius_amd._eval import config
    _engine.require_gpu()
    L, vp = _engine.lib(), _engine._vp
    lines = ["projection benchmark: MI355X (gfx950), 1 GPU; tol %g, at most %d steps; kernels by device events, the median of "
             "%d launches after %d warm-up launches; host loops by the wall clock, one run" % (TOL, MAX_ITER, args.reps, args.warmup)]
    jobs = [("cfg2", "uniform"), ("cfg5", "uniform"), ("cfg2", "mesh")]
    for name, kind in jobs:
        geo, size, desc = workloads.build(name, ns)
        if kind == "uniform":
            rng = np.random.default_rng(5)
            p = np.stack([rng.uniform(-s / 2, s / 2, args.points) for s in size]).astype(np.float32)
            what = "%d uniform points in the box" % args.points
        else:
            m = mesh.from_geometry(geo, size, (args.mesh,) * 3)
            p = np.ascontiguousarray(m.vertices.T, dtype=np.float32)
            what = "%d vertices of its isosurface on %d^3" % (p.shape[1], args.mesh)
        n = p.shape[1]
        low, origin = autodiff._lower(workloads.build(name, ns)[0], shortcuts=True)
        prog = autodiff._program(low, origin)
        groups = int(L.sdfk_project_workgroups(n))
        waves = (n + 63) // 64
        with _engine.DeviceVectorField.from_host(p, config.device) as d_p, _engine.DeviceVectorField(n, config.device) as d_q, \
                _engine.DeviceVectorField(n, config.device) as d_g, _engine.DeviceField(n, config.device) as d_v, \
                _engine.DeviceField(n, config.device) as d_s, _engine.DeviceBuffer(4 * n) as d_info, \
                _engine.DeviceBuffer(4 * groups) as d_trips, _engine.DeviceBuffer(12 * low.params.size + 4) as d_dp:
            def project(max_iter=MAX_ITER):
                _engine.check(L.sdfk_project_points_device(prog.handle, d_p.at(), n, d_p.stride, 0.0, TOL, max_iter, 1.0, d_q.at(),
                                                           d_q.stride, d_v.at(), d_g.at(), d_g.stride, d_s.at(), d_info.at(), None),
                              "sdfk_project_points_device")

            def jvp():
                _engine.check(L.sdfk_eval_jvp_device(prog.handle, d_p.at(), n, d_p.stride, d_dp.at(), 3, 1, d_v.at(), d_g.at(),
                                                     d_g.stride, None), "sdfk_eval_jvp_device")
            d_dp.upload(np.zeros(3 * low.params.size + 1, dtype=np.float32))
            t_jvp, t_jvp_min = timed(jvp, args.reps, args.warmup)
            t_one, t_one_min = timed(lambda: project(0), args.reps, args.warmup)
            t_prj, t_prj_min = timed(project, args.reps, args.warmup)
            d_trips.upload(np.zeros(groups, dtype=np.uint32))
            _engine.check(L.sdfk_project_points_counted_device(prog.handle, d_p.at(), n, d_p.stride, 0.0, TOL, MAX_ITER, 1.0,
                                                               d_q.at(), d_q.stride, d_v.at(), d_g.at(), d_g.stride, d_s.at(),
                                                               d_info.at(), d_trips.at(), None), "sdfk_project_points_counted_device")
            _engine.check(L.sdfk_sync(None), "sdfk_sync")
            trips = int(d_trips.download(np.zeros(groups, dtype=np.uint32)).astype(np.int64).sum())
            info = d_info.download(np.zeros(n, dtype=np.int32))
            q_dev = d_q.numpy()
        status, its = info & 255, (info >> 8) & 255
        per_eval, per_jvp = t_prj / trips, t_jvp / waves
        lines.append("")
        lines.append("%s, %s (%d instructions, %s register file)" % (desc, what, len(low.code),
                                                                     "small" if low.n_creg <= 2 and low.n_vreg <= 3 else "full"))
        lines.append("  (a) project: %.3f ms per launch (min %.3f); steps per point mean %.3f max %d; status shares converged %.5f "
                     "maxiter %.5f stalled %.5f nonfinite %.5f" % ((t_prj, t_prj_min, its.mean(), its.max())
                                                                 + tuple(float(np.mean(status == k)) for k in range(4))))
        lines.append("      wave evaluations %d over %d waves = %.3f per wave (a wave runs until its last point stops)"
                     % (trips, waves, trips / waves))
        for resident in (True, False):
            secs, evaluations, q_host, st_host = host_loop(workloads.build(name, ns)[0], p, resident)
            same = bool(np.array_equal(q_host.view(np.uint32), q_dev.view(np.uint32)) and np.array_equal(st_host, status))
            lines.append("  (b) host loop, %s: %.1f ms for %d evaluations of all points (%.1f x the launch); result equal to the "
                         "kernel's bit for bit: %s" % ("points resident" if resident else "host arrays", 1e3 * secs, evaluations,
                                                        1e3 * secs / t_prj, same))
        lines.append("  (c) jvp point-mode launch %.3f ms (min %.3f) = %.3f ns per wave evaluation; project %.3f ns per wave "
                     "evaluation; ratio %.3f" % (t_jvp, t_jvp_min, 1e6 * per_jvp, 1e6 * per_eval, per_eval / per_jvp))
        lines.append("      project with max_iter = 0 (every wave evaluates once): %.3f ms (min %.3f), ratio to the jvp launch %.3f"
                     % (t_one, t_one_min, t_one / t_jvp))
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
