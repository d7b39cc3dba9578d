"""Secondary-ray benchmark (aegolius_amd.render.visibility / ambient_occlusion): one scene per call.
    python tools/bench_secondary.py cfg2 [--width 1920 --height 1080 --reps 7 --warmup 2]
scenes: cfg2, cfg5, union<N>. The perspective camera of tools/bench_render.py. The primary frame (the camera kernel with
normals, what render() launches) is rendered once; its hit pixels give the shadow rays of one directional light as
illuminate() builds them (render.shadow_rays, softness 8) and the points and normals of the ambient-occlusion march (5
samples, radius 0.2), both in the order illuminate() marches them in (render.tile_order) and uploaded before anything is
timed. Then five launches of the same build are timed ALTERNATELY in one process after the warm-up of all of them, device
events around the launch alone (outputs pre-allocated, kernels already built): `primary`, `shadow`, `shadow_hard` (the
same rays with softness 0: the march without the penumbra term and its division), `shadow_rows` (the same rays in
row-major pixel order: what the tile order is worth) and `ao`. A chain-mode scene (the unions) is timed culled (MODE_SPECIALIZED) and without
the survivor lists (MODE_NOCULL). Per kernel: median and smallest ms, rays, evaluations, the WAVE evaluations — the sum over
the waves (8 x 8 tiles of the primary frame, 64 consecutive rays of the arrays) of the most evaluations of a ray in the wave,
which is the trip count of that wave's loop; the primary adds the 4 stencil evaluations of a wave with a hit — and ns per
wave evaluation = time / wave evaluations. Prints one JSON line."""
import argparse
import contextlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

LIGHT = (1.0, 1.0, 2.0)
SOFTNESS, AO_RADIUS, AO_SAMPLES = 8.0, 0.2, 5


def tile_max(x):
    h, w = x.shape
    padded = np.zeros(((h + 7) // 8 * 8, (w + 7) // 8 * 8), dtype=np.int64)
    padded[:h, :w] = x
    return padded.reshape(padded.shape[0] // 8, 8, padded.shape[1] // 8, 8).max(axis=(1, 3))


def run_max(x):
    flat = np.zeros((x.size + 63) // 64 * 64, dtype=np.int64)
    flat[:x.size] = x
    return flat.reshape(-1, 64).max(axis=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("scene")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--t-max", type=float, default=8.0)
    ap.add_argument("--max-steps", type=int, default=256)
    args = ap.parse_args()
    import __graft_entry__
    __graft_entry__.build()
    import bench_render
    from aegolius_amd import _engine, render
    from aegolius_amd._eval import config, program_for
    _engine.require_gpu()
    L = _engine.lib()
    vp = _engine._vp
    geo = bench_render.scene(args.scene)
    low, _ = render.lower(geo)
    prog = program_for(low)
    cam = render.Camera(bench_render.EYE, (0, 0, 0), (0, 0, 1), 40.0)
    W, H = args.width, args.height
    n = W * H
    inv = float(np.float32(1.0 / low.lipschitz))
    t_max = float(np.float32(args.t_max))
    img = render.render(geo, cam, W, H, 0.0, args.t_max, args.max_steps)
    eps, cone = float(np.float32(img.eps)), float(np.float32(img.cone))
    rec = cam.record(W, H)
    facing, origins, directions, _, eps2 = render.shadow_rays(img, render.Light.directional(LIGHT))
    eps2, t_far = float(np.float32(eps2)), float(np.float32(img.t.max()))
    hit = img.status == render.HIT
    nrm = np.ascontiguousarray(img.normals[hit].T)
    unit = np.abs((nrm.astype(np.float64) ** 2).sum(axis=0) - 1.0) <= 1e-5
    pts, nrm = np.ascontiguousarray(img.points()[:, unit]), np.ascontiguousarray(nrm[:, unit])
    order = render._pixel_order(hit, facing)
    rows_o, rows_d = origins, directions
    origins, directions = np.ascontiguousarray(origins[:, order]), np.ascontiguousarray(directions[:, order])
    order = render._pixel_order(hit, unit)
    pts, nrm = np.ascontiguousarray(pts[:, order]), np.ascontiguousarray(nrm[:, order])
    n_sh, n_ao = origins.shape[1], pts.shape[1]
    result = {"scene": args.scene, "width": W, "height": H, "instructions": int(low.code.shape[0]), "chain_members": prog.chain_members,
              "max_steps": args.max_steps, "softness": SOFTNESS, "ao_samples": AO_SAMPLES, "ao_radius": AO_RADIUS, "shadow_eps": eps2,
              "hit_pixels": int(hit.sum()), "shadow_rays": n_sh, "ao_points": n_ao, "device": "MI355X (gfx950), 1 GPU", "kernels": {}}
    modes = {"specialised": _engine.MODE_SPECIALIZED}
    if prog.chain_members:
        modes["nocull"] = _engine.MODE_NOCULL
    result["build_primary"] = prog.compile_flavour(_engine.FLAVOUR_RAYS)
    result["build_secondary"] = prog.compile_flavour(_engine.FLAVOUR_SECONDARY)
    dev = config.device
    with contextlib.ExitStack() as stack:
        t, normals, d_status, d_steps = render._outputs(stack, stack, n, True)
        d_o, d_d, d_p, d_n, r_o, r_d = (stack.enter_context(_engine.DeviceVectorField.from_host(x, dev))
                                        for x in (origins, directions, pts, nrm, rows_o, rows_d))
        vis = stack.enter_context(_engine.DeviceField(max(n_sh, 1), dev))
        ao = stack.enter_context(_engine.DeviceField(max(n_ao, 1), dev))
        s_status = stack.enter_context(_engine.DeviceBuffer(max(n_sh, 64)))
        s_steps = stack.enter_context(_engine.DeviceBuffer(max(n_sh, 16) * 4))

        def primary(m):
            def launch():
                _engine.check(L.sdfk_trace_camera_device(prog.handle, _engine._ptr(rec), W, H, 0, 0.0, t_max, eps, cone, inv,
                                                         args.max_steps, vp(t.ptr), d_status.at(), d_steps.at(), vp(normals.ptr),
                                                         normals.stride, None, m), "sdfk_trace_camera_device")
            return launch

        def shadow(m, softness=SOFTNESS, o=None, d=None):
            o, d = (d_o, d_d) if o is None else (o, d)

            def launch():
                _engine.check(L.sdfk_visibility_rays_device(prog.handle, vp(o.ptr), o.stride, vp(d.ptr), d.stride, n_sh, 0.0,
                                                            t_far, eps2, 0.0, inv, args.max_steps, softness, None, vp(vis.ptr),
                                                            s_status.at(), s_steps.at(), None, m), "sdfk_visibility_rays_device")
            return launch

        def occlusion(m):
            def launch():
                _engine.check(L.sdfk_occlusion_rays_device(prog.handle, vp(d_p.ptr), d_p.stride, vp(d_n.ptr), d_n.stride, n_ao,
                                                           AO_RADIUS, AO_SAMPLES, 1.0, inv, vp(ao.ptr), None, m),
                              "sdfk_occlusion_rays_device")
            return launch
        launches = {}
        for name, m in modes.items():
            launches["primary/" + name], launches["shadow/" + name], launches["ao/" + name] = primary(m), shadow(m), occlusion(m)
            launches["shadow_hard/" + name], launches["shadow_rows/" + name] = shadow(m, 0.0), shadow(m, SOFTNESS, r_o, r_d)
        times = bench_render.alternating_ms(launches, args.reps, args.warmup)
        for name, launch in launches.items():
            launch()
            _engine.check(L.sdfk_sync(None), "sdfk_sync")
            k = {"ms": times[name][0], "ms_min": times[name][1]}
            if name.startswith("primary"):
                status, steps = render._small(n, d_status, d_steps)
                evals = (steps.astype(np.int64) + (status == render.HIT)).reshape(H, W)
                waves = tile_max(evals) + 4 * (tile_max((status == render.HIT).reshape(H, W)) > 0)
                k.update(rays=n, hits=int((status == render.HIT).sum()), evaluations=int(evals.sum()) + 4 * int((status == render.HIT).sum()))
            elif name.startswith("shadow"):
                status, steps = render._small(n_sh, s_status, s_steps)
                evals = steps.astype(np.int64) + (status == render.HIT)
                waves = run_max(evals)
                v = vis.numpy()[:n_sh]
                k.update(rays=n_sh, blocked=int((status == render.HIT).sum()), penumbra=int(((v > 0) & (v < 1)).sum()),
                         vis_sum=float(v.sum(dtype=np.float64)), evaluations=int(evals.sum()), max_evaluations=int(evals.max()))
            else:
                status = np.zeros(0, dtype=np.uint8)
                waves = np.full((n_ao + 63) // 64, AO_SAMPLES, dtype=np.int64)
                k.update(rays=n_ao, ao_sum=float(ao.numpy()[:n_ao].sum(dtype=np.float64)), evaluations=n_ao * AO_SAMPLES)
            k["step_limit"] = int((status == render.LIMIT).sum())
            k["wave_evaluations"] = int(waves.sum())
            k["ns_per_wave_evaluation"] = k["ms"] * 1e6 / k["wave_evaluations"]
            k["ns_per_ray"] = k["ms"] * 1e6 / k["rays"]
            result["kernels"][name] = k
        for name in modes:
            a = result["kernels"]["primary/" + name]
            for march in ("shadow", "shadow_hard", "shadow_rows", "ao"):
                b = result["kernels"][march + "/" + name]
                result["%s_cost_per_wave_evaluation_ratio/%s" % (march, name)] = b["ns_per_wave_evaluation"] / a["ns_per_wave_evaluation"]
                result["%s_cost_per_ray_ratio/%s" % (march, name)] = b["ns_per_ray"] / a["ns_per_ray"]
    print(json.dumps(result))


if __name__ == "__main__":
    main()
