"""A numpy model of the per-wave survivor lists of the culled ray kernels (csrc/sdfk_raycull.h, SdfkCullField):
what the rule costs in member evaluations, in float64 on the CPU. It predicts counts, not time.

    python tools/ray_cull_model.py [--members 1000 --width 320 --height 240 --cap 192 --depth 3 --look 0 --tiles 150]

The scene is workloads.sphere_union (the same draws, kept here as centres and radii), the view the bench camera. A wave
is one 8 x 8 pixel tile. At every iteration of the marching loop the marching lanes' points are bounded by a sphere
(c, rho); every member is evaluated at c; member k survives unless e_k - m >= thr0 + 1e-6 |e_k| with
thr0 = 1.0001 K R + K cmag + 1e-6 (1 + |m|), K = 2 (two spheres), R = (1 + look) rho; the list is kept while
every marching lane stays within R of c. More than `cap` survivors: the lanes are split at the middle of their t range,
at most `depth` deep, then every member is evaluated — for the whole wave when its groups together would cost more than
every member once, and then the next 4 rebuilds do not try to split. Counted per wave and evaluation, as the kernel's statistics do:
    members per evaluation = (evaluations of the builds / 64 + entries of the lists + members per group without a list)
against `members` for the plain kernel. (The four stencil evaluations of the normals are not modelled.)"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EYE = (2.2, 1.6, 1.9)
KMAX = 2.0
HOLD = 4          # rebuilds without a split after one whose split did not pay


def spheres(count=1000, seed=31, radius=0.05, extent=0.9):
    """Centres (count, 3) and radii (count,) of workloads.sphere_union(count, seed, radius, extent): the same draws."""
    rng = np.random.default_rng(seed)
    radii, centres = np.empty(count), np.empty((count, 3))
    for k in range(count):
        radii[k] = float(radius * rng.uniform(0.5, 1.5))
        centres[k] = rng.uniform(-extent, extent, 3)
    return centres, radii


def members_at(centres, radii, points):
    """(n, 3) points -> (n, members) values of every member."""
    return np.linalg.norm(points[:, None, :] - centres[None], axis=2) - radii[None]


def bounding_sphere(points):
    """Centre of the box of the points, and the rounded-up radius 1.0001 max|p - c| + tiny."""
    c = 0.5 * (points.min(axis=0) + points.max(axis=0))
    return c, 1.0001 * float(np.linalg.norm(points - c, axis=1).max()) + 1e-30


def survivors(centres, radii, c, rho, look=0.0):
    """The rule: indices of the members kept for the sphere (c, R), in index order, and R."""
    e = np.linalg.norm(centres - c, axis=1) - radii
    m = float(e.min())
    R = rho + look * rho
    cmag = 1e-6 * (np.abs(c).sum() + R)
    thr0 = 1.0001 * KMAX * R + KMAX * cmag + 1e-6 * (1.0 + abs(m))
    return np.flatnonzero(~(e - m >= thr0 + 1e-6 * np.abs(e))), R


def camera_rays(width, height, eye=EYE, target=(0.0, 0.0, 0.0), up=(0.0, 0.0, 1.0), fov=40.0):
    """Perspective rays of aegolius_amd.render.Camera (the formula of its module text) -> o (3,), d (H, W, 3), cone."""
    eye, target, up = (np.asarray(v, dtype=np.float64) for v in (eye, target, up))
    fwd = (target - eye) / np.linalg.norm(target - eye)
    right = np.cross(fwd, up)
    right /= np.linalg.norm(right)
    upv = np.cross(right, fwd)
    half = np.tan(np.radians(0.5 * fov))
    a = (2.0 * np.arange(width) + 1.0) / width - 1.0
    b = 1.0 - (2.0 * np.arange(height) + 1.0) / height
    w = fwd[None, None] + a[None, :, None] * (right * half * width / height)[None, None] + b[:, None, None] * (upv * half)[None, None]
    return eye, w / np.linalg.norm(w, axis=2, keepdims=True), half / height


def trace_tile(centres, radii, o, d, live, cone, cap, depth, look, pool, t_max, max_steps, counts):
    """One wave: d (64, 3), live (64,) lanes with a ray. Adds to counts; -> (t, status) of the lanes."""
    n = centres.shape[0]
    t = np.zeros(64)
    status = np.full(64, 2)
    marching = live.copy()
    gc, gR = np.zeros((64, 3)), np.full(64, -1.0)
    groups, hold = [], 0
    for _ in range(max_steps):
        if not marching.any():
            break
        p = o[None] + t[:, None] * d
        need = marching & ~(1.0001 * np.linalg.norm(p - gc, axis=1) <= gR)
        if need.any():
            gR[:] = -1.0
            groups, used = [], 0
            queue = [(marching.copy(), 0)]
            while queue:
                mask, dep = queue.pop(0)
                c, rho = bounding_sphere(p[mask])
                keep, R = survivors(centres, radii, c, rho, look)
                counts["builds"] += 1
                room = min(cap, pool - used)
                # (the values at c are kept, between the pass for m and the comparison, in the pool beyond the list's room)
                counts["build_evaluations"] += n + max(0, n - (pool - used - room))
                if keep.size > room:
                    tm = t[mask]
                    lo = mask & (t <= 0.5 * (tm.min() + tm.max()))
                    hi = mask & ~lo
                    if dep < depth and lo.any() and hi.any() and hold == 0:
                        counts["splits"] += 1
                        queue.insert(0, (lo, dep + 1))
                        queue.append((hi, dep + 1))
                        continue
                    groups.append((mask, None))
                    continue
                used += keep.size
                gc[mask], gR[mask] = c, R
                groups.append((mask, keep))
            if len(groups) > 1 and sum(n if keep is None else keep.size for _, keep in groups) >= n:
                groups = [(marching.copy(), None)]               # together dearer than every member once: one group
                gR[:] = -1.0
                hold = HOLD + 1
            hold = max(0, hold - 1)
        f = np.full(64, np.inf)
        for mask, keep in groups:
            if keep is None:
                counts["plain_evaluations"] += 64
                f[mask] = members_at(centres, radii, p[mask]).min(axis=1)
            else:
                counts["survivor_evaluations"] += 64 * keep.size
                f[mask] = members_at(centres[keep], radii[keep], p[mask]).min(axis=1)
        counts["point_evaluations"] += 1
        thr = cone * t
        hit = marching & (f <= thr)
        status[hit] = 1
        go = marching & ~hit
        t[go] += f[go]
        counts["lane_steps"] += int(go.sum())
        miss = go & (t > t_max)
        status[miss] = 0
        marching = go & ~miss
    return t, status


def model(members=1000, width=320, height=240, cap=192, depth=3, look=0.0, tiles=150, seed=0, pool=1024, central=False,
          t_max=8.0, max_steps=256):
    """-> the counts and `members_per_evaluation`. tiles: how many 8 x 8 tiles to sample (0: all); central: from the central
    half of the image only."""
    centres, radii = spheres(members)
    o, d, cone = camera_rays(width, height)
    tx, ty = (width + 7) // 8, (height + 7) // 8
    ids = [(j, i) for j in range(ty) for i in range(tx)
           if not central or (tx // 4 <= i < tx - tx // 4 and ty // 4 <= j < ty - ty // 4)]
    if tiles and tiles < len(ids):
        pick = np.random.default_rng(seed).choice(len(ids), tiles, replace=False)
        ids = [ids[k] for k in sorted(pick)]
    counts = dict(builds=0, build_evaluations=0, survivor_evaluations=0, plain_evaluations=0, splits=0, point_evaluations=0,
                  lane_steps=0)
    for j, i in ids:
        lane = np.arange(64)
        ix, iy = 8 * i + (lane & 7), 8 * j + (lane >> 3)
        live = (ix < width) & (iy < height)
        dd = d[np.minimum(iy, height - 1), np.minimum(ix, width - 1)]
        trace_tile(centres, radii, o, dd, live, cone, cap, depth, look, pool, t_max, max_steps, counts)
    counts["tiles"] = len(ids)
    counts["members"] = members
    counts["members_per_evaluation"] = ((counts["build_evaluations"] + counts["survivor_evaluations"] +
                                         members * counts["plain_evaluations"]) / 64.0 / max(1, counts["point_evaluations"]))
    return counts


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--members", type=int, default=1000)
    ap.add_argument("--width", type=int, default=320)
    ap.add_argument("--height", type=int, default=240)
    ap.add_argument("--cap", type=int, default=192)
    ap.add_argument("--depth", type=int, default=3)
    ap.add_argument("--look", type=float, default=0.0)
    ap.add_argument("--pool", type=int, default=1024)
    ap.add_argument("--tiles", type=int, default=150)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--central", action="store_true")
    args = ap.parse_args()
    print(json.dumps(model(args.members, args.width, args.height, args.cap, args.depth, args.look, args.tiles, args.seed,
                           args.pool, args.central)))


if __name__ == "__main__":
    sys.exit(main())
