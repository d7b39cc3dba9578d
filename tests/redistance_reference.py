"""numpy restatement of the definition of aegolius_amd.redistance (the test oracle of the redistance kernels); shares no
code with the package's module. Also the scenes and grids of tests/test_redistance_cpu.py and tests/test_gpu_redistance.py.

All float32, each operation rounded once, in the order written:
 1. inside iff f <= level (NaN: outside); point (i, j, k) owns its +x, +y, +z edges; an edge whose ends differ in the inside
    test carries one seed at xa + t (xb - xa), t = (level - fa) / (fb - fa) (one end NaN: the seed sits at the other end;
    a NaN position is dropped); the seeds of the edges along axis a are family a.
 2. per family, its own axis first, the others after it in increasing order: pass 1 along the family's axis, per line,
    g(i) = min over the line's seeds of (x_i - s) (x_i - s) (+inf without one); then per further axis b the min-plus pass
    g'(j) = min over j' of g(j') + (b_j - b_j') (b_j - b_j'). Q = min over the families.
    `brute` is the min over ALL seeds of the family's expression instead; `separable` the passes. Same bits.
 3. D = sqrt(Q); D = min(D, float32(band)) with a band.
 4. near="gradient": at the ends of crossing edges, g_a = (f+ - f-) / (a+ - a-) (one-sided at the ends of an axis),
    m = sqrt((gx gx + gy gy) + gz gz), e = |f - level| / m; D = min(e, D) if every field value used, m, |f - level| and e
    are finite and m > 0.
 5. out = -D where inside, else +D.
"""
import numpy as np

import aegolius_amd.cores as ns
from aegolius_amd import workloads

F32 = np.float32
INF = F32(np.inf)


def tables(axes):
    return [np.asarray(a, dtype=np.float64).ravel().astype(F32) for a in axes]


def inside(f, level):
    f = np.asarray(f, dtype=F32)
    with np.errstate(invalid="ignore"):
        return (f <= F32(level)) & ~np.isnan(f)


def _order(a, D):
    return [a] + [b for b in range(D) if b != a]


# ---- seeds ------------------------------------------------------------------------------------------------------------
def seeds(f, axes, level=0.0):
    """Per family a: (idx, pos) — idx (D, S) the owning point of every crossing edge along axis a (C order), pos (S,)
    float32 its seed's coordinate along a. NaN positions are dropped."""
    tab = tables(axes)
    shape = tuple(t.size for t in tab)
    D = len(shape)
    f = np.asarray(f, dtype=F32).reshape(shape)
    ins = inside(f, level)
    lv = F32(level)
    out = []
    for a in range(D):
        lo = tuple(slice(0, shape[a] - 1) if o == a else slice(None) for o in range(D))
        hi = tuple(slice(1, None) if o == a else slice(None) for o in range(D))
        idx = np.stack(np.nonzero(ins[lo] != ins[hi])).astype(np.int64)
        up = idx.copy()
        up[a] += 1
        fa, fb = f[tuple(idx)], f[tuple(up)]
        xa, xb = tab[a][idx[a]], tab[a][up[a]]
        with np.errstate(all="ignore"):
            t = (lv - fa) / (fb - fa)
            pos = xa + t * (xb - xa)
        pos = np.where(np.isnan(fa), xb, np.where(np.isnan(fb), xa, pos)).astype(F32)
        keep = ~np.isnan(pos)
        out.append((idx[:, keep], pos[keep]))
    return out


def seed_points(f, axes, level=0.0):
    """(S, D) float32 coordinates of all seeds (every family)."""
    tab = tables(axes)
    D = len(tab)
    rows = []
    for a, (idx, pos) in enumerate(seeds(f, axes, level)):
        pts = np.stack([tab[o][idx[o]] for o in range(D)], axis=1).astype(F32).reshape(-1, D)
        pts[:, a] = pos
        rows.append(pts)
    return np.concatenate(rows) if rows else np.zeros((0, D), F32)


def seed_count(f, axes, level=0.0):
    """Crossing edges (what the device counts: a dropped NaN position still counts)."""
    tab = tables(axes)
    shape = tuple(t.size for t in tab)
    ins = inside(np.asarray(f, dtype=F32).reshape(shape), level)
    return int(sum(np.count_nonzero(np.diff(ins.astype(np.int8), axis=a)) for a in range(len(shape))))


# ---- squared distance ---------------------------------------------------------------------------------------------------
def brute(f, axes, level=0.0, chunk=1 << 22):
    """Q (shape of the grid): per family the min over all its seeds of ((d_a d_a + d_b d_b) + d_c d_c), a the family's axis,
    b < c the others; then the min over the families."""
    tab = tables(axes)
    shape = tuple(t.size for t in tab)
    D = len(shape)
    n = int(np.prod(shape))
    Q = np.full(n, INF, dtype=F32)
    pidx = np.stack(np.unravel_index(np.arange(n), shape))
    for a, (idx, pos) in enumerate(seeds(f, axes, level)):
        S = pos.size
        if S == 0:
            continue
        step = max(1, chunk // S)
        for p0 in range(0, n, step):
            pi = pidx[:, p0:p0 + step]
            d = tab[a][pi[a]][:, None] - pos[None, :]
            acc = d * d
            for b in _order(a, D)[1:]:
                d = tab[b][pi[b]][:, None] - tab[b][idx[b]][None, :]
                acc = acc + d * d
            Q[p0:p0 + step] = np.minimum(Q[p0:p0 + step], acc.min(axis=1))
    return Q.reshape(shape)


def _pass1(f, ins, tab, a, level):
    """g of pass 1 of family a, axis a moved to the end: (..., n_a)."""
    fm = np.moveaxis(f, a, -1)
    im = np.moveaxis(ins, a, -1)
    x = tab[a]
    lv = F32(level)
    g = np.full(fm.shape, INF, dtype=F32)
    for k in range(x.size - 1):
        cross = im[..., k] != im[..., k + 1]
        if not cross.any():
            continue
        fa, fb = fm[..., k], fm[..., k + 1]
        with np.errstate(all="ignore"):
            t = (lv - fa) / (fb - fa)
            s = x[k] + t * (x[k + 1] - x[k])
        s = np.where(np.isnan(fa), x[k + 1], np.where(np.isnan(fb), x[k], s)).astype(F32)
        ok = cross & ~np.isnan(s)
        with np.errstate(all="ignore"):
            d = x[None, :] - s.reshape(-1, 1)
            cand = np.where(ok.reshape(-1, 1), d * d, INF).reshape(g.shape)
        g = np.minimum(g, cand)
    return g


def _minplus(g, x):
    """The min-plus pass along the LAST axis of g with the table x."""
    out = np.full(g.shape, INF, dtype=F32)
    for jp in range(x.size):
        d = x - x[jp]
        out = np.minimum(out, g[..., jp:jp + 1] + d * d)
    return out


def separable(f, axes, level=0.0):
    """Q by the passes of the definition, every family on its own (9 passes in 3-D)."""
    tab = tables(axes)
    shape = tuple(t.size for t in tab)
    D = len(shape)
    f = np.asarray(f, dtype=F32).reshape(shape)
    ins = inside(f, level)
    Q = np.full(shape, INF, dtype=F32)
    for a in range(D):
        g = np.moveaxis(_pass1(f, ins, tab, a, level), -1, a)
        for b in _order(a, D)[1:]:
            g = np.moveaxis(_minplus(np.moveaxis(g, b, -1), tab[b]), -1, b)
        Q = np.minimum(Q, g)
    return Q


# ---- finish -------------------------------------------------------------------------------------------------------------
def near_estimate(f, axes, level=0.0):
    """(touch, valid, e): the points at the ends of crossing edges, where step 4's estimate may be used, and the estimate."""
    tab = tables(axes)
    shape = tuple(t.size for t in tab)
    D = len(shape)
    f = np.asarray(f, dtype=F32).reshape(shape)
    ins = inside(f, level)
    touch = np.zeros(shape, dtype=bool)
    used = np.isfinite(f)
    mm = None
    with np.errstate(all="ignore"):
        for a in range(D):
            lo = tuple(slice(0, shape[a] - 1) if o == a else slice(None) for o in range(D))
            hi = tuple(slice(1, None) if o == a else slice(None) for o in range(D))
            cross = ins[lo] != ins[hi]
            touch[lo] |= cross
            touch[hi] |= cross
            fm = np.moveaxis(f, a, -1)
            x = tab[a]
            n = x.size
            ia = np.maximum(np.arange(n) - 1, 0)
            ib = np.minimum(np.arange(n) + 1, n - 1)
            g = (fm[..., ib] - fm[..., ia]) / (x[ib] - x[ia])
            used &= np.moveaxis(np.isfinite(fm[..., ib]) & np.isfinite(fm[..., ia]), -1, a)
            g = np.moveaxis(g, -1, a).astype(F32)
            mm = g * g if mm is None else mm + g * g
        m = np.sqrt(mm)
        num = np.abs(f - F32(level))
        e = (num / m).astype(F32)
        valid = used & np.isfinite(m) & (m > 0) & np.isfinite(num) & np.isfinite(e)
    return touch, valid, e


def finish(Q, f, axes, level=0.0, band=None, near="gradient"):
    shape = tuple(t.size for t in tables(axes))
    f = np.asarray(f, dtype=F32).reshape(shape)
    D = np.sqrt(np.asarray(Q, dtype=F32).reshape(shape))
    if band is not None:
        D = np.minimum(D, F32(band))
    if near == "gradient":
        touch, valid, e = near_estimate(f, axes, level)
        use = touch & valid
        D = np.where(use, np.minimum(np.where(use, e, INF), D), D)
    else:
        assert near == "seeds"
    return np.where(inside(f, level), -D, D).astype(F32).ravel()


def redistance(f, axes, level=0.0, band=None, near="gradient", method=separable):
    return finish(method(f, axes, level), f, axes, level, band, near)


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


# ---- grids and scenes of the tests --------------------------------------------------------------------------------------
def box(shape, size=2.0):
    return [np.linspace(-size / 2, size / 2, n) for n in shape]


def nonuniform(shape=(9, 11, 13), seed=5):
    rng = np.random.default_rng(seed)
    out = []
    for n in shape:
        steps = rng.uniform(0.4, 1.6, n - 1)
        a = np.concatenate([[0.0], np.cumsum(steps)])
        out.append(2.0 * a / a[-1] - 1.0)
    return out


# name -> axis tables (float64, as a caller gives them)
GRIDS = {
    "2x2x2": [np.array([-0.35, 0.4])] * 3,                    # the smallest grid
    "17x13x11": box((17, 13, 11)),                            # odd sizes, all different
    "5x67x130": box((5, 67, 130)),                            # lines that are no multiple of a wave, a z line over two waves
    "3x3x1100": [np.linspace(-0.35, 0.35, 3)] * 2 + [np.linspace(-1, 1, 1100)],   # a line longer than one staging window
    "9x11x13nu": nonuniform(),                                # non-uniform tables
    "33x29": box((33, 29)),                                   # 2-D
    "3x130": box((3, 130)),
}


def _union3(n):
    return workloads.cfg2_tree(n, count=4, width=0.25)


def _chain(n):
    b = workloads.cfg3_chain(n)
    b.rescale(0.45)                                            # the grids span [-1, 1]^3; cfg 3 lives in [-2, 2]^3
    return b


def _sign(n):
    t = n.Torus(0.55, 0.22)
    t.rotate(0.5, (1, 0.3, 0))
    t.sign()
    return t


def _circles(n):
    a = n.Circle(0.45)
    a.move((0.2, -0.1, 0))
    b = n.Rectangle(0.9, 0.5)
    b.rotate(0.4, (0, 0, 1))
    return n.CombineGeometry("SMOOTH_UNION2").combine_parametric(a, b, parameters=0.2)


def _sign2d(n):
    c = n.NGon(0.6, 5)
    c.sign()
    return c


SCENES_3D = {"smooth_union": _union3, "twist_bend": _chain, "sign": _sign}
SCENES_2D = {"smooth_union": _circles, "sign": _sign2d}


def scenes_for(grid):
    return SCENES_2D if len(GRIDS[grid]) == 2 else SCENES_3D


def build(scene, grid):
    return scenes_for(grid)[scene](ns)


def coords(axes):
    """The (3, N) float64 coordinate array of the grid (z fastest), what create() takes."""
    ax = [np.asarray(a, dtype=np.float64) for a in axes] + [np.zeros(1)] * (3 - len(axes))
    g = np.meshgrid(*ax, indexing="ij")
    return np.stack([x.ravel() for x in g])
