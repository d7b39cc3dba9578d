"""Float64 reference of aegolius_amd.render.spans / thickness: the span march over a field (the rule of the module text of
render.py and of csrc/sdfk_raydev.h, operation by operation but in float64), closed-form crossings of rays with a sphere,
a spherical shell and a rotated box, and the ray sample and comparisons that the CPU and the GPU span tests share. Test
infrastructure — never on a product code path."""
import numpy as np

import render_reference as ref

COMPLETE, LIMIT = 0, 2


class Spans:
    """chord, count, inside0, status, steps (n,), crossings (K, n) NaN past count, t_last (n,): the last evaluated t."""

    def __init__(self, n, k):
        self.chord = np.zeros(n)
        self.count = np.zeros(n, dtype=np.int32)
        self.inside0 = np.zeros(n, dtype=bool)
        self.status = np.full(n, LIMIT, dtype=np.uint8)
        self.steps = np.zeros(n, dtype=np.int32)
        self.crossings = np.full((k, n), np.nan)
        self.t_last = np.zeros(n)


def trace_spans(field, origins, directions, t_min, t_max, eps, cone, lipschitz, max_steps, max_crossings):
    """The span march in float64, vectorised over the rays that still march. field: (3, n) float64 -> (n,). -> Spans."""
    o = np.asarray(origins, dtype=np.float64)
    d = np.asarray(directions, dtype=np.float64)
    n, k = o.shape[1], int(max_crossings)
    out = Spans(n, k)
    t = np.full(n, float(t_min))
    t_prev = t.copy()
    f_prev = np.zeros(n)
    t_in = t.copy()
    was = np.zeros(n, dtype=bool)
    inv_l = 1.0 / float(lipschitz)
    active = np.arange(n)
    for e in range(int(max_steps)):
        if active.size == 0:
            break
        a = active
        ta = t[a]
        f = field(o[:, a] + ta * d[:, a])
        inside = f <= 0.0
        if e == 0:
            was[a] = inside
            out.inside0[a] = inside
        else:
            ch = inside != was[a]
            c, fc, tp = a[ch], f[ch], t_prev[a[ch]]
            af = np.abs(f_prev[c])
            tc = tp + (ta[ch] - tp) * (af / (af + np.abs(fc)))
            keep = out.count[c] < k
            out.crossings[out.count[c][keep], c[keep]] = tc[keep]
            out.count[c] += 1
            enter = inside[ch]
            t_in[c[enter]] = tc[enter]
            out.chord[c[~enter]] += tc[~enter] - t_in[c[~enter]]
            was[c] = enter
        thr = np.maximum(eps, cone * ta)
        t_prev[a] = ta
        f_prev[a] = f
        t_next = ta + np.maximum(np.abs(f) * inv_l, thr)
        out.steps[a] += 1
        stuck = ~(t_next > ta)                                  # (status stays LIMIT)
        t[a[~stuck]] = t_next[~stuck]
        done = ~stuck & (t_next > t_max)
        fin = a[done]
        out.chord[fin[was[fin]]] += t_max - t_in[fin[was[fin]]]
        out.status[fin] = COMPLETE
        active = a[~stuck & ~done]
    lim = np.flatnonzero((out.status == LIMIT) & was)
    out.chord[lim] += t_prev[lim] - t_in[lim]
    out.t_last = t_prev
    return out


def intervals(crossings, count, inside0, status, t_min, t_max, t_last):
    """(t_enter, t_exit) pairs of ONE ray from all its crossings: what RaySpans.intervals returns."""
    ts = [float(x) for x in crossings[:int(count)]]
    if inside0:
        ts.insert(0, float(t_min))
    if len(ts) % 2:
        ts.append(float(t_max) if status == COMPLETE else float(t_last))
    return list(zip(ts[0::2], ts[1::2]))


# ---- closed forms: ALL crossings of a ray, t in (t_min, t_max) ---------------------------------------------------------------
def _sphere_roots(o, d, centre, radius):
    oc = o - np.asarray(centre, dtype=np.float64)[:, None]
    b = (oc * d).sum(axis=0)
    disc = b * b - ((oc * oc).sum(axis=0) - radius * radius)
    root = np.sqrt(np.where(disc > 0, disc, np.nan))
    return np.stack([-b - root, -b + root])


def _box_roots(o, d, size, rotation, centre):
    R = np.asarray(rotation, dtype=np.float64)
    ol = R.T.dot(o - np.asarray(centre, dtype=np.float64)[:, None])
    dl = R.T.dot(d)
    half = 0.5 * np.asarray(size, dtype=np.float64)[:, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        t1, t2 = (-half - ol) / dl, (half - ol) / dl
    lo, hi = np.minimum(t1, t2), np.maximum(t1, t2)
    par = dl == 0
    within = np.abs(ol) <= half
    lo = np.where(par, np.where(within, -np.inf, np.inf), lo)
    hi = np.where(par, np.where(within, np.inf, -np.inf), hi)
    t_in, t_out = lo.max(axis=0), hi.min(axis=0)
    ok = t_in < t_out
    return np.stack([np.where(ok, t_in, np.nan), np.where(ok, t_out, np.nan)])


SHELL_R, SHELL_W, SHELL_S = 0.3, 0.05, 2.5


def shell():
    """Sphere(0.3).onion(0.05) rescaled by 2.5: the solid between the spheres of radius 0.625 and 0.875."""
    return ref.onion_scaled()


def bodies():
    """name -> (float64 field, all roots of the LINE (o, d) -> (R, n) sorted per ray with NaN for none, geometry builder)."""
    from test_render_cpu import closed_form_cases
    cases = closed_form_cases()
    c = np.array([0.2, -0.1, 0.15])
    r_in, r_out = (SHELL_R - SHELL_W) * SHELL_S, (SHELL_R + SHELL_W) * SHELL_S

    def shell_field(p):
        return np.abs(np.linalg.norm(p, axis=0) - SHELL_R * SHELL_S) - SHELL_W * SHELL_S

    def shell_roots(o, d):
        return np.sort(np.concatenate([_sphere_roots(o, d, (0, 0, 0), r_out), _sphere_roots(o, d, (0, 0, 0), r_in)]), axis=0)
    # the rotated box of the render tests: its field and builder from there, its size / rotation / centre restated
    from test_render_cpu import _rot
    R, bc, size = _rot(0.7, (1, 2, 0.5)), np.array([-0.1, 0.2, 0.05]), np.array([0.9, 0.6, 0.5])
    return {
        "sphere": (cases["sphere"][0], lambda o, d: _sphere_roots(o, d, c, 0.5), cases["sphere"][2]),
        "shell": (shell_field, shell_roots, shell),
        "box": (cases["box"][0], lambda o, d: _box_roots(o, d, size, R, bc), cases["box"][2]),
    }


def exact(field, roots_of, o, d, t_min, t_max):
    """-> (roots (R, n) inside (t_min, t_max), sorted, NaN-padded at the end; exact count (n,); exact chord (n,))."""
    r = roots_of(o, d)
    r = np.where((r > t_min) & (r < t_max), r, np.nan)
    r = np.sort(r, axis=0)                                      # NaN last
    count = np.isfinite(r).sum(axis=0)
    knots = np.concatenate([np.full((1, r.shape[1]), float(t_min)), np.where(np.isfinite(r), r, float(t_max)),
                            np.full((1, r.shape[1]), float(t_max))])
    chord = np.zeros(r.shape[1])
    for a, b in zip(knots[:-1], knots[1:]):
        chord += np.where(field(o + 0.5 * (a + b) * d) <= 0.0, b - a, 0.0)
    return r, count, chord


def incidence(field, o, d, roots):
    """|d f / d t| of the exact distance field at the roots (central difference, h = 1e-6): the cosine between the ray and
    the surface normal there. (R, n), NaN where there is no root."""
    h = 1e-6
    out = np.full(roots.shape, np.nan)
    for k, r in enumerate(roots):
        ok = np.isfinite(r)
        rr = np.where(ok, r, 0.0)
        out[k] = np.where(ok, np.abs(field(o + (rr + h) * d) - field(o + (rr - h) * d)) / (2 * h), np.nan)
    return out


def sample_rays(n=20000, seed=23):
    """Jittered rays: a third from the perspective eye of the render tests into the unit ball, a third nearly parallel
    ones from the plane x = 3, a third from random origins (some inside the bodies) in random directions. (3, n) float64,
    unit directions."""
    rng = np.random.default_rng(seed)
    m = n // 3
    eye = np.asarray(ref.EYE, dtype=np.float64)[:, None]
    aim = rng.normal(size=(3, m))
    aim *= rng.uniform(0.0, 1.0, m) ** (1.0 / 3.0) / np.linalg.norm(aim, axis=0)
    o1, d1 = np.repeat(eye, m, axis=1), aim - eye
    o2 = np.stack([np.full(m, 3.0), rng.uniform(-1.1, 1.1, m), rng.uniform(-1.1, 1.1, m)])
    d2 = np.stack([-np.ones(m), rng.uniform(-0.02, 0.02, m), rng.uniform(-0.02, 0.02, m)])
    o3 = rng.uniform(-1.2, 1.2, (3, n - 2 * m))
    d3 = rng.normal(size=(3, n - 2 * m))
    o, d = np.concatenate([o1, o2, o3], axis=1), np.concatenate([d1, d2, d3], axis=1)
    return o, d / np.linalg.norm(d, axis=0)


OPTIONS = ((1e-3, 0.0), (1e-4, 2e-3), (1e-2, 0.0))     # (eps, cone) of the closed-form tests
T_MIN, T_MAX = 0.0, 8.0                                  # (every root of the sample lies below 7: none near t_max)
THIN_CAP = 0.02


def check_closed_form(got, roots, n_exact, chord_exact, eps, cone, thin_extra=None, tol_extra=None):
    """The conditions of the closed-form test on a result with fields count, chord, crossings (K >= the largest exact
    count). A ray is THIN when two of its exact roots lie closer than 4 thr (or `thin_extra` marks it). thr is taken at
    the exact root: the bracket of a crossing is the floor step max(eps, cone t_prev) from t_prev below the root, no longer
    than that. tol_extra (R, n): what an fp32 tracer adds to the tolerance of each crossing. -> the share of thin rays.
      not thin: count = exact; |crossing_k - root_k| <= thr_k (+ extra); |chord - exact| <= sum_k (thr_k (+ extra))
      thin    : count = exact - 2 j, j >= 0; chord <= exact + 2 thr (+ extras), thr the largest of the ray."""
    thr = np.maximum(eps, cone * np.where(np.isfinite(roots), roots, 0.0))
    thr = np.where(np.isfinite(roots), thr, 0.0)
    extra = np.zeros_like(thr) if tol_extra is None else np.where(np.isfinite(roots), tol_extra, 0.0)
    gap = np.diff(roots, axis=0)
    with np.errstate(invalid="ignore"):
        thin = np.any(gap < 4.0 * np.maximum(thr[:-1], thr[1:]), axis=0)
    if thin_extra is not None:
        thin = thin | thin_extra
    ok = ~thin
    count = np.asarray(got.count)
    chord = np.asarray(got.chord, dtype=np.float64)
    cross = np.asarray(got.crossings, dtype=np.float64)
    assert cross.shape[0] >= roots.shape[0]
    assert np.array_equal(count[ok], n_exact[ok])
    err = np.abs(cross[:roots.shape[0]] - roots)
    has = np.isfinite(roots)
    assert np.all(np.isnan(cross[:roots.shape[0]][:, ok][~has[:, ok]]))           # nothing stored past the count
    assert np.all(np.isnan(cross[roots.shape[0]:][:, ok]))
    tol = thr + extra + 1e-12
    worst = float((err[:, ok][has[:, ok]] / tol[:, ok][has[:, ok]]).max()) if has[:, ok].any() else 0.0
    assert np.all(err[:, ok][has[:, ok]] <= tol[:, ok][has[:, ok]]), worst
    assert np.all(np.abs(chord - chord_exact)[ok] <= tol.sum(axis=0)[ok])
    missed = n_exact[thin] - count[thin]
    assert np.all((missed >= 0) & (missed % 2 == 0))
    assert np.all(chord[thin] <= chord_exact[thin] + 2.0 * thr.max(axis=0)[thin] + extra.sum(axis=0)[thin] + 1e-12)
    return float(thin.mean()), worst


# ---- the oracle scenes: the reference and the rays it is ill-conditioned on -------------------------------------------------
SCENE_EPS, SCENE_CONE, SCENE_STEPS, SCENE_K = 2e-3, 0.0, 1024, 16


def shifted_field(geometry, lipschitz, sign):
    """The oracle moved by sign * slack (render_reference.slack: what an fp32 evaluation may differ by)."""
    def field(p):
        f, s = ref.slack(geometry, p, lipschitz)
        return f + sign * s
    return field


def conditioned_reference(geometry, lipschitz, o, d, t_min, t_max, eps, cone, max_steps, k):
    """-> (the reference spans over the oracle, ill (n,) bool). A ray is ILL-CONDITIONED, by the reference alone, when its
    count changes with the oracle shifted by +slack or by -slack, when two of its stored crossings are closer than 2 thr,
    or when it reaches the step limit."""
    base = trace_spans(ref.oracle_field(geometry), o, d, t_min, t_max, eps, cone, lipschitz, max_steps, k)
    ill = base.status == LIMIT
    for sign in (-1.0, 1.0):
        other = trace_spans(shifted_field(geometry, lipschitz, sign), o, d, t_min, t_max, eps, cone, lipschitz, max_steps, k)
        ill |= other.count != base.count
    thr = np.maximum(eps, cone * base.crossings)
    with np.errstate(invalid="ignore"):
        ill |= np.any(np.diff(base.crossings, axis=0) < 2.0 * np.maximum(thr[:-1], thr[1:]), axis=0)
    return base, ill
