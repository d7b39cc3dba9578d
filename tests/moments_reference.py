"""numpy restatement of the definition of aegolius_amd.moments (the test oracle of the moments kernels and of the host
conversion); shares no code with the package's moments module. Lattice, tables, scenes and grids: tests/occupancy_reference.py.

Sub-sample j of cell i on an axis of n cells with k sub-samples has the fine index g = i k + j and the odd lattice coordinate
u = 2 g + 1. M = the sums of 1, u_a, u_a u_b over the inside sub-samples: (N, U0, U1, U2, U00, U01, U02, U11, U12, U22) in
3-D, (N, U0, U1, U00, U01, U11) in 2-D, as Python ints. World quantities: h = (a[-1] - a[0]) / (n - 1) and lo = a_0 - h / 2
in float64, s = h / k, sample u at lo + u s / 2; everything after that in exact rational arithmetic (world())."""
from fractions import Fraction

import numpy as np

import occupancy_reference as occ
from oracle import sdf_oracle


def _ints(values):
    return np.array([int(v) for v in values], dtype=object)


def lattice_moments(inside, axes, k):
    """The integer tuple M of a boolean field on the fine grid occupancy_reference.tables(axes, k) span (its layout: z
    fastest). The counts are added by numpy (small), the weights and weighted sums are Python ints."""
    d = len(axes)
    ks = occ.per_axis(axes, k)
    n = [a.size for a in occ.three(axes)]
    fine = [n[a] * ks[a] for a in range(3)]
    b = np.asarray(inside, dtype=bool).reshape(fine)
    u = [_ints(2 * g + 1 for g in range(fine[a])) for a in range(d)]
    first, second = [], []
    for a in range(d):
        line = _ints(b.sum(axis=tuple(x for x in range(3) if x != a), dtype=np.int64))
        first.append(int((line * u[a]).sum()))
        for c in range(a, d):
            if c == a:
                second.append(int((line * u[a] * u[a]).sum()))
            else:
                plane = b.sum(axis=tuple(x for x in range(3) if x not in (a, c)), dtype=np.int64)
                weights = u[a][:, None] * u[c][None, :]
                second.append(int(sum(int(v) * int(w) for v, w in zip(plane.ravel(), weights.ravel()))))
    return (int(b.sum(dtype=np.int64)),) + tuple(first) + tuple(second)


def brute_moments(inside, axes, k):
    """The same by a loop over the inside sub-samples (for small fields: the check of lattice_moments itself)."""
    d = len(axes)
    ks = occ.per_axis(axes, k)
    fine = [a.size * ks[i] for i, a in enumerate(occ.three(axes))]
    M = [0] * (1 + d + d * (d + 1) // 2)
    for g in np.argwhere(np.asarray(inside, dtype=bool).reshape(fine)):
        u = [2 * int(g[a]) + 1 for a in range(d)]
        M[0] += 1
        at = 1 + d
        for a in range(d):
            M[1 + a] += u[a]
            for c in range(a, d):
                M[at] += u[a] * u[c]
                at += 1
    return tuple(M)


def oracle_fields(geometry, axes, k, level):
    """(inside, knife-edge) per sub-sample by the float64 oracle, occupancy_reference.oracle_counts' definition before its
    block sums: on the knife edge when |f - level| <= 1e-6 max(1, |f|, magnitude)."""
    lv = float(np.float32(level))
    f, mag = sdf_oracle.evaluate_with_magnitude(geometry, occ.grid_points(occ.tables(axes, k)))
    return f <= lv, np.abs(f - lv) <= 1e-6 * np.maximum(1.0, np.maximum(np.abs(f), mag))


def lattice(axes, k):
    """(lo, s) per axis as Fractions of the float64 values the definition names."""
    lo, s = [], []
    for a in axes:
        a = np.asarray(a, dtype=np.float64)
        h = (a[-1] - a[0]) / (a.size - 1)
        lo.append(Fraction(float(a[0] - h / 2.0)))
        s.append(Fraction(float(h)) / k)
    return lo, s


def world(M, axes, k, density):
    """volume, mass, centroid, second_moments and inertia (3-D) or polar (2-D) from M by the formulas of the module text,
    in exact rational arithmetic, rounded to float64 once at the end. The empty solid: zeros and a NaN centroid."""
    d = len(axes)
    lo, s = lattice(axes, k)
    rho = Fraction(float(density))
    N, U, second = M[0], M[1:1 + d], M[1 + d:]
    dV = Fraction(1)
    for x in s:
        dV *= x
    volume = N * dV
    S = [[Fraction(0)] * d for _ in range(d)]
    at = 0
    for a in range(d):
        for c in range(a, d):
            if N:
                S[a][c] = S[c][a] = rho * dV * (s[a] * s[c] / 4) * (second[at] - Fraction(U[a] * U[c], N))
                if a == c:
                    S[a][a] += rho * dV * N * s[a] * s[a] / 12
            at += 1
    out = {"volume": float(volume), "mass": float(rho * volume),
           "centroid": np.array([float(lo[a] + Fraction(U[a], N) * s[a] / 2) if N else np.nan for a in range(d)]),
           "second_moments": np.array([[float(v) for v in row] for row in S])}
    trace = sum(S[a][a] for a in range(d))
    if d == 3:
        out["inertia"] = np.array([[float((trace if a == c else 0) - S[a][c]) for c in range(3)] for a in range(3)])
    else:
        out["polar"] = float(trace)
    return out


def box_moments(first, count):
    """M of the box of sub-cells first_a <= g_a < first_a + count_a (fine indices), in closed form per axis."""
    d = len(first)
    one = list(count)
    lin = [sum(2 * g + 1 for g in range(f, f + c)) for f, c in zip(first, count)]
    sq = [sum((2 * g + 1) ** 2 for g in range(f, f + c)) for f, c in zip(first, count)]
    total = 1
    for c in count:
        total *= c
    M = [total] + [lin[a] * (total // one[a]) for a in range(d)]
    for a in range(d):
        for c in range(a, d):
            M.append(sq[a] * (total // one[a]) if a == c else lin[a] * lin[c] * (total // (one[a] * one[c])))
    return tuple(M)


def ulp_distance(got, want, scale=None):
    """max |got - want| in units of the float64 spacing at max(|want|, scale) (per element)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    at = np.abs(want) if scale is None else np.maximum(np.abs(want), scale)
    return float(np.max(np.abs(got - want) / np.spacing(at)))
