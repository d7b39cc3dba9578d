"""GPU: interval enclosures (aegolius_amd.enclosure) — soundness against create() with tolerance zero, the Lipschitz
ball, agreement with the float64 restatement (tests/enclosure_reference.py), and the octree: volume brackets, bounding
boxes, classification, the refusal of a refinement that outgrows max_boxes."""
import numpy as np
import pytest

import aegolius_amd.cores as ns
import enclosure_reference as ref
import enclosure_scenes as S
from aegolius_amd import enclosure
from aegolius_amd.render import lower

pytestmark = pytest.mark.gpu

N_BOXES, PER_BOX = 4097, 64          # 64 waves and a tail

_cache = {}


def _case(name):
    """Per scene, once: boxes, the GPU's enclosures, create() at the sample points, the restatement."""
    if name not in _cache:
        build, size = S.SCENES[name]
        geometry = build(ns)
        low, _ = lower(geometry)
        lo, hi = S.boxes(name, size, N_BOXES)
        rows = slice(0, len(size))
        glo, ghi = enclosure.enclose(geometry, lo[rows], hi[rows])
        pts = S.sample_points(lo, hi, PER_BOX)
        f = np.asarray(build(ns).create(pts.astype(np.float64)), dtype=np.float32).reshape(N_BOXES, PER_BOX)
        rlo, rhi, mag = ref.enclose(low, enclosure.factors(low), lo, hi, enclosure.pad_ulps())
        T = len(low.code) * enclosure.pad_ulps() * 2.0 ** -23 * mag
        _cache[name] = dict(geometry=geometry, low=low, lo=lo, hi=hi, glo=glo, ghi=ghi, f=f, rlo=rlo, rhi=rhi, T=T, size=size)
    return _cache[name]


@pytest.mark.parametrize("name", sorted(S.SCENES))
def test_sound(engine, name):
    c = _case(name)
    glo, ghi, f = c["glo"], c["ghi"], c["f"]
    assert glo.dtype == np.float32 and ghi.dtype == np.float32 and glo.shape == (N_BOXES,) and ghi.shape == (N_BOXES,)
    assert not np.any(np.isnan(glo)) and not np.any(np.isnan(ghi))
    assert not np.any(np.isnan(f))
    below, above = f < glo[:, None], f > ghi[:, None]
    worst = float(max(np.max(glo[:, None] - f), np.max(f - ghi[:, None])))
    print("%s: %d values outside their enclosure, worst excess %.3e, median width %.3e"
          % (name, int(below.sum() + above.sum()), worst, float(np.median(ghi - glo))))
    assert not below.any(), "box %d: a value below its enclosure" % int(np.argmax(below.any(axis=1)))     # tolerance zero
    assert not above.any(), "box %d: a value above its enclosure" % int(np.argmax(above.any(axis=1)))


@pytest.mark.parametrize("name", sorted(S.SCENES))
def test_agrees_with_the_restatement(engine, name):
    """Each interval lies inside the other widened by T: a rule that is sound only because it returns something huge
    does not pass."""
    c = _case(name)
    glo, ghi = c["glo"].astype(np.float64), c["ghi"].astype(np.float64)
    rlo, rhi, T = c["rlo"], c["rhi"], c["T"]
    ok = (glo >= rlo - T) & (ghi <= rhi + T) & (rlo >= glo - T) & (rhi <= ghi + T)          # (equal infinities compare true)
    with np.errstate(invalid="ignore"):
        diff = np.maximum(np.abs(glo - rlo), np.abs(ghi - rhi))
    excess = np.where(np.isfinite(diff), diff, 0.0) - T
    print("%s: %d boxes disagree, largest |difference| - T = %.3e" % (name, int((~ok).sum()), float(excess.max())))
    assert ok.all(), "box %d: GPU [%r, %r], restatement [%r, %r], T %r" % (
        int(np.argmin(ok)), glo[np.argmin(ok)], ghi[np.argmin(ok)], rlo[np.argmin(ok)], rhi[np.argmin(ok)], T[np.argmin(ok)])


@pytest.mark.parametrize("name", S.FINITE_L)
def test_never_looser_than_the_lipschitz_ball(engine, name):
    c = _case(name)
    L = float(c["low"].lipschitz)
    assert np.isfinite(L)
    lo32, hi32 = c["lo"], c["hi"]
    centre = np.float32(0.5) * lo32 + np.float32(0.5) * hi32                       # the kernel's centre, in float32
    fc = np.asarray(S.SCENES[name][0](ns).create(centre.astype(np.float64)), dtype=np.float64)
    lo64, hi64 = lo32.astype(np.float64), hi32.astype(np.float64)
    r = np.sqrt(np.sum(np.maximum(hi64 - centre, centre - lo64) ** 2, axis=0))
    T = c["T"]
    glo, ghi = c["glo"].astype(np.float64), c["ghi"].astype(np.float64)
    print("%s: largest hi - (f(c) + L r + T) = %.3e, largest (f(c) - L r - T) - lo = %.3e"
          % (name, float(np.max(ghi - (fc + L * r + T))), float(np.max((fc - L * r - T) - glo))))
    assert np.all(ghi <= fc + L * r + T)
    assert np.all(glo >= fc - L * r - T)
    flat = np.all(lo32 == hi32, axis=0)
    assert flat.sum() > 100 and np.all((ghi - glo)[flat] <= 2 * T[flat])


def test_empty_and_single(engine):
    c = _case("cfg2")
    lo, hi = enclosure.enclose(c["geometry"], np.zeros((3, 0)), np.zeros((3, 0)))
    assert lo.shape == (0,) and hi.shape == (0,) and lo.dtype == np.float32
    for k in (0, 1, 100, N_BOXES - 1):
        lo, hi = enclosure.enclose(c["geometry"], c["lo"][:, k:k + 1], c["hi"][:, k:k + 1])
        assert lo[0] == c["glo"][k] and hi[0] == c["ghi"][k]
    # float64 ends are rounded outward: the enclosure of the rounded box
    lo64 = c["lo"][:, :64].astype(np.float64) + 1e-12
    hi64 = np.maximum(c["hi"][:, :64].astype(np.float64) + 3e-12, lo64)
    lo32, hi32 = enclosure.round_out(lo64, hi64)
    a = enclosure.enclose(c["geometry"], lo64, hi64)
    b = enclosure.enclose(c["geometry"], lo32, hi32)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


# ---- octree ------------------------------------------------------------------------------------------------------------
# The Box is rotated and moved so that its faces lie in no plane of the octree: a box aligned with the dyadic planes has
# whole faces that fall just inside or just outside a layer of cells at alternating depths, and its bracket shrinks by
# 3/4 and 1/4 in turns instead of the 1/2 per level that "mixed leaves scale with the surface" describes.
def _placed(b):
    b.rotate(0.7, (1, 2, 3))
    b.move((0.1, -0.05, 0.08))
    return b


def _twisted():
    b = ns.Box(0.6, 0.3, 0.2)
    b.twist(np.pi / 2)
    return _placed(b)


SOLIDS = {
    "sphere": (lambda: ns.Sphere(0.5), 4.0 * np.pi * 0.5 ** 3 / 3.0),
    "box": (lambda: _placed(ns.Box(0.6, 0.3, 0.2)), 0.6 * 0.3 * 0.2),
    "twisted_box": (_twisted, 0.6 * 0.3 * 0.2),          # a twist preserves volume
}
DOMAIN = (2, 2, 2)


@pytest.mark.parametrize("name", sorted(SOLIDS))
def test_volume_bounds(engine, name):
    build, volume = SOLIDS[name]
    width = {}
    for depth in range(3, 8):
        v = enclosure.volume_bounds(build(), DOMAIN, depth=depth)
        print("%s depth %d: %.9g <= %.9g <= %.9g, width %.6g, mixed leaves %d" % (name, depth, v.lower, volume, v.upper, v.width, v.mixed[-1]))
        assert v.lower <= volume <= v.upper
        assert len(v.inside) == depth + 1 and v.inside[0] + v.outside[0] + v.mixed[0] == 1
        for l in range(depth):
            assert v.inside[l + 1] + v.outside[l + 1] + v.mixed[l + 1] == 8 * v.mixed[l]
        width[depth] = v.width
    for d in (4, 5, 6):
        assert width[d + 1] <= 0.75 * width[d]
    again = enclosure.volume_bounds(build(), DOMAIN, depth=7)
    assert (again.lower, again.upper, again.inside, again.outside, again.mixed) == (v.lower, v.upper, v.inside, v.outside, v.mixed)
    assert np.float64(again.lower).tobytes() == np.float64(v.lower).tobytes()


@pytest.mark.parametrize("name", sorted(SOLIDS))
def test_bounding_box(engine, name):
    build, _ = SOLIDS[name]
    depth = 6
    lo, hi, tight = enclosure.bounding_box(build(), DOMAIN, depth=depth)
    assert tight
    co, _res = ns.generate_grid(DOMAIN, (65, 65, 65))
    co = np.asarray(co, dtype=np.float32)
    f = build().create(co.astype(np.float64))
    inside = co[:, np.asarray(f) <= 0].astype(np.float64)
    assert inside.shape[1] > 0
    assert np.all(inside >= lo[:, None]) and np.all(inside <= hi[:, None])
    again = enclosure.bounding_box(build(), DOMAIN, depth=depth)
    assert np.array_equal(again[0], lo) and np.array_equal(again[1], hi) and again[2] == tight
    if name == "sphere":
        leaf = 2.0 / (1 << depth)
        assert np.all(lo <= -0.5) and np.all(lo >= -0.5 - 2 * leaf) and np.all(hi >= 0.5) and np.all(hi <= 0.5 + 2 * leaf)


def test_bounding_box_outside_and_cut(engine):
    far = ns.Sphere(0.5)
    far.move((5.0, 0.0, 0.0))
    assert enclosure.bounding_box(far, DOMAIN, depth=5) is None
    v = enclosure.volume_bounds(far, DOMAIN, depth=5)
    assert v.lower == 0.0 and v.upper == 0.0
    cut = ns.Sphere(0.5)
    cut.move((0.8, 0.0, 0.0))
    lo, hi, tight = enclosure.bounding_box(cut, DOMAIN, depth=5)
    assert not tight and hi[0] == 1.0 and lo[0] <= 0.3
    # a 2-D scene through the quadtree
    lo, hi, tight = enclosure.bounding_box(ns.Circle(0.4), (2, 2), depth=6)
    leaf = 2.0 / 64
    assert tight and lo.shape == (2,) and np.all(lo <= -0.4) and np.all(lo >= -0.4 - 2 * leaf) and np.all(hi >= 0.4) and np.all(hi <= 0.4 + 2 * leaf)
    a = enclosure.volume_bounds(ns.Circle(0.4), (2, 2), depth=7)
    assert a.lower <= np.pi * 0.16 <= a.upper and a.width < 0.1


# Subdivisions (unequal, odd and even counts). A box can only be decided where the rules are not loose by design: cfg 3
# repeats with cells of 2 and twists by pi / 2 per unit of z, so a box must be small against the cell (a box of width w
# crosses a cell border, and becomes the whole cell, with probability about 3 w / 2) and turn by well under a radian:
# w = 4 / 32 crosses one time in five and turns by 0.2 rad. cfg 2 and cfg 4 have neither and are decided at a third of a unit.
DIVISIONS = {"cfg2": (12, 9, 7), "cfg3": (33, 31, 29), "cfg4": (12, 9)}


@pytest.mark.parametrize("name", sorted(DIVISIONS))
def test_classify(engine, name):
    """classify() is statuses(enclose(subdivision())) by definition, so the comparison with that expression checks only its
    plumbing (shape, order of the boxes, dtype); the independent check is the last one: a box called inside or outside
    holds only sample points of create() on that side."""
    build, size = S.SCENES[name]
    div = DIVISIONS[name]
    status = enclosure.classify(build(ns), size, div)
    assert status.dtype == np.int8 and status.shape == div
    lo, hi, shape = enclosure.subdivision(size, div)
    assert shape == div
    elo, ehi = enclosure.enclose(build(ns), lo[:len(size)], hi[:len(size)])
    want = np.where(ehi <= np.float32(0.0), -1, np.where(elo > np.float32(0.0), 1, 0)).astype(np.int8).reshape(div)
    assert np.array_equal(status, want)
    assert (status == 1).any() and (status == 0).any()
    # boxes called inside / outside hold only points of that side
    pts = S.sample_points(lo, hi, 16)
    f = np.asarray(build(ns).create(pts.astype(np.float64))).reshape(-1, 16)
    flat = status.ravel()
    assert np.all(f[flat == -1] <= 0) and np.all(f[flat == 1] > 0)


def test_max_boxes_refusal(engine):
    """A refinement that outgrows max_boxes is refused cleanly (the kernel never writes past the list's capacity) and the
    device stays usable."""
    sphere = ns.Sphere(0.5)
    with pytest.raises(ValueError, match=r"max_boxes = 64: level \d+ .* needs \d+ boxes"):
        enclosure.volume_bounds(sphere, DOMAIN, depth=6, max_boxes=64)
    with pytest.raises(ValueError, match=r"max_boxes = 64"):
        enclosure.bounding_box(sphere, DOMAIN, depth=6, max_boxes=64)
    lo, hi = enclosure.enclose(sphere, np.array([[-0.1], [-0.1], [-0.1]]), np.array([[0.1], [0.1], [0.1]]))
    assert lo[0] <= -0.5 <= hi[0] and hi[0] < 0.0
    v = enclosure.volume_bounds(sphere, DOMAIN, depth=4, max_boxes=4096)
    assert v.lower <= 4.0 * np.pi * 0.125 / 3.0 <= v.upper
