"""Sphere tracing of geometries on the GPU: ray casts, depth / normal images, spans — every crossing of a ray with
the solid, chords and thickness images — and secondary rays: visibility of segments, soft shadows and ambient occlusion
(kernels: csrc/sdfk_rays.inc).

    from aegolius_amd import render
    cam = render.Camera(eye=(2.2, 1.6, 1.9), target=(0, 0, 0), fov=40)
    img = render.render(geometry, cam, 1920, 1080, t_min=0.0, t_max=8.0)
    img.save_pgm("part.pgm", img.shade(light=(1, 1, 2)))
    hits = render.cast(geometry, origins, directions, t_max=8.0)          # arbitrary rays, (3, N) arrays
    sp = render.spans(geometry, origins, directions, t_max=8.0)           # every crossing, the chord, parity
    xray = render.thickness(geometry, cam, 1920, 1080, t_max=8.0)         # chord per pixel: a radiograph
    render.illuminate(geometry, img, render.Light.directional((1, 1, 2)), ao_radius=0.2)     # img.shadow, img.ao
    img.save_pgm("lit.pgm", img.shade(light=(1, 1, 2), shadow=img.shadow, occlusion=img.ao))
    free = render.visibility(geometry, origins, directions, t_max=3.0)    # is the segment clear of the solid?

No field and no grid are made: the geometry's program (create()'s own) is evaluated along every ray.

The marching rule (one definition: the kernels, tests/render_reference.py and this text), per ray, in float32:

    t = t_min
    repeat at most max_steps times:
        f   = field(o + t d)                      # fmaf(t, d, o) per component
        thr = max(eps, cone * t)
        if f <= thr: status = HIT; stop           # a ray that starts inside or within thr of the surface hits at t_min
        t   = t + f / L                           # fmaf(f, float32(1 / L), t); steps += 1
        if t > t_max: status = MISS; stop
    otherwise: status = LIMIT                     # never folded into hit or miss

L is a Lipschitz bound of the field with respect to the point, so that a step can never cross the surface. The lowering
tracks it (`LoweredProgram.lipschitz`: 1 for distance functions under rigid transforms, the matrix 2-norm under shear,
sqrt(2) for an extrusion, the sum for SUM, ...). Where it is infinite — twist, bend, repetition cells, sign, nearest
instance — the caller must pass `lipschitz=` (the usual "step scale" of sphere tracers; too small a value lets rays
pass through the surface, and that is the caller's responsibility). Trees that need a staged evaluation (signed,
conv_*, custom_*, Python callables) are refused with autodiff.UnsupportedOpError, as the derivative paths do.

`steps` counts the advances of t (int32): 0 for a ray that hits at t_min, so a hit ray cost steps + 1 evaluations.
2-D geometries ignore z: they trace as infinite prisms along z.

Pixel (ix, iy) of a W x H image, row iy = 0 at the top; a = (2 ix + 1) / W - 1, b = 1 - (2 iy + 1) / H; with the unit
vectors fwd = (target - eye) / |target - eye|, right = fwd x up / |fwd x up|, upv = right x fwd:

    perspective : o = eye,                  d = normalised(fwd + a du + b dv),  du = right tan(fov / 2) W / H,
                                                                                dv = upv tan(fov / 2)
    orthographic: o = eye + a du + b dv,    d = fwd,                            du = right (height / 2) W / H,
                                                                                dv = upv height / 2

(`fov`: the vertical field of view in degrees; `height`: the world height of the orthographic image.) `render` hands
the kernel the record {eye, fwd, du, dv} in float32 and the kernel generates the rays itself — no ray array exists;
`Camera.rays` is the same formula on the host in float64. The hit threshold is the pixel's footprint: `cone` defaults
to tan(fov / 2) / H, half the angular size of a pixel (orthographic: `eps` defaults to height / (2 H), half a pixel).

Spans: what lies behind the first surface. `spans` (arbitrary rays) and `thickness` (camera rays) march on through the
solid { f <= 0 } and report every entry and exit crossing and the length of the ray inside it, the chord (one definition:
the kernels, tests/spans_reference.py and this text), per ray, in float32:

    t = t_min; count = 0; chord = 0
    repeat at most max_steps times (evaluation index e = 0, 1, ...):
        f      = field(o + t d)                       # fmaf(t, d, o) per component
        inside = (f <= 0)
        if e == 0:  was = inside; inside0 = inside; t_in = t_min       # starting inside is not a crossing
        else if inside != was:                                        # a sign change between t_prev and t
            tc = fmaf(t - t_prev, |f_prev| / (|f_prev| + |f|), t_prev)   # secant; the denominator is > 0
            if count < K: crossings[count] = tc
            count += 1
            if inside: t_in = tc   else: chord += tc - t_in
            was = inside
        thr    = max(eps, cone * t)
        t_prev = t; f_prev = f
        t_next = t + max(|f| * (1/L), thr)            # float32(1 / L); steps += 1
        if not (t_next > t): status = LIMIT; stop     # no progress in float32: never loop in place
        t = t_next
        if t > t_max: if was: chord += t_max - t_in;  status = COMPLETE; stop
    otherwise: status = LIMIT
    on LIMIT, either way: if was: chord += t_prev - t_in              # t_prev: the last evaluated parameter

With a valid bound L a step of |f| / L cannot cross the surface, so the sign changes only inside floor steps of length
thr: the inside / outside state at every evaluated point is the field's own, every recorded crossing is bracketed within
thr, and only features thinner than thr along the ray can be missed, and then as a pair of crossings. `eps` must be
positive and at least 2^-20 max(|t_min|, |t_max|), so that a floor step always advances t in float32. `count` counts all
crossings, `crossings` keeps the first K = max_crossings (0 to 32) of them; `steps` counts the evaluations. Parity gives
point-in-solid (`inside0`, or count odd for a ray from outside), the chord is the optical path length through the part,
`intervals` the wall thicknesses along a ray, and `ThicknessImage.volume()` of an orthographic image the ray-integrated
volume to put next to `enclosure.volume_bounds`. Refusals and `lipschitz=` are those of `cast`.

Long hard unions and intersections (from 64 members on, among the trees the field kernels run "in chain mode") are culled along
the rays. The 64 rays of a wave — an 8 x 8 pixel tile in `render`, 64 consecutive rays in `cast` — bound the points they
are about to evaluate by a sphere, every member is evaluated once at its centre, and only the members that can be the
minimum (maximum) somewhere in that sphere are folded per ray, in their original order; waves whose rays have drifted apart
split into up to 8 groups by t, and what still does not fit runs every member. The members left out are larger than the
minimum at every point of the sphere, so the result has the bits of the kernel without culling (`config.mode =
MODE_NOCULL` runs that one; tests/test_gpu_render_cull.py compares the two), whatever the order of the rays. Coherent rays
are what makes it fast: a 1000-sphere union costs a few dozen member evaluations per step instead of 1000.

Secondary rays: what a surface point sees. `visibility` marches arbitrary rays as `cast` does and reports how much of the
segment [t_min, t_end] is free of the solid (one definition: the kernels, tests/secondary_reference.py and this text), per
ray i, in float32:

    t = t_min; vis = 1; t_end = min(t_max, limits[i]) if limits is given, else t_max
    repeat at most max_steps times:
        f   = field(o + t d)                      # fmaf(t, d, o) per component
        thr = max(eps, cone * t)
        if f <= thr: vis = 0; status = HIT; stop  # blocked
        if k > 0: vis = min(vis, k * (f * (1/L)) / t)     # the penumbra estimate; t = 0 gives +inf, since f > 0
        t   = t + f / L                           # fmaf(f, float32(1 / L), t); steps += 1
        if t > t_end: status = MISS; stop         # clear
    otherwise: status = LIMIT                     # vis is what was seen so far, never folded into 0 or 1

k = `softness`; 0 is the hard test, vis 0 or 1. f / L is the radius of a ball around o + t d that is free of the solid, so
k (f / L) / t < 1 says the ray passes the solid within the cone of half-angle about 1 / k around it: a light of that angular
radius is partly hidden, and vis is the smallest such ratio along the ray, the usual soft shadow of distance-field
tracers (an estimate, never larger than it should be by more than the field's own error: the marched points are points
of the ray). `t_min` must not be negative, so vis stays in [0, 1]. `limits` is the end of every ray, what a point light
needs. The advance and both tests are those of `cast`: with `limits=None`, status and steps equal cast's bit for bit.

`ambient_occlusion` measures how open the half-space above a surface point p with unit normal n is, m = `samples` (1 to
16), in float32:

    occ = 0
    for i = 1 .. m:
        h   = radius * float32(i) * float32(1 / m)
        f   = field(p + h n)                      # fmaf(h, n, p) per component
        occ = fmaf(2^-i, max(0, h - f * float32(1 / L)), occ)
    ao = min(1, max(0, 1 - strength * occ * float32(1 / radius)))

Above a plane f / L = h at every sample and ao is exactly 1; whatever else comes within h of a sample lowers f there and
darkens the point, the near samples counting most. `illuminate` builds both kinds of rays on the host from the hit points
and the normals of an Image — shadow rays toward a `Light.directional(toward)` or a `Light.point(position)`, from origins
lifted off the surface by a bias of 4 stencil widths of the pixel — and fills `image.shadow` and `image.ao`;
`Image.shade(shadow=, occlusion=)` computes ambient * ao + (1 - ambient) * lambert * shadow. Long unions are culled along these rays as along the primary ones, with
the same bits. Refusals and `lipschitz=` are those of `cast`.
"""
import contextlib
import ctypes

import numpy as np

from . import _engine, _lipschitz, _ops
from ._eval import config, device_coords, program_for
from ._lower import OWNED, NeedsStage, _deep
from .autodiff import UnsupportedOpError, _TracingLowerer      # (autodiff.py marks the lowerer as used from here)

MISS, HIT, LIMIT = 0, 1, 2
COMPLETE = 0                                  # spans / thickness: the ray was followed to t_max (LIMIT = 2 as above)
_INSIDE0 = 4                                  # the kernels' status byte carries inside0 as this bit
MAX_CROSSINGS = 32                            # csrc/sdfk_raydev.h SDFK_SPAN_MAX_CROSSINGS
SPAN_EPS_FLOOR = 2.0 ** -20                   # eps >= this * max(|t_min|, |t_max|): t + eps > t in float32 on the whole ray
MAX_AO_SAMPLES = 16                           # csrc/sdfk_raydev.h SDFK_AO_MAX_SAMPLES
STENCIL_FLOOR = np.float32(2.0 ** -16)        # csrc/sdfk_raydev.h sdfk_ray_stencil_width


# ---- lowering ---------------------------------------------------------------------------------------------------------
class _RayLowerer(_TracingLowerer):
    """Remembers the first instruction whose destination has no finite Lipschitz bound."""

    def __init__(self):
        _TracingLowerer.__init__(self, True)
        self.first_unbounded = None

    def emit(self, opname, a, b=0, c=0, params=(), _fold=True):
        _TracingLowerer.emit(self, opname, a, b, c, params, _fold)
        if self.first_unbounded is None and self.code:
            word = self.code[-1][0]
            info = _ops.OPS[word & 255]
            dst = (word >> 8) & 255
            bound = (self.lip_c if info.kind == "C_C" else self.lip_v).get(dst, _lipschitz.INF)
            if not np.isfinite(bound):
                self.first_unbounded = (len(self.code) - 1, info.name, self.origin[-1] if self.origin else "the geometry")


def lower(geometry):
    """-> (LoweredProgram — create()'s own program —, first unbounded instruction (index, opcode, origin) or None)."""
    L = _RayLowerer()
    try:
        v = _deep(lambda: L.lower_node(geometry, 0, OWNED))
    except NeedsStage as exc:
        raise UnsupportedOpError("%r needs a staged evaluation (signed / conv_* / custom_* / Python callables cannot be "
                                 "traced along rays)" % (exc.expr.name,)) from None
    return L.finish(v), L.first_unbounded


def _bound(low, first, lipschitz):
    if lipschitz is not None:
        return _lipschitz.given(lipschitz)
    if not np.isfinite(low.lipschitz):
        if first is not None:
            where = "instruction %d (%s, from %s) has no finite Lipschitz bound" % first
        else:
            where = "its field has no finite Lipschitz bound"
        raise ValueError("this geometry cannot be sphere-traced with a derived step: %s; pass lipschitz= (an upper bound of "
                         "|grad f| over the region the rays cross)" % where)
    if not low.lipschitz > 0.0:
        raise ValueError("the field's Lipschitz bound is 0 (a constant field has no surface); pass lipschitz=")
    return float(low.lipschitz)


def _options(t_min, t_max, eps, cone, max_steps):
    t_min, t_max, eps, cone = float(t_min), float(t_max), float(eps), float(cone)
    if not (np.isfinite(t_min) and np.isfinite(t_max)):
        raise ValueError("t_min and t_max must be finite")
    if t_max < t_min:
        raise ValueError("t_max (%g) < t_min (%g)" % (t_max, t_min))
    if int(max_steps) < 1:
        raise ValueError("max_steps must be at least 1; got %r" % (max_steps,))
    if not (np.isfinite(eps) and eps >= 0.0 and np.isfinite(cone) and cone >= 0.0):
        raise ValueError("eps and cone must be finite and not negative")
    return tuple(float(np.float32(x)) for x in (t_min, t_max, eps, cone)) + (int(max_steps),)   # as the kernel sees them


def _span_options(t_min, t_max, eps, cone, max_steps, max_crossings):
    t_min, t_max, eps, cone, max_steps = _options(t_min, t_max, eps, cone, max_steps)
    floor = SPAN_EPS_FLOOR * max(abs(t_min), abs(t_max))
    if not (eps > 0.0 and eps >= floor):
        raise ValueError("eps must be positive and at least 2^-20 max(|t_min|, |t_max|) = %.3g, so that a floor step always "
                         "advances t in float32; got %g" % (floor, eps))
    k = int(max_crossings)
    if not 0 <= k <= MAX_CROSSINGS:
        raise ValueError("max_crossings from 0 to %d; got %r" % (MAX_CROSSINGS, max_crossings))
    return t_min, t_max, eps, cone, max_steps, k


def _program(low):
    prog = program_for(low)
    bad = ctypes.c_int(-1)
    rc = _engine.lib().sdfk_program_rays_check(prog.handle, ctypes.byref(bad))
    if rc == 1:
        raise UnsupportedOpError("the program reads an auxiliary field (staged evaluation): it exists on a grid only")
    _engine.check(rc, "sdfk_program_rays_check")
    return prog


def stencil_width(t, points, eps, cone):
    """Half-width h of the kernels' normal stencil at the hits (t (N,), points (3, N)), in their float32 arithmetic:
    max(thr, 2^-16 max(|x|, |y|, |z|)) with thr = max(eps, cone t)."""
    t = np.asarray(t, dtype=np.float32)
    p = np.abs(np.asarray(points, dtype=np.float32))
    thr = np.maximum(np.float32(eps), np.float32(cone) * t)
    return np.maximum(thr, STENCIL_FLOOR * p.max(axis=0))


# ---- results ----------------------------------------------------------------------------------------------------------
class RayHits:
    """Result of cast(): t (N,) float32 — where the ray stopped —, status (N,) uint8 (MISS 0: t passed t_max, HIT 1,
    LIMIT 2: max_steps reached), steps (N,) int32 (advances made), normals (3, N) float32 or None (zero for non-hits).
    With resident=True, t is a DeviceField and normals a DeviceVectorField; status and steps are host arrays."""

    def __init__(self, t, status, steps, normals, origins, directions):
        self.t, self.status, self.steps, self.normals = t, status, steps, normals
        self.origins, self.directions = origins, directions

    def __repr__(self):
        return "RayHits(%d rays, %d hits, %d at the step limit)" % (self.status.size, int(np.count_nonzero(self.status == HIT)),
                                                                    int(np.count_nonzero(self.status == LIMIT)))

    def points(self):
        """o + t d of the rays that hit, (3, M) float32 (computed in float64 from the float32 o, d, t), in ray order."""
        def host(x):
            return x.numpy() if isinstance(x, (_engine.DeviceField, _engine.DeviceVectorField)) else np.asarray(x)
        hit = self.status == HIT
        o = host(self.origins).astype(np.float32).astype(np.float64)[:, hit]
        d = host(self.directions).astype(np.float32).astype(np.float64)[:, hit]
        return (o + host(self.t).astype(np.float64)[hit] * d).astype(np.float32)


class RayVisibility:
    """Result of visibility(): vis (N,) float32 in [0, 1] — 0 blocked, 1 clear, between the two in a penumbra —, status (N,)
    uint8 (MISS 0: clear, the ray passed its end; HIT 1: blocked; LIMIT 2: max_steps reached, vis is what was seen so far),
    steps (N,) int32 (advances made). With resident=True, vis is a DeviceField; status and steps are host arrays."""

    def __init__(self, vis, status, steps):
        self.vis, self.status, self.steps = vis, status, steps

    def __repr__(self):
        return "RayVisibility(%d rays, %d blocked, %d at the step limit)" % (
            self.status.size, int(np.count_nonzero(self.status == HIT)), int(np.count_nonzero(self.status == LIMIT)))


class Light:
    """A light for illuminate(): Light.directional(toward) — parallel rays, `toward` points from the scene TO the light — or
    Light.point(position)."""

    def __init__(self, toward=None, position=None):
        if (toward is None) == (position is None):
            raise ValueError("a light has a direction (Light.directional) or a position (Light.point)")
        v = np.asarray(toward if position is None else position, dtype=np.float64).reshape(3)
        if not np.all(np.isfinite(v)):
            raise ValueError("the light's vector is not finite")
        self.position = v if toward is None else None
        self.toward = None
        if toward is not None:
            n = np.linalg.norm(v)
            if not n > 0.0:
                raise ValueError("the light direction is the zero vector")
            self.toward = v / n

    @classmethod
    def directional(cls, toward):
        return cls(toward=toward)

    @classmethod
    def point(cls, position):
        return cls(position=position)

    def rays(self, points):
        """-> (unit directions (3, M) float64 from `points` (3, M) toward the light, distances to it (M,) or None for a
        directional light). A point AT a point light gets the zero direction and the distance 0."""
        p = np.asarray(points, dtype=np.float64)
        if self.position is None:
            return np.repeat(self.toward[:, None], p.shape[1], axis=1), None
        w = self.position[:, None] - p
        dist = np.linalg.norm(w, axis=0)
        return np.divide(w, dist, out=np.zeros_like(w), where=dist > 0), dist


class Camera:
    """A pinhole camera (or, from Camera.orthographic, a parallel one); see the module text for the pixel formula."""

    def __init__(self, eye, target, up=(0, 0, 1), fov=40.0):
        self.eye = np.asarray(eye, dtype=np.float64).reshape(3)
        self.target = np.asarray(target, dtype=np.float64).reshape(3)
        self.up = np.asarray(up, dtype=np.float64).reshape(3)
        self.fov, self.height, self.ortho = float(fov), None, False
        if not 0.0 < self.fov < 180.0:
            raise ValueError("fov is the vertical field of view in degrees, between 0 and 180; got %r" % (fov,))
        self._basis()

    @classmethod
    def orthographic(cls, eye, target, up=(0, 0, 1), height=2.0):
        self = cls(eye, target, up, 40.0)
        self.fov, self.height, self.ortho = None, float(height), True
        if not (np.isfinite(self.height) and self.height > 0.0):
            raise ValueError("height is the world height of the image, positive; got %r" % (height,))
        return self

    def _basis(self):
        fwd = self.target - self.eye
        n = np.linalg.norm(fwd)
        if not (np.isfinite(n) and n > 0.0):
            raise ValueError("eye and target must be two different finite points")
        self.fwd = fwd / n
        right = np.cross(self.fwd, self.up)
        n = np.linalg.norm(right)
        if not (np.isfinite(n) and n > 1e-12 * max(1.0, np.linalg.norm(self.up))):
            raise ValueError("up is parallel to the viewing direction")
        self.right = right / n
        self.upv = np.cross(self.right, self.fwd)

    def _check(self, width, height):
        width, height = int(width), int(height)
        if not (1 <= width <= 32768 and 1 <= height <= 32768):
            raise ValueError("image sizes from 1 to 32768; got %d x %d" % (width, height))
        return width, height

    def frame(self, width, height):
        """(du, dv) in float64: the right / up vectors scaled by half the extent of the image plane."""
        width, height = self._check(width, height)
        half = 0.5 * self.height if self.ortho else np.tan(np.radians(0.5 * self.fov))
        return self.right * (half * width / height), self.upv * half

    def record(self, width, height):
        """The 12 float32 {eye, fwd, du, dv} the kernel generates its rays from."""
        du, dv = self.frame(width, height)
        return np.concatenate([self.eye, self.fwd, du, dv]).astype(np.float32)

    def footprint(self, width, height):
        """(eps, cone) of a pixel: half its world size (orthographic) or half its angular size (perspective)."""
        width, height = self._check(width, height)
        if self.ortho:
            return 0.5 * self.height / height, 0.0
        return 0.0, float(np.tan(np.radians(0.5 * self.fov)) / height)

    def rays(self, width, height):
        """(origins, directions), both (3, W H) float64, row-major pixel order (index iy W + ix, row 0 at the top)."""
        width, height = self._check(width, height)
        du, dv = self.frame(width, height)
        a = (2.0 * np.arange(width) + 1.0) / width - 1.0
        b = 1.0 - (2.0 * np.arange(height) + 1.0) / height
        a, b = np.meshgrid(a, b, indexing="xy")                 # (H, W)
        q = a.ravel()[None] * du[:, None] + b.ravel()[None] * dv[:, None]
        if self.ortho:
            return self.eye[:, None] + q, np.repeat(self.fwd[:, None], width * height, axis=1)
        w = self.fwd[:, None] + q
        return np.repeat(self.eye[:, None], width * height, axis=1), w / np.linalg.norm(w, axis=0)


class Image:
    """Result of render(): depth (H, W) float32 — t of the hit, +inf where the ray did not hit (miss or step limit) —,
    status (H, W) uint8, steps (H, W) int32, normals (H, W, 3) float32 or None (zero where not hit), t (H, W) float32
    (where every ray stopped, hit or not) and the camera, eps and cone it was made with."""

    def __init__(self, depth, status, steps, normals, t=None, camera=None, eps=0.0, cone=0.0):
        self.depth, self.status, self.steps, self.normals = depth, status, steps, normals
        self.t = depth if t is None else t
        self.camera, self.eps, self.cone = camera, eps, cone
        self.shadow = self.ao = None                            # (H, W) float32 once illuminate() has filled them

    def __repr__(self):
        h, w = self.status.shape
        return "Image(%d x %d, %d hits)" % (w, h, int(np.count_nonzero(self.status == HIT)))

    def points(self):
        """Hit points (3, M) float32 in row-major pixel order, from Camera.rays in float64."""
        h, w = self.status.shape
        o, d = self.camera.rays(w, h)
        hit = (self.status == HIT).ravel()
        return (o[:, hit] + self.t.ravel().astype(np.float64)[hit] * d[:, hit]).astype(np.float32)

    def exact_normals(self, geometry):
        """Replace the stencil normals by the unit gradient of `geometry` at the hit points
        (autodiff.value_and_grad_points, normalised on the host as Mesh.compute_normals does). Raises that function's
        UnsupportedOpError for trees without a dual rule."""
        from .autodiff import value_and_grad_points
        pts = np.ascontiguousarray(self.points(), dtype=np.float32)
        _, grad = value_and_grad_points(geometry, pts)
        g = np.asarray(grad, dtype=np.float64).reshape(3, -1).T
        norm = np.linalg.norm(g, axis=1, keepdims=True)
        unit = np.divide(g, norm, out=np.zeros_like(g), where=norm > 0).astype(np.float32)
        out = np.zeros(self.status.shape + (3,), dtype=np.float32)
        out[self.status == HIT] = unit
        self.normals = out
        return out

    def shade(self, light=(1.0, 1.0, 2.0), ambient=0.15, color=None, background=0.0, dtype=np.uint8, shadow=None,
              occlusion=None):
        """Lambert shading from normals and status on the host: ambient ao + (1 - ambient) max(0, n . l) shadow at the hits
        (l the unit vector TOWARD the light; `shadow`, `occlusion`: (H, W) arrays in [0, 1] such as illuminate()'s
        image.shadow and image.ao, None: 1 everywhere), `background` elsewhere. -> (H, W), or (H, W, 3) with an RGB
        `color` in [0, 1]; uint8 (0..255, rounded) or float32 in [0, 1]."""
        if self.normals is None:
            raise ValueError("shade needs normals: render(..., normals=True) or exact_normals()")
        l = np.asarray(light, dtype=np.float64).reshape(3)
        n = np.linalg.norm(l)
        if not n > 0.0:
            raise ValueError("the light direction is the zero vector")
        lam = np.clip(np.asarray(self.normals, dtype=np.float64).dot(l / n), 0.0, 1.0)
        lit, amb = (1.0 - float(ambient)) * lam, float(ambient)
        for name, factor in (("shadow", shadow), ("occlusion", occlusion)):
            if factor is not None and np.shape(factor) != self.status.shape:
                raise ValueError("%s must have the image's shape %r; got %r" % (name, self.status.shape, np.shape(factor)))
        if shadow is not None:
            lit = lit * np.asarray(shadow, dtype=np.float64)
        if occlusion is not None:
            amb = amb * np.asarray(occlusion, dtype=np.float64)
        value = np.where(self.status == HIT, amb + lit, float(background))
        if color is not None:
            rgb = np.asarray(color, dtype=np.float64).reshape(3)
            value = np.where((self.status == HIT)[..., None], value[..., None] * rgb, float(background))
        value = np.clip(value, 0.0, 1.0)
        if np.dtype(dtype) == np.uint8:
            return np.rint(value * 255.0).astype(np.uint8)
        return value.astype(np.float32)

    @staticmethod
    def _pnm(path, pixels, magic, channels):
        px = np.asarray(pixels)
        if px.dtype != np.uint8:
            px = np.rint(np.clip(px.astype(np.float64), 0.0, 1.0) * 255.0).astype(np.uint8)
        want = 2 if channels == 1 else 3
        if px.ndim != want or (channels == 3 and px.shape[2] != 3):
            raise ValueError("expected %s pixels; got shape %r" % ("(H, W)" if channels == 1 else "(H, W, 3)", px.shape))
        with open(path, "wb") as f:
            f.write(("%s\n%d %d\n255\n" % (magic, px.shape[1], px.shape[0])).encode("ascii"))
            f.write(np.ascontiguousarray(px).tobytes())

    def save_pgm(self, path, pixels=None):
        """Binary PGM (P5) of (H, W) pixels, uint8 or float in [0, 1]; default: shade()."""
        self._pnm(path, self.shade() if pixels is None else pixels, "P5", 1)

    def save_ppm(self, path, pixels=None):
        """Binary PPM (P6) of (H, W, 3) pixels; default: shade(color=(1, 1, 1))."""
        self._pnm(path, self.shade(color=(1.0, 1.0, 1.0)) if pixels is None else pixels, "P6", 3)

    def save_npz(self, path):
        arrays = {"depth": self.depth, "status": self.status, "steps": self.steps, "t": self.t}
        for name in ("normals", "shadow", "ao"):
            if getattr(self, name) is not None:
                arrays[name] = getattr(self, name)
        np.savez_compressed(path, **arrays)


def _intervals(crossings, count, inside0, status, chord, t_min, t_max):
    """The (t_enter, t_exit) pairs of one ray from its stored crossings (float64)."""
    n = int(count)
    if n > len(crossings):
        raise ValueError("the ray has %d crossings and %d are stored: raise max_crossings" % (n, len(crossings)))
    ts = [float(x) for x in crossings[:n]]
    if inside0:
        ts.insert(0, float(t_min))
    if len(ts) % 2:                                             # still inside where the march ended
        closed = sum(b - a for a, b in zip(ts[0:-1:2], ts[1::2]))
        # COMPLETE: the ray was followed to t_max. LIMIT: to the last evaluated t, which the chord was closed with
        ts.append(float(t_max) if status == COMPLETE else ts[-1] + max(float(chord) - closed, 0.0))
    return list(zip(ts[0::2], ts[1::2]))


class RaySpans:
    """Result of spans(): chord (N,) float32 — the length of the ray inside the solid —, count (N,) int32 (all crossings,
    also those beyond K), inside0 (N,) bool (inside at t_min), status (N,) uint8 (COMPLETE 0: followed to t_max, LIMIT 2:
    max_steps reached, or no progress in float32), steps (N,) int32 (evaluations made), crossings (K, N) float32 (the
    first K crossing parameters in order, NaN past count), truncated (N,) bool (count > K). With resident=True, chord is a
    DeviceField and crossings a DeviceRows (None for K = 0); the small arrays are host arrays."""

    def __init__(self, chord, count, status, steps, crossings, t_min, t_max, max_crossings):
        status = np.asarray(status, dtype=np.uint8)
        self.chord, self.count, self.steps, self.crossings = chord, count, steps, crossings
        self.inside0 = (status & _INSIDE0) != 0
        self.status = status & np.uint8(3)
        self.t_min, self.t_max, self.max_crossings = float(t_min), float(t_max), int(max_crossings)
        self.truncated = np.asarray(count) > self.max_crossings

    def __repr__(self):
        return "RaySpans(%d rays, %d crossings, %d at the step limit)" % (self.status.size, int(np.sum(self.count, dtype=np.int64)),
                                                                          int(np.count_nonzero(self.status == LIMIT)))

    def intervals(self, i):
        """The (t_enter, t_exit) pairs of ray i, in order. The first opens at t_min when inside0; a ray that is still
        inside where it ended closes at t_max, or on LIMIT at the last evaluated t. ValueError if the ray is truncated."""
        def host(x):
            return x.numpy() if isinstance(x, _engine.DeviceField) else x.download_rows() if isinstance(x, _engine.DeviceRows) else x
        cr = np.zeros((0, self.status.size), dtype=np.float32) if self.crossings is None else host(self.crossings)
        return _intervals(cr[:, i], self.count[i], self.inside0[i], self.status[i], host(self.chord)[i], self.t_min, self.t_max)


class ThicknessImage:
    """Result of thickness(): chord (H, W) float32, count (H, W) int32, inside0 (H, W) bool, status (H, W) uint8
    (COMPLETE / LIMIT), steps (H, W) int32, crossings (K, H, W) float32 (NaN past count) or None for K = 0, and the camera,
    eps, cone, t_min and t_max it was made with."""

    def __init__(self, chord, count, status, steps, crossings, camera=None, eps=0.0, cone=0.0, t_min=0.0, t_max=0.0):
        status = np.asarray(status, dtype=np.uint8)
        self.chord, self.count, self.steps, self.crossings = chord, count, steps, crossings
        self.inside0 = (status & _INSIDE0) != 0
        self.status = status & np.uint8(3)
        self.camera, self.eps, self.cone, self.t_min, self.t_max = camera, eps, cone, t_min, t_max

    def __repr__(self):
        h, w = self.status.shape
        return "ThicknessImage(%d x %d, largest chord %g)" % (w, h, float(np.max(self.chord)) if self.chord.size else 0.0)

    def volume(self):
        """Sum of chord x pixel area in float64: the midpoint rule over the image plane of an ORTHOGRAPHIC camera, whose
        rays are parallel — the volume of the solid between t_min and t_max inside the image's prism."""
        if self.camera is None or not self.camera.ortho:
            raise ValueError("volume() is the sum of chord x pixel area over parallel rays: it needs an orthographic camera")
        h, w = self.status.shape
        side = self.camera.height / h                           # square pixels: the image is height W / H wide
        return float(np.sum(self.chord, dtype=np.float64) * side * side)

    def save_pgm(self, path, scale=None):
        """Binary PGM (P5) radiograph: chord / scale, clipped to [0, 1] (default scale: the largest chord), 0 = empty."""
        top = float(np.max(self.chord)) if scale is None else float(scale)
        Image._pnm(path, np.asarray(self.chord, dtype=np.float64) / top if top > 0.0 else np.zeros(self.chord.shape), "P5", 1)

    def save_npz(self, path):
        arrays = {"chord": self.chord, "count": self.count, "inside0": self.inside0, "status": self.status, "steps": self.steps}
        if self.crossings is not None:
            arrays["crossings"] = self.crossings
        np.savez_compressed(path, **arrays)


# ---- device plumbing ----------------------------------------------------------------------------------------------------
def _outputs(fields, scratch, n, normals):
    """The trace kernels' outputs, entered on two ExitStacks: t (DeviceField) and the normals (DeviceVectorField or
    None) on `fields`, the status bytes and int32 steps (DeviceBuffers) on `scratch`."""
    t = fields.enter_context(_engine.DeviceField(n, config.device))
    nrm = fields.enter_context(_engine.DeviceVectorField(n, config.device)) if normals else None
    d_status = scratch.enter_context(_engine.DeviceBuffer(max(n, 64), what="render"))
    d_steps = scratch.enter_context(_engine.DeviceBuffer(max(n, 16) * 4, what="render"))
    return t, nrm, d_status, d_steps


def _small(n, d_status, d_steps):
    return d_status.download(np.empty(n, dtype=np.uint8)), d_steps.download(np.empty(n, dtype=np.int32))


def _rows(rows):
    """The (pointer, row stride) arguments of an optional strided output: the normals, the crossings."""
    return (None, 0) if rows is None else (rows.at(), rows.stride)


def _span_outputs(fields, scratch, n, k):
    """The span kernels' outputs: the chord (DeviceField) and the (k, n) crossings (DeviceRows filled with NaN, None for
    k = 0) on `fields`; count, status and steps (DeviceBuffers) on `scratch`."""
    chord = fields.enter_context(_engine.DeviceField(n, config.device))
    cross = None
    if k:
        cross = fields.enter_context(_engine.DeviceRows(k, n, config.device, what="render"))
        # rows past a ray's count are never written: NaN everywhere first. One row crosses PCIe, the others are copies of
        # what is already there, doubling.
        cross.upload(np.full(cross.stride, np.nan, dtype=np.float32))
        done = 1
        while done < k:
            rows = min(done, k - done)
            cross.copy_from(cross.ptr, cross.offset(rows), cross.offset(done))
            done += rows
    d_count = scratch.enter_context(_engine.DeviceBuffer(max(n, 16) * 4, what="render"))
    d_status = scratch.enter_context(_engine.DeviceBuffer(max(n, 64), what="render"))
    d_steps = scratch.enter_context(_engine.DeviceBuffer(max(n, 16) * 4, what="render"))
    return chord, cross, d_count, d_status, d_steps


def _check_rays(origins, directions):
    """The checks of cast() on a pair of ray arrays -> the number of rays."""
    for name, x in (("origins", origins), ("directions", directions)):
        if not isinstance(x, _engine.DeviceVectorField):
            shape = np.shape(x)
            if len(shape) != 2 or shape[0] != 3:
                raise ValueError("%s must have shape (3, N); got %r" % (name, shape))
    if not isinstance(directions, _engine.DeviceVectorField):
        d32 = np.asarray(directions, dtype=np.float32).astype(np.float64)
        len2 = (d32 * d32).sum(axis=0)
        bad = ~(np.abs(len2 - 1.0) <= 1e-5)
        if bad.any():
            raise ValueError("directions must be unit vectors: ray %d has |d|^2 = %.9g" %
                             (int(np.argmax(bad)), float(len2[np.argmax(bad)])))
    n_o = origins.n if isinstance(origins, _engine.DeviceVectorField) else int(np.shape(origins)[1])
    n_d = directions.n if isinstance(directions, _engine.DeviceVectorField) else int(np.shape(directions)[1])
    if n_o != n_d:
        raise ValueError("%d origins for %d directions" % (n_o, n_d))
    return n_o


def _lowered(geometry, lipschitz):
    """-> (the geometry's lowered program, float32(1 / L) of its Lipschitz bound or of the caller's `lipschitz`)."""
    low, first = lower(geometry)
    return low, float(np.float32(1.0 / _bound(low, first, lipschitz)))


def _on_device(low):
    """-> the program of `low`, checked for the marches, with the device selected."""
    prog = _program(low)
    _engine.require_gpu()
    _engine.check(_engine.lib().sdfk_set_device(config.device), "sdfk_set_device")
    return prog


def _setup(geometry, lipschitz):
    """What every march needs of its geometry -> (the program, float32(1 / L)), with the device selected."""
    low, inv = _lowered(geometry, lipschitz)
    return _on_device(low), inv


@contextlib.contextmanager
def _source(rays=None, camera=None, size=None):
    """The rays of a march -> the arguments of its entry point between the program and the options: `rays` = (origins,
    directions, their number) for the *_rays_device entry points, host arrays being on the device for the duration, or a
    camera and its image `size` = (width, height) for the *_camera_device ones."""
    if camera is None:
        with device_coords(rays[0], "render") as co, device_coords(rays[1], "render") as cd:
            yield _engine._vp(co.ptr), co.stride, _engine._vp(cd.ptr), cd.stride, rays[2]
    else:
        rec = camera.record(*size)                              # (lives as long as the block that uses its address)
        yield _engine._ptr(rec), size[0], size[1], 1 if camera.ortho else 0


def _march(entry, prog, source, options, inv_lipschitz, outputs, n, d_status, d_steps):
    """One call of the entry point `entry` (sdfk_{trace,span}_{rays,camera}_device): the program, the source's arguments,
    the options every march shares, the march's own `outputs`, the default stream and the configured mode; waits for it.
    -> (status, steps) on the host."""
    t_min, t_max, eps, cone, max_steps = options
    L = _engine.lib()
    _engine.check(getattr(L, entry)(prog.handle, *source, t_min, t_max, eps, cone, inv_lipschitz, max_steps, *outputs, None,
                                    config.mode), entry)
    _engine.check(L.sdfk_sync(None), "sdfk_sync")
    return _small(n, d_status, d_steps)


# ---- public interface ---------------------------------------------------------------------------------------------------
def cast(geometry, origins, directions, t_min=0.0, t_max=100.0, eps=1e-4, cone=0.0, max_steps=256, lipschitz=None,
         normals=False, resident=False):
    """First hit of arbitrary rays with `geometry`. `origins`, `directions`: (3, N) host arrays (used as float32) or
    DeviceVectorFields; the directions must be unit vectors (checked for host arrays: | |d|^2 - 1 | <= 1e-5).
    -> RayHits. See the module text for the marching rule, `lipschitz` and the refusals."""
    options = _options(t_min, t_max, eps, cone, max_steps)
    low, inv = _lowered(geometry, lipschitz)
    n = _check_rays(origins, directions)                        # (before anything asks for the GPU)
    prog = _on_device(low)
    with contextlib.ExitStack() as on_error, contextlib.ExitStack() as stack:
        source = stack.enter_context(_source(rays=(origins, directions, n)))
        t, nrm, d_status, d_steps = _outputs(on_error, stack, n, normals)
        status, steps = _march("sdfk_trace_rays_device", prog, source, options, inv,
                               (t.at(), d_status.at(), d_steps.at()) + _rows(nrm), n, d_status, d_steps)
        if resident:
            on_error.pop_all()
            return RayHits(t, status, steps, nrm, origins, directions)
        return RayHits(t.numpy(), status, steps, nrm.numpy() if normals else None, origins, directions)


def render(geometry, camera, width, height, t_min=0.0, t_max=100.0, max_steps=256, lipschitz=None, normals=True, eps=None,
           cone=None):
    """Depth / normal image of `geometry` from `camera`: the kernel generates the W x H rays from the camera record.
    `eps` / `cone` default to the pixel's footprint (Camera.footprint). -> Image."""
    width, height = camera._check(width, height)
    fe, fc = camera.footprint(width, height)
    eps = fe if eps is None else eps
    cone = fc if cone is None else cone
    options = _options(t_min, t_max, eps, cone, max_steps)
    eps, cone = options[2:4]                                    # (as the kernel sees them)
    prog, inv = _setup(geometry, lipschitz)
    with contextlib.ExitStack() as stack:
        source = stack.enter_context(_source(camera=camera, size=(width, height)))
        n = width * height
        t, nrm, d_status, d_steps = _outputs(stack, stack, n, normals)
        status, steps = _march("sdfk_trace_camera_device", prog, source, options, inv,
                               (t.at(), d_status.at(), d_steps.at()) + _rows(nrm), n, d_status, d_steps)
        t = t.numpy().reshape(height, width)
        nrm = np.ascontiguousarray(nrm.numpy().T).reshape(height, width, 3) if normals else None
    status = status.reshape(height, width)
    depth = np.where(status == HIT, t, np.float32(np.inf)).astype(np.float32)
    return Image(depth, status, steps.reshape(height, width), nrm, t=t, camera=camera, eps=float(eps), cone=float(cone))


def spans(geometry, origins, directions, t_min=0.0, t_max=100.0, eps=1e-4, cone=0.0, max_steps=1024, lipschitz=None,
          max_crossings=8, resident=False):
    """Every crossing of arbitrary rays with the solid of `geometry`, and their chords. `origins`, `directions` as for
    cast(). -> RaySpans. See the module text for the rule, the floor of `eps`, `lipschitz` and the refusals."""
    *options, k = _span_options(t_min, t_max, eps, cone, max_steps, max_crossings)
    t_min, t_max = options[:2]
    low, inv = _lowered(geometry, lipschitz)
    n = _check_rays(origins, directions)                        # (before anything asks for the GPU)
    prog = _on_device(low)
    with contextlib.ExitStack() as on_error, contextlib.ExitStack() as stack:
        source = stack.enter_context(_source(rays=(origins, directions, n)))
        chord, cross, d_count, d_status, d_steps = _span_outputs(on_error, stack, n, k)
        status, steps = _march("sdfk_span_rays_device", prog, source, options, inv,
                               (chord.at(), d_count.at(), d_status.at(), d_steps.at()) + _rows(cross) + (k,), n, d_status, d_steps)
        count = d_count.download(np.empty(n, dtype=np.int32))
        if resident:
            on_error.pop_all()
            return RaySpans(chord, count, status, steps, cross, t_min, t_max, k)
        crossings = cross.download_rows() if k else np.empty((0, n), dtype=np.float32)
        return RaySpans(chord.numpy(), count, status, steps, crossings, t_min, t_max, k)


def thickness(geometry, camera, width, height, t_min=0.0, t_max=100.0, max_steps=1024, lipschitz=None, eps=None, cone=None,
              max_crossings=0):
    """Thickness / radiograph image of `geometry` from `camera`: the chord of every pixel's ray, generated in the kernel
    from the camera record as in render(). `eps` / `cone` default to the pixel's footprint (Camera.footprint), `eps`
    raised to its floor 2^-20 max(|t_min|, |t_max|) where the footprint's is smaller (the perspective camera's is 0).
    -> ThicknessImage."""
    width, height = camera._check(width, height)
    fe, fc = camera.footprint(width, height)
    if eps is None:
        floor = SPAN_EPS_FLOOR * max(abs(float(t_min)), abs(float(t_max)))
        eps = max(fe, float(np.nextafter(np.float32(floor), np.float32(np.inf)))) if np.isfinite(floor) else fe
    cone = fc if cone is None else cone
    *options, k = _span_options(t_min, t_max, eps, cone, max_steps, max_crossings)
    t_min, t_max, eps, cone = options[:4]
    prog, inv = _setup(geometry, lipschitz)
    with contextlib.ExitStack() as stack:
        source = stack.enter_context(_source(camera=camera, size=(width, height)))
        n = width * height
        chord, cross, d_count, d_status, d_steps = _span_outputs(stack, stack, n, k)
        status, steps = _march("sdfk_span_camera_device", prog, source, options, inv,
                               (chord.at(), d_count.at(), d_status.at(), d_steps.at()) + _rows(cross) + (k,), n, d_status, d_steps)
        count = d_count.download(np.empty(n, dtype=np.int32))
        chord = chord.numpy().reshape(height, width)
        crossings = cross.download_rows().reshape(k, height, width) if k else None
    return ThicknessImage(chord, count.reshape(height, width), status.reshape(height, width), steps.reshape(height, width),
                          crossings, camera=camera, eps=float(eps), cone=float(cone), t_min=t_min, t_max=t_max)


def visibility(geometry, origins, directions, t_min=0.0, t_max=100.0, eps=1e-4, cone=0.0, max_steps=256, lipschitz=None,
               softness=0.0, limits=None, resident=False):
    """How much of each ray's segment [t_min, min(t_max, limits)] is free of `geometry`: 0 blocked, 1 clear, and with
    `softness` = k > 0 the penumbra estimate min k (f / L) / t in between. `origins`, `directions` as for cast(); `limits`:
    (N,) per-ray ends (host array or DeviceField) or None. -> RayVisibility. See the module text for the rule."""
    options = _options(t_min, t_max, eps, cone, max_steps)
    if options[0] < 0.0:
        raise ValueError("t_min must not be negative (vis stays in [0, 1] without a clamp); got %g" % options[0])
    softness = float(softness)
    if not (np.isfinite(softness) and softness >= 0.0):
        raise ValueError("softness must be finite and not negative; got %r" % (softness,))
    low, inv = _lowered(geometry, lipschitz)
    n = _check_rays(origins, directions)                        # (before anything asks for the GPU)
    if limits is not None:
        n_l = limits.n if isinstance(limits, _engine.DeviceField) else np.shape(limits)
        if n_l != (n if isinstance(limits, _engine.DeviceField) else (n,)):
            raise ValueError("limits must have shape (%d,), one end per ray; got %r" % (n, n_l))
    prog = _on_device(low)
    with contextlib.ExitStack() as on_error, contextlib.ExitStack() as stack:
        source = stack.enter_context(_source(rays=(origins, directions, n)))
        vis = on_error.enter_context(_engine.DeviceField(n, config.device))
        d_status = stack.enter_context(_engine.DeviceBuffer(max(n, 64), what="render"))
        d_steps = stack.enter_context(_engine.DeviceBuffer(max(n, 16) * 4, what="render"))
        d_limits = None
        if limits is not None and n:
            lim = limits if isinstance(limits, _engine.DeviceField) else \
                stack.enter_context(_engine.DeviceField.from_host(limits, config.device))
            d_limits = lim.at()
        status, steps = _march("sdfk_visibility_rays_device", prog, source, options, inv,
                               (softness, d_limits, vis.at(), d_status.at(), d_steps.at()), n, d_status, d_steps)
        if resident:
            on_error.pop_all()
            return RayVisibility(vis, status, steps)
        return RayVisibility(vis.numpy(), status, steps)


def ambient_occlusion(geometry, points, normals, radius, samples=5, strength=1.0, lipschitz=None, resident=False):
    """Ambient occlusion of the surface points `points` with the unit `normals` (both as the rays of cast()): 1 open, 0
    closed; `samples` (1 to 16) field evaluations per point along the normal, out to `radius`. -> (N,) float32, or a
    DeviceField with resident=True. See the module text for the rule."""
    radius, strength, samples = float(radius), float(strength), int(samples)
    if not (np.isfinite(radius) and radius > 0.0):
        raise ValueError("radius must be finite and positive; got %r" % (radius,))
    if not 1 <= samples <= MAX_AO_SAMPLES:
        raise ValueError("samples from 1 to %d; got %r" % (MAX_AO_SAMPLES, samples))
    if not (np.isfinite(strength) and strength >= 0.0):
        raise ValueError("strength must be finite and not negative; got %r" % (strength,))
    low, inv = _lowered(geometry, lipschitz)
    n = _check_rays(points, normals)                            # (before anything asks for the GPU)
    prog = _on_device(low)
    with contextlib.ExitStack() as on_error, contextlib.ExitStack() as stack:
        source = stack.enter_context(_source(rays=(points, normals, n)))
        ao = on_error.enter_context(_engine.DeviceField(n, config.device))
        L = _engine.lib()
        _engine.check(L.sdfk_occlusion_rays_device(prog.handle, *source, radius, samples, strength, inv, ao.at(), None,
                                                   config.mode), "sdfk_occlusion_rays_device")
        _engine.check(L.sdfk_sync(None), "sdfk_sync")
        if resident:
            on_error.pop_all()
            return ao
        return ao.numpy()


BIAS_WIDTHS = 4.0             # illuminate(): the default bias in stencil widths of the pixel


def shadow_rays(image, light, bias=None):
    """The secondary rays illuminate() marches for the shadow of `light` -> (facing, origins, directions, limits, eps):
    `facing` (M,) bool marks, among the M hit pixels in row-major order, those that face the light (n . l > 0, and a unit
    normal: a degenerate stencil leaves the zero vector); they have a ray each: `origins`, `directions` (3, F) float32,
    `limits` (F,) float32 — the distance from the origin to a point light — or None, and `eps`, the threshold of the march:
    half the smallest bias. See illuminate() for the rule."""
    if not isinstance(light, Light):
        raise TypeError("light must be a render.Light; got %r" % (type(light).__name__,))
    if image.normals is None or image.camera is None:
        raise ValueError("secondary rays need an Image with normals and its camera: render(..., normals=True)")
    hit = image.status == HIT
    nrm = np.asarray(image.normals, dtype=np.float64)[hit].T    # (3, M), row-major pixel order
    p32 = image.points()
    if bias is None:
        lift = BIAS_WIDTHS * stencil_width(image.t[hit], p32, image.eps, image.cone).astype(np.float64)
    else:
        if not (np.isfinite(float(bias)) and float(bias) > 0.0):
            raise ValueError("bias must be finite and positive; got %r" % (bias,))
        lift = np.full(p32.shape[1], float(bias))
    org = p32.astype(np.float64) + lift * nrm
    to_light, dist = light.rays(org)
    facing = ((nrm * to_light).sum(axis=0) > 0.0) & (np.abs((nrm * nrm).sum(axis=0) - 1.0) <= 1e-5)
    d32 = to_light[:, facing].astype(np.float32).astype(np.float64)
    d32 = np.divide(d32, np.linalg.norm(d32, axis=0)).astype(np.float32)
    limits = None if dist is None else dist[facing].astype(np.float32)
    return facing, org[:, facing].astype(np.float32), d32, limits, 0.5 * float(lift[facing].min()) if facing.any() else 0.0


def tile_order(mask):
    """The True pixels of the (H, W) `mask`, numbered in row-major order -> those numbers sorted by 8 x 8 pixel tile (tiles
    in row-major order, the pixels of a tile in row-major order): 64 consecutive entries lie close together in the image, as
    the 64 rays of a wave of the camera kernels do. The culled kernels bound a wave's points by one sphere, and a run of 64
    pixels along an image row makes a far larger one (DESIGN 4.19 has the measurement); results do not depend on the order."""
    iy, ix = np.nonzero(mask)
    key = ((iy >> 3) * ((mask.shape[1] + 7) // 8) + (ix >> 3)) * 64 + (iy & 7) * 8 + (ix & 7)
    return np.argsort(key, kind="stable")


def _pixel_order(hit, among):
    """tile_order of the hit pixels marked by `among` (M,) bool."""
    mask = np.zeros(hit.shape, dtype=bool)
    mask[hit] = among
    return tile_order(mask)


def illuminate(geometry, image, light, softness=8.0, bias=None, ao_radius=None, ao_samples=5, ao_strength=1.0, lipschitz=None,
               max_steps=256, t_max=None):
    """Shadows and ambient occlusion of a rendered Image (render(..., normals=True), or exact_normals()): fills
    `image.shadow` — visibility of the `light` from every hit pixel, (H, W) float32 — and, when `ao_radius` is given,
    `image.ao` (ambient_occlusion with `ao_samples`, `ao_strength` at the hit points); both are 1 where the pixel did not
    hit. -> the image.

    The secondary rays are built on the host (shadow_rays; marched in the order of tile_order), in float64 from Image.points() and the normals, and rounded to
    float32: origin p + bias n, direction toward the light (renormalised after rounding), for a point light `limits` = the
    distance from the origin to the light. Pixels with n . l <= 0 face away and get shadow 0 without a ray. `bias` lifts the
    origin off the surface it lies on: by default BIAS_WIDTHS = 4 times the pixel's own stencil width (stencil_width: its
    hit threshold max(eps, cone t), floored at 2^-16 max|p|) — the hit point lies within one threshold of the surface, so
    the origin is at least three thresholds clear of it and a convex body never shadows itself —, or the given length for
    all pixels. The shadow march runs with cone = 0 and eps = half the smallest bias, so no ray starts within its own hit
    threshold, and as far as `t_max` (default: the image's longest ray, image.t.max(), for a directional light; the
    largest distance to a point light). `softness`, `max_steps`, `lipschitz` as in visibility()."""
    facing, origins, directions, limits, eps = shadow_rays(image, light, bias)
    hit = image.status == HIT
    shadow = np.zeros(facing.size, dtype=np.float32)
    if facing.any():
        if t_max is None:
            t_max = float(np.max(image.t)) if limits is None else float(limits.max())
        order = _pixel_order(hit, facing)                       # (rays of one wave from one tile of the image)
        vis = np.empty(order.size, dtype=np.float32)
        vis[order] = visibility(geometry, np.ascontiguousarray(origins[:, order]), np.ascontiguousarray(directions[:, order]), 0.0,
                                t_max, eps, 0.0, max_steps, lipschitz, softness, None if limits is None else limits[order]).vis
        shadow[facing] = vis
    image.shadow = np.ones(hit.shape, dtype=np.float32)
    image.shadow[hit] = shadow
    if ao_radius is not None:
        nrm = np.ascontiguousarray(np.asarray(image.normals, dtype=np.float32)[hit].T)
        unit = np.abs((nrm.astype(np.float64) ** 2).sum(axis=0) - 1.0) <= 1e-5      # (no AO on a degenerate stencil)
        ao = np.ones(facing.size, dtype=np.float32)
        if unit.any():
            order = np.flatnonzero(unit)[_pixel_order(hit, unit)]
            ao[order] = ambient_occlusion(geometry, np.ascontiguousarray(image.points()[:, order]),
                                          np.ascontiguousarray(nrm[:, order]), ao_radius, ao_samples, ao_strength, lipschitz)
        image.ao = np.ones(hit.shape, dtype=np.float32)
        image.ao[hit] = ao
    return image
