"""Liquid-crystal waveguide (LCWG) director fields (reference cores/vector_functions_special.py:14-251).

The stencil forms (`lcwg1_2d`, `lcwg1_p1`, `lcwg1_m1`) run as one fused kernel on the GPU (libsdfk.so, sdfk_lcwg_eval):
numpy.gradient of the scalar field, the rotations and the normalisations in one pass, in float64 from the fp32 inputs.
The automatic sign is `compute_crossings_2d` on the device (sdfk_field_crossings_2d). The field inputs may be host
arrays or `DeviceField`s from `create_resident`; a resident field never crosses PCIe. There is no NumPy evaluation here.
"""
import numpy as np

from .. import _engine
from .._eval import _grid_shape, config

_VARIANT = {"lcwg1_2d": 0, "lcwg1_p1": 1, "lcwg1_m1": 2}


def _field(a):
    """(DeviceField, owned) of an (N,) operand."""
    if isinstance(a, _engine.DeviceField):
        return a, False
    return _engine.DeviceField.from_host(np.asarray(a, dtype=np.float64).ravel(), config.device), True


def _host_out(dev):
    out = dev.numpy()
    dev.free()
    return out if config.output_dtype is np.float32 else out.astype(config.output_dtype)


def compute_crossings_2d(sdf_grid, thr=0.06):
    """Splits a 2-D scalar field into regions of +1 and -1, switching where a row reaches the field's minimum.

    Along every row (axis 1) a crossing is counted where the field comes within `thr` of its minimum after not being
    there one column before; the parity of the running count is smoothed by two 5x5 box averages and thresholded.

    Args:
        sdf_grid: (n0, n1) signed distance field or any scalar field.
        thr: absolute tolerance of the closeness test against the minimum.
    Returns:
        (n0, n1) int64 array of +1 / -1.
    """
    a = np.asarray(sdf_grid)
    if a.ndim != 2:
        raise NotImplementedError("compute_crossings_2d takes a 2-D array; got %d dimensions" % a.ndim)
    if a.size == 0:
        raise ValueError("zero-size array to reduction operation minimum which has no identity")
    field, _ = _field(a)
    with field, _engine.DeviceBuffer(a.size, what="compute_crossings_2d") as d_sign:
        _engine.check(_engine.lib().sdfk_field_crossings_2d(_engine._vp(field.ptr), None, a.shape[0], a.shape[1], 1, 1.0, 1.0,
                                                            float(thr), d_sign.at(), None), "sdfk_field_crossings_2d")
        out = d_sign.download(np.empty(a.shape, dtype=np.int8))
    return out.astype(np.int64)


def _lcwg_resident(name, uuww, p, co_resolution, sign):
    """The (3, N) field of lcwg1_2d / lcwg1_p1 / lcwg1_m1 as a DeviceVectorField."""
    variant = _VARIANT[name]
    res = np.asarray(co_resolution)
    if res.ndim != 1 or res.shape[0] != 3:                       # the reference indexes a third axis everywhere
        raise IndexError("co_resolution must have 3 entries; got %r" % (co_resolution,))
    if variant == 0:
        w, d = float(p), 1.0
        inputs = [uuww]
    else:
        w, d = float(p[0]), float(p[1])
        inputs = [uuww[0], uuww[1]]
    owned = []
    try:
        fields = []
        for a in inputs:
            f, own = _field(a)
            fields.append(f)
            if own:
                owned.append(f)
        n = fields[0].n
        if any(f.n != n for f in fields):
            raise ValueError("uu and ww must have the same number of points")
        shape = _grid_shape(n, co_resolution)
        if min(shape) < 2:
            raise ValueError("Shape of array too small to calculate a numerical gradient, at least (edge_order + 1) "
                             "elements are required.")
        lib, vp = _engine.lib(), _engine._vp
        uu_ptr, ww_ptr = vp(fields[0].ptr), vp(fields[1].ptr) if variant else None
        kind, value, d_sign = 0, 0.0, None
        if sign is None or isinstance(sign, float):              # python float / np.float64: the threshold of the auto sign
            thr = abs(sign) if sign is not None else 0.06
            if variant == 0 and int(co_resolution[2]) != shape[2]:
                # lcwg1_2d repeats the sign plane by the unconverted co_resolution[2] (:157)
                raise ValueError("operands could not be broadcast together with shapes (%d,) (%d,)"
                                 % (shape[0] * shape[1] * int(co_resolution[2]), n))
            plane = _engine.DeviceField((shape[0] * shape[1] + 3) // 4, config.device)   # int8 plane in float storage
            owned.append(plane)
            _engine.check(lib.sdfk_field_crossings_2d(uu_ptr, ww_ptr, shape[0], shape[1], shape[2], w, d, float(thr),
                                                      vp(plane.ptr), None), "sdfk_field_crossings_2d")
            kind, d_sign = 1, vp(plane.ptr)
        elif isinstance(sign, _engine.DeviceField):
            if sign.n != n:
                raise ValueError("operands could not be broadcast together with shapes (%d,) (%d,)" % (sign.n, n))
            kind, d_sign = 2, vp(sign.ptr)
        else:
            s = np.asarray(sign, dtype=np.float64)
            if s.size == 1:
                value = float(s.reshape(-1)[0])
            elif s.shape == (n,):
                row = _engine.DeviceField.from_host(s, config.device)
                owned.append(row)
                kind, d_sign = 2, vp(row.ptr)
            else:
                raise ValueError("operands could not be broadcast together with shapes %r (%d,)" % (s.shape, n))
        out = _engine.DeviceVectorField(n, config.device)
        try:
            _engine.check(lib.sdfk_lcwg_eval(variant, uu_ptr, ww_ptr, shape[0], shape[1], shape[2], w, d, kind, value,
                                             d_sign, vp(out.ptr), out.stride, None), "sdfk_lcwg_eval")
        except Exception:
            out.free()
            raise
        return out
    finally:
        for f in owned:
            f.free()


def lcwg1_2d(uu, p, co_resolution, sign):
    """Director field of a liquid-crystal waveguide that does not depend on z.

    The raw numpy.gradient of `uu` on the grid is turned about z by sign * (clip(2 uu / w, 0, 1) pi + pi / 2) and
    normalised.

    Args:
        uu: (N,) distance field of the waveguide's centre line (ndarray or DeviceField).
        p: total width w of the waveguide.
        co_resolution: resolution of the grid the field was created on (3 entries).
        sign: None or a float (the automatic sign of compute_crossings_2d on grid plane k = 0, the float's absolute
            value as its threshold), or a number or (N,) array that multiplies the angle as given.
    Returns:
        (3, N) array of unit vectors (zero where the rotated gradient is zero).
    """
    return _host_out(_lcwg_resident("lcwg1_2d", uu, p, co_resolution, sign))


def lcwg1_p1(uuww, p, co_resolution, sign):
    """P1 director field of a liquid-crystal waveguide: winding number +1 in the yz plane.

    With pp = |(2 uu / w, ww / d)|, the normalised gradient of pp is turned about vec x e1 by
    sign * (clip(pp, 0, 1) pi + pi / 2), e1 = the normalised (-vec_y, vec_x, 0), then about e1 by -2 alpha,
    alpha = arctan2(2 ww / d^2, 8 uu / w^2), and normalised.

    Args:
        uuww: (uu, ww): the distances across and along the thickness of the waveguide, each (N,) (ndarrays or
            DeviceFields), or one (>= 2, N) array.
        p: (w, d): total width and thickness of the waveguide.
        co_resolution: resolution of the grid the fields were created on (3 entries).
        sign: as for lcwg1_2d; the automatic sign is taken from pp.
    Returns:
        (3, N) array of unit vectors.
    """
    return _host_out(_lcwg_resident("lcwg1_p1", uuww, p, co_resolution, sign))


def lcwg1_m1(uuww, p, co_resolution, sign):
    """M1 director field of a liquid-crystal waveguide: winding number -1 in the yz plane (lcwg1_p1 with
    alpha = -arctan2(2 ww / d^2, 8 uu / w^2))."""
    return _host_out(_lcwg_resident("lcwg1_m1", uuww, p, co_resolution, sign))


def _old(variant, r, uu, p):
    if variant == 0:
        w, d = float(p), 1.0
    else:
        w, d = float(p[0]), float(p[1])
    rows = 2 if variant == 0 else 3
    if isinstance(r, _engine.DeviceVectorField):
        rv, own_r = r, False
    else:
        ra = np.asarray(r, dtype=np.float64)
        if ra.ndim != 2 or ra.shape[0] < rows:
            raise IndexError("r must hold at least %d rows of coordinates; got shape %r" % (rows, ra.shape))
        full = np.zeros((3, ra.shape[1]))
        full[:min(3, ra.shape[0])] = ra[:3]
        rv, own_r = _engine.DeviceVectorField.from_host(full, config.device), True
    field, own_u = _field(uu)
    try:
        if field.n != rv.n:
            raise ValueError("r and uu must have the same number of points")
        out = _engine.DeviceVectorField(rv.n, config.device)
        vp = _engine._vp
        _engine.check(_engine.lib().sdfk_lcwg_old_eval(variant, vp(rv.ptr), rv.stride, vp(field.ptr), rv.n, w, d,
                                                       vp(out.ptr), out.stride, None), "sdfk_lcwg_old_eval")
        return _host_out(out)
    finally:
        if own_r:
            rv.free()
        if own_u:
            field.free()


def lcwg1_2d_old(r, uu, p):
    """Straight waveguide along x: (-cos(pi qq), -sin(pi qq), 0) with qq = clip(uu, 0, 1) where |r_y| <= w / 2,
    (1, 0, 0) elsewhere; p = w."""
    return _old(0, r, uu, p)


def lcwg1_p1_old(r, uu, p):
    """Straight waveguide along x: (-cos(pi qq), -sin(pi qq) cos a, -sin(pi qq) sin a), normalised,
    a = arctan2(2 r_z / d^2, 8 r_y / w^2), where |r_y| <= w / 2, (1, 0, 0) elsewhere; p = (w, d)."""
    return _old(1, r, uu, p)


def lcwg1_m1_old(r, uu, p):
    """lcwg1_p1_old with a = -arctan2(2 r_z / d^2, 8 r_y / w^2)."""
    return _old(2, r, uu, p)


for _name in _VARIANT:
    globals()[_name]._vec_leaf = _name
