"""Golden-vector generator for the liquid-crystal waveguide fields — runs ONLY in the build container, where the
reference is mounted read-only at /root/reference. It imports the real SPOMSO implementation, runs the scenes of
tests/lcwg_scenes.py and stores inputs + float64 outputs next to this script (data only):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/generate_lcwg_golden.py

Besides the outputs it stores, per point, how far the reference itself moves when its field inputs move by one fp32 ulp
(the sign held fixed): the conditioning slack of the GPU tests (tests/test_gpu_vector.py uses the same rule)."""
import contextlib
import io
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, "/root/reference/Code/spomso")
sys.dont_write_bytecode = True

import spomso.cores as ref  # noqa: E402  (the real reference)
from spomso.cores import geom_vector_special as gvs  # noqa: E402
from spomso.cores import vector_functions_special as vfs  # noqa: E402
import lcwg_scenes as ls  # noqa: E402


def up(a):
    """every entry one fp32 ulp up"""
    return np.nextafter(np.asarray(a, dtype=np.float32), np.float32(np.inf)).astype(np.float64)


def f16_up(a):
    """float16 that is never below `a` (slack bounds are stored at half precision)"""
    h = np.asarray(a, dtype=np.float16)
    return np.where(h.astype(np.float64) < a, np.nextafter(h, np.float16(np.inf)), h)


def effective_sign(cls, uu, ww, res, sign, shape):
    """The sign array the reference multiplies by (the automatic plane repeated along axis 2)."""
    if sign is None or isinstance(sign, float):
        thr = abs(sign) if sign is not None else 0.06
        plane = (uu if cls == "LCWG2D" else np.linalg.norm([2 * uu / ls.W, ww / ls.D], axis=0)).reshape(shape)[:, :, 0]
        return vfs.compute_crossings_2d(plane, thr=thr), np.repeat(vfs.compute_crossings_2d(plane, thr=thr)[:, :, None],
                                                                    shape[2], axis=2).ravel()
    return None, sign


def run(cls, params, res, sign, inp, read="create"):
    with contextlib.redirect_stdout(io.StringIO()), np.errstate(all="ignore"):
        f = getattr(gvs, cls)(params, res, sign)
        return np.asarray(getattr(f, read)(inp), dtype=np.float64)


def main():
    out, meta = {}, {"numpy": np.__version__, "reference": "peterropac/Aegolius SPOMSO 1.4.0", "small_res": ls.SMALL_RES,
                     "fields": {}, "crossings": {}, "raising": {}}
    # (a) compute_crossings_2d; the planes themselves are seeded (lcwg_scenes.crossing_planes), only the results are kept
    for name, plane, thr in ls.crossing_planes():
        got = vfs.compute_crossings_2d(plane, thr=thr)
        assert got.dtype == np.int64
        out["crossings/" + name] = got.astype(np.int8)
        meta["crossings"][name] = {"thr": thr, "shape": list(plane.shape), "minus": int((got < 0).sum())}
    # (b) every class x sign on the small example grid, kept at a fixed subset plus every zero vector; the read-outs are
    # numpy functions of the field (checked here on the whole grid), so only the field and its slack are stored
    uu, ww = ls.example_inputs(ref, ls.SMALL_RES)
    shape = tuple(ref.resolution_conversion(r) for r in ls.SMALL_RES)
    n = uu.size
    out["small/uu"], out["small/ww"] = uu.astype(np.float32), ww.astype(np.float32)
    fields, slacks = {}, {}
    for cls in ls.CLASSES:
        params, inp = ls.field_args(cls, uu, ww)
        _, inp_up = ls.field_args(cls, up(uu), up(ww))
        for label in ls.SIGN_LABELS:
            sign = ls.sign_value(label, n)
            plane, fixed = effective_sign(cls, uu, ww, ls.SMALL_RES, sign, shape)
            if plane is not None:
                out["plane/%s/%s" % (cls, label)] = plane.astype(np.int8)
            got = run(cls, params, ls.SMALL_RES, sign, inp)
            moved = run(cls, params, ls.SMALL_RES, fixed, inp_up)
            for read in ls.READ_OUTS:
                assert np.array_equal(run(cls, params, ls.SMALL_RES, sign, inp, read), ls.read_out(got, read),
                                      equal_nan=True), (cls, label, read)
            key = "%s/%s" % (cls, label)
            fields[key] = got
            slacks[key] = {read: 8.0 * np.abs(ls.read_out(moved, read) - ls.read_out(got, read)) for read in ls.SLACK_READS}
            meta["fields"][key] = {"zero_vectors": int((got == 0).all(axis=0).sum())}
    zero = np.flatnonzero(np.any([(v == 0).all(axis=0) for v in fields.values()], axis=0))
    fpick = np.union1d(ls.pick(n, ls.FIELD_PICK, 3), zero)
    out["small/pick"] = fpick.astype(np.int32)
    for key, got in fields.items():
        out["field/" + key] = got[:, fpick]
        for read, sl in slacks[key].items():
            out["slack/%s/%s" % (key, read)] = f16_up(sl[..., fpick])
    # (d) one modification on an LCWG field
    with contextlib.redirect_stdout(io.StringIO()):
        f = gvs.LCWG3Dm1((ls.W, ls.D), ls.SMALL_RES, 1)
        f.rotate_phi(0.4)
        out["modified/LCWG3Dm1/rotate_phi"] = np.asarray(f.create((uu, ww)), dtype=np.float64)[:, fpick]
    # (c) the degenerate straight guide: every degenerate point and a fixed subset of the others
    suu, sww, sres = ls.segment_inputs(ref)
    sshape = tuple(int(r) for r in sres)
    out["segment/uu"], out["segment/ww"] = suu.astype(np.float32), sww.astype(np.float32)
    pp = np.linalg.norm([2 * suu / ls.SEGMENT_WD[0], sww / ls.SEGMENT_WD[1]], axis=0)
    vec = np.asarray(np.gradient(pp.reshape(sshape))).reshape(3, -1)
    degenerate = np.flatnonzero((vec[0] == 0) & (vec[1] == 0))
    spick = np.union1d(ls.pick(suu.size, ls.SEGMENT_PICK, 4), degenerate)
    out["segment/pick"] = spick.astype(np.int32)
    out["segment/degenerate"] = np.isin(spick, degenerate)
    for cls in ("LCWG3Dm1", "LCWG3Dp1"):
        for label in ("none", "int_1", "int_-1"):
            got = run(cls, ls.SEGMENT_WD, sres, ls.sign_value(label, suu.size), (suu, sww))
            out["segment/%s/%s" % (cls, label)] = got[:, spick]
    meta["segment"] = {"res": list(sshape), "degenerate": int(degenerate.size)}
    # (f) the example at full size: device SDF -> device field; a fixed subset and the whole sign planes. The device
    # SDFs match the reference's to 1e-6 * max(1, |v|) (tests/test_gpu_parity.py), not to fp32 rounding, and the
    # gradient of the field passes that on: the slack is 8x the reference's movement under input changes of that size
    # (random signs, two trials, the sign plane held fixed)
    euu, eww = ls.example_inputs(ref, ls.EXAMPLE_RES)
    coor, _ = ref.generate_grid(ls.co_size(), ls.EXAMPLE_RES)
    wg, vertical = ls.quarter_circle(ref)
    euu64, eww64 = wg.create(coor), vertical.create(coor)
    eshape = tuple(ref.resolution_conversion(r) for r in ls.EXAMPLE_RES)
    pick = ls.pick(euu.size, ls.SUBSET, 5)
    out["example/pick"] = pick.astype(np.int32)
    for cls, res in (("LCWG3Dm1", ls.EXAMPLE_RES), ("LCWG2D", (101, 101, 51))):
        params, inp = ls.field_args(cls, euu64, eww64)
        plane, fixed = effective_sign(cls, euu64, eww64, res, None, eshape)
        plane32, _ = effective_sign(cls, euu, eww, res, None, eshape)
        assert np.array_equal(plane, plane32), "the example's sign plane moves under fp32 rounding"
        got = run(cls, params, res, None, inp)
        out["example/%s" % cls] = got[:, pick]
        moved = np.zeros_like(got)
        for trial in range(2):
            s = np.random.default_rng(11 + trial).choice([-1.0, 1.0], size=(2, euu.size))
            puu = euu64 + 1e-6 * s[0] * np.maximum(1.0, np.abs(euu64))
            pww = eww64 + 1e-6 * s[1] * np.maximum(1.0, np.abs(eww64))
            _, pin = ls.field_args(cls, puu, pww)
            moved = np.fmax(moved, np.abs(run(cls, params, res, fixed, pin) - got))
        out["example_slack/%s" % cls] = f16_up(8.0 * moved[:, pick])
        out["example_plane/%s" % cls] = plane.astype(np.int8)
    # (g) the pointwise _old forms on the seeded inputs of lcwg_scenes.old_inputs
    r, ou = ls.old_inputs()
    out["old/lcwg1_2d_old"] = vfs.lcwg1_2d_old(r, ou, ls.W)
    out["old/lcwg1_p1_old"] = vfs.lcwg1_p1_old(r, ou, (ls.W, ls.D))
    out["old/lcwg1_m1_old"] = vfs.lcwg1_m1_old(r, ou, (ls.W, ls.D))
    # (e) the reference's exceptions
    raising = {
        "missing_sign": lambda: gvs.LCWG2D(ls.W, ls.SMALL_RES),
        "even_z_2d_auto": lambda: gvs.LCWG2D(ls.W, (20, 20, 6), None).create(uu),
        "two_entry_resolution": lambda: gvs.LCWG3Dm1((ls.W, ls.D), (21, 147), 1).create((uu, ww)),
    }
    for name, fn in raising.items():
        try:
            with contextlib.redirect_stdout(io.StringIO()), np.errstate(all="ignore"):
                fn()
            meta["raising"][name] = None
        except Exception as e:  # noqa: BLE001
            meta["raising"][name] = type(e).__name__
    np.savez_compressed(os.path.join(HERE, "lcwg_golden.npz"), **out)
    with open(os.path.join(HERE, "lcwg_golden_meta.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
    print("crossings: %d, fields: %d, degenerate: %d, raising: %r"
          % (len(meta["crossings"]), len(meta["fields"]), meta["segment"]["degenerate"], meta["raising"]))


if __name__ == "__main__":
    main()
