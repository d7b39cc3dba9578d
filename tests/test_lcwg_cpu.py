"""Liquid-crystal waveguide fields without a GPU: the public surface against the reference's (recorded by
tests/golden/generate_api_signatures_special.py), the exceptions raised before any device work, and the golden's meta."""
import inspect
import json
import os

import numpy as np
import pytest

import lcwg_scenes as ls

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")


def _params(obj):
    return [[p.name, p.kind.name, None if p.default is inspect.Parameter.empty else repr(p.default)]
            for p in inspect.signature(obj).parameters.values()]


def test_special_modules_match_the_reference_signatures():
    import importlib
    rec = json.load(open(os.path.join(GOLDEN, "reference_api_special.json")))
    diffs = []
    for mod_name, names in rec["modules"].items():
        mod = importlib.import_module("aegolius_amd.cores." + mod_name)
        for name, d in names.items():
            obj = getattr(mod, name, None)
            if obj is None:
                diffs.append("%s.%s missing" % (mod_name, name))
            elif d["kind"] == "function":
                if _params(obj) != d["signature"]:
                    diffs.append("%s.%s%r, reference %r" % (mod_name, name, _params(obj), d["signature"]))
            else:
                for meth, want in d["methods"].items():
                    if _params(getattr(obj, meth)) != want:
                        diffs.append("%s.%s.%s" % (mod_name, name, meth))
                diffs += ["%s.%s.%s (property) missing" % (mod_name, name, p) for p in d["properties"] if not hasattr(obj, p)]
                diffs += ["%s.%s base %s" % (mod_name, name, b) for b in d["bases"] if b not in [c.__name__ for c in obj.__mro__]]
    assert not diffs, "\n".join(diffs)


def test_package_exports_compute_crossings_2d():
    import aegolius_amd.cores as ns
    from aegolius_amd.cores import vector_functions_special
    assert ns.compute_crossings_2d is vector_functions_special.compute_crossings_2d
    assert str(inspect.signature(ns.compute_crossings_2d)) == "(sdf_grid, thr=0.06)"
    assert hasattr(ns, "geom_vector_special") and hasattr(ns, "vector_functions_special")


@pytest.mark.parametrize("cls", ls.CLASSES)
def test_missing_sign_raises_type_error(cls):
    from aegolius_amd.cores import geom_vector_special as gvs
    with pytest.raises(TypeError):
        getattr(gvs, cls)((ls.W, ls.D), ls.SMALL_RES)


def test_crossings_take_two_dimensional_arrays_only():
    import aegolius_amd.cores as ns
    with pytest.raises(NotImplementedError):
        ns.compute_crossings_2d(np.zeros((3, 3, 3)))
    with pytest.raises(NotImplementedError):
        ns.compute_crossings_2d(np.zeros(9))


def test_lcwg_golden_meta_is_consistent():
    meta = json.load(open(os.path.join(GOLDEN, "lcwg_golden_meta.json")))
    g = np.load(os.path.join(GOLDEN, "lcwg_golden.npz"))
    names = set(g.files)
    assert tuple(meta["small_res"]) == ls.SMALL_RES
    assert len(meta["crossings"]) == len(ls.crossing_planes())
    for name, plane, thr in ls.crossing_planes():
        assert meta["crossings"][name]["thr"] == thr
        assert meta["crossings"][name]["shape"] == list(plane.shape) == list(g["crossings/" + name].shape)
        assert set(np.unique(g["crossings/" + name])) <= {-1, 1}
    n = int(np.prod(ls.SMALL_RES))
    pick = g["small/pick"]
    assert pick.size >= ls.FIELD_PICK and np.all(np.diff(pick) > 0) and 0 <= pick[0] and pick[-1] < n
    for cls in ls.CLASSES:
        for label in ls.SIGN_LABELS:
            key = "%s/%s" % (cls, label)
            assert key in meta["fields"]
            assert g["field/" + key].shape == (3, pick.size)
            for read in ls.SLACK_READS:
                assert g["slack/%s/%s" % (key, read)].shape == ((3, pick.size) if read == "create" else (pick.size,))
    assert int(g["segment/degenerate"].sum()) == meta["segment"]["degenerate"] > 0
    assert g["segment/LCWG3Dm1/none"].shape == (3, g["segment/pick"].size)
    r, uu = ls.old_inputs()
    assert g["old/lcwg1_2d_old"].shape == r.shape and uu.shape == (r.shape[1],)
    assert g["example/pick"].size == ls.SUBSET
    assert g["example_plane/LCWG3Dm1"].shape == (101, 101)
    assert meta["raising"] == {"missing_sign": "TypeError", "even_z_2d_auto": "ValueError",
                               "two_entry_resolution": "IndexError"}
