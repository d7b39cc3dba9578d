"""Meshing a geometry without a field (aegolius_amd.mesh, geometry path) without a GPU: the scratch bound of the C-ABI,
argument checks that come before any device work, and from_geometry making no coordinate array."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from aegolius_amd import mesh  # noqa: E402

ENTRIES = ("sdfk_eval_grid_isosurface_scratch", "sdfk_eval_grid_isosurface", "sdfk_eval_grid_isosurface_finish",
           "sdfk_eval_grid_contour2d_scratch", "sdfk_eval_grid_contour2d", "sdfk_eval_grid_contour2d_finish")


def test_entries_are_declared_and_exported(built):
    header = open(os.path.join(os.path.dirname(HERE), "include", "sdfk.h")).read()
    for name in ENTRIES:
        assert name in built.SIGNATURES and hasattr(built.lib(), name)
        assert name + "(" in header


@pytest.mark.parametrize("shape", [(4097, 4097, 4097), (33, 33, 33), (4097, 4097, 2), (5, 5, 333), (2049, 2049, 2049),
                                   (3, 5, 7), (7, 50, 40)])
def test_isosurface_scratch_is_at_most_one_byte_per_point(built, shape):
    n = int(np.prod(shape, dtype=np.int64))
    got = built.lib().sdfk_eval_grid_isosurface_scratch(*shape)
    assert got <= n + (1 << 20)
    assert got >= built.lib().sdfk_field_isosurface_scratch(*shape)      # it holds the mesh state of the field path


@pytest.mark.parametrize("shape", [(65537, 65537), (1025, 1025), (33, 33), (5, 333), (65537, 2), (201, 301)])
def test_contour_scratch_is_at_most_one_byte_per_point(built, shape):
    n = int(np.prod(shape, dtype=np.int64))
    got = built.lib().sdfk_eval_grid_contour2d_scratch(*shape)
    assert got <= n + (1 << 20)
    assert got >= built.lib().sdfk_field_contour2d_scratch(*shape)


def test_the_bound_at_4097_cubed_is_near_the_mesh_state(built):
    n = 4097 ** 3
    assert built.lib().sdfk_eval_grid_isosurface_scratch(4097, 4097, 4097) <= 0.76 * n


def test_bad_input_raises_value_error_before_device_work(built):
    from aegolius_amd.cores import Sphere
    ax = [np.linspace(-1, 1, 9)] * 3
    with pytest.raises(ValueError, match="NaN"):
        mesh.isosurface(Sphere(0.5), ax, float("nan"))
    with pytest.raises(ValueError, match="NaN"):
        mesh.contour(Sphere(0.5), ax[:2], float("nan"))
    with pytest.raises(ValueError, match="increasing"):
        mesh.isosurface(Sphere(0.5), [ax[0], ax[1][::-1], ax[2]])
    with pytest.raises(ValueError, match="increasing"):
        mesh.isosurface(Sphere(0.5), [ax[0], np.r_[ax[1][:4], ax[1][3:]], ax[2]])
    with pytest.raises(ValueError, match="expected 3 axis tables"):
        mesh.isosurface(Sphere(0.5), ax[:2])
    with pytest.raises(ValueError, match="contour"):
        mesh.contour(Sphere(0.5), ax)                            # a 3-D grid
    with pytest.raises(ValueError, match="NaN"):
        mesh.from_geometry(Sphere(0.5), (2, 2, 2), (9, 9, 9), level=float("nan"))


def test_from_geometry_makes_no_coordinate_array(built, monkeypatch):
    import aegolius_amd.cores as ns

    class Sentinel(Exception):
        pass

    def no_grid(*args, **kwargs):
        raise Sentinel("generate_grid was called")
    monkeypatch.setattr(ns, "generate_grid", no_grid)
    if built.device_count() > 0:
        m = mesh.from_geometry(ns.Sphere(0.5), (2, 2, 2), (65, 65, 65))
        assert len(m.vertices) > 0 and len(m.faces) > 0
    else:
        with pytest.raises(built.SdfkError, match="no HIP device"):
            mesh.from_geometry(ns.Sphere(0.5), (2, 2, 2), (65, 65, 65))


def test_abi_refuses_bad_calls_without_touching_the_device(built):
    import ctypes
    L = built.lib()
    t = [np.ascontiguousarray(np.linspace(-1, 1, 5), dtype=np.float32)] * 3
    nv, nf = ctypes.c_int64(-1), ctypes.c_int64(-1)
    rc = L.sdfk_eval_grid_isosurface(None, built._ptr(t[0]), 5, built._ptr(t[1]), 5, built._ptr(t[2]), 5, 0.0,
                                     ctypes.byref(nv), ctypes.byref(nf), ctypes.c_void_p(4096), None, 0)
    assert rc != 0
    rc = L.sdfk_eval_grid_contour2d(None, built._ptr(t[0]), 5, built._ptr(t[1]), 5, 0.0, ctypes.byref(nv), ctypes.byref(nf),
                                    ctypes.c_void_p(4096), None, 0)
    assert rc != 0
