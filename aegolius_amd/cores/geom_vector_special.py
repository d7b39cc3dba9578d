"""Liquid-crystal waveguide vector fields (reference cores/geom_vector_special.py): a `VectorField` bound to one of the
stencil forms of `vector_functions_special`. `create(uu)` / `create((uu, ww))` takes the distance field(s) sampled on the
grid, not coordinates; the fields may be `DeviceField`s from `create_resident`, and `create_resident` leaves the result
in HBM. Modifications and the x / y / z / phi / theta / length read-outs work as for every other vector field."""
from .geom import VectorField
from .vector_functions_special import lcwg1_2d, lcwg1_m1, lcwg1_p1


class LCWG2D(VectorField):
    """Director field of a liquid-crystal waveguide, independent of z; cartesian components.

    Args:
        parameters: total width of the waveguide.
        co_resolution: number of points along each axis of the grid on which the SDF is evaluated.
        sign: None (sign computed automatically), a float (the threshold of the automatic sign), an int (+1 or -1:
            the same sign everywhere) or an array of +1 / -1, one per point.
    """

    def __init__(self, parameters, co_resolution, sign):
        self._parameters = parameters
        VectorField.__init__(self, lcwg1_2d, parameters, co_resolution, sign)

    @property
    def parameters(self):
        return self._parameters


class LCWG3Dm1(VectorField):
    """M1 director field of a liquid-crystal waveguide: winding number -1 in the yz plane; cartesian components.
    `create` takes (uu, ww): the distances across the width and along the thickness.

    Args:
        parameters: (total width, thickness) of the waveguide.
        co_resolution: number of points along each axis of the grid on which the SDF is evaluated.
        sign: as for LCWG2D.
    """

    def __init__(self, parameters, co_resolution, sign):
        self._parameters = parameters
        VectorField.__init__(self, lcwg1_m1, parameters, co_resolution, sign)

    @property
    def parameters(self):
        return self._parameters


class LCWG3Dp1(VectorField):
    """P1 director field of a liquid-crystal waveguide: winding number +1 in the yz plane; otherwise as LCWG3Dm1.

    Args:
        parameters: (total width, thickness) of the waveguide.
        co_resolution: number of points along each axis of the grid on which the SDF is evaluated.
        sign: as for LCWG2D.
    """

    def __init__(self, parameters, co_resolution, sign):
        self._parameters = parameters
        VectorField.__init__(self, lcwg1_p1, parameters, co_resolution, sign)

    @property
    def parameters(self):
        return self._parameters
