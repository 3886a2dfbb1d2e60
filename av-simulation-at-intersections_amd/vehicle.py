"""Minimal stand-ins for the two reference types the MPC surface touches, so the drop-in can be used
(and tested) without the reference tree: `State` (main/lib/simulation.py:11-19, field order x, y, yaw, v)
and a car-dimensions object exposing `distance_back_to_front_wheel` (main/lib/car_dimensions.py:82-90).
Any object with those attributes works; the reference's own classes are accepted unchanged.  And a vehicle's shape as the loops and
the recorder's evaluators take it: car_circles, vehicle_shape."""
import math
from dataclasses import dataclass


@dataclass
class State:
    x: float = 0.0
    y: float = 0.0
    yaw: float = 0.0
    v: float = 0.0


class BicycleModelDimensions:
    @property
    def distance_back_to_front_wheel(self) -> float:
        return 2.86


def car_circles(L: float = 2.86, width: float = 2.0, extra_length: float = 0.64):
    """Collision circles of the reference's BicycleModelDimensions (main/lib/car_dimensions.py:62-79,82-90): bounding
    box (width, L + 0.64), radius = width / sqrt(2), two centres on the body axis at L/2 +- (length/2 - width/2) from the
    rear axle.  Returns (radius, (front_offset, rear_offset))."""
    length = L + extra_length
    offset = length / 2 - width / 2
    return width / (2 ** .5), (L / 2 + offset, L / 2 - offset)


DIMS_KEYS = ("L", "width", "extra_length")


def vehicle_shape(dims=None, L: float = 2.86, width: float = 2.0, extra_length: float = 0.64):
    """One row of the shape table of jsim_loop_set_vehicle_shapes, (cc_front, cc_rear, radius, wheelbase), from the fields of
    `obstacle_dims`: dims = dict(L=..., width=..., extra_length=...) (any missing key: the keyword's value) through car_circles.
    Raises ValueError on an unknown key or a size that is not positive (extra_length: negative)."""
    if dims is not None:
        unknown = sorted(set(dims) - set(DIMS_KEYS))
        if unknown:
            raise ValueError(f"unknown dims key(s) {unknown}: a vehicle's dims holds {list(DIMS_KEYS)}")
        L, width, extra_length = (float(dims.get(k, d)) for k, d in zip(DIMS_KEYS, (L, width, extra_length)))
    if not (L > 0 and width > 0 and extra_length >= 0 and math.isfinite(L + width + extra_length)):
        raise ValueError(f"a vehicle's L and width must be positive and its extra_length not negative (L={L}, width={width}, "
                         f"extra_length={extra_length})")
    radius, (c0, c1) = car_circles(L, width, extra_length)
    return (c0, c1, radius, L)
