"""Alias of pivlfn.viz and pivlfn.flo under the reference's import path (src/utils_plot.py): motion_to_color and quiver_plot on the
GPU, next to the .flo reader and writer the reference keeps in the same module."""
from pivlfn.flo import flowname_modifier, read_flow, write_flow  # noqa: F401
from pivlfn.viz import (PngWriter, color_wheel_image, decimate_flow, flow_to_color, motion_to_color, quiver_plot,  # noqa: F401
                        scalar_to_color, vorticity_image, write_png)
