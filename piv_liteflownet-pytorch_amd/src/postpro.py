"""Alias of pivlfn.postpro under the reference's import path (src/postpro.py): calc_vorticity and de_vort on the GPU."""
from pivlfn.postpro import FlowStats, calc_vorticity, de_vort, flow_fields  # noqa: F401
