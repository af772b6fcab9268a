"""Alias of pivlfn.postpro under the reference's import path (src/postpro.py): calc_vorticity and de_vort on the GPU; vector
validation (pivlfn.validate) is re-exported next to them."""
from pivlfn.postpro import FlowStats, calc_vorticity, de_vort, flow_fields  # noqa: F401
from pivlfn.validate import MaskedFlowStats, validate_flow  # noqa: F401
