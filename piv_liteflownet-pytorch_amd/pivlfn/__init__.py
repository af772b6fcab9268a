"""pivlfn -- MI355X-native PIV-LiteFlowNet inference path (drop-in for the reference's
`src/models.py` + `src/correlation.py` + `inference.estimate`).

The compute is in `libpivlfn.so` (hand-written HIP for gfx950, C ABI in include/pivlfn.h); this package is
the thin Python host side that mirrors the reference's names and argument meaning.  There is no CPU
fallback: importing works anywhere, but every op raises if the library or a GPU is missing.
"""
from .correlation import FunctionCorrelation, ModuleCorrelation          # noqa: F401
from .models import LiteFlowNet, LiteFlowNet2, Network, backwarp, hui_liteflownet, piv_liteflownet  # noqa: F401
from .inference import Inference, estimate                               # noqa: F401
from .stereo import estimate_stereo                                      # noqa: F401
from .validate import MaskedFlowStats, validate_flow                     # noqa: F401
from .preproc import FrameBackground, preprocess_frames                  # noqa: F401
from .evaluate import ErrorStats, FlowErrors, flow_errors, level_errors  # noqa: F401
from .quality import CENTRE_OUT, FEW, FLAT, NO_PEAK, MatchQuality, match_quality  # noqa: F401
from .uncertainty import FlowUncertainty, UncertaintyStats, flow_uncertainty, uncertainty_coverage  # noqa: F401
from .vortex import VortexField, vortex_gamma                           # noqa: F401
from .flowmap import LOST, OUT, UNDEFINED, FlowMap, FTLEField           # noqa: F401
from .pod import FlowPOD, PODResult                                     # noqa: F401
from .twopoint import TwoPointResult, TwoPointStats                     # noqa: F401
from .distribution import DistributionResult, FlowDistribution          # noqa: F401
from .spectrum import TemporalSpectrum, TemporalSpectrumResult          # noqa: F401
from .ensemble import EnsembleCorrelation, EnsembleResult, predictor_offsets  # noqa: F401
from .pressure import PressureField, PressureResult                     # noqa: F401
from .smooth import Smoothed, dct2, smooth_flow, smooth_param, smooth_wavelength, weights_from_uncertainty  # noqa: F401
from .calibrate import (calibrate_camera, dewarp_frames, find_markers, fit_mapping, gen_template, index_lattice,  # noqa: F401
                        target_points, template_match, write_coeff)
from .particles import BAD, PairParticles, ParticleImageGen, ParticleImages, displace_particles, render_particles  # noqa: F401
from .viz import (PngWriter, color_wheel_image, decimate_flow, field_absmax, flow_maxrad, flow_to_color, motion_to_color,  # noqa: F401
                  quiver_plot, scalar_to_color, vorticity_image, write_png, write_png_gray, GrayPngWriter)

__all__ = ["FunctionCorrelation", "ModuleCorrelation", "LiteFlowNet", "LiteFlowNet2", "Network", "backwarp",
           "hui_liteflownet", "piv_liteflownet", "estimate", "Inference", "estimate_stereo", "validate_flow", "MaskedFlowStats",
           "preprocess_frames", "FrameBackground", "flow_errors", "level_errors", "FlowErrors", "ErrorStats", "flow_to_color", "motion_to_color",
           "flow_maxrad", "scalar_to_color", "field_absmax", "vorticity_image", "decimate_flow", "quiver_plot", "color_wheel_image",
           "write_png", "PngWriter", "write_png_gray", "GrayPngWriter", "match_quality", "MatchQuality", "FEW", "FLAT", "NO_PEAK", "CENTRE_OUT",
           "flow_uncertainty", "FlowUncertainty", "UncertaintyStats", "uncertainty_coverage",
           "vortex_gamma", "VortexField", "FlowMap", "FTLEField", "OUT", "LOST", "UNDEFINED", "FlowPOD", "PODResult", "TwoPointStats", "TwoPointResult",
           "FlowDistribution", "DistributionResult",
           "TemporalSpectrum", "TemporalSpectrumResult", "PressureField", "PressureResult",
           "EnsembleCorrelation", "EnsembleResult", "predictor_offsets",
           "smooth_flow", "Smoothed", "smooth_param", "smooth_wavelength", "weights_from_uncertainty", "dct2",
           "gen_template", "template_match", "target_points", "find_markers", "index_lattice", "fit_mapping", "dewarp_frames", "calibrate_camera",
           "write_coeff", "ParticleImageGen", "ParticleImages", "PairParticles", "displace_particles", "render_particles", "BAD"]
