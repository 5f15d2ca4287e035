"""iq_tool_amd -- MI355X-native replacement for iq_tool's pre_processor -> resampler ->
post_processor sample path.  The compute lives in lib/libiqgpu.so (HIP, gfx950);
importing the package never falls back to a CPU implementation."""
from ._lib import FMT, IqgpuError, LIB_PATH, load          # noqa: F401
from .chain import Chain, DeviceBuffer, PinnedBuffer, bind_thread_to_device, design_out_frames, design_out_frames_range, design_preroll_frames, design_preroll_frames_dcrms, design_preroll_frames_rms, design_state_size, make_desc, state_inspect   # noqa: F401
from .iq_optimizer import IqOptimizer                            # noqa: F401
from .psd import Psd                                             # noqa: F401
from .sgram import Sgram                                         # noqa: F401
from .stats import Stats                                         # noqa: F401
from .env import Env                                             # noqa: F401
from .lag import Lag                                             # noqa: F401
from .match import Match                                         # noqa: F401

__all__ = ["Chain", "DeviceBuffer", "PinnedBuffer", "IqOptimizer", "Psd", "Sgram", "Stats", "Env", "Lag", "Match", "make_desc", "FMT", "IqgpuError", "load", "LIB_PATH"]
