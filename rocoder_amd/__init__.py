"""rocoder_amd — MI355X (gfx950) engine for rocoder's analysis -> kernel -> resynthesis ->
overlap-add stretch path. The compute lives in librocoder_hip.so (hand-written HIP, C-ABI in
include/rocoder_hip.h); this package is the host-side mirror of the reference interface."""
from .stretcher import (AudioBus, AudioSpec, Bus, DeviceKernelCompileError, Engine, MultiEngine, ReFFT,  # noqa: F401
                        RocoderError, Stretcher, StretcherProcessor, autocrop_points, compile_device_kernel, derive_params,
                        device_kernel_cross_channel, device_kernel_feedback, device_kernel_history, device_kernel_sums,
                        RC_PHASE_LOCKED, RC_PHASE_PROPAGATE, RC_PHASE_RANDOM, load_kernel_library, mix_envelope, phase_envelope,
                        offline_output_len, pinned_empty, split_mono_map, stretch, time_map_curve, time_map_output_len, warp_curve, warp_table)

__version__ = "0.1.0"
