"""The channel peaks and the split-mono decision of include/rocoder_hip.h (rc_engine_frames_channel_peaks,
rc_split_mono_map) stated in numpy: the yardstick of tests/test_frames_map_host.py and tests/test_gpu_frames_map.py. The
block is decoded with tests/autocroputil.py (one float32 division per sample), the sign bit of the bits is cleared and the
maximum of the uint32 view is taken per channel; the decision is recorder::auto_split_mono (src/recorder.rs:118-144) as it
stands, on those peaks: a channel is empty where every sample == 0.0, which is where its peak == 0.0."""
import numpy as np

import autocroputil as au


def channel_peaks(x):
    """float32 [n_frames, channels] -> float32 [channels]: the float whose bits are the largest bits of |x| of the channel
    (a NaN above +inf above every finite magnitude); +0.0 for no frames"""
    x = np.ascontiguousarray(x, np.float32)
    bits = x.view(np.uint32) & np.uint32(0x7FFFFFFF)
    if x.shape[0] == 0:
        return np.zeros(x.shape[1], np.float32)
    return bits.max(axis=0).astype(np.uint32).view(np.float32)


def raw_channel_peaks(raw, fmt, channels):
    return channel_peaks(au.decode(bytes(raw), fmt, channels))


def split_mono_map(peaks):
    """(map, found): auto_split_mono's loop over the channels, `all(|s| *s == 0.0)` read off the channel's peak"""
    peaks = np.asarray(peaks, np.float32)
    n_empty, last_nonempty = 0, None
    for i, p in enumerate(peaks):
        if p == np.float32(0.0):  # (NaN == 0.0 is false: not empty)
            n_empty += 1
        else:
            last_nonempty = i
    if not (n_empty == len(peaks) - 1 and last_nonempty is not None):
        return list(range(len(peaks))), False
    return [last_nonempty] * len(peaks), True
