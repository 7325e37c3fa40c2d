"""The autocrop of include/rocoder_hip.h (rc_engine_frames_power, rc_autocrop_points) stated in numpy float32: the
yardstick of tests/test_frames_power_host.py and tests/test_gpu_frames_power.py. The reader's decode is one float32
division per sample, the peaks are `abs` and a maximum, and nothing is computed in float64. The decibels are numpy's
float32 log10, which need not round as the C library's log10f does: tests that compare crop points keep their bins either
bit-equal or 1 % apart, so that no order depends on it."""
import numpy as np

F = np.float32
MIN_DECIBELS = F(-99999999.0)
PCM_BYTES = {"u8": 1, "i16": 2, "i24": 3, "i32": 4, "f32": 4}
PCM_K = {"u8": 127, "i16": 32767, "i24": 8388608, "i32": 2147483647}


def decode(raw, fmt, channels):
    """bytes of whole little-endian frames -> float32 [n_frames, channels], the reader's (float)n / K (one division)"""
    b = np.frombuffer(raw, np.uint8)
    if fmt == "f32":
        x = b.view("<f4").astype(np.float32)
    else:
        if fmt == "u8":
            n = b.astype(np.int32) - 128
        elif fmt == "i16":
            n = b.view("<i2").astype(np.int32)
        elif fmt == "i24":
            t = b.reshape(-1, 3).astype(np.int32)
            n = t[:, 0] | (t[:, 1] << 8) | (t[:, 2] << 16)
            n = np.where(n >= 1 << 23, n - (1 << 24), n).astype(np.int32)
        else:
            n = b.view("<i4").astype(np.int32)
        x = n.astype(np.float32) / F(PCM_K[fmt])  # int32 -> float32 rounds to nearest even; F(2147483647) is 2^31
    return x.reshape(-1, channels)


def bin_peaks(x, bin_frames):
    """float32 [n_frames, channels] -> float32 [ceil(n_frames / bin_frames)]: the largest |x| of each bin over all
    channels, NaN skipped, +0.0 for a bin of nothing but zeros or NaN"""
    x = np.asarray(x, np.float32)
    if x.shape[0] == 0:
        return np.zeros(0, np.float32)
    a = np.abs(x)
    a[np.isnan(a)] = F(0)
    per_frame = a.max(axis=1)
    return np.maximum.reduceat(per_frame, np.arange(0, x.shape[0], bin_frames, dtype=np.int64)).astype(np.float32)


def decibels(peaks):
    """power::relative_decibels (src/power.rs:6-8)"""
    with np.errstate(divide="ignore"):
        return np.maximum(np.log10(np.abs(np.asarray(peaks, np.float32))) * F(20), MIN_DECIBELS).astype(np.float32)


def noise_threshold(values, percentile):
    """determine_noise_threshold (src/recorder.rs:165-173) on any values that order: the index is computed in float32"""
    v = np.sort(np.asarray(values, np.float32))
    return v[int(np.floor(F(percentile) / F(100) * F(v.size)))]


def crop_bins(values, percentile):
    """determine_autocrop_points (src/recorder.rs:176-191) in bin indices: (first, min(last + 1, n - 1)) or None"""
    values = np.asarray(values, np.float32)
    above = np.nonzero(values > noise_threshold(values, percentile))[0]
    if above.size == 0:
        return None
    return int(above[0]), int(min(above[-1] + 1, values.size - 1))


def autocrop_points(peaks, bin_frames, percentile):
    """rc_autocrop_points on linear peaks: (start, end) in frames, or None"""
    got = crop_bins(decibels(peaks), percentile)
    return None if got is None else (got[0] * bin_frames, got[1] * bin_frames)
