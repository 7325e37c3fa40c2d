"""The output fade of include/rocoder_hip.h (rc_engine_set_output_fade) stated in numpy float32: the yardstick of
tests/test_frames_fade_host.py and tests/test_gpu_frames_fade.py. Every operation below is one float32 operation of
numpy - one correctly rounded IEEE operation - in the order the header states them; nothing is computed in float64."""
import numpy as np

NONE = 2 ** 64 - 1  # RC_FADE_NONE
F = np.float32


def sq(p, d, falling):
    """sq(p, d) for an array of positions p < d: float32"""
    p = np.asarray(p, np.uint64)
    r = p.astype(np.float32) / np.array([d], np.uint64).astype(np.float32)[0]  # u64 -> f32: round to nearest even
    b = r * F(2) - F(1)
    if falling:
        b = -b
    return np.sqrt(F(0.5) * (F(1) + np.maximum(b, F(-1))))


def apply_fade(y, in_len=0, out_start=NONE, out_len=0, axis=0):
    """z of the definition for the float32 result y, whose frames run along `axis` (0: [frames, channels] as
    stretch_frames gives them; 1: [channels, frames] as stretch_host does). A copy: y is left as it is."""
    z = np.array(y, np.float32, copy=True)
    v = np.moveaxis(z, axis, 0)  # a view: [frames, ...]
    T = v.shape[0]
    assert in_len <= T and (out_start == NONE or out_start + out_len <= T), (in_len, out_start, out_len, T)
    shape = (-1,) + (1,) * (v.ndim - 1)
    with np.errstate(invalid="ignore"):
        if in_len:
            v[:in_len] = v[:in_len] * sq(np.arange(in_len, dtype=np.uint64), in_len, False).reshape(shape)
        if out_start != NONE:
            if out_len:
                g = sq(np.arange(out_len, dtype=np.uint64), out_len, True).reshape(shape)
                v[out_start:out_start + out_len] = v[out_start:out_start + out_len] * g
            v[out_start + out_len:] = F(0)  # assigned: +0.0 whatever was there
    return z
