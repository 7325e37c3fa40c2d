"""The dither of rc_engine_set_output_dither (include/rocoder_hip.h) in numpy - the yardstick of tests/test_frames_dither_host.py,
tests/test_gpu_frames_dither_kernels.py and tests/test_gpu_frames_dither.py - and the test-hook entry of the dithered pack
launchers (rc_test_frames_pack_pcm_dither, rc_frames_hooks.hip): its ctypes prototype and the host-side size checks, in the
manner of tests/frameskernelutil.py, whose device buffers and byte helpers are used here.

The definition, for output frame t (absolute) and job channel c:
  K(c) = phase_key(seed, c, 2^40 - 1);  h(c, t) = phase_hash(K(c), t mod 2^32)
  tpdf     i = (h >> 16) - (h & 0xFFFF)
  tpdf-hp  i = (h(c, t) >> 16) - (h(c, t - 1 mod 2^32) >> 16)
  d = i * 2^-16 (exact in f32);  t1 = x * S, t2 = t1 + d, one f32 operation each;  rint, NaN -> 0, clamp
phase_key and phase_hash are oracle/oracle_np.py's, which tests/test_cabi_host.py ties to the library's."""
import ctypes as C

import numpy as np

from frameskernelutil import BYTES, DevBuf, _check_planar, _done, _fmt_id, bytes_ints, guarded, int_bytes, planar_host  # noqa: F401
from oracle import oracle_np as onp
from rocoder_amd import _lib
from test_frames_pcm_host import PCM

MODES = {"none": 0, "tpdf": 1, "tpdf-hp": 2}
DITHER_FORMATS = ["u8", "i16", "i24"]
DITHER_HOP = (1 << 40) - 1  # the hop index of the dither's keys: one that no job reaches


def key(seed, channel):
    return onp.phase_key(seed, channel, DITHER_HOP)


def draws_i(mode, seed, channel, t):
    """the integers i of the frames t (any non-negative integers, taken mod 2^32) of one channel, as int64"""
    assert mode in ("tpdf", "tpdf-hp")
    t32 = (np.asarray(t, np.uint64) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    k = key(seed, channel)
    h = onp.phase_hash(k, t32).astype(np.int64)
    if mode == "tpdf":
        return (h >> 16) - (h & 0xFFFF)
    with np.errstate(over="ignore"):
        before = onp.phase_hash(k, t32 - np.uint32(1)).astype(np.int64)
    return (h >> 16) - (before >> 16)


def dither(mode, seed, channel, t):
    """d of the frames t of one channel: float32, exact"""
    d = (draws_i(mode, seed, channel, t).astype(np.float32) * np.float32(2.0 ** -16)).astype(np.float32)
    assert (np.abs(d) < 1).all()
    return d


def quantise_dithered(x, fmt, mode, seed, t0=0, channel0=0):
    """frames x[n, C] (frame-major, float32) -> int64 codes [n, C]: row f is absolute frame t0 + f, column c job channel
    channel0 + c. mode "none": the undithered quantiser."""
    x = np.asarray(x, np.float32)
    assert x.ndim == 2 and fmt in DITHER_FORMATS
    s, lo, hi, _ = PCM[fmt]
    n, ch = x.shape
    t = np.uint64(t0 % 2 ** 64) + np.arange(n, dtype=np.uint64)
    with np.errstate(invalid="ignore", over="ignore"):
        t1 = (x * np.float32(s)).astype(np.float32)
        if mode != "none":
            d = np.stack([dither(mode, seed, channel0 + c, t) for c in range(ch)], axis=1) if n else np.zeros((0, ch), np.float32)
            t1 = (t1 + d).astype(np.float32)
        r = np.where(np.isnan(t1), 0, np.rint(t1))
    return np.clip(r.astype(np.float64), lo, hi).astype(np.int64)


def dithered_bytes(x, fmt, mode, seed, t0=0, channel0=0):
    """frames x[n, C] -> the bytes of the frame-major block, as a uint8 array"""
    return np.asarray(int_bytes(quantise_dithered(x, fmt, mode, seed, t0, channel0), fmt), np.uint8).reshape(-1)


def keys_host(seed, n_channels):
    """the job's key table: K(c), c < n_channels, as host bytes"""
    return np.array([key(seed, c) for c in range(n_channels)], np.uint64).view(np.uint8)


# ------------------------------------------------------------------------------------------------------------- the hook
_u32, _u64, _p = C.c_uint32, C.c_uint64, C.c_void_p
PROTOTYPE = [_u32, _p, _u64, _p, _u32, _u32, _u64, _p, _p, C.c_float, _u32, _u32, _u64, _u32, _p]
_handle = None


def hooks():
    global _handle
    if _handle is None:
        with _lib.hooks_library() as H:
            fn = H.rc_test_frames_pack_pcm_dither
            fn.restype = C.c_int
            fn.argtypes = PROTOTYPE
            _handle = H
    return _handle


def pack_pcm_dither(fmt, planar, planar_off, stride, target, target_off, phase, channels, n_frames, clipped, mode, t0, channel0,
                    keys, norm=None, target_peak=1.0, store_gain=1):
    """launch_frames_pack_pcm_dither, or launch_frames_pack_pcm_gain_dither where `norm` (a DevBuf of the two words) is
    given. The block starts at byte target_off + phase of `target`; clipped: a DevBuf of one uint64; keys: a DevBuf of
    the job's table, which holds at least the entries [channel0, channel0 + channels)."""
    assert fmt in DITHER_FORMATS and mode in (1, 2) and 0 <= t0 < 2 ** 64
    assert 0 <= phase <= 3 and target_off % 4 == 0 and target.base % 4 == 0 and clipped.nbytes == 8
    assert target_off + phase + n_frames * channels * BYTES[fmt] <= target.nbytes, "the block ends behind the target"
    assert keys.base % 8 == 0 and 8 * (channel0 + channels) <= keys.nbytes, "the key table ends in front of the launch's channels"
    _check_planar(planar, planar_off, stride, channels, n_frames)
    if norm is not None:
        assert norm.nbytes == 8
    rc = hooks().rc_test_frames_pack_pcm_dither(_fmt_id(fmt), planar.ptr(4 * planar_off), stride, target.ptr(target_off), phase,
                                                channels, n_frames, clipped.ptr(), norm.ptr() if norm is not None else None,
                                                target_peak, store_gain, mode, t0, channel0, keys.ptr())
    return _done("rc_test_frames_pack_pcm_dither", rc)
