"""The launchers of rocoder_amd/csrc/rc_frames.h, called directly through the test-hook entries rc_test_frames_*
(rc_frames_hooks.hip, librocoder_hip_hooks.so only): the ctypes prototypes, device buffers cut out of guarded torch
tensors, and the host-side size checks. A wrapper call with wrong sizes is an out-of-bounds access on the device, so
every call below asserts, on the host and before it launches, that every byte the launcher may read or write lies
inside the buffers it was given - the rules are those of rc_frames.h and of the caller in rc_engine.cpp (raw 16-byte
aligned, raw_dwords a multiple of 4 that covers every byte of the frames asked for).

Also here, because tests/test_frames_kernels_host.py (CPU) and tests/test_gpu_frames_kernels.py share them: the reader's
decode formula in numpy, and the thinned case lists of the byte-layout sweep."""
import ctypes as C

import numpy as np

from rocoder_amd import _lib

FORMATS = ["u8", "i16", "i24", "i32", "f32"]
BYTES = {"u8": 1, "i16": 2, "i24": 3, "i32": 4, "f32": 4}
DECODE_K = {"u8": 127, "i16": 32767, "i24": 8388608, "i32": 2147483647}  # the header's K: the reader's divisors
GUARD = 0xA5
DEVICE = "cuda"

_u32, _u64, _p = C.c_uint32, C.c_uint64, C.c_void_p
PROTOTYPES = {
    "rc_test_frames_unpack": [_u32, _p, _u64, _u32, _u32, _u64, _u64, _p, _u64],
    "rc_test_frames_unpack_map": [_u32, _p, _u64, _u32, _u32, _u64, _u64, _p, _u64, _p],
    "rc_test_frames_pack": [_p, _u64, _p, _u64, _u32],
    "rc_test_frames_pack_pcm": [_u32, _p, _u64, _p, _u32, _u32, _u64, _p],
    "rc_test_frames_pack_pcm_gain": [_u32, _p, _u64, _p, _u32, _u32, _u64, _p, _p, C.c_float, _u32],
    "rc_test_frames_peak": [_p, _u64, _u64, _u32, _p],
    "rc_test_frames_fade": [_p, _u64, _u32, _u64, _u64, _u64, _u64, _u64],
}
_handle = None


def hooks():
    """the test-hook library with the prototypes of the seven entries set"""
    global _handle
    if _handle is None:
        with _lib.hooks_library() as H:
            for name, args in PROTOTYPES.items():
                fn = getattr(H, name)
                fn.restype = C.c_int
                fn.argtypes = args
            _handle = H
    return _handle


# ---------------------------------------------------------------------------------------------- numpy side of the formats
def decode_ints(n, fmt):
    """the reader's float of the integer sample n: (float)n / K, one f32 division"""
    return (np.asarray(n).astype(np.float32) / np.float32(DECODE_K[fmt])).astype(np.float32)


def int_bytes(n, fmt):
    """integer samples -> the little-endian bytes of the block (u8: n + 128)"""
    n = np.asarray(n, np.int64).reshape(-1)
    if fmt == "u8":
        return (n + 128).astype(np.uint8)
    if fmt == "i16":
        return n.astype("<i2").view(np.uint8)
    if fmt == "i32":
        return n.astype("<i4").view(np.uint8)
    assert fmt == "i24"
    return np.ascontiguousarray((n & 0xFFFFFF).astype("<u4").view(np.uint8).reshape(-1, 4)[:, :3]).reshape(-1)


def bytes_ints(b, fmt):
    """the bytes of a block of an integer format -> its samples as int64"""
    b = np.asarray(b, np.uint8).reshape(-1)
    if fmt == "u8":
        return b.astype(np.int64) - 128
    if fmt == "i16":
        return b.view("<i2").astype(np.int64)
    if fmt == "i32":
        return b.view("<i4").astype(np.int64)
    assert fmt == "i24"
    t = b.reshape(-1, 3).astype(np.int64)
    v = t[:, 0] | (t[:, 1] << 8) | (t[:, 2] << 16)
    return v - ((v & 0x800000) << 1)


def decode_bytes(b, fmt):
    """the bytes of a block -> the reader's floats (f32: the bits as they are)"""
    if fmt == "f32":
        return np.asarray(b, np.uint8).reshape(-1).view("<f4")
    return decode_ints(bytes_ints(b, fmt), fmt)


def bits(x):
    """the bits of float32 values, as uint32 of the same shape (a scalar: 0-d)"""
    a = np.asarray(x, np.float32)
    return (np.ascontiguousarray(a) if a.ndim else a).view(np.uint32)


def same_floats(got, want, nan_payloads=True):
    """bit for bit; with nan_payloads False a NaN of `want` asks for a NaN, of any payload (where an IEEE operation made
    it: the standard leaves its payload open)"""
    g, w = bits(got).reshape(-1), bits(want).reshape(-1)
    if g.shape != w.shape:
        return False
    if nan_payloads:
        return bool((g == w).all())
    wn = (w & 0x7FFFFFFF) > 0x7F800000
    gn = (g & 0x7FFFFFFF) > 0x7F800000
    return bool((wn == gn).all() and (g[~wn] == w[~wn]).all())


# ------------------------------------------------------------------------------------------------------- device buffers
class DevBuf:
    """A block of device memory (a torch uint8 tensor, its base 16-byte aligned) uploaded from host bytes. Byte phases,
    float offsets and guard regions are cut out of it with byte offsets; read() brings the whole block back."""

    def __init__(self, host):
        import torch

        host = np.ascontiguousarray(host).reshape(-1).view(np.uint8)
        self.nbytes = int(host.size)
        self.t = torch.from_numpy(host.copy()).to(DEVICE)
        assert self.t.data_ptr() % 16 == 0
        self.base = self.t.data_ptr()

    @classmethod
    def wrap(cls, t):
        """an existing contiguous uint8 tensor on the device, as it is (the jobs too large to build on the host)"""
        import torch

        assert t.dtype == torch.uint8 and t.is_contiguous() and t.dim() == 1 and t.data_ptr() % 16 == 0
        self = cls.__new__(cls)
        self.nbytes, self.t, self.base = int(t.numel()), t, t.data_ptr()
        return self

    def ptr(self, off=0):
        assert 0 <= off <= self.nbytes
        return self.base + off

    def read(self):
        return self.t.cpu().numpy()


def guarded(nbytes):
    """host bytes, every one the guard byte"""
    return np.full(int(nbytes), GUARD, np.uint8)


def planar_host(x, stride, base, tail=8):
    """Rows x[C, n] (float32, taken by their bits) at floats base + c * stride of a guard-filled block: (host bytes, the
    byte offsets of the floats that belong to a row)"""
    x = np.ascontiguousarray(x, np.float32)
    ch, n = x.shape
    assert stride >= n and 0 <= base
    total = base + (ch - 1) * stride + n + tail
    h = guarded(4 * total).view(np.uint32)
    idx = (base + np.arange(ch)[:, None] * stride + np.arange(n)[None, :]).reshape(-1)
    h[idx] = x.view(np.uint32).reshape(-1)
    return h.view(np.uint8), idx


def rows_of(planar_bytes, ch, n, stride, base):
    """the rows [C, n] of a block laid out by planar_host, and a mask of the floats outside them"""
    f = np.asarray(planar_bytes).view(np.uint32)
    idx = (base + np.arange(ch)[:, None] * stride + np.arange(n)[None, :]).reshape(-1)
    outside = np.ones(f.size, bool)
    outside[idx] = False
    return f[idx].view(np.float32).reshape(ch, n), f[outside]


GUARD_WORD = 0xA5A5A5A5


# ------------------------------------------------------------------------------------------------------------- the calls
def _fmt_id(fmt):
    return _lib.PCM_FORMATS[fmt]


def _done(name, rc):
    """Every call of these tests is a valid one, so a launcher that reports an error has met a device error. Nothing
    more is launched on a device in that state: the session ends there."""
    if rc != 0:
        import pytest

        pytest.exit(f"{name}: hipError_t {rc}; no further launches on this device", returncode=3)
    return rc


def _check_planar(buf, off_floats, stride, channels, n):
    assert channels >= 1 and n >= 1 and off_floats >= 0
    assert 4 * (off_floats + (channels - 1) * stride + n) <= buf.nbytes, "planar rows end behind the buffer"


def unpack(fmt, raw, phase, channels, frame0, n_frames, planar, planar_off, stride, chan_map=None):
    """launch_frames_unpack / launch_frames_unpack_map (chan_map: a DevBuf of `channels` uint32). raw: the whole DevBuf
    is the block; planar_off: the float of `planar` that is row 0, frame 0."""
    assert 0 <= phase <= 3 and raw.base % 16 == 0 and raw.nbytes % 16 == 0
    assert phase + (frame0 + n_frames) * channels * BYTES[fmt] <= raw.nbytes, "the frames end behind raw"
    _check_planar(planar, planar_off, stride, channels, frame0 + n_frames)
    args = [_fmt_id(fmt), raw.ptr(), raw.nbytes // 4, phase, channels, frame0, n_frames, planar.ptr(4 * planar_off), stride]
    if chan_map is None:
        return _done("rc_test_frames_unpack", hooks().rc_test_frames_unpack(*args))
    assert chan_map.nbytes == 4 * channels
    return _done("rc_test_frames_unpack_map", hooks().rc_test_frames_unpack_map(*args, chan_map.ptr()))


def pack(planar, planar_off, stride, frames, frames_off, n_frames, channels):
    """launch_frames_pack: frames_off is the float of `frames` the block starts at"""
    _check_planar(planar, planar_off, stride, channels, n_frames)
    assert 4 * (frames_off + n_frames * channels) <= frames.nbytes, "the frames end behind the buffer"
    return _done("rc_test_frames_pack", hooks().rc_test_frames_pack(planar.ptr(4 * planar_off), stride, frames.ptr(4 * frames_off), n_frames, channels))


def pack_pcm(fmt, planar, planar_off, stride, target, target_off, phase, channels, n_frames, clipped, norm=None,
             target_peak=1.0, store_gain=1):
    """launch_frames_pack_pcm, or launch_frames_pack_pcm_gain where `norm` (a DevBuf of the two words) is given. The block
    starts at byte target_off + phase of `target`; clipped: a DevBuf of one uint64."""
    assert 0 <= phase <= 3 and target_off % 4 == 0 and target.base % 4 == 0 and clipped.nbytes == 8
    assert target_off + phase + n_frames * channels * BYTES[fmt] <= target.nbytes, "the block ends behind the target"
    _check_planar(planar, planar_off, stride, channels, n_frames)
    args = [_fmt_id(fmt), planar.ptr(4 * planar_off), stride, target.ptr(target_off), phase, channels, n_frames, clipped.ptr()]
    if norm is None:
        return _done("rc_test_frames_pack_pcm", hooks().rc_test_frames_pack_pcm(*args))
    assert norm.nbytes == 8
    return _done("rc_test_frames_pack_pcm_gain", hooks().rc_test_frames_pack_pcm_gain(*args, norm.ptr(), target_peak, store_gain))


def peak(planar, planar_off, stride, n_frames, channels, norm):
    assert norm.nbytes == 8
    _check_planar(planar, planar_off, stride, channels, n_frames)
    return _done("rc_test_frames_peak", hooks().rc_test_frames_peak(planar.ptr(4 * planar_off), stride, n_frames, channels, norm.ptr()))


def fade(planar, planar_off, stride, channels, in_len, out_start, out_len, t0, t1):
    """launch_frames_fade: planar_off is the float of channel 0 at frame t0"""
    assert t1 > t0 and (out_start == 2 ** 64 - 1 or out_start + out_len < 2 ** 64)
    _check_planar(planar, planar_off, stride, channels, t1 - t0)
    return _done("rc_test_frames_fade", hooks().rc_test_frames_fade(planar.ptr(4 * planar_off), stride, channels, in_len, out_start, out_len, t0, t1))


def norm_words(peak_bits, gain):
    """the two words of FramesNormWords as host bytes"""
    return np.array([int(peak_bits), int(bits(np.float32(gain))[()])], np.uint32).view(np.uint8)


# ---------------------------------------------------------------------------------------------------- the layout sweep
CHANNELS = [1, 2, 3, 5, 7, 8, 9, 10, 63, 64, 65, 67, 128, 129, 130]
FRAMES = {"narrow": [1, 2, 3, 4, 5, 7, 1023, 1024, 1025, 2047, 2049, 3073], "wide": [1, 2, 3, 4, 5, 7, 63, 64, 65, 127, 129, 193]}
FRAME0 = {"narrow": [0, 1, 1023, 1024, 1029], "wide": [0, 1, 63, 64, 67]}
AXES = ("channels", "n_frames", "phase", "frame0", "pad", "base", "tbase")


def layout_cases(width):
    """The sweep of one width ('narrow': up to 8 channels, 'wide': above), thinned: channels x n_frames x phase crossed
    in full; the other axes - frame0 (unpack), the row stride's padding (stride = row length + pad), the row base
    (floats off a 16-byte boundary) and the target's dword within its 16-byte group - take, case by case, the value that
    pairs with the most values of the case's other axes for the first time. tests/test_frames_kernels_host.py asserts
    that every pair of values of any two axes occurs."""
    drawn = {"frame0": FRAME0[width], "pad": [0, 1, 3], "base": [0, 1, 2, 3], "tbase": [0, 1, 2, 3]}
    seen = set()
    out = []
    for ch in (c for c in CHANNELS if (c <= 8) == (width == "narrow")):
        for n in FRAMES[width]:
            for phase in range(4):
                case = dict(channels=ch, n_frames=n, phase=phase)
                for axis, values in drawn.items():
                    new = [sum((a, case[a], axis, v) not in seen for a in case) for v in values]
                    case[axis] = values[max(range(len(values)), key=lambda i: (new[i], -((i - len(out)) % len(values))))]
                    seen.update((a, case[a], axis, case[axis]) for a in case if a != axis)
                out.append(case)
    return out
