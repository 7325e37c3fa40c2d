"""Host-side mirror of the reference's interface for the hot path, above the C-ABI.

Names, argument meaning and error behaviour follow the reference (file:line = rocoder v0.4.0):
  * `Stretcher`          — src/stretcher.rs:12-136 (`new`, `next_window`, `is_done`, `channel_bound`)
  * `ReFFT`              — src/fft.rs:15-109 (`forward_fft`, `resynth`)
  * `StretcherProcessor` — src/stretcher_processor.rs:21-89 (one thread, round-robin channels,
                           bounded queues, Shutdown control message)
  * `AudioSpec`/`AudioBus` — src/audio.rs:31-37,141-224
All numerics run in the HIP engine (librocoder_hip.so); nothing here computes audio on the CPU.
"""
from __future__ import annotations

import ctypes as C
import functools
import queue
import threading
from dataclasses import dataclass
from typing import Callable, List, Optional, Sequence

import numpy as np

from . import _lib
from ._lib import RC_EINVAL, RC_WOULD_BLOCK, RocoderError, check, rc_config, rc_params


@dataclass(frozen=True)
class AudioSpec:  # src/audio.rs:31-37
    channels: int = 2
    sample_rate: int = 44100


def _fp(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _wrap_kernel(pyfunc):
    """Python callable (time_ms, complex64[N]) -> complex64[N] as the C-ABI rc_freq_kernel.
    Raising (or returning the wrong length) is the equivalent of a panic (src/fft.rs:100-106)."""
    if pyfunc is None:
        return C.cast(None, _lib.FREQ_KERNEL)
    if isinstance(pyfunc, _lib.FREQ_KERNEL):
        return pyfunc

    def tramp(time_ms, pin, pout, n, _user):
        try:
            a = np.ctypeslib.as_array(pin, shape=(2 * n,)).view(np.complex64)
            r = np.asarray(pyfunc(int(time_ms), a.copy()), dtype=np.complex64)
            if r.size != n:
                return 2
            np.ctypeslib.as_array(pout, shape=(2 * n,))[:] = r.view(np.float32)
            return 0
        except Exception:  # noqa: BLE001 - a panicking kernel must not poison the batch
            return 1

    return _lib.FREQ_KERNEL(tramp)


def load_kernel_library(path: str):
    """dlopen a shared object exporting the C symbol `apply` with the rc_freq_kernel signature
    (the C-ABI form of README.md:106-112; src/fft.rs:93-94 resolves the same name)."""
    so = C.CDLL(path)
    fn = so.apply
    fn.restype = C.c_int
    fn.argtypes = [C.c_uint64, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_size_t, C.c_void_p]
    k = C.cast(fn, _lib.FREQ_KERNEL)
    k._keepalive = so  # keep the library loaded, like the kernel stack at src/fft.rs:21
    return k


class DeviceKernelCompileError(RocoderError):
    """A user device kernel that does not compile: `log` holds the compiler's output."""

    def __init__(self, code: int, msg: str, log: str):
        super().__init__(code, msg + ("\n" + log if log else ""))
        self.log = log


def compile_device_kernel(src, name: Optional[str] = None) -> bytes:
    """HIP source defining `__device__ float2 rc_apply(const rc_spectrum &X, uint32_t j, const rc_hop &h)` -> gfx950
    code object (rc_dk_compile; pure host, no device). `name` is the file name diagnostics give (default
    rc_user_dk.hip). Raises DeviceKernelCompileError carrying the compiler log."""
    L = _lib.lib()
    text = src.encode() if isinstance(src, str) else bytes(src)
    if name is not None:
        text = f'#line 1 "{name}"\n'.encode() + text
    n = C.c_size_t(0)
    log = C.create_string_buffer(1 << 16)
    rc = L.rc_dk_compile(text, len(text), None, 0, C.byref(n), log, len(log))
    if rc == _lib.RC_ECAPACITY:
        code = C.create_string_buffer(n.value)
        rc = L.rc_dk_compile(text, len(text), code, n.value, C.byref(n), log, len(log))
        if rc == _lib.RC_OK:
            return code.raw[:n.value]
    raise DeviceKernelCompileError(rc, L.rc_last_error().decode(errors="replace"),
                                   log.value.decode(errors="replace"))


def _code_object_symbols(code: bytes):
    """(name, size) of every symbol of an ELF64 little-endian code object."""
    import struct

    b = bytes(code)
    if len(b) < 64 or b[:4] != b"\x7fELF" or b[4] != 2 or b[5] != 1:
        raise ValueError("not an ELF64 little-endian code object")
    shoff, = struct.unpack_from("<Q", b, 40)
    shentsize, shnum = struct.unpack_from("<HH", b, 58)
    if shentsize != 64 or shoff + shnum * 64 > len(b):
        raise ValueError("bad ELF section header table")
    secs = [struct.unpack_from("<IIQQQQIIQQ", b, shoff + i * 64) for i in range(shnum)]
    for _name, typ, _flags, _addr, off, size, link, _info, _align, ent in secs:
        if typ not in (2, 11) or ent != 24 or link >= shnum or off + size > len(b):  # SHT_SYMTAB, SHT_DYNSYM
            continue
        stroff, strsize = secs[link][4], secs[link][5]
        strtab = b[stroff:stroff + strsize]
        for s in range(off, off + size - 23, 24):
            st_name, _i, _o, _shndx, _value, st_size = struct.unpack_from("<IBBHQQ", b, s)
            end = strtab.find(b"\0", st_name)
            yield strtab[st_name:end if end >= 0 else None], int(st_size)


def device_kernel_cross_channel(code: bytes) -> bool:
    """Whether a code object from compile_device_kernel declares `#define RC_CROSS_CHANNEL 1` (rc_apply reads the other
    channels' spectra through X.channel(c)). Pure Python: the declaration is the ELF symbol rc_user_dk_channels."""
    return any(name == b"rc_user_dk_channels" for name, _size in _code_object_symbols(code))


def device_kernel_sums(code: bytes) -> int:
    """The number of whole-hop sums a code object from compile_device_kernel declares (`#define RC_SUMS S` in its source:
    rc_apply reads X.sum(0..S-1), the sums of rc_sum_term over a hop's bins), 0 for a source without them. Pure Python:
    S is the size of the ELF symbol rc_user_dk_sums less one, and a code object without that symbol has none."""
    for name, size in _code_object_symbols(code):
        if name == b"rc_user_dk_sums":
            return max(0, size - 1)
    return 0


def device_kernel_feedback(code: bytes) -> int:
    """The feedback depth a code object from compile_device_kernel declares (`#define RC_FEEDBACK F` in its source:
    rc_apply reads X.out(1..F), what it returned for the F hops before), 0 for a source without it. Pure Python: F is the
    size of the ELF symbol rc_user_dk_feedback less one, and a code object without that symbol has none."""
    for name, size in _code_object_symbols(code):
        if name == b"rc_user_dk_feedback":
            return max(0, size - 1)
    return 0


def device_kernel_history(code: bytes) -> int:
    """The history depth a code object from compile_device_kernel declares (`#define RC_HISTORY D` in its source: the
    earlier hops X.past(1..D) that rc_apply reads), 0 for a source without one. Pure Python: the depth is the size of
    the ELF symbol rc_user_dk_history less one, and a code object without that symbol has depth 0."""
    import struct

    b = bytes(code)
    if len(b) < 64 or b[:4] != b"\x7fELF" or b[4] != 2 or b[5] != 1:
        raise ValueError("not an ELF64 little-endian code object")
    shoff, = struct.unpack_from("<Q", b, 40)
    shentsize, shnum = struct.unpack_from("<HH", b, 58)
    if shentsize != 64 or shoff + shnum * 64 > len(b):
        raise ValueError("bad ELF section header table")
    secs = [struct.unpack_from("<IIQQQQIIQQ", b, shoff + i * 64) for i in range(shnum)]
    for _name, typ, _flags, _addr, off, size, link, _info, _align, ent in secs:
        if typ not in (2, 11) or ent != 24 or link >= shnum or off + size > len(b):  # SHT_SYMTAB, SHT_DYNSYM
            continue
        stroff, strsize = secs[link][4], secs[link][5]
        strtab = b[stroff:stroff + strsize]
        for s in range(off, off + size - 23, 24):
            st_name, _i, _o, _shndx, _value, st_size = struct.unpack_from("<IBBHQQ", b, s)
            if strtab[st_name:st_name + 19] == b"rc_user_dk_history\0":
                return max(0, int(st_size) - 1)
    return 0


def _params_array(params):
    vals = [float(v) for v in params]
    return (C.c_float * max(1, len(vals)))(*vals), len(vals)


def make_config(window_len=16384, factor=1.0, amplitude=1.0, pitch_multiple=1, sample_rate=44100,
                channels=1, buffer_secs=1.0, seed=0, device=0, window=None, kernel=None,
                kernel_time_ms=0, max_batch_hops=0, kernel_threads=0, device_kernel=None):
    """device_kernel: None, ("gain", g), ("band", lo_bin, hi_bin, gain_inside, gain_outside) or
    ("shift", bins) - the curated on-GPU frequency kernels of include/rocoder_hip.h (RC_DK_*)."""
    cfg = rc_config()
    cfg.struct_size = C.sizeof(rc_config)
    cfg.window_len = int(window_len)
    cfg.factor = float(factor)
    cfg.amplitude = float(amplitude)
    cfg.pitch_multiple = int(pitch_multiple)
    cfg.sample_rate = int(sample_rate)
    cfg.channels = int(channels)
    cfg.buffer_secs = float(buffer_secs)
    cfg.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    cfg.device = int(device)
    cfg.max_batch_hops = int(max_batch_hops)
    keep = []
    if window is not None:
        w = np.ascontiguousarray(window, dtype=np.float32)
        if w.size != window_len:
            raise ValueError("window length mismatch")
        cfg.window = _fp(w)
        keep.append(w)
    k = _wrap_kernel(kernel)
    cfg.kernel = k
    keep.append(k)
    cfg.kernel_time_ms = int(kernel_time_ms)
    cfg.kernel_threads = int(kernel_threads)
    if device_kernel is not None:
        kind = device_kernel[0]
        if kind == "gain":
            cfg.device_kernel, cfg.dk_gain = _lib.RC_DK_GAIN, float(device_kernel[1])
        elif kind == "band":
            cfg.device_kernel = _lib.RC_DK_BAND
            cfg.dk_lo_bin, cfg.dk_hi_bin = int(device_kernel[1]), int(device_kernel[2])
            cfg.dk_gain, cfg.dk_gain_outside = float(device_kernel[3]), float(device_kernel[4])
        elif kind == "shift":
            cfg.device_kernel, cfg.dk_shift_bins = _lib.RC_DK_SHIFT, int(device_kernel[1])
        else:
            raise ValueError(f"unknown device kernel {kind!r}")
    return cfg, keep


def derive_params(**kw) -> rc_params:
    """Stretcher::new parameter derivation (src/stretcher.rs:40-56) — host only, no device."""
    cfg, _keep = make_config(**kw)
    out = rc_params()
    check(_lib.lib().rc_derive_params(C.byref(cfg), C.byref(out)))
    return out


def offline_output_len(in_len: int, **kw) -> int:
    cfg, _keep = make_config(**kw)
    return int(_lib.lib().rc_offline_output_len(C.byref(cfg), in_len))


def time_map_output_len(n_hops: int, **kw) -> int:
    """The output frames of a time map of `n_hops` hops under the configuration `kw` (rc_time_map_output_len): n_hops /
    hops_per_window * window_out_len, 0 where n_hops is no multiple of hops_per_window. Pure host code."""
    if not 0 <= int(n_hops) < 2 ** 64:
        raise ValueError("n_hops is an unsigned integer")
    cfg, _keep = make_config(**kw)
    return int(_lib.lib().rc_time_map_output_len(C.byref(cfg), int(n_hops)))


def time_map_curve(in_len: int, at, factors, **kw) -> np.ndarray:
    """The time map (int64 [K], what `Engine.set_time_map` takes) of a stretch factor that varies along an input of
    `in_len` samples (rc_time_map_curve; the definition is in include/rocoder_hip.h): the factor is `factors[i]` at input
    sample `at[i]`, linear in between and constant outside the points; hop k + 1 lies N / (2 psf(f(q_k))) samples behind
    hop k, in doubles, and the map ends with the window in which the input runs out. Pure host code. Points out of order,
    a factor outside [2^-10, 2^20] or a curve of 2^28 hops or more raise (RC_EINVAL)."""
    a = np.ascontiguousarray(at, np.float64).reshape(-1)
    f = np.ascontiguousarray(factors, np.float64).reshape(-1)
    if a.size != f.size or a.size == 0:
        raise ValueError("at and factors hold the same number of points, at least one")
    if not 0 <= int(in_len) < 2 ** 64:
        raise ValueError("in_len is an unsigned integer")
    cfg, _keep = make_config(**kw)
    L = _lib.lib()
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int64)
    n = C.c_size_t(0)
    rc = L.rc_time_map_curve(C.byref(cfg), int(in_len), a.ctypes.data_as(dp), f.ctypes.data_as(dp), a.size, None, 0, C.byref(n))
    if rc != _lib.RC_ECAPACITY:
        check(rc, L)
    out = np.empty(n.value, np.int64)
    check(L.rc_time_map_curve(C.byref(cfg), int(in_len), a.ctypes.data_as(dp), f.ctypes.data_as(dp), a.size, out.ctypes.data_as(ip),
                              out.size, C.byref(n)), L)
    return out


def resample_len(n: int, num: int, den: int) -> int:
    """The frames a resample of `n` frames by the step num / den gives (rc_resample_len): the m with m * num / den < n."""
    if not (0 <= int(n) < 2 ** 64 and 0 <= int(num) < 2 ** 32 and 0 <= int(den) < 2 ** 32):
        raise ValueError("n, num and den are unsigned integers")
    return int(_lib.lib().rc_resample_len(int(n), int(num), int(den)))


def resample_table(num: int, den: int) -> np.ndarray:
    """The filter table the engine uploads for the step num / den (rc_resample_table; the definition is in
    include/rocoder_hip.h): float32 [reduced den, T], row p the T = 2 W coefficients of phase p. Pure host code. A step
    `Engine.set_output_resample` refuses raises (RC_EINVAL)."""
    if not (0 <= int(num) < 2 ** 32 and 0 <= int(den) < 2 ** 32):
        raise ValueError("num and den are unsigned 32-bit integers")
    L = _lib.lib()
    phases, taps = C.c_uint32(0), C.c_uint32(0)
    check(L.rc_resample_table(int(num), int(den), None, 0, C.byref(phases), C.byref(taps)), L)
    out = np.empty((phases.value, taps.value), np.float32)
    check(L.rc_resample_table(int(num), int(den), _fp(out), out.size, C.byref(phases), C.byref(taps)), L)
    return out


def resample_ratio(step: float):
    """(num, den): the best rational of float32(`step`) with den <= 1024 (rc_resample_ratio, continued fractions) - what
    `Engine.set_output_resample` takes for a pitch ratio r and a change of rate, step = r * rate_in / rate_out. A step
    outside [1/8, 8] or not finite raises (RC_EINVAL)."""
    L = _lib.lib()
    num, den = C.c_uint32(0), C.c_uint32(0)
    check(L.rc_resample_ratio(float(step), C.byref(num), C.byref(den)), L)
    return int(num.value), int(den.value)


def warp_table(tier: int) -> np.ndarray:
    """The filter table of tier `tier` (0 ... 12) of an output warp (rc_warp_table; the definition is in
    include/rocoder_hip_warp.h): float32 [257, T], row p the T = 2 W coefficients of phase p / 256. Pure host code."""
    if not 0 <= int(tier) < 2 ** 32:
        raise ValueError("tier is an unsigned 32-bit integer")
    L = _lib.lib()
    rows, taps = C.c_uint32(0), C.c_uint32(0)
    check(L.rc_warp_table(int(tier), None, 0, C.byref(rows), C.byref(taps)), L)
    out = np.empty((rows.value, taps.value), np.float32)
    check(L.rc_warp_table(int(tier), _fp(out), out.size, C.byref(rows), C.byref(taps)), L)
    return out


def warp_curve(n: int, at, ratios, hop_pos=None, n_hops: Optional[int] = None, **kw):
    """(anchors int64 [A], n_out): what `Engine.set_output_warp` takes for a pitch ratio that varies along the input of a
    job whose rows have `n` frames (rc_warp_curve; the definition is in include/rocoder_hip_warp.h). The ratio is
    `ratios[i]` (in [1/8, 8]) at input sample `at[i]`, linear in between and constant outside the points. `hop_pos` is
    the job's time map, or None with `n_hops` for the engine's own grid k * sample_step_len. Pure host code."""
    a = np.ascontiguousarray(at, np.float64).reshape(-1)
    r = np.ascontiguousarray(ratios, np.float64).reshape(-1)
    if a.size != r.size or a.size == 0:
        raise ValueError("at and ratios hold the same number of points, at least one")
    if not 0 <= int(n) < 2 ** 64:
        raise ValueError("n is an unsigned integer")
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int64)
    pos, pos_p = None, None
    if hop_pos is not None:
        pos = np.ascontiguousarray(hop_pos, np.int64).reshape(-1)
        pos_p, n_hops = pos.ctypes.data_as(ip), pos.size
    if n_hops is None or not 0 <= int(n_hops) < 2 ** 64:
        raise ValueError("give hop_pos, or n_hops for the engine's grid")
    cfg, _keep = make_config(**kw)
    L = _lib.lib()
    na, no = C.c_size_t(0), C.c_size_t(0)
    args = (C.byref(cfg), pos_p, int(n_hops), a.ctypes.data_as(dp), r.ctypes.data_as(dp), a.size, int(n))
    rc = L.rc_warp_curve(*args, None, 0, C.byref(na), C.byref(no))
    if rc != _lib.RC_ECAPACITY:
        check(rc, L)
    out = np.empty(na.value, np.int64)
    check(L.rc_warp_curve(*args, out.ctypes.data_as(ip), out.size, C.byref(na), C.byref(no)), L)
    return out, int(no.value)


def _mix_keys(keys):
    """keys: None or a sequence of (frame, amp) -> (uint64 frames, float32 amps)."""
    if keys is None or len(keys) == 0:
        return np.zeros(0, np.uint64), np.zeros(0, np.float32)
    for k in keys:
        if len(k) != 2 or not 0 <= int(k[0]) < 2 ** 64:
            raise ValueError("keys is a sequence of (frame, amp), frame an unsigned integer")
    kf = np.array([int(k[0]) for k in keys], np.uint64)
    with np.errstate(over="ignore"):
        ka = np.array([k[1] for k in keys], np.float32)
    return kf, ka


def mix_envelope(keys, t0: int, n: int) -> np.ndarray:
    """amp(t0 + i), i < n: the keyframed envelope of a mix layer (rc_mix_envelope; the definition - the reference's
    math::sqrt_interp between the keys, the first and the last amplitude outside them - is in include/rocoder_hip_mix.h).
    `keys` is a sequence of (frame, amp) with strictly increasing frames. Pure host code."""
    kf, ka = _mix_keys(keys)
    if not (0 <= int(t0) < 2 ** 64 and 0 <= int(n) < 2 ** 63):
        raise ValueError("t0 and n are unsigned integers")
    out = np.empty(int(n), np.float32)
    L = _lib.lib()
    check(L.rc_mix_envelope(kf.ctypes.data_as(C.POINTER(C.c_uint64)), _fp(ka), kf.size, int(t0), int(n), _fp(out)), L)
    return out


RC_PHASE_RANDOM, RC_PHASE_PROPAGATE, RC_PHASE_LOCKED = _lib.RC_PHASE_RANDOM, _lib.RC_PHASE_PROPAGATE, _lib.RC_PHASE_LOCKED


def phase_envelope(window) -> np.ndarray:
    """env[i] = 1 / (w[i]^2 + w[i + n/2]^2), i < n/2, in float32: the overlap-add envelope of the phase modes
    (rc_phase_envelope; include/rocoder_hip_phase.h). Raises for a window whose sum falls below 2^-10 of its maximum
    anywhere. Pure host code."""
    w = np.ascontiguousarray(window, np.float32)
    if w.ndim != 1:
        raise ValueError("window is one-dimensional")
    out = np.empty(w.size // 2, np.float32)
    L = _lib.lib()
    if L.rc_phase_envelope(_fp(w), w.size, _fp(out)) != _lib.RC_OK:
        raise RocoderError(_lib.RC_EINVAL, "phase_envelope: an even window of at least 2 finite samples whose w[i]^2 + w[i + n/2]^2 "
                                           "stays above 2^-10 of its maximum")
    return out


class Bus:
    """A device-resident mix bus (rc_bus): `channels` planar float32 rows of `n_frames` frames on `device`, all zero when
    created and after `clear()`. `Engine.mix_frames` accumulates layers into it, `Engine.bus_frames` reads it out through an
    engine's master stages."""

    def __init__(self, channels: int, n_frames: int, device: int = 0):
        if not (0 <= int(channels) < 2 ** 32 and 0 <= int(n_frames) < 2 ** 64):
            raise ValueError("channels and n_frames are unsigned integers")
        self._L = _lib.lib()
        h = C.c_void_p()
        check(self._L.rc_bus_create(int(device), int(channels), int(n_frames), C.byref(h)), self._L)
        self._h = h
        self.channels, self.n_frames, self.device = int(channels), int(n_frames), int(device)

    @property
    def layers(self) -> int:
        n = C.c_uint32(0)
        check(self._L.rc_bus_info(self._h, None, None, C.byref(n)), self._L)
        return int(n.value)

    def clear(self):
        check(self._L.rc_bus_clear(self._h), self._L)

    def device_rows(self):
        """(device address of row 0, row stride in floats): for device callers."""
        p, stride = C.POINTER(C.c_float)(), C.c_size_t(0)
        check(self._L.rc_bus_device_rows(self._h, C.byref(p), C.byref(stride)), self._L)
        return C.cast(p, C.c_void_p).value or 0, int(stride.value)

    def close(self):
        if getattr(self, "_h", None):
            self._L.rc_bus_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


def autocrop_points(bin_peak, bin_frames: int, n_frames: int, percentile: int = 30):
    """The reference's crop points (determine_noise_threshold + determine_autocrop_points, src/recorder.rs:165-191) from
    the peaks `Engine.frames_power` gives: (start, end) in frames - the job's frames [start, end) are what remains - or
    None where no bin lies above the threshold (the reference crops nothing then). The comparisons run on decibels, the
    threshold is the value at index floor(percentile / 100 * n_bins) of the sorted bins, and `end` is the first frame of
    the bin behind the last one above the threshold - of that bin itself where it is the job's last (the reference's
    quirk, kept). Pure host code (rc_autocrop_points): no device is touched."""
    peaks = np.ascontiguousarray(bin_peak, np.float32).reshape(-1)
    start, end, found = C.c_uint64(0), C.c_uint64(0), C.c_int(0)
    if not (0 <= int(percentile) < 2 ** 32 and 0 <= int(bin_frames) < 2 ** 64 and int(n_frames) >= 0):
        raise ValueError("percentile, bin_frames and n_frames are unsigned integers")
    L = _lib.lib()
    check(L.rc_autocrop_points(_fp(peaks), peaks.size, int(bin_frames), int(n_frames), int(percentile), C.byref(start),
                               C.byref(end), C.byref(found)), L)
    return (int(start.value), int(end.value)) if found.value else None


def split_mono_map(chan_peak):
    """The reference's auto_split_mono decision (src/recorder.rs:118-144) from the peaks `Engine.frames_channel_peaks`
    gives: (map, found). Where all channels but one are silent (peak == 0; a NaN peak is not silent), `map` sends every row
    to that channel and `found` is True - one live channel alone included, where the map is the identity; otherwise the
    identity map and False. `map` is what `Engine.set_channel_map` takes. Pure host code (rc_split_mono_map)."""
    peaks = np.ascontiguousarray(chan_peak, np.float32).reshape(-1)
    out = np.zeros(max(peaks.size, 1), np.uint32)
    found = C.c_int(0)
    L = _lib.lib()
    check(L.rc_split_mono_map(_fp(peaks), peaks.size, out.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(found)), L)
    return [int(v) for v in out[:peaks.size]], bool(found.value)


class _ViewOwner:
    """`base` of the arrays next_window_view hands out: keeps the engine alive and knows whether it is still current."""

    def __init__(self, engine, channel: int, ptr: int, nbytes: int):
        self.engine, self.channel, self.current = engine, channel, True
        self.__array_interface__ = {"shape": (nbytes,), "typestr": "|u1", "data": (ptr, True), "version": 3}


class _PinnedBlock:
    """Owner of one rc_host_alloc block; numpy arrays made over it keep it alive through their `base` chain."""

    def __init__(self, nbytes: int):
        self._L = _lib.lib()
        p = C.c_void_p()
        check(self._L.rc_host_alloc(nbytes, C.byref(p)), self._L)
        self.ptr, self.nbytes = p.value, nbytes
        self.__array_interface__ = {"shape": (max(nbytes, 1),), "typestr": "|u1", "data": (self.ptr, False), "version": 3}

    def __del__(self):
        p, self.ptr = getattr(self, "ptr", None), None
        if p:
            self._L.rc_host_free(C.c_void_p(p))


def pinned_empty(shape, dtype=np.float32) -> np.ndarray:
    """numpy array in page-locked host memory (rc_host_alloc): rows handed to `Engine.stretch_host` /
    `MultiEngine.stretch_host` from here cross PCIe by DMA without a staging copy. The block is freed when the last
    array (or view) over it is garbage-collected."""
    shape = tuple(int(v) for v in np.atleast_1d(shape))
    dt = np.dtype(dtype)
    n = int(np.prod(shape))
    blk = _PinnedBlock(n * dt.itemsize)
    return np.asarray(blk)[:n * dt.itemsize].view(dt).reshape(shape)


class Engine:
    """Thin RAII wrapper of rc_engine (all channels of one job)."""

    def __init__(self, **kw):
        self._L = _lib.lib()  # (the test-hook build inside `_lib.hooks_library()`)
        self._check = functools.partial(check, L=self._L)
        self._cfg, self._keep = make_config(**kw)
        h = C.c_void_p()
        self._check(self._L.rc_engine_create(C.byref(self._cfg), C.byref(h)))
        self._h = h
        self.params = rc_params()
        self._check(self._L.rc_engine_get_params(self._h, C.byref(self.params)))
        self.channels = int(self._cfg.channels)
        self.window_len = int(self._cfg.window_len)
        self._resample = None  # set_output_resample: (num, den) while a step is set
        self._limiter = False  # set_output_limiter: a limiter is set
        self._map_hops = None  # set_time_map: the hops of the map while one is set
        self._warp_out = None  # set_output_warp: n_out while a warp is set

    def close(self):
        for o in list((getattr(self, "_views", None) or {}).values()):
            o.current = False
        if getattr(self, "_h", None):
            self._L.rc_engine_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # ---- streaming seam
    def push_input(self, channel: int, samples):
        s = np.ascontiguousarray(samples, dtype=np.float32)
        self._check(self._L.rc_engine_push_input(self._h, channel, _fp(s), s.size))

    def close_input(self, channel: int):
        self._check(self._L.rc_engine_close_input(self._h, channel))

    def next_window(self, channel: int) -> Optional[np.ndarray]:
        """One Stretcher::next_window; None when the reference would block on recv()."""
        out = np.empty(self.params.window_out_len, np.float32)
        n = C.c_size_t(0)
        rc = self._check(self._L.rc_engine_next_window(self._h, channel, _fp(out), out.size, C.byref(n)))
        if rc == RC_WOULD_BLOCK:
            return None
        return out[: n.value]

    def next_window_view(self, channel: int) -> Optional[np.ndarray]:
        """The same hand-out without the copy (rc_engine_next_window_view): a read-only array over the engine's
        pinned block. None when the reference would block.

        LIFETIME: the array aliases memory the engine owns. It is valid only until the NEXT hand-out of this channel
        (next_window / next_window_view) or close(): after that the block may be refilled with other windows or freed,
        and reading a retained array is undefined (stale data or a fault) - numpy cannot be told. Consume it (write it
        to the sink, src/main.rs:197-203) or copy it before asking for the next window; use next_window() for an array
        you may keep. The array keeps the Engine object itself alive (its `base` chain refers to it), so garbage
        collection never closes an engine under a live view; `view_is_current(a)` tells whether `a` is still the
        latest hand-out of its channel."""
        p = C.POINTER(C.c_float)()
        n = C.c_size_t(0)
        rc = self._check(self._L.rc_engine_next_window_view(self._h, channel, C.byref(p), C.byref(n)))
        if rc == RC_WOULD_BLOCK:
            return None
        owner = _ViewOwner(self, channel, C.addressof(p.contents), n.value * 4)
        # weak: the owner refers to the engine (an array keeps its engine alive), the engine must not refer back -
        # a cycle through an object with __del__ would leave the engine, its HBM and its pinned blocks to a cyclic GC
        # pass instead of the refcount
        if getattr(self, "_views", None) is None:
            import weakref

            self._views = weakref.WeakValueDictionary()
        prev = self._views.get(channel)
        if prev is not None:
            prev.current = False
        self._views[channel] = owner
        a = np.asarray(owner).view(np.float32)
        a.flags.writeable = False
        return a

    def view_is_current(self, a: np.ndarray) -> bool:
        """True while `a` (from next_window_view) is the latest hand-out of its channel on an open engine."""
        o = a
        while o is not None and not isinstance(o, _ViewOwner):
            o = getattr(o, "base", None)
        return bool(o is not None and o.current and o.engine is self and self._h)

    def is_done(self, channel: int) -> bool:
        return bool(self._check(self._L.rc_engine_is_done(self._h, channel)))

    def channel_bound(self) -> int:
        return int(self._L.rc_engine_channel_bound(self._h))

    # ---- offline
    def output_len(self, in_len: int) -> int:
        """The frames of a whole job on `in_len` input frames; while a time map is set (set_time_map), the map's."""
        if self._map_hops is not None:
            return int(self._L.rc_time_map_output_len(C.byref(self._cfg), self._map_hops))
        return int(self._L.rc_offline_output_len(C.byref(self._cfg), in_len))

    def set_time_map(self, hop_pos=None):
        """Hop k of every whole job from now on reads its window at input sample `hop_pos[k]`, silence where that leaves
        the input, instead of at k * sample_step_len (rc_engine_set_time_map; the definition is in
        include/rocoder_hip.h): positions may repeat (a hold), decrease (reverse), be negative or lie past the end. The
        number of hops is a multiple of `params.hops_per_window`, and the job has `output_len` = hops / hops_per_window *
        window_out_len frames whatever its input length. It applies to `stretch_host`, `stretch_frames`,
        `stretch_frames_loud` and `stretch_tensor` / `stretch_device_ptr`, under every output stage and kernel. While a
        map is set `stretch_device_range_ptr` and the streaming calls raise (RC_EINVAL). None (or an empty list) clears
        it. `time_map_curve` builds the map of a varying stretch factor. A bad length or a position beyond +-2^48 raises
        (RC_EINVAL) and the previous map stays."""
        if hop_pos is None or len(hop_pos) == 0:
            self._check(self._L.rc_engine_set_time_map(self._h, None, 0))
            self._map_hops = None
            return
        if any(not -2 ** 63 <= int(v) < 2 ** 63 for v in hop_pos):
            raise ValueError("positions are signed 64-bit integers")
        pos = np.ascontiguousarray(hop_pos, np.int64).reshape(-1)
        self._check(self._L.rc_engine_set_time_map(self._h, pos.ctypes.data_as(C.POINTER(C.c_int64)), pos.size))
        self._map_hops = int(pos.size)

    def _host_output_len(self, in_len: int) -> int:
        # what `stretch_host` and `stretch_frames` give: output_len, resampled where a step is set
        n = self.output_len(in_len)
        if self._warp_out is not None:
            return self._warp_out
        return n if self._resample is None else int(self._L.rc_resample_len(n, *self._resample))

    def stretch_host(self, channels_in, out: Optional[np.ndarray] = None) -> np.ndarray:
        """Host arrays in, host arrays out (rc_engine_stretch_host). `out` (float32 [channels, >= output_len], rows
        contiguous) is filled and returned when given - reuse it across calls, and allocate both sides with
        `pinned_empty` to let the DMA engines read / write them directly (no staging copy)."""
        x = np.atleast_2d(channels_in)
        if x.dtype != np.float32 or x.strides[-1] != 4:
            x = np.ascontiguousarray(x, dtype=np.float32)
        if x.shape[0] != self.channels:
            raise ValueError("channel count mismatch")
        n_out = self._host_output_len(x.shape[1])
        if out is None:
            out = np.empty((self.channels, n_out), np.float32)
        elif (out.dtype != np.float32 or out.ndim != 2 or out.shape[0] != self.channels or out.shape[1] < n_out
              or out.strides[1] != 4):
            raise ValueError(f"out must be float32 [{self.channels}, >= {n_out}] with contiguous rows")
        fp = C.POINTER(C.c_float)
        ins = (fp * self.channels)(*[_fp(x[c]) for c in range(self.channels)])
        outs = (fp * self.channels)(*[_fp(out[c]) for c in range(self.channels)])
        got = C.c_size_t(0)
        self._check(self._L.rc_engine_stretch_host(self._h, ins, x.shape[1], outs, out.shape[1], C.byref(got)))
        assert got.value == n_out
        self._read_limiter_stats()
        return out[:, :n_out]

    last_clipped: Optional[int] = None  # stretch_frames(out_fmt=...): output samples beyond full scale (or NaN) of the last call
    last_peak: Optional[float] = None   # stretch_frames(normalize=...): the largest finite |sample| before the gain ...
    last_gain: Optional[float] = None   # ... and the gain it was multiplied by (both np.float32)
    # stretch_frames / stretch_host while a limiter is set (set_output_limiter): (the smallest gain as np.float32, the
    # number of frames turned down) of the last call
    last_limiter_stats: Optional[tuple] = None

    def _read_limiter_stats(self):
        if self._limiter:
            g, f = C.c_float(0), C.c_uint64(0)
            self._check(self._L.rc_engine_last_limiter_stats(self._h, C.byref(g), C.byref(f)))
            self.last_limiter_stats = (np.float32(g.value), int(f.value))

    def _raw_frames(self, frames, fmt):
        """What `stretch_frames` documents for `frames` and `fmt` -> (the block's bytes, the RC_PCM_* code, n_frames)."""
        by_dtype = {"uint8": "u8", "int16": "i16", "int32": "i32", "float32": "f32"}
        if fmt is None:
            a = np.asarray(frames)
            if a.dtype.name not in by_dtype or a.ndim != 2:
                raise ValueError("frames must be [n_frames, channels] uint8 / int16 / int32 / float32, or bytes with fmt=")
            fmt = by_dtype[a.dtype.name]
            if a.shape[1] != self.channels:
                raise ValueError("channel count mismatch")
        elif fmt not in _lib.PCM_FORMATS:
            raise ValueError(f"fmt must be one of {sorted(_lib.PCM_FORMATS)}")
        else:
            a = np.frombuffer(frames, np.uint8) if isinstance(frames, (bytes, bytearray, memoryview)) else np.asarray(frames)
        code = _lib.PCM_FORMATS[fmt]
        if not a.flags.c_contiguous:
            a = np.ascontiguousarray(a)
        raw = a.reshape(-1).view(np.uint8)
        frame_bytes = _lib.PCM_BYTES[code] * self.channels
        if raw.size % frame_bytes:
            raise ValueError(f"{raw.size} bytes are no whole number of {frame_bytes}-byte frames")
        n = raw.size // frame_bytes
        return raw, code, n

    def stretch_frames(self, frames, fmt: Optional[str] = None, out: Optional[np.ndarray] = None,
                       out_fmt: Optional[str] = None, normalize: Optional[float] = None) -> np.ndarray:
        """Interleaved PCM frames in, interleaved float32 frames out (rc_engine_stretch_frames): both format changes run
        on the GPU, and the result is `stretch_host` of the decoded rows, transposed, bit for bit. `frames` is a
        C-contiguous [n_frames, channels] array of uint8 / int16 / int32 / float32 (the format is the dtype's), or, with
        an explicit `fmt` ("u8", "i16", "i24", "i32", "f32"), `bytes` or a uint8 array of whole little-endian frames at
        any byte alignment - the only way to pass "i24". Returns [output_len, channels]; `out` (float32, C-contiguous,
        [>= output_len, channels], e.g. from `pinned_empty`) is filled and its first output_len rows returned.

        With `out_fmt` ("u8", "i16", "i24", "i32", "f32") the result is quantised and packed on the GPU as well
        (rc_engine_stretch_frames_pcm; x * S rounded to nearest even and clamped, S = 127 / 32767 / 8388608 / 2147483647):
        "i16" returns '<i2', "i32" '<i4', "u8" uint8 and "f32" float32, each [output_len, channels]; "i24" returns uint8
        [output_len, channels, 3], the samples' little-endian bytes. `out` is then any C-contiguous writable array of at
        least that many bytes, at any byte alignment; it is filled from its first byte, nothing else of it is written,
        and the result is a view of it. `last_clipped` holds the number of output samples beyond full scale.

        With `normalize=p` (a finite float above 0) the result is peak-normalised on the GPU in front of the quantiser
        (rc_engine_stretch_frames_norm): peak = the largest finite |sample| of the whole job, gain = p / peak in one f32
        division (1 where the peak is 0 or the quotient overflows), every sample times gain in one f32 multiplication.
        `out_fmt=None` then means "f32". `last_peak`, `last_gain` and `last_clipped` (counted after the gain) are set."""
        if normalize is not None:
            with np.errstate(over="ignore"):
                normalize = float(np.float32(normalize))  # (the C-ABI takes an f32)
            if not (normalize > 0 and np.isfinite(normalize)):
                raise ValueError("normalize must be a finite float32 above 0")
            if out_fmt is None:
                out_fmt = "f32"
        raw, code, n = self._raw_frames(frames, fmt)
        n_out = self._host_output_len(n)
        if out_fmt is not None:
            if out_fmt not in _lib.PCM_FORMATS:
                raise ValueError(f"out_fmt must be one of {sorted(_lib.PCM_FORMATS)}")
            ocode = _lib.PCM_FORMATS[out_fmt]
            dtype, tail = {"u8": (np.uint8, ()), "i16": ("<i2", ()), "i24": (np.uint8, (3,)), "i32": ("<i4", ()),
                           "f32": ("<f4", ())}[out_fmt]
            need = n_out * self.channels * _lib.PCM_BYTES[ocode]
            if out is None:
                out = np.empty(max(need, 1), np.uint8)
            elif not (isinstance(out, np.ndarray) and out.flags.c_contiguous and out.flags.writeable and out.nbytes >= need):
                raise ValueError(f"out must be a C-contiguous writable array of at least {need} bytes")
            dst = out.reshape(-1).view(np.uint8)
            got, clipped = C.c_size_t(0), C.c_uint64(0)
            src = C.c_void_p(raw.ctypes.data if raw.size else dst.ctypes.data)  # (no frames: any non-null pointer)
            cap = dst.size // (self.channels * _lib.PCM_BYTES[ocode])
            if normalize is not None:
                peak, gain = C.c_float(0), C.c_float(0)
                self._check(self._L.rc_engine_stretch_frames_norm(
                    self._h, src, n, code, C.c_void_p(dst.ctypes.data), cap, ocode, C.c_float(normalize), C.byref(got),
                    C.byref(peak), C.byref(gain), C.byref(clipped)))
                self.last_peak, self.last_gain = np.float32(peak.value), np.float32(gain.value)
            else:
                self._check(self._L.rc_engine_stretch_frames_pcm(
                    self._h, src, n, code, C.c_void_p(dst.ctypes.data), cap, ocode, C.byref(got), C.byref(clipped)))
            assert got.value == n_out
            self.last_clipped = int(clipped.value)
            self._read_limiter_stats()
            return dst[:need].view(dtype).reshape((n_out, self.channels) + tail)
        if out is None:
            out = np.empty((n_out, self.channels), np.float32)
        elif (out.dtype != np.float32 or out.ndim != 2 or out.shape[1] != self.channels or out.shape[0] < n_out
              or not out.flags.c_contiguous):
            raise ValueError(f"out must be C-contiguous float32 [>= {n_out}, {self.channels}]")
        got = C.c_size_t(0)
        src = C.c_void_p(raw.ctypes.data if raw.size else out.ctypes.data)  # (no frames: any non-null pointer)
        self._check(self._L.rc_engine_stretch_frames(self._h, src, n, code, _fp(out), out.shape[0], C.byref(got)))
        assert got.value == n_out
        self._read_limiter_stats()
        return out[:n_out]

    def mix_frames(self, frames, bus: "Bus", offset: int = 0, keys=None, send=None, fmt: Optional[str] = None) -> int:
        """One layer of a mix (rc_engine_mix_frames): the job `stretch_frames(frames, fmt)` would run under the engine's
        current state, with its planar float32 result accumulated on the GPU into `bus` instead of being downloaded:
        bus[cb][offset + t] += s[cb][t] * amp(t). `keys` is a sequence of (frame, amp) on the layer's own clock
        (`mix_envelope`; None: 1), `send` a [bus.channels, self.channels] matrix (None: the channels as they are, which
        needs equal counts). Frames that fall outside the bus are dropped; returns the number that landed. The call
        blocks: layers are summed in call order."""
        raw, code, n = self._raw_frames(frames, fmt)
        kf, ka = _mix_keys(keys)
        send_p = None
        if send is not None:
            with np.errstate(over="ignore"):
                send_a = np.ascontiguousarray(send, np.float32)
            if send_a.shape != (bus.channels, self.channels):
                raise ValueError(f"send must be [{bus.channels}, {self.channels}]")
            send_p = _fp(send_a)
        if not -2 ** 63 <= int(offset) < 2 ** 63:
            raise ValueError("offset is a signed 64-bit integer")
        mixed = C.c_uint64(0)
        src = C.c_void_p(raw.ctypes.data) if raw.size else None
        self._check(self._L.rc_engine_mix_frames(self._h, src, n, code, bus._h, int(offset), kf.ctypes.data_as(C.POINTER(C.c_uint64)),
                                                 _fp(ka), kf.size, send_p, C.byref(mixed)))
        self._read_limiter_stats()
        return int(mixed.value)

    def bus_frames(self, bus: "Bus", out_format: str = "f32", target_peak: Optional[float] = None, out: Optional[np.ndarray] = None):
        """The master of a mix (rc_engine_bus_frames): the rows of `bus` through this engine's output fade, limiter, peak
        normalisation (`target_peak`, None: none), dither and quantiser into interleaved frames of `out_format`. No hops
        run: the channel map, time map, resampler, warp and device kernels do not apply. The bus is not changed. Returns
        (frames, stats): what `stretch_frames(out_fmt=out_format)` returns for that format, [bus.n_frames, channels], and
        {"peak", "gain", "clipped"} (also in `last_peak`, `last_gain`, `last_clipped`)."""
        if out_format not in _lib.PCM_FORMATS:
            raise ValueError(f"out_format must be one of {sorted(_lib.PCM_FORMATS)}")
        tp = 0.0
        if target_peak is not None:
            with np.errstate(over="ignore"):
                tp = float(np.float32(target_peak))
            if not (tp > 0 and np.isfinite(tp)):
                raise ValueError("target_peak must be a finite float32 above 0")
        ocode = _lib.PCM_FORMATS[out_format]
        dtype, tail = {"u8": (np.uint8, ()), "i16": ("<i2", ()), "i24": (np.uint8, (3,)), "i32": ("<i4", ()), "f32": ("<f4", ())}[out_format]
        n_out = bus.n_frames
        need = n_out * self.channels * _lib.PCM_BYTES[ocode]
        if out is None:
            out = np.empty(max(need, 1), np.uint8)
        elif not (isinstance(out, np.ndarray) and out.flags.c_contiguous and out.flags.writeable and out.nbytes >= need):
            raise ValueError(f"out must be a C-contiguous writable array of at least {need} bytes")
        dst = out.reshape(-1).view(np.uint8)
        got, clipped, peak, gain = C.c_size_t(0), C.c_uint64(0), C.c_float(0), C.c_float(0)
        cap = dst.size // (self.channels * _lib.PCM_BYTES[ocode])
        self._check(self._L.rc_engine_bus_frames(self._h, bus._h, C.c_void_p(dst.ctypes.data), cap, ocode, C.c_float(tp), C.byref(got),
                                                 C.byref(peak), C.byref(gain), C.byref(clipped)))
        assert got.value == n_out
        self.last_peak, self.last_gain, self.last_clipped = np.float32(peak.value), np.float32(gain.value), int(clipped.value)
        self._read_limiter_stats()
        stats = {"peak": self.last_peak, "gain": self.last_gain, "clipped": self.last_clipped}
        return dst[:need].view(dtype).reshape((n_out, self.channels) + tail), stats

    last_lufs: Optional[float] = None       # stretch_frames_loud: the integrated loudness before the gain (np.float32, -inf: none) ...
    last_true_peak: Optional[float] = None  # ... and the true peak before the gain (np.float32); last_gain is the gain

    def stretch_frames_loud(self, frames, target_lufs: float, max_true_peak: float = 0.0, fmt: Optional[str] = None,
                            out: Optional[np.ndarray] = None, out_fmt: str = "f32", sample_rate: int = 0) -> np.ndarray:
        """`stretch_frames(..., out_fmt=...)` with the result loudness-normalised on the GPU in front of the quantiser
        (rc_engine_stretch_frames_loud): the integrated loudness of BS.1770-4 / EBU R 128 (K-weighting, 400 ms blocks at
        75 % overlap, the gates at -70 LUFS and 10 LU below, every channel at weight 1) and the 4 x oversampled true peak of
        the whole job are measured on the device; gain = 10^((target_lufs - lufs) / 20), lowered to max_true_peak /
        true_peak where `max_true_peak` (linear, 0: no ceiling) asks for less. `sample_rate` is the rate of the OUTPUT
        (0: the engine's). `last_lufs`, `last_true_peak`, `last_gain` and `last_clipped` (counted after the gain) are set."""
        with np.errstate(over="ignore"):
            target_lufs, max_true_peak = float(np.float32(target_lufs)), float(np.float32(max_true_peak))
        if not np.isfinite(target_lufs):
            raise ValueError("target_lufs must be a finite float32")
        if not max_true_peak >= 0:
            raise ValueError("max_true_peak must be a float32 of at least 0 (0: no ceiling)")
        if out_fmt not in _lib.PCM_FORMATS:
            raise ValueError(f"out_fmt must be one of {sorted(_lib.PCM_FORMATS)}")
        raw, code, n = self._raw_frames(frames, fmt)
        n_out = self._host_output_len(n)
        ocode = _lib.PCM_FORMATS[out_fmt]
        dtype, tail = {"u8": (np.uint8, ()), "i16": ("<i2", ()), "i24": (np.uint8, (3,)), "i32": ("<i4", ()), "f32": ("<f4", ())}[out_fmt]
        need = n_out * self.channels * _lib.PCM_BYTES[ocode]
        if out is None:
            out = np.empty(max(need, 1), np.uint8)
        elif not (isinstance(out, np.ndarray) and out.flags.c_contiguous and out.flags.writeable and out.nbytes >= need):
            raise ValueError(f"out must be a C-contiguous writable array of at least {need} bytes")
        dst = out.reshape(-1).view(np.uint8)
        got, clipped = C.c_size_t(0), C.c_uint64(0)
        lufs, tp, gain = C.c_float(0), C.c_float(0), C.c_float(0)
        src = C.c_void_p(raw.ctypes.data if raw.size else dst.ctypes.data)  # (no frames: any non-null pointer)
        cap = dst.size // (self.channels * _lib.PCM_BYTES[ocode])
        self._check(self._L.rc_engine_stretch_frames_loud(
            self._h, src, n, code, C.c_void_p(dst.ctypes.data), cap, ocode, int(sample_rate), C.c_float(target_lufs),
            C.c_float(max_true_peak), C.byref(got), C.byref(lufs), C.byref(tp), C.byref(gain), C.byref(clipped)))
        assert got.value == n_out
        self.last_lufs, self.last_true_peak, self.last_gain = np.float32(lufs.value), np.float32(tp.value), np.float32(gain.value)
        self.last_clipped = int(clipped.value)
        self._read_limiter_stats()
        return dst[:need].view(dtype).reshape((n_out, self.channels) + tail)

    def frames_power(self, frames, fmt: Optional[str] = None, bin_frames: int = 4410) -> np.ndarray:
        """The peak of every bin of `bin_frames` whole frames of a block of interleaved PCM frames, measured on the GPU
        on the raw block (rc_engine_frames_power): float32 [ceil(n_frames / bin_frames)], the largest |x| over all
        channels of the bin, x the reader's float of a sample, NaN samples skipped; linear, not decibels. `frames` and
        `fmt` are `stretch_frames`'s. It is the reference's `chunked_audio_power` (src/recorder.rs:94-113), the input of
        `autocrop_points`. The engine's fade, kernels and streaming state are left as they were."""
        bin_frames = int(bin_frames)
        if not 1 <= bin_frames < 2 ** 64:
            raise ValueError("bin_frames must be an integer of 1 ... 2^64 - 1")
        raw, code, n = self._raw_frames(frames, fmt)
        n_bins = int(self._L.rc_frames_power_bins(n, bin_frames))
        out = np.empty(max(n_bins, 1), np.float32)
        got = C.c_size_t(0)
        src = C.c_void_p(raw.ctypes.data if raw.size else out.ctypes.data)  # (no frames: any non-null pointer)
        self._check(self._L.rc_engine_frames_power(self._h, src, n, code, bin_frames, _fp(out), n_bins, C.byref(got)))
        assert got.value == n_bins
        return out[:n_bins]

    def frames_channel_peaks(self, frames, fmt: Optional[str] = None) -> np.ndarray:
        """The peak of every channel of a block of interleaved PCM frames, measured on the GPU on the raw block
        (rc_engine_frames_channel_peaks): float32 [channels], the float whose bits are the largest bits of |x| over the
        channel's samples - a NaN sample wins, then +-inf, then the largest finite magnitude; exactly 0 where the
        reference's all-zero test (src/recorder.rs:122) holds. `frames` and `fmt` are `stretch_frames`'s. The input of
        `split_mono_map`. The engine's fade, channel map, kernels and streaming state are left as they were."""
        raw, code, n = self._raw_frames(frames, fmt)
        out = np.empty(self.channels, np.float32)
        src = C.c_void_p(raw.ctypes.data if raw.size else out.ctypes.data)  # (no frames: any non-null pointer)
        self._check(self._L.rc_engine_frames_channel_peaks(self._h, src, n, code, _fp(out), self.channels))
        return out

    def stretch_device_ptr(self, d_in: int, in_stride: int, in_len: int, d_out: int, out_stride: int,
                           out_cap: int, stream: int = 0) -> int:
        got = C.c_size_t(0)
        self._check(self._L.rc_engine_stretch_device(self._h, C.c_void_p(d_in), in_stride, in_len,
                                               C.c_void_p(d_out), out_stride, out_cap, C.byref(got),
                                               C.c_void_p(stream)))
        return got.value

    def stretch_device_range_ptr(self, d_in: int, in_stride: int, in_len: int, ch_first: int,
                                 ch_count: int, win_first: int, win_count: int, d_out: int,
                                 out_stride: int, out_cap: int, stream: int = 0):
        self._check(self._L.rc_engine_stretch_device_range(self._h, C.c_void_p(d_in), in_stride, in_len,
                                                     ch_first, ch_count, win_first, win_count,
                                                     C.c_void_p(d_out), out_stride, out_cap,
                                                     C.c_void_p(stream)))

    def stretch_tensor(self, x, out=None, stream=None):
        """x: torch float32 CUDA tensor [channels, L] (device-resident). Returns [channels, n_out].
        Asynchronous on the caller's stream: a device-side failure (a run-seam wait that expired leaves samples
        unwritten) is raised by the NEXT call on this engine - call `synchronize()` once the stream is synced
        before trusting `out` when no further call follows."""
        import torch

        assert x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1
        n_out = self.output_len(x.shape[1])
        if out is None:
            out = torch.empty((self.channels, n_out), dtype=torch.float32, device=x.device)
        s = torch.cuda.current_stream(x.device).cuda_stream if stream is None else stream
        if s == 0:
            # legacy default stream: handle 0 means "the engine's own stream" in the C-ABI, so
            # order the call by hand (inputs ready before, outputs ready after)
            torch.cuda.current_stream(x.device).synchronize()
        self.stretch_device_ptr(x.data_ptr(), x.stride(0), x.shape[1], out.data_ptr(), out.stride(0),
                                out.shape[1], s)
        if s == 0:
            self.synchronize()
        return out

    def synchronize(self):
        self._check(self._L.rc_engine_synchronize(self._h))

    def last_kernel_stats(self):
        ms, hops, launches = C.c_float(0), C.c_uint64(0), C.c_uint32(0)
        self._check(self._L.rc_engine_last_kernel_stats(self._h, C.byref(ms), C.byref(hops),
                                                  C.byref(launches)))
        return float(ms.value), int(hops.value), int(launches.value)

    def kernel_times(self, n: int = 64) -> List[float]:
        """Event times (ms) of the kernel launches of the last min(n, 64) offline calls, oldest first."""
        buf = (C.c_float * n)()
        got = C.c_size_t(0)
        self._check(self._L.rc_engine_kernel_times(self._h, buf, n, C.byref(got)))
        return [float(buf[i]) for i in range(got.value)]

    # ---- single hop (ReFFT seam)
    def forward_fft(self, samples) -> np.ndarray:
        s = np.ascontiguousarray(samples, dtype=np.float32)
        assert s.size == self.window_len
        out = np.empty(2 * self.window_len, np.float32)
        self._check(self._L.rc_engine_forward_fft(self._h, _fp(s), _fp(out)))
        return out.view(np.complex64)

    def resynth(self, channel: int, hop: int, samples) -> np.ndarray:
        s = np.ascontiguousarray(samples, dtype=np.float32)
        assert s.size == self.window_len
        out = np.empty(self.window_len, np.float32)
        self._check(self._L.rc_engine_resynth(self._h, channel, hop, _fp(s), _fp(out)))
        return out

    # ---- user device kernel (rc_engine_load_device_kernel)
    def load_device_kernel(self, code: Optional[bytes]):
        """Load a code object from compile_device_kernel (None: remove the kernel); it runs from the next call."""
        self._check(self._L.rc_engine_load_device_kernel(self._h, code, 0 if code is None else len(code)))

    def set_device_kernel_source(self, src, name: Optional[str] = None):
        """compile_device_kernel + load_device_kernel."""
        self.load_device_kernel(compile_device_kernel(src, name))

    def set_channel_map(self, channel_map: Optional[Sequence[int]] = None):
        """Row c of every `stretch_frames` call from now on reads channel `channel_map[c]` of the frame block
        (rc_engine_set_channel_map): one index below `channels` per channel; a source channel may feed several rows, or
        none. The result is what the call gives with no map on the block `frames[:, channel_map]`. None (or an empty
        list) clears the map. `stretch_host`, `frames_power`, `frames_channel_peaks`, the device and streaming calls
        are untouched. A list of the wrong length or with an index out of range raises (RC_EINVAL) and the previous map
        stays."""
        if channel_map is None or len(channel_map) == 0:
            self._check(self._L.rc_engine_set_channel_map(self._h, None, 0))
            return
        vals = [int(v) for v in channel_map]
        if any(not 0 <= v < 2 ** 32 for v in vals):
            raise ValueError("channel indices are unsigned 32-bit integers")
        arr = (C.c_uint32 * len(vals))(*vals)
        self._check(self._L.rc_engine_set_channel_map(self._h, arr, len(vals)))

    def set_phase_mode(self, mode="random"):
        """How the whole-job calls resynthesise (rc_engine_set_phase_mode; the definition is in
        include/rocoder_hip_phase.h): "random" (the default) is the reference's magnitude x random phase, "propagate" lets
        every bin carry its own phase from hop to hop, "locked" gives every bin the rotation of its nearest spectral peak.
        `mode` is a name or one of RC_PHASE_*. The streaming calls, `stretch_device_range`, `resynth`, kernels, time maps
        and output warps do not go with a mode other than "random": whichever comes second raises."""
        if isinstance(mode, str):
            if mode not in _lib.PHASE_MODES:
                raise ValueError(f"phase mode {mode!r} is none of {sorted(_lib.PHASE_MODES)}")
            mode = _lib.PHASE_MODES[mode]
        if not 0 <= int(mode) < 2 ** 32:
            raise ValueError("phase mode is one of RC_PHASE_RANDOM, RC_PHASE_PROPAGATE, RC_PHASE_LOCKED")
        self._check(self._L.rc_engine_set_phase_mode(self._h, int(mode)))

    @property
    def phase_mode(self) -> int:
        m = C.c_uint32(0)
        self._check(self._L.rc_engine_get_phase_mode(self._h, C.byref(m)))
        return int(m.value)

    def set_output_fade(self, fade_in: int = 0, fade_out_start: Optional[int] = None, fade_out_len: int = 0):
        """The reference's sqrt fade-in over the first `fade_in` output frames and fade-out over `fade_out_len` frames
        from frame `fade_out_start` on, zeros behind it (rc_engine_set_output_fade; the definition is in
        include/rocoder_hip.h). Applied on the GPU by `stretch_host` and `stretch_frames` in front of the peak, the gain,
        the quantiser and the clipped count; `stretch_device`, the streaming calls and MultiEngine are untouched.
        `fade_out_start=None` is no fade-out, `fade_out_len=0` with a start a hard cut; the defaults clear the fade.
        A call whose output is shorter than a fade raises (RC_EINVAL) and writes nothing."""
        start = _lib.RC_FADE_NONE if fade_out_start is None else int(fade_out_start)
        for v in (int(fade_in), start, int(fade_out_len)):
            if not 0 <= v <= _lib.RC_FADE_NONE:
                raise ValueError("fade frame counts are unsigned 64-bit integers")
        self._check(self._L.rc_engine_set_output_fade(self._h, int(fade_in), start, int(fade_out_len)))

    def set_output_dither(self, mode: str = "none", seed: int = 0):
        """Dither in front of the integer quantiser of `stretch_frames(out_fmt="u8" | "i16" | "i24")`, with or without
        `normalize` (rc_engine_set_output_dither; the definition is in include/rocoder_hip.h): "tpdf" is triangular noise
        of 2 LSB peak to peak, "tpdf-hp" the same triangle high-passed, "none" (the default) clears it. The dither of
        a sample depends on `seed`, its channel and its output frame alone. i32 and f32 output, the f32 result,
        `stretch_host`, the device and streaming calls and MultiEngine are untouched. An unknown mode raises and the
        previous state stays."""
        if mode not in _lib.DITHER_MODES:
            raise ValueError(f"dither mode {mode!r} is none of {sorted(_lib.DITHER_MODES)}")
        if not 0 <= int(seed) < 2 ** 64:
            raise ValueError("the dither seed is an unsigned 64-bit integer")
        self._check(self._L.rc_engine_set_output_dither(self._h, _lib.DITHER_MODES[mode], int(seed)))

    def set_output_resample(self, num: int = 0, den: int = 0):
        """Band-limited resampling of the result of `stretch_host` and `stretch_frames` on the GPU by the step num / den
        input frames per output frame (rc_engine_set_output_resample; the definition is in include/rocoder_hip.h): a
        pitch ratio r on an engine created with factor * r, a change of sample rate as rate_in / rate_out, or both in
        one ratio (`resample_ratio`). The result has `resample_len(output_len(n), num, den)` frames, and the fade, the
        peak, the gain, the dither and the clipped count work on resampled frames. num == den (the defaults included)
        clears it. `output_len`, `stretch_device`, the streaming calls and MultiEngine are untouched. A step outside
        [1/8, 8] or with a reduced denominator above 1024 raises (RC_EINVAL) and the previous state stays."""
        if not (0 <= int(num) < 2 ** 32 and 0 <= int(den) < 2 ** 32):
            raise ValueError("num and den are unsigned 32-bit integers")
        self._check(self._L.rc_engine_set_output_resample(self._h, int(num), int(den)))
        self._resample = None if int(num) == int(den) else (int(num), int(den))

    def set_output_warp(self, anchors=None, n_out: int = 0):
        """Band-limited resampling of the result of `stretch_host` and `stretch_frames` on the GPU by a step that varies
        along the output - a glide, a tape stop, a vibrato (rc_engine_set_output_warp; the definition is in
        include/rocoder_hip_warp.h). `anchors` are int64 positions in the rows of the stretch result with 32 fractional
        bits, one per block of 64 output frames and one behind the last; a block's step lies in [1/8, 8]. The result has
        exactly `n_out` frames, and the fade, the limiter, the peak, the dither and the clipped count work on them.
        `warp_curve` builds the anchors of a pitch curve. None (or an empty list) clears it. The alternative of
        `set_output_resample`: each raises (RC_EINVAL) while the other is set, as bad anchors do, and the previous state
        stays."""
        if anchors is None or len(anchors) == 0:
            self._check(self._L.rc_engine_set_output_warp(self._h, None, 0, 0))
            self._warp_out = None
            return
        if any(not -2 ** 63 <= int(v) < 2 ** 63 for v in anchors):
            raise ValueError("anchors are signed 64-bit integers")
        if not 0 <= int(n_out) < 2 ** 64:
            raise ValueError("n_out is an unsigned integer")
        a = np.ascontiguousarray(anchors, np.int64).reshape(-1)
        self._check(self._L.rc_engine_set_output_warp(self._h, a.ctypes.data_as(C.POINTER(C.c_int64)), a.size, int(n_out)))
        self._warp_out = int(n_out)

    def set_output_limiter(self, drive: float = 1.0, ceiling: float = 0.0, lookahead: int = 0):
        """A look-ahead peak limiter on the result of `stretch_host` and `stretch_frames`, on the GPU, behind the resampler
        and the fade and in front of the peak of `normalize`, the dither and the quantiser (rc_engine_set_output_limiter;
        the definition is in include/rocoder_hip.h): every sample times `drive`, then a channel-linked gain that keeps
        every |sample| at or below `ceiling` and ramps over `lookahead` frames to either side of an over; a frame further
        than 2 * lookahead frames from every over keeps its bits (drive 1). `ceiling=0` (the default) clears it.
        `last_limiter_stats` is set by those calls while a limiter is set. `stretch_device`, the streaming calls and
        MultiEngine are untouched. A drive or ceiling that is not finite or not above 0, or a lookahead above 2048, raises
        (RC_EINVAL) and the previous state stays."""
        if not 0 <= int(lookahead) < 2 ** 32:
            raise ValueError("lookahead is an unsigned 32-bit integer")
        with np.errstate(over="ignore"):
            d, c = float(np.float32(drive)), float(np.float32(ceiling))
        self._check(self._L.rc_engine_set_output_limiter(self._h, C.c_float(d), C.c_float(c), int(lookahead)))
        self._limiter = c != 0.0

    def set_device_kernel_params(self, params: Sequence[float]):
        """Up to 16 floats, h.param(i) in the kernel; they take effect from the next call."""
        arr, n = _params_array(params)
        self._check(self._L.rc_engine_set_device_kernel_params(self._h, arr, n))



class MultiEngine:
    """One process, several GPUs of one node (include/rocoder_hip.h, rc_multi): one engine + one host thread per
    listed device, the job cut by `rc_shard_plan`, every shard copied once into its place. The multi-PROCESS layer
    (one rank per GPU over torch.distributed / RCCL) is `rocoder_amd.distributed`; both cut a job identically."""

    def __init__(self, device_ids: Sequence[int], **kw):
        self._L = _lib.lib()
        self._check = functools.partial(check, L=self._L)
        self._cfg, self._keep = make_config(**kw)
        ids = (C.c_int32 * len(device_ids))(*device_ids)
        h = C.c_void_p()
        self._check(self._L.rc_multi_create(C.byref(self._cfg), ids, len(device_ids), C.byref(h)))
        self._h = h
        self.device_ids = [int(d) for d in device_ids]
        self.channels = int(self._cfg.channels)
        self.params = derive_params(**kw)

    def close(self):
        if getattr(self, "_h", None):
            self._L.rc_multi_destroy(self._h)
            self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def output_len(self, in_len: int) -> int:
        return int(self._L.rc_offline_output_len(C.byref(self._cfg), in_len))

    def stretch_host(self, x: np.ndarray, out: Optional[np.ndarray] = None) -> np.ndarray:
        x = np.atleast_2d(x)
        if x.dtype != np.float32 or x.strides[-1] != 4:
            x = np.ascontiguousarray(x, dtype=np.float32)
        assert x.shape[0] == self.channels
        n_out = self.output_len(x.shape[1])
        if out is None:
            out = np.empty((self.channels, n_out), np.float32)
        elif (out.dtype != np.float32 or out.ndim != 2 or out.shape[0] != self.channels or out.shape[1] < n_out
              or out.strides[1] != 4):
            raise ValueError(f"out must be float32 [{self.channels}, >= {n_out}] with contiguous rows")
        fp = C.POINTER(C.c_float)
        ins = (fp * self.channels)(*[r.ctypes.data_as(fp) for r in x])
        outs = (fp * self.channels)(*[r.ctypes.data_as(fp) for r in out])
        got = C.c_size_t(0)
        self._check(self._L.rc_multi_stretch_host(self._h, ins, x.shape[1], outs, out.shape[1], C.byref(got)))
        assert got.value == n_out
        return out[:, :n_out]

    def load_device_kernel(self, code: Optional[bytes]):
        """The code object on every listed device's engine (None: remove the kernel)."""
        self._check(self._L.rc_multi_load_device_kernel(self._h, code, 0 if code is None else len(code)))

    def set_device_kernel_source(self, src, name: Optional[str] = None):
        self.load_device_kernel(compile_device_kernel(src, name))

    def set_device_kernel_params(self, params: Sequence[float]):
        arr, n = _params_array(params)
        self._check(self._L.rc_multi_set_device_kernel_params(self._h, arr, n))

    def set_staging(self, force: bool):
        """Diagnostic (rc_multi_set_staging): shares on the root's own device take the copy path of a remote one."""
        self._check(self._L.rc_multi_set_staging(self._h, 1 if force else 0))

    def stretch_tensor(self, x, out=None, root: int = 0):
        """x, out: torch float32 CUDA tensors on the ROOT device of the list (device_ids[root]). Blocking."""
        import torch

        if not 0 <= root < len(self.device_ids):
            raise RocoderError(RC_EINVAL, f"root {root} is not an index of the device list {self.device_ids}")
        assert x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1
        assert x.shape[0] == self.channels, (x.shape, self.channels)
        assert x.device.index == self.device_ids[root], \
            f"x lives on cuda:{x.device.index}, the root of the list is cuda:{self.device_ids[root]}"
        n_out = self.output_len(x.shape[1])
        if out is None:
            out = torch.empty((self.channels, n_out), dtype=torch.float32, device=x.device)
        assert out.device == x.device and out.dtype == torch.float32 and out.dim() == 2
        assert out.shape[0] == self.channels and out.shape[1] >= n_out and out.stride(1) == 1, (out.shape, out.stride())
        got = C.c_size_t(0)
        s = torch.cuda.current_stream(x.device)
        s.synchronize()
        self._check(self._L.rc_multi_stretch_device(self._h, root, C.c_void_p(x.data_ptr()), x.stride(0), x.shape[1],
                                                   C.c_void_p(out.data_ptr()), out.stride(0), out.shape[1],
                                                   C.byref(got), None))
        return out


class ReFFT:
    """src/fft.rs ReFFT: `new(window, kernel_src)`, `forward_fft`, `resynth`. The unseedable
    thread_rng of src/fft.rs:64 is replaced by the (seed, channel, hop) phase key."""

    def __init__(self, window, kernel=None, seed=0, channel_index=0, device=0, kernel_time_ms=0):
        w = np.ascontiguousarray(window, dtype=np.float32)
        self.window_len = w.size
        self.channel_index = channel_index
        self.hop = 0
        self._e = Engine(window_len=w.size, window=w, channels=channel_index + 1, seed=seed,
                         device=device, kernel=kernel, kernel_time_ms=kernel_time_ms)

    def forward_fft(self, samples) -> np.ndarray:  # src/fft.rs:50-61
        return self._e.forward_fft(samples)

    def resynth(self, samples, hop: Optional[int] = None) -> np.ndarray:  # src/fft.rs:42-48
        k = self.hop if hop is None else hop
        out = self._e.resynth(self.channel_index, k, samples)
        if hop is None:
            self.hop += 1
        return out


class Stretcher:
    """src/stretcher.rs Stretcher — one channel. `input` is the Receiver<Vec<f32>> side: a
    `queue.Queue` carrying float arrays, `None` meaning the Sender was dropped."""

    def __init__(self, spec: AudioSpec, input: "queue.Queue", factor: float, amplitude: float,  # noqa: A002
                 pitch_multiple: int, window, buffer_dur: float = 1.0, frequency_kernel=None,
                 seed: int = 0, channel_index: int = 0, device: int = 0, _engine: Engine = None,
                 kernel_time_ms: int = 0):
        self.spec = spec
        self.input = input
        self.channel_index = channel_index
        w = np.ascontiguousarray(window, dtype=np.float32)
        self._e = _engine or Engine(
            window_len=w.size, window=w, factor=factor, amplitude=amplitude,
            pitch_multiple=pitch_multiple, sample_rate=spec.sample_rate,
            channels=max(spec.channels, channel_index + 1), buffer_secs=buffer_dur, seed=seed,
            device=device, kernel=frequency_kernel, kernel_time_ms=kernel_time_ms)
        self.window_len = w.size
        self._closed = False

    def is_done(self) -> bool:  # src/stretcher.rs:78-80
        return self._e.is_done(self.channel_index)

    def channel_bound(self) -> int:  # src/stretcher.rs:82-85
        return self._e.channel_bound()

    def _pump(self, block: bool) -> bool:
        """Move chunks from the input queue into the engine; True if anything arrived."""
        got = False
        while not self._closed:
            try:
                chunk = self.input.get(block=block and not got)
            except queue.Empty:
                break
            got = True
            if chunk is None:
                self._e.close_input(self.channel_index)
                self._closed = True
            else:
                self._e.push_input(self.channel_index, chunk)
        return got

    def next_window(self) -> np.ndarray:  # src/stretcher.rs:87-121
        self._pump(block=False)
        while True:
            w = self._e.next_window(self.channel_index)
            if w is not None:
                return w
            # the reference blocks in self.input.recv() (src/stretcher.rs:125)
            self._pump(block=True)


class AudioBus:  # src/audio.rs:141-224
    def __init__(self, spec: AudioSpec, channels: List["queue.Queue"],
                 expected_total_samples: Optional[int]):
        self.spec = spec
        self.channels = channels
        self.expected_total_samples = expected_total_samples

    def into_audio(self, timeout: float = 0.005) -> List[np.ndarray]:  # src/audio.rs:152-172
        out: List[List[np.ndarray]] = [[] for _ in self.channels]
        closed = [False] * len(self.channels)
        while not all(closed):
            for i, ch in enumerate(self.channels):
                if closed[i]:
                    continue
                try:
                    chunk = ch.get(timeout=timeout)
                except queue.Empty:
                    continue
                if chunk is None:
                    closed[i] = True
                else:
                    out[i].append(chunk)
        return [np.concatenate(c) if c else np.zeros(0, np.float32) for c in out]


class StretcherProcessor:
    """src/stretcher_processor.rs: ONE thread, `loop { ctrl; for ch { if done break 'outer;
    send(next_window()) } }`, bounded(channel_bound()) output queues (back-pressure)."""

    SHUTDOWN = "Shutdown"  # StretcherProcessorControlMessage::Shutdown (:11-19)

    def __init__(self, channel_stretchers: Sequence[Stretcher],
                 expected_total_samples: Optional[int] = None):
        self.spec = channel_stretchers[0].spec
        self._channels = []
        receivers = []
        for s in channel_stretchers:  # :33-37
            q: "queue.Queue" = queue.Queue(maxsize=max(1, s.channel_bound()))
            self._channels.append((q, s))
            receivers.append(q)
        self.bus = AudioBus(self.spec, receivers, expected_total_samples)
        self._ctrl: "queue.Queue" = queue.Queue()
        self._finished = threading.Event()
        self._thread: Optional[threading.Thread] = None
        self.error: Optional[BaseException] = None

    @classmethod
    def new(cls, channel_stretchers, expected_total_samples=None):  # :26-46
        p = cls(channel_stretchers, expected_total_samples)
        return p, p.bus

    def _handle_control_messages(self) -> bool:  # :77-88 (non-blocking try_recv)
        try:
            msg = self._ctrl.get_nowait()
        except queue.Empty:
            return False
        return msg == self.SHUTDOWN

    def _run(self):
        try:
            running = True
            while running:  # :56-71
                if self._handle_control_messages():
                    break
                for out, stretcher in self._channels:
                    if stretcher.is_done():  # :64-68 "assuming each stretcher finishes at the same time"
                        running = False
                        break
                    out.put(stretcher.next_window())  # :69 blocks when the bounded queue is full
        except BaseException as e:  # noqa: BLE001
            self.error = e
        finally:
            for out, _ in self._channels:  # Senders dropped when the thread ends
                out.put(None)
            self._finished.set()  # :72

    def start(self):  # :50-75
        self._thread = threading.Thread(target=self._run, name="stretcher-processor", daemon=True)
        self._thread.start()
        return self

    def shutdown(self):  # Node::shutdown, src/signal_flow/node.rs:45-48
        self._ctrl.put(self.SHUTDOWN)

    def join(self, timeout=None):  # Node::join, src/signal_flow/node.rs:50-52
        if self._thread:
            self._thread.join(timeout)
        if self.error:
            raise self.error

    def is_finished(self) -> bool:  # src/signal_flow/node.rs:54-56
        return self._finished.is_set()


def stretch(channels_in, window_len=16384, factor=1.0, amplitude=1.0, pitch_multiple=1, seed=0,
            sample_rate=44100, kernel=None, device=0, kernel_time_ms=0, kernel_threads=0,
            device_kernel=None, device_kernel_source=None, device_kernel_params=None) -> np.ndarray:
    """Offline `-o` run (src/main.rs:124-160 minus file I/O): host [C, L] -> host [C, n_out].
    device_kernel_source: HIP source of a user device kernel (compile_device_kernel), with device_kernel_params."""
    x = np.ascontiguousarray(np.atleast_2d(channels_in), dtype=np.float32)
    with Engine(window_len=window_len, factor=factor, amplitude=amplitude,
                pitch_multiple=pitch_multiple, sample_rate=sample_rate, channels=x.shape[0],
                seed=seed, device=device, kernel=kernel, kernel_time_ms=kernel_time_ms,
                kernel_threads=kernel_threads, device_kernel=device_kernel) as e:
        if device_kernel_source is not None:
            e.set_device_kernel_source(device_kernel_source)
        if device_kernel_params is not None:
            e.set_device_kernel_params(device_kernel_params)
        return e.stretch_host(x)


__all__ = ["AudioSpec", "AudioBus", "Engine", "ReFFT", "Stretcher", "StretcherProcessor", "stretch",
           "derive_params", "offline_output_len", "load_kernel_library", "RocoderError", "compile_device_kernel",
           "DeviceKernelCompileError", "time_map_output_len", "time_map_curve", "warp_table", "warp_curve", "Bus", "mix_envelope"]
