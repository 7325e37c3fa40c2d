"""Helpers of the signal-class tests (tests/test_signal_classes_host.py, tests/test_gpu_signal_classes.py): inputs that
are zero except for single samples (clicks), constant, alternating (Nyquist) or scaled by a power of two, the part of
the output a click can reach (its support), and one table of kernel paths with the default window. The gates and the
oracle driver are those of tests/windowutil.py. No GPU, no product import."""
import functools
from collections import namedtuple

import numpy as np

import windowutil as wu
from oracle import cbind as oc
from oracle import oracle_np as onp
from test_gpu_window_parity import _hermitian_breaking, _np_band, _np_shift  # the oracle's side of the spectrum paths

SEED = 3


# ------------------------------------------------------------------ inputs
def clicks(ch, L, positions, amp=0.75):
    """zeros with single samples set to `amp`, in channel 0 only: every other channel stays all-zero"""
    x = np.zeros((ch, L), np.float32)
    x[0, np.asarray(sorted(set(positions)), np.int64)] = np.float32(amp)
    return x


def click_positions(N, step, L):
    """0; k step - 1 and k step for one k a third of the way in; L - 1 (it lies in the zero-padded tail hop); for
    N = 16384 and 65536, the kernels that hand a half-frame from run to run, one more position three and a half steps in
    front of the pair; then two lone clicks (below). The run length is the engine's own (plan_runs) and not visible from
    Python; at the lengths of CASES a job has fewer hops than the chip has resident workgroups, so every run is ONE hop
    and every pair of neighbouring hops a seam: the hops of the extra click (and of the pair) straddle N / step of them.
    The long job of tests/test_gpu_signal_classes.py, whose runs are several hops long, spaces its clicks by a prime
    number of hops."""
    k = max(1, (L // step) // 3)
    pos = [0, k * step - 1, k * step, L - 1]
    if N in (16384, 65536):
        pos.append((k - 3) * step - step // 2)
    # Two lone clicks behind the pair (an addition: tests/test_signal_classes_host.py shows why). The pair hides a read
    # that strays by ONE sample: hop k, which would read x[k step - 1] in front of its frame, holds the click at k step
    # and is inside the support anyway, and so is the hop that would read x[k step] behind its frame when step divides N.
    # `past` is the first sample behind the frame of hop k + 4, which is outside the support, three silent hops behind
    # the pair's; `before` is the last sample in front of the frame of hop m, the first hop behind those that hold `past`.
    nh = -(-N // step)
    past = (k + 4) * step + N
    before = (k + 6 + nh) * step - 1
    pos += [q for q in (past, before) if q < L - 1 - N]
    if step > N:  # every click above lies on w[0] = 0 or between two frames: one in the middle of the frame of hop k - 2
        pos.append((k - 2) * step + N // 2)
    return [q for i, q in enumerate(pos) if 0 <= q < L and q not in pos[:i]]


def dc(ch, L):
    return np.full((ch, L), 0.5, np.float32)


def nyquist(ch, L):
    return np.broadcast_to(np.where(np.arange(L) & 1, np.float32(-0.5), np.float32(0.5)), (ch, L)).copy()


def scaled(x, k):
    """x 2^k: exact in f32 while nothing overflows or goes subnormal"""
    return (np.asarray(x, np.float32) * np.float32(2.0 ** k)).astype(np.float32)


# ------------------------------------------------------------------ the support of a set of clicks
def click_hops(N, step, positions):
    """sorted hops k with k step <= pos < k step + N for some click (hops past the job's last one included)"""
    hops = set()
    for pos in positions:
        hops.update(range(max(0, (pos - N) // step + 1), pos // step + 1))
    return sorted(hops)


def support_mask(N, step, H, p, n_out, positions):
    """bool [n_out] for pitch p >= 1: hop k holds a click at pos iff k step <= pos < k step + N; it adds to
    O[k H .. k H + N), and output sample t is O[t p]. Outside the mask every hop that contributes is a zero frame."""
    assert p >= 1
    tp = np.arange(n_out, dtype=np.int64) * p
    blocks = np.zeros(tp[-1] // H + 2 if n_out else 1, bool)  # O in blocks of H: hop k covers blocks k and k + 1
    for k in click_hops(N, step, positions):
        if k < blocks.size:
            blocks[k:k + N // H] = True
    return blocks[tp // H]


def support_mask_of_windows(ref, wout):
    """bool [n_out] for negative pitch, in whole output windows: a window is inside iff the reference's is not all-zero"""
    ref = np.asarray(ref)
    live = (ref.reshape(-1, wout) != 0).any(axis=1)
    return np.repeat(live, wout)


def window_out_len(N, p):
    return N if p > 0 else (-(-N // -p) - 1) * -p  # (S - 1) |p| with S = ceil(N / |p|)


def first_leak(got, mask, H, p):
    """(hop, offset in hop) of the first nonzero sample outside the support, in O's coordinates; None if silent"""
    bad = np.flatnonzero((np.asarray(got) != 0) & ~mask)
    if bad.size == 0:
        return None
    o = int(bad[0]) * max(p, 1)
    return (o // H, o % H)


# ------------------------------------------------------------------ kernel paths, default window
Case = namedtuple("Case", "path N f p ch L spec")  # spec: None, "host", ("band", ...), ("shift", s), ("gain", g)

L16 = 80 * 1024 + 777
CASES = [
    # the generic slots kernel
    Case("generic", 32, 1.0, 1, 1, 500, None), Case("generic", 64, 2.0, 1, 3, 5000, None),
    Case("generic", 256, 4.0, 2, 2, 9999, None), Case("generic", 128, 0.3, 1, 2, 20000, None),
    # wave-local: pitch 1, and pitch 2 / 3 (compile time) or 5 (run time)
    Case("wave", 512, 2.0, 1, 2, 40 * 128 + 77, None), Case("wave", 512, 2.0, 5, 1, 9000, None),
    Case("wave", 1024, 4.0, 1, 2, 40 * 128 + 333, None), Case("wave", 1024, 4.0, 3, 1, 33333, None),
    Case("wave", 2048, 8.0, 1, 2, 30000, None), Case("wave", 2048, 3.0, 2, 2, 50001, None),
    Case("wave", 4096, 0.25, 1, 2, 100000, None), Case("wave", 4096, 2.0, 3, 1, 30001, None),
    Case("wave", 8192, 1.0, 1, 2, 20 * 4096 + 333, None), Case("wave", 8192, 2.0, 2, 3, 60001, None),
    # 16384: hop4 (pitch 1), the decimating instantiations, three channels
    Case("16384", 16384, 8.0, 1, 2, L16, None), Case("16384", 16384, 8.0, 2, 2, L16, None),
    Case("16384", 16384, 8.0, 3, 2, L16, None), Case("16384", 16384, 8.0, 5, 2, L16, None),
    Case("16384", 16384, 8.0, 1, 3, L16, None),
    # big5s, big5
    Case("quarter", 32768, 8.0, 2, 2, 6 * 32768 + 777, None), Case("quarter", 65536, 16.0, 1, 2, 6 * 65536 + 777, None),
    Case("chirpz", 1000, 4.0, 2, 2, 20000, None), Case("chirpz", 3000, 8.0, 1, 1, 24000, None),
    Case("chirpz", 24000, 3.0, 1, 1, 130000, None),
    Case("long", 131072, 4.0, 1, 2, 6 * 131072 + 777, None), Case("long", 65538, 4.0, 1, 1, 6 * 65538 + 777, None),
    Case("negative", 2048, 3.0, -2, 2, 40000, None), Case("negative", 16384, 8.0, -3, 1, 100000, None),
    Case("negative", 3000, 3.0, -2, 1, 40000, None),
    # spectrum paths: analysis half, kernel, synthesis half
    Case("host", 2048, 4.0, 2, 2, 6 * 2048 + 777, "host"), Case("host", 16384, 8.0, 1, 2, 6 * 16384 + 777, "host"),
    Case("band", 4096, 4.0, 1, 2, 6 * 4096 + 777, ("band", 4096 // 64, 4096 // 8, 1.25, 0.1)),
    Case("band", 16384, 8.0, 1, 2, 6 * 16384 + 777, ("band", 16384 // 64, 16384 // 8, 1.25, 0.1)),  # fused into hop4
    Case("shift", 4096, 4.0, 1, 2, 6 * 4096 + 777, ("shift", 37)),
    Case("shift", 16384, 8.0, 1, 2, 6 * 16384 + 777, ("shift", 37)),
    Case("gain", 1024, 2.0, 1, 2, 40 * 256 + 333, ("gain", -1.5)),
]


def case_id(c):
    return f"{c.path}-{c.N}-f{c.f}-p{c.p}-ch{c.ch}-L{c.L}"


def is_pow2(N):
    return N & (N - 1) == 0


def engine_kwargs(c):
    """what Engine(...) takes for the case's spectrum path, beside the geometry"""
    if c.spec is None:
        return {}
    if c.spec == "host":
        return dict(kernel=_hermitian_breaking, kernel_time_ms=123)
    return dict(device_kernel=c.spec)


def oracle_kernel(c):
    if c.spec is None:
        return None
    if c.spec == "host":
        return _hermitian_breaking
    if c.spec[0] == "band":
        return _np_band(*c.spec[1:])
    if c.spec[0] == "shift":
        return _np_shift(c.spec[1])
    g = np.float32(c.spec[1])
    return lambda t, s: s * g


def geometry(c):
    """(step, H, n_out) of the case"""
    d = onp.derive(c.N, c.f, 1.0, c.p)
    return d["step"], d["H"], oc.offline_output_len(c.L, c.N, c.f, c.p)


def make_input(c, signal):
    if signal == "white":
        return wu.white_input(c.ch, c.L)
    if signal == "clicks":
        return clicks(c.ch, c.L, click_positions(c.N, geometry(c)[0], c.L))
    return {"dc": dc, "nyquist": nyquist}[signal](c.ch, c.L)


@functools.lru_cache(maxsize=2)
def reference(c, signal):
    """[ch, n_out] f64, read-only: the C oracle for powers of two up to 65536, the f64 twin elsewhere
    (windowutil.oracle_with_window), driven with the default window's f32 table. A test and its mask share one
    computation; only the two latest are kept (the largest is 100 MB)."""
    ref = wu.oracle_with_window(make_input(c, signal), c.N, c.f, c.p, oc.hanning(c.N), SEED, kernel=oracle_kernel(c))
    ref.setflags(write=False)
    return ref


def case_mask(c, positions=None, ref=None):
    """the support of the case's clicks: the arithmetic for p >= 1, the reference's live windows for p < 0"""
    step, H, n_out = geometry(c)
    if c.p >= 1:
        return support_mask(c.N, step, H, c.p, n_out, click_positions(c.N, step, c.L) if positions is None else positions)
    ref = reference(c, "clicks") if ref is None else ref
    return support_mask_of_windows(ref[0], window_out_len(c.N, c.p))
