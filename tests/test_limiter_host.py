"""CPU tests (-m "not gpu") of the look-ahead limiter's definition as tests/limiterutil.py states it in numpy - the yardstick
of the GPU tests - and of the two C-ABI entries' argument checks, which need no device. Each property is also run on the
mutants it must catch: a window of L instead of 2 L frames, a gain per channel, a missing clamp."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
rocoder_amd = pytest.importorskip("rocoder_amd")
from rocoder_amd import _lib  # noqa: E402

import limiterutil as U  # noqa: E402

ONE = U.ONE


def bits(x):
    a = np.asarray(x, np.float32)
    return (np.ascontiguousarray(a) if a.ndim else a).view(np.uint32)


def worked_input():
    x = np.full((1, 4000), 0.25, np.float32)
    x[0, 2000] = 2.0
    return x


def test_the_worked_answer_to_the_bit():
    y, g, S = U.limit(worked_input(), 1.0, 1.0, 5)
    for k in range(0, 12):
        for t in (2000 - k, 2000 + k):
            assert int(S[t]) == ONE * 11 - (ONE // 2) * (11 - k), (k, t)
    assert g[2000] == np.float32(0.5)
    assert int(bits(g[1995])) == 0x3F3A2E8C and g[1995] == np.float32(0.72727275)
    assert g[1989] == np.float32(1.0) and g[2011] == np.float32(1.0)
    assert y[0, 2000] == np.float32(1.0) and y[0, 1995] == np.float32(0.18181819)
    assert list(np.nonzero(S < np.uint64(11 * ONE))[0]) == list(range(1990, 2011))
    assert U.stats_of(g, S, 5) == (int(bits(np.float32(0.5))), 21)
    # everything else left with the bits it came with
    far = np.ones(4000, bool)
    far[1990:2011] = False
    assert np.array_equal(bits(y[0, far]), bits(worked_input()[0, far]))


@pytest.mark.parametrize("mutant", ["half_window", "no_clamp"])
def test_the_worked_answer_refuses_the_mutants(mutant):
    y, g, S = U.limit(worked_input(), 1.0, 1.0, 5, mutant=mutant)
    if mutant == "half_window":  # the notch is 11 frames wide, not 21, and never reaches r
        assert g[2000] != np.float32(0.5) and g[1992] == np.float32(1.0)
    else:  # this input needs no clamp: the mutant passes here and is caught on noise below
        assert y[0, 2000] == np.float32(1.0)


def test_no_lookahead_is_a_gain_per_frame():
    rng = np.random.default_rng(3)
    x = (rng.standard_normal((2, 300)) * 0.6).astype(np.float32)
    y, g, S = U.limit(x, 1.0, 1.0, 0)
    a = np.abs(x).max(axis=0)
    want_g = np.where(a > 1, (np.float32(1) / a), np.float32(1)).astype(np.float32)
    rq = (want_g * np.float32(16777216.0)).astype(np.uint32)
    assert np.array_equal(S, rq.astype(np.uint64))
    assert np.array_equal(g, (rq.astype(np.float32) / np.float32(ONE)).astype(np.float32))
    assert (a > 1).sum() > 5 and np.array_equal(bits(y[:, a <= 1]), bits(x[:, a <= 1]))
    assert np.abs(y).max() <= 1.0


@pytest.mark.parametrize("L", [0, 1, 5, 64])
def test_the_shortest_jobs(L):
    for n in sorted({0, 1, 2 * L, 2 * L + 1}):
        x = np.full((2, n), 0.5, np.float32)
        if n:
            x[1, n // 2] = -4.0
        y, g, S = U.limit(x, 1.0, 1.0, L)
        assert y.shape == (2, n) and g.shape == (n,) and S.shape == (n,)
        if n:
            assert g[n // 2] == np.float32(0.25) and y[1, n // 2] == np.float32(-1.0)
            assert np.abs(y).max() <= 1.0
            assert U.stats_of(g, S, L) == (int(bits(np.float32(0.25))), n)  # every frame lies within 2 L of the over
        else:
            assert U.stats_of(g, S, L) == (U.ONE_BITS, 0)


@pytest.mark.parametrize("at", ["first", "last"])
def test_an_over_in_the_first_and_in_the_last_frame(at):
    """the window leaves [0, n): rq is ONE outside, so the notch is the inner half of the triangle"""
    n, L = 200, 8
    x = np.full((1, n), 0.125, np.float32)
    u0 = 0 if at == "first" else n - 1
    x[0, u0] = 4.0
    y, g, S = U.limit(x, 1.0, 1.0, L)
    T = 2 * L + 1
    for k in range(0, 2 * L + 3):
        t = u0 + k if at == "first" else u0 - k
        want = T * ONE - (ONE - ONE // 4) * max(T - k, 0)
        assert int(S[t]) == want, (k, t)
    assert g[u0] == np.float32(0.25) and y[0, u0] == np.float32(1.0)
    assert U.stats_of(g, S, L)[1] == T


def test_nan_and_inf_are_skipped_in_the_maximum_and_passed_or_clamped():
    x = np.full((2, 100), 0.5, np.float32)
    x[0, 10] = np.nan
    x[0, 30] = np.inf
    x[1, 50] = -np.inf
    x[0, 70] = np.nan
    x[1, 70] = 3.0  # the other channel of a NaN frame still sets the gain
    y, g, S = U.limit(x, 1.0, 1.0, 3)
    assert np.isnan(y[0, 10]) and y[1, 10] == np.float32(0.5) and g[10] == np.float32(1.0)
    assert y[0, 30] == np.float32(1.0) and g[30] == np.float32(1.0)    # +inf * 1 clamps to the ceiling
    assert y[1, 50] == np.float32(-1.0) and g[50] == np.float32(1.0)
    # rq = trunc(fl(1 / 3) * 2^24) = 5592405, and g = rq / 2^24 exactly: a hair below 1 / 3
    assert np.isnan(y[0, 70]) and int(S[70]) == 7 * 5592405 + 0 * ONE and g[70] == np.float32(5592405.0 / 16777216.0)
    assert y[1, 70] == np.float32(3.0) * g[70] and y[1, 70] <= np.float32(1.0)
    assert U.stats_of(g, S, 3)[1] == 13  # the one over's notch, 4 L + 1 frames
    finite = np.isfinite(y)
    assert np.abs(y[finite]).max() <= 1.0
    # a frame of NaN alone: a = 0, no gain change
    z = np.full((1, 9), np.nan, np.float32)
    y, g, S = U.limit(z, 1.0, 0.5, 2)
    assert np.isnan(y).all() and (g == 1).all()


def test_two_channels_share_the_louder_ones_gain():
    x = np.full((2, 400), 0.25, np.float32)
    x[0, 200] = 2.0
    y, g, S = U.limit(x, 1.0, 1.0, 5)
    assert y[0, 200] == np.float32(1.0) and y[1, 200] == np.float32(0.125)  # the quiet channel is turned down too
    assert y[1, 195] == np.float32(0.18181819)
    ym, gm, Sm = U.limit(x, 1.0, 1.0, 5, mutant="unlinked")
    assert ym[1, 200] == np.float32(0.25) and not np.array_equal(bits(ym), bits(y))  # the mutant leaves it alone: caught


def gaussian(channels, n, seed, sigma=0.2):
    return (np.random.default_rng(seed).standard_normal((channels, n)) * sigma).astype(np.float32)


@pytest.mark.parametrize("L", [0, 1, 7, 64, 2048])
@pytest.mark.parametrize("heavy", [False, True])
def test_on_noise_nothing_finite_leaves_above_the_ceiling_and_untouched_frames_keep_their_bits(L, heavy):
    x = gaussian(2, 10000, 11 + L)
    P = np.abs(x).max()
    ceiling = np.float32(0.7)
    drive = np.float32(3 * ceiling / P) if heavy else np.float32(1.0)
    if not heavy:
        ceiling = np.float32(0.9 * P)
    y, g, S = U.limit(x, drive, ceiling, L)
    T = 2 * L + 1
    assert np.abs(y).max() <= ceiling
    assert (g <= 1).all() and (g >= 0).all()
    full = S == np.uint64(T * ONE)
    assert (g[full] == 1).all()
    if not heavy:
        assert 0 < (~full).sum() and np.array_equal(bits(y[:, full]), bits(x[:, full]))
        if L <= 64:
            assert (~full).sum() < x.shape[1] // 2
    # a notch reaches every frame within 2 L of an over and none beyond
    over = np.abs((x * drive).astype(np.float32)).max(axis=0) > ceiling
    near = np.convolve(over.astype(np.int64), np.ones(4 * L + 1, np.int64), mode="same") > 0 if 4 * L + 1 <= x.shape[1] else np.full(x.shape[1], over.any())
    assert np.array_equal(~full, near)
    # mutants: a window of L frames lets samples through above the ceiling in front of the clamp
    if heavy and L >= 1:
        yh, gh, Sh = U.limit(x, drive, ceiling, L, mutant="half_window")
        assert not np.array_equal(gh, g) and (gh >= g).all()


def test_the_clamp_is_needed_on_noise():
    """the roundings of r, g and the product leave some samples an ulp above the ceiling: without the clamp the bound fails"""
    above = 0
    for L in (0, 1, 7, 64):
        x = gaussian(1, 10000, 500 + L)
        ceiling = np.float32(0.3)
        y, g, S = U.limit(x, 1.0, ceiling, L, mutant="no_clamp")
        above += int((np.abs(y) > ceiling).sum())
        y, g, S = U.limit(x, 1.0, ceiling, L)
        assert np.abs(y).max() <= ceiling
    assert above > 0


def test_sliding_min_against_a_plain_loop():
    rng = np.random.default_rng(0)
    a = rng.integers(0, ONE + 1, 300).astype(np.uint32)
    for T in (1, 2, 3, 4, 5, 15, 16, 17, 129, 300):
        want = np.array([a[j:j + T].min() for j in range(a.size - T + 1)], np.uint32)
        assert np.array_equal(U.sliding_min(a, T), want)


def test_the_entries_refuse_a_null_engine_without_a_device():
    """fails on a build without the two entries"""
    L = _lib.lib()
    assert _lib.RC_LIMITER_MAX_LOOKAHEAD == U.MAX_LOOKAHEAD == 2048
    assert L.rc_engine_set_output_limiter(None, 1.0, 1.0, 64) == _lib.RC_EINVAL
    assert L.rc_engine_set_output_limiter(None, 1.0, 0.0, 0) == _lib.RC_EINVAL  # (a null engine has no state to clear)
    g, f = C.c_float(7.0), C.c_uint64(7)
    assert L.rc_engine_last_limiter_stats(None, C.byref(g), C.byref(f)) == _lib.RC_EINVAL
    assert g.value == 7.0 and f.value == 7
    assert L.rc_engine_last_limiter_stats(None, None, None) == _lib.RC_EINVAL
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rocoder_hip.h")).read()
    assert "#define RC_LIMITER_MAX_LOOKAHEAD 2048" in header
