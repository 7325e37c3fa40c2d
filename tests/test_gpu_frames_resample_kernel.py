"""launch_frames_resample (rocoder_amd/csrc/rc_frames_resample.hip) through the test hook rc_test_frames_resample, on white
noise in [-1, 1] from a seeded generator. The gate, for every output: |y_gpu - y_f64| <= gamma * sum_j |h_j| |x_j| + 1e-30
with gamma = T u / (1 - T u), u = 2^-24 - the standard bound of a length-T f32 dot product in any order, with or without
fma. y_f64 uses the engine's own f32 table, so the bound has no table term; tests/test_resample_host.py asserts the gate
on a CPU f32 implementation and on the mutants it must refuse."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
rocoder_amd = pytest.importorskip("rocoder_amd")
from rocoder_amd.stretcher import resample_table  # noqa: E402

import resampleutil as R  # noqa: E402

pytestmark = pytest.mark.gpu

RATIOS = [(3, 2), (2, 3), (160, 147), (147, 160), (1069, 1009), (824, 873), (8, 1), (1, 8)]
_tables = {}


def table(num, den):
    if (num, den) not in _tables:
        _tables[(num, den)] = resample_table(num, den)
    return _tables[(num, den)]


def noise(channels, n, seed):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, (channels, n)).astype(np.float32)


def gate(y, rows, t, num, den, **kw):
    want, bound = R.resample_f64(rows, t, num, den, **kw)
    assert y.shape == want.shape
    err = np.abs(y.astype(np.float64) - want)
    worst = (err / bound).max() if err.size else 0.0
    print(f"{num}/{den}: {y.shape} outputs, worst error {err.max() if err.size else 0.0:.3e}, {worst:.3f} of its bound")
    assert (err <= bound).all()


@pytest.mark.parametrize("channels", [1, 2, 3])
@pytest.mark.parametrize("num,den", RATIOS)
def test_a_job_in_one_launch_meets_the_gate_and_keeps_its_guards(num, den, channels):
    t = table(num, den)
    x = noise(channels, 5000, 1000 * num + den + channels)
    status, y, guards = R.gpu_resample(x, t, num, den, pad=3)
    assert status == 0 and guards
    assert y.shape == (channels, R.resample_len(5000, num, den)) and y.shape[1] <= 40000
    gate(y, x, t, num, den)


@pytest.mark.parametrize("num,den", RATIOS)
def test_jobs_shorter_than_the_filter(num, den):
    t = table(num, den)
    W = t.shape[1] // 2
    for n in (1, 5, W):
        x = noise(2, n, 31 * n + num)
        status, y, guards = R.gpu_resample(x, t, num, den, pad=1)
        assert status == 0 and guards and y.shape[1] == R.resample_len(n, num, den)
        gate(y, x, t, num, den)


@pytest.mark.parametrize("n", ["0", "1", "W - 1", "W", "T", "T + 1"])
def test_sizes_around_the_filter(n):
    num, den = 160, 147
    t = table(num, den)
    W, T = t.shape[1] // 2, t.shape[1]  # noqa: F841 (read by eval)
    n = eval(n)
    x = noise(3, n, 77 + n)
    status, y, guards = R.gpu_resample(x, t, num, den, n=n, pad=2)
    assert status == 0 and guards and y.shape == (3, R.resample_len(n, num, den))
    gate(y, x, t, num, den, n=n)


@pytest.mark.parametrize("num,den", [(3, 2), (147, 160), (1069, 1009), (8, 1)])
def test_cuts_into_launches_are_bit_identical(num, den):
    """one launch; [0, 1), [1, 1025), [1025, n_rs); single frames around a tile edge: a sample's bits do not depend on the
    launch or the tile that computed it"""
    t = table(num, den)
    n = 5000 if num <= den else 3000 * num // den
    x = noise(2, n, 5 + num)
    n_rs = R.resample_len(n, num, den)
    assert n_rs > 2100
    status, whole, guards = R.gpu_resample(x, t, num, den)
    assert status == 0 and guards
    gate(whole, x, t, num, den)
    status, cut, guards = R.gpu_resample(x, t, num, den, ranges=[(0, 1), (1, 1025), (1025, n_rs)])
    assert status == 0 and guards and np.array_equal(cut.view(np.uint32), whole.view(np.uint32))
    singles = [(0, 1020)] + [(m, m + 1) for m in range(1020, 1030)] + [(1030, 2047), (2047, 2048), (2048, 2049), (2049, n_rs)]
    status, cut, guards = R.gpu_resample(x, t, num, den, ranges=singles)
    assert status == 0 and guards and np.array_equal(cut.view(np.uint32), whole.view(np.uint32))


@pytest.mark.parametrize("num,den", [(160, 147), (2, 3), (8, 1)])
def test_positions_are_64_bit(num, den):
    """m0 near 2^33 with src0 to match and a buffer of a few thousand frames"""
    t = table(num, den)
    W = t.shape[1] // 2
    m0, count = 2 ** 33 + 12345, 2500
    lo = m0 * num // den - (W - 1)
    hi = (m0 + count - 1) * num // den + W + 1
    src0 = lo - 7
    x = noise(2, hi - src0 + 9, 91)
    n = 2 ** 40
    status, y, guards = R.gpu_resample(x, t, num, den, n=n, src0=src0, m0=m0, m1=m0 + count, pad=5)
    assert status == 0 and guards
    gate(y, x, t, num, den, n=n, src0=src0, m0=m0, m1=m0 + count)
    assert np.abs(y).max() > 0.1


def test_the_end_of_the_job_is_zero_beyond_n():
    """taps beyond n read zeros although the buffer holds noise there: src_len > n - src0"""
    num, den = 3, 2
    t = table(num, den)
    x = noise(1, 4000, 3)
    n = 3000
    status, y, guards = R.gpu_resample(x, t, num, den, n=n)
    assert status == 0 and guards and y.shape[1] == R.resample_len(n, num, den)
    gate(y, x[:, :n], t, num, den, n=n)


def test_a_range_whose_taps_lie_outside_src_is_refused_and_writes_nothing():
    num, den = 160, 147
    t = table(num, den)
    W = t.shape[1] // 2
    x = noise(2, 2000, 9)
    # the job has 4000 frames, src holds [1000, 3000): outputs whose taps stay inside are computed, a range one tap beyond
    # either end is refused
    first = -(-(1000 + W - 1) * den // num)          # the first m with q - (W - 1) >= 1000
    last = ((3000 - W - 1) * den + den - 1) // num   # the last m with q + W <= 2999
    assert first * num // den - (W - 1) >= 1000 and last * num // den + W <= 2999
    assert (first - 1) * num // den - (W - 1) < 1000 and (last + 1) * num // den + W > 2999
    status, y, guards = R.gpu_resample(x, t, num, den, n=4000, src0=1000, m0=first, m1=last + 1)
    assert status == 0 and guards
    gate(y, x, t, num, den, n=4000, src0=1000, m0=first, m1=last + 1)
    for a, b in ((first - 1, last + 1), (first, last + 2)):
        status, y, guards = R.gpu_resample(x, t, num, den, n=4000, src0=1000, m0=a, m1=b)
        assert status != 0 and guards and not y.any()
