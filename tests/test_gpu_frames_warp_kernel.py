"""launch_frames_warp (rocoder_amd/csrc/rc_frames_warp.hip) through the test hook rc_test_frames_warp, on rows of 2 channels
by 3000 white frames in [-1, 1] from a seeded generator. At the constant steps where the warp IS the rational resampler the
yardstick is launch_frames_resample with rc_resample_table's table, bit for bit. On a glide the gate is, for every output,
|y_gpu - y_f64| <= gamma_{T+3} * (sum |h_p||x| + sum |h_{p+1}||x|) + 1e-30, gamma_k = k u / (1 - k u), u = 2^-24, y_f64 the
definition of tests/warputil.py over the engine's own f32 tables; tests/test_warp_host.py asserts that gate on a CPU f32
implementation and on the mutants it must refuse."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
rocoder_amd = pytest.importorskip("rocoder_amd")
from rocoder_amd.stretcher import resample_table, warp_table  # noqa: E402

import resampleutil as R  # noqa: E402
import warputil as Wp  # noqa: E402

pytestmark = pytest.mark.gpu

_tables = {}


def tables(tiers):
    for t in tiers:
        if t not in _tables:
            _tables[t] = warp_table(t)
    return {t: _tables[t] for t in tiers}


def tiers_of(anchors):
    return {Wp.tier_of(int(d)) for d in np.diff(anchors)}


def same_bits(got, want):
    return got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))


def gate(y, rows, anchors, n_out, what, **kw):
    want, bound = Wp.warp_f64(rows, tables(tiers_of(anchors)), anchors, n_out, **kw)
    assert y.shape == want.shape
    err = np.abs(y.astype(np.float64) - want)
    print(f"{what}: {y.shape} outputs, worst error {err.max():.3e}, {(err / bound).max():.3f} of its bound")
    assert (err <= bound).all()


@pytest.fixture(scope="module")
def glide():
    rows = Wp.white_rows()
    anchors, n_out = Wp.glide_case()
    status, whole, guards = Wp.gpu_warp(rows, tables(tiers_of(anchors)), anchors, n_out, pad=3)
    assert status == 0 and guards
    whole.flags.writeable = False
    return rows, anchors, n_out, whole


@pytest.mark.parametrize("num,den", [(1, 2), (3, 4), (3, 8), (1, 1), (2, 1), (4, 1)])
def test_constant_steps_are_the_rational_resampler_bit_for_bit(num, den):
    rows = Wp.white_rows()
    n_out = R.resample_len(rows.shape[1], num, den)
    anchors = Wp.constant_anchors(num, den, n_out)
    status, want, guards = R.gpu_resample(rows, resample_table(num, den), num, den)
    assert status == 0 and guards and want.shape == (2, n_out) and np.abs(want).max() > 0.1
    status, got, guards = Wp.gpu_warp(rows, tables(tiers_of(anchors)), anchors, n_out, pad=1)
    assert status == 0 and guards
    assert same_bits(got, want)


def test_a_glide_over_seven_tiers_meets_the_gate_and_keeps_its_guards(glide):
    rows, anchors, n_out, whole = glide
    t = [Wp.tier_of(int(d)) for d in np.diff(anchors)]
    assert set(t) == set(range(7)) and any(a != b for a, b in zip(t, t[1:])) and any(a > b for a, b in zip(t, t[1:]))
    assert n_out > 2 * 1024 - 64 and whole.shape == (2, n_out)
    gate(whole, rows, anchors, n_out, "glide 0.5 ... 2.5")


def test_cuts_into_launches_are_bit_identical(glide):
    """one launch; [0, 1), [1, 1025), [1025, n_out); single frames around a block edge and a tile edge: a sample's bits do
    not depend on the launch, the tile or the range that computed it"""
    rows, anchors, n_out, whole = glide
    tb = tables(tiers_of(anchors))
    status, cut, guards = Wp.gpu_warp(rows, tb, anchors, n_out, ranges=[(0, 1), (1, 1025), (1025, n_out)])
    assert status == 0 and guards and same_bits(cut, whole)
    singles = [(0, 63), (63, 64), (64, 65), (65, 66), (66, 1023), (1023, 1024), (1024, 1025), (1025, 1026), (1026, n_out)]
    status, cut, guards = Wp.gpu_warp(rows, tb, anchors, n_out, ranges=singles, pad=2)
    assert status == 0 and guards and same_bits(cut, whole)
    # an inner range of its own, with dst at its first frame
    status, part, guards = Wp.gpu_warp(rows, tb, anchors, n_out, m0=70, m1=1500, pad=5)
    assert status == 0 and guards and same_bits(part, whole[:, 70:1500])


def test_positions_are_64_bit(glide):
    """the same glide 2^29 - 4000 frames into a job of 2^29 + 100 frames, src0 to match and a buffer of a few thousand
    frames: the anchors lie just below 2^61, and the bits are those of the glide at the origin where no tap leaves the job"""
    rows, anchors, n_out, whole = glide
    shift = 2 ** 29 - 4000
    far = anchors + (shift << 32)
    assert far[-1] < 2 ** 62
    n = 2 ** 29 + 100
    w0 = Wp.W[Wp.tier_of(int(anchors[1] - anchors[0]))]
    src0 = shift - (w0 - 1) - 7
    buf = np.zeros((2, rows.shape[1] + w0 + 6 + 300), np.float32)
    buf[:, w0 + 6:w0 + 6 + rows.shape[1]] = rows
    status, y, guards = Wp.gpu_warp(buf, tables(tiers_of(anchors)), far, n_out, n=n, src0=src0, pad=1)
    assert status == 0 and guards
    assert same_bits(y, whole)


def test_outside_the_job_reads_zeros(glide):
    """taps beyond n read zeros although the buffer holds noise there, and so do taps in front of frame 0"""
    rows, anchors, n_out, whole = glide
    n = 2000
    status, y, guards = Wp.gpu_warp(rows, tables(tiers_of(anchors)), anchors, n_out, n=n)
    assert status == 0 and guards
    gate(y, rows[:, :n], anchors, n_out, "n = 2000 of 3000", n=n)
    last = max(m for m in range(n_out) if Wp.position(anchors, m)[0] >> 32 < n - 260)
    assert same_bits(y[:, :last], whole[:, :last]) and not same_bits(y, whole)
    beyond = min(m for m in range(n_out) if (Wp.position(anchors, m)[0] >> 32) - 255 >= n)
    assert not y[:, beyond:].any() and y[:, :beyond].any()


def test_the_launchers_refusals_write_nothing(glide):
    rows, anchors, n_out, whole = glide
    tb = tables(tiers_of(anchors))
    # the job has 4000 frames, src holds [1000, 3000), the step is 1 (W = 32): outputs whose taps stay inside are computed,
    # a range one tap beyond either end is refused
    one = Wp.constant_anchors(1, 1, 4000)
    x = rows[:, :2000]
    first, last = 1000 + 31, 2999 - 32
    status, y, guards = Wp.gpu_warp(x, tables({0}), one, 4000, n=4000, src0=1000, m0=first, m1=last + 1)
    assert status == 0 and guards
    gate(y, x, one, 4000, "src = [1000, 3000)", n=4000, src0=1000, m0=first, m1=last + 1)
    for a, b in ((first - 1, last + 1), (first, last + 2)):
        status, y, guards = Wp.gpu_warp(x, tables({0}), one, 4000, n=4000, src0=1000, m0=a, m1=b)
        assert status != 0 and guards and not y.any()
    # a host table with a step out of range in a block of the range (the device's copy stays the good one)
    for bad_step in (Wp.D_MIN - 1, Wp.D_MAX + 1, 0, -Wp.D[0]):
        bad = anchors.copy()
        bad[5:] += bad_step - (bad[5] - bad[4])
        status, y, guards = Wp.gpu_warp(rows, tb, anchors, n_out, host_anchor=bad)
        assert status != 0 and guards and not y.any()
        status, y, guards = Wp.gpu_warp(rows, tb, anchors, n_out, host_anchor=bad, m1=256)  # (a range in front of it is served)
        assert status == 0 and guards and same_bits(y, whole[:, :256])
    # an empty range launches nothing
    status, y, guards = Wp.gpu_warp(rows, tb, anchors, n_out, m0=100, m1=100)
    assert status == 0 and guards and y.shape == (2, 0)
