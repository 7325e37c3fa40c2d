"""launch_frames_loud_energy and launch_frames_true_peak (rocoder_amd/csrc/rc_frames_loud.hip) through the test hooks, against
the numpy statement of the definition (tests/loudnessutil.py). Sub-block energies: within 2.3e-3 relative (0.01 dB, the
energy equivalent of the loudness gate) of the f64 definition for every sub-block whose own loudness is above -70 LUFS, and
within that fraction of the energy of -70 LUFS below; tests/test_loudness_host.py shows what these bounds catch. The kernel
runs in f64 and rounds a word once, so what it gives lies near 6e-8: the largest error seen is printed. True peak: bit for
bit - a maximum of order-fixed fmaf chains."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
rocoder_amd = pytest.importorskip("rocoder_amd")

import loudnessutil as U  # noqa: E402

pytestmark = pytest.mark.gpu

RATE, SUB = 8000, 800
SIZES = [0, 799, 800, 3199, 3200, 3201, 80000 + 37]
KINDS = ["white", "tone", "dc", "burst"]
_cache = {}


def rows(kind, channels, n):
    key = (kind, channels, n)
    if key not in _cache:
        x = U.test_input(kind, channels, n, RATE)
        x.setflags(write=False)
        _cache[key] = x
    return _cache[key]


@pytest.fixture(scope="module")
def table():
    return U.table_1_4()


def check_energies(x, **kw):
    want = U.sub_energies(x, RATE)
    got, guards = U.gpu_energies(x, RATE, launches=2, **kw)
    assert guards and got.shape[1:] == want.shape
    assert np.array_equal(got[0].view(np.uint32), got[1].view(np.uint32)), "two launches, two results"
    rel, quiet = U.energy_errors(got[0], want, SUB)
    print(f"energies {x.shape}: largest relative error {rel:.3e}, below -70 LUFS {quiet:.3e} of the gate's energy")
    assert np.isfinite(got).all() and rel <= U.GATE_REL and quiet <= U.GATE_REL, (rel, quiet)
    return rel


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("kind", KINDS)
def test_sub_block_energies_against_the_f64_definition(kind, channels, n):
    if n > 4000 and kind == "burst" and channels == 3:
        n = 24000 + 37  # (the burst begins at 16000: the long 3-channel case need not be the longest)
    check_energies(rows(kind, channels, n))


@pytest.mark.parametrize("kind", KINDS)
def test_energies_over_several_spans_with_a_stride_and_an_unaligned_row(kind):
    """a row of more than three workgroup spans, whatever span the launcher chose for it; the rows 3 and 1 floats off a
    16-byte boundary, their stride 5 floats longer than a row"""
    channels = 2
    span = U.loud_span(channels, (80000 + 37) // SUB)
    n = max(80000 + 37, (3 * span + 1) * SUB + 5)
    assert (n // SUB) / U.loud_span(channels, n // SUB) > 3
    x = rows(kind, channels, n)
    worst = max(check_energies(x, pad=5, base=3), check_energies(x[:, :3201], pad=1, base=1))
    assert worst <= 1e-5  # f64 arithmetic and one rounding to f32: far above this is a bug, not rounding


def check_peak(x, table, **kw):
    want = U.true_peak(x, table)
    got, gain_word = U.gpu_true_peak(x, table, **kw)
    assert gain_word == 0xA5A5A5A5
    assert np.float32(got).view(np.uint32) == np.float32(want).view(np.uint32), (got, want)
    return got


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("channels", [1, 3])
def test_true_peak_is_the_definition_bit_for_bit(channels, n, table):
    for kind in (KINDS if n < 4000 else ["white", "dc"]):
        check_peak(rows(kind, channels, n), table)
    if n:
        check_peak(rows("white", channels, n), table, pad=7, base=3)


def test_true_peak_of_chosen_rows(table):
    x = np.array(rows("white", 2, 3201))
    x[0, 17] = np.nan
    x[1, 2000] = np.inf
    x[1, 2100] = -np.inf
    got = check_peak(x, table)  # the chains a NaN or an inf enters are skipped, the others count
    assert np.isfinite(got) and got > 0
    assert check_peak(np.zeros((3, 3201), np.float32), table) == 0.0
    click = np.zeros((1, 2049), np.float32)
    click[0, 0] = 0.75
    assert check_peak(click, table) == np.float32(0.75)
    click = np.zeros((2, 2049), np.float32)
    click[1, -1] = -0.75
    assert check_peak(click, table) == np.float32(0.75)
    # the tone at R / 4, phase 45 degrees, under a 512-frame raised-cosine fade: the crest lies between the samples
    n = 4096
    k = np.arange(n, dtype=np.float64)
    env = np.ones(n)
    env[:512] = 0.5 - 0.5 * np.cos(np.pi * k[:512] / 512)
    env[-512:] = env[:512][::-1]
    tone = (env * np.sin(2.0 * np.pi * k / 4.0 + np.pi / 4.0)).astype(np.float32)[None, :]
    got = check_peak(tone, table)
    assert U.finite_peak(tone) == np.float32(0.70710677) and abs(float(got) - 1.0000061) < 2e-6
