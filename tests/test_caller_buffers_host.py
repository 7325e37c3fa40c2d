"""CPU proof that the caller-buffer checks (tests/layoututil.py, used on the GPU by tests/test_gpu_caller_buffers.py) are
sound and bite.

Sound: a numpy stand-in for the engine, which reads and writes flat buffers by base and stride and computes with the
oracle, passes every check of the GPU file on three small cases. Biting: ten mutants of the stand-in, each one
addressing mistake a kernel or its launch code can make at the edges of the caller's buffers, are each refused by the
checks named in REFUSED_BY - and every one of them passes what the suite had before: the same job in the contiguous,
aligned layout with nothing around the rows, held to the oracle and (for a range) to the full job. That is the gap.
(One of them, the read of x[L], passes there in the last row and in a mono job only: asserted as it is.)

It also holds layoututil.range_span to the engine's input_span by hand-written answers, and layoututil's restated
geometry to rc_derive_params on every case of tests/signalutil.py."""
import numpy as np
import pytest

import layoututil as lu
import signalutil as su
import windowutil as wu
from layoututil import GUARD, POISON, Layout, StandIn

SMALL = [su.Case("generic", 64, 2.0, 1, 2, 1000, None), su.Case("wave", 1024, 4.0, 3, 2, 9000, None),
         su.Case("negative", 2048, 3.0, -2, 2, 12000, None)]
RANGE_OFFSETS = (1, 3)  # the layout of the range test: both bases 4 but not 8 bytes aligned
TAIL_OFFSETS = (1, 1)


def _geometry(c, L=None):
    step = su.geometry(c)[0]
    L = c.L if L is None else L
    total = lu.total_windows(L, c.N, step, c.p)
    return step, total, total * lu.window_out_len(c.N, c.p)


# ------------------------------------------------------------------ the layout and its helpers
def test_the_two_poisons_are_distinct_quiet_nans():
    for word in (POISON, GUARD):
        assert word & 0x7FC00000 == 0x7FC00000 and word & 0x003FFFFF  # exponent all ones, quiet bit, a payload
        assert np.isnan(np.array([word], np.uint32).view(np.float32)[0])
    assert POISON != GUARD


@pytest.mark.parametrize("in_off,out_off", lu.OFFSETS)
def test_layout_is_what_it_says(in_off, out_off):
    ch, L, n_out, N = 3, 1000, 1984, 64
    lay = Layout(ch, L, n_out, N, in_off, out_off)
    assert lay.in_stride == 1065 and lay.out_stride == 2049  # the smallest odd numbers >= L + N + 1, n_out + N + 1
    assert Layout(1, 1001, 1985, 64).in_stride == 1067 and Layout(1, 1001, 1985, 64).out_stride == 2051
    assert lay.in_row(0) == N + in_off and lay.out_row(0) == N + out_off
    assert {lay.in_row(c) & 1 for c in range(ch)} == {0, 1} == {lay.out_row(c) & 1 for c in range(ch)}
    x = wu.white_input(ch, L)
    buf = lu.pack_input(x, lay)
    assert buf.ctypes.data % 256 == 0 and buf.dtype == np.uint32 and buf.size == lay.in_words
    inside = np.zeros(buf.size, bool)
    for c in range(ch):
        assert np.array_equal(buf[lay.in_row(c):lay.in_row(c) + L].view(np.float32), x[c])
        assert (buf[lay.in_row(c) - N:lay.in_row(c)] == POISON).all()          # a window in front of every row
        assert (buf[lay.in_row(c) + L:lay.in_row(c) + L + N + 1] == POISON).all()  # and behind it, the last included
        inside[lay.in_row(c):lay.in_row(c) + L] = True
    assert (buf[~inside] == POISON).all() and np.isfinite(buf[inside].view(np.float32)).all()
    out = lu.blank_output(lay)
    assert out.ctypes.data % 256 == 0 and out.size == lay.out_words and (out == GUARD).all()
    assert lay.out_words - (lay.out_row(ch - 1) + n_out) >= N + 1
    assert lu.first_damage(out, lay) is None and lu.rows_of(out, lay).shape == (ch, n_out)
    kept = lu.pack_input(x, lay, keep=(2, 100, 300))
    assert np.array_equal(kept[lay.in_row(2) + 100:lay.in_row(2) + 300].view(np.float32), x[2, 100:300])
    assert np.count_nonzero(kept != POISON) == 200


def test_first_damage_names_the_stray_store():
    lay = Layout(2, 500, 640, 64, 1, 2)
    for word, want in ((lay.out_row(0) - 1, (0, -1)), (lay.out_row(0) + 640, (0, 1)), (lay.out_row(1) - 1, (1, -1)),
                       (lay.out_row(1) + 640 + 64, (1, 65)), (0, (0, -66)), (lay.out_row(1) - 3, (1, -3))):
        out = lu.blank_output(lay)
        out[lay.out_row(0):lay.out_row(0) + 640] = 0  # (rows may hold anything)
        out[word] = 0x3F800000
        assert lu.first_damage(out, lay) == want, word
        assert "damage" in lu.hostile_checks(out, lay, lu.rows_of(out, lay))
    out = lu.blank_output(lay)
    out[5] = POISON  # (the other NaN is damage too: compared as words)
    assert lu.first_damage(out, lay) == (0, 5 - lay.out_row(0))


# ------------------------------------------------------------------ the span of a range
def test_range_span_by_hand():
    """input_span (rc_engine.cpp) with history 0: first = h0 > 1 ? h0 - 1 : 0 with h0 = w0 hpw, [first step,
    (w1 hpw - 1) step + N), both cut at in_len. The answers below are worked by hand from that."""
    # N = 1024, f = 4, p = 1: step 128, two hops per window, L = 10000: k_d = 71, 36 windows
    assert lu.range_span(128, 1024, 2, 0, 2, 10000) == (0, 1408)        # w0 = 0: hops 0 .. 3
    assert lu.range_span(128, 1024, 2, 1, 3, 10000) == (128, 1664)      # w0 = 1: hops 1 .. 5 (1 is the recomputed one)
    assert lu.range_span(128, 1024, 2, 30, 36, 10000) == (7552, 10000)  # hops 59 .. 71: 71 * 128 + 1024 = 10112 > L
    assert lu.total_windows(10000, 1024, 128, 1) == 36
    # N = 2048, f = 3, p = -2: step 682, ONE hop per window
    assert lu.range_span(682, 2048, 1, 5, 10, 12000) == (2728, 8186)    # hops 4 .. 9
    assert lu.range_span(682, 2048, 1, 0, 1, 12000) == (0, 2048)
    assert lu.range_span(682, 2048, 1, 14, 16, 12000) == (8866, 12000)  # hop 15 starts at 10230: 1770 samples + zeros


@pytest.mark.parametrize("c", su.CASES, ids=su.case_id)
def test_restated_geometry_is_the_engines(c):
    """rc_derive_params / rc_offline_output_len (host code, no device) against layoututil's restatement, and the
    range of tests/test_gpu_caller_buffers.py: a third of the job, at least two windows in."""
    from rocoder_amd import stretcher as st

    par = st.derive_params(window_len=c.N, factor=c.f, pitch_multiple=c.p, channels=c.ch)
    step, total, n_out = _geometry(c)
    assert (par.sample_step_len, par.hops_per_window, par.window_out_len) == (step, lu.hops_per_window(c.p), lu.window_out_len(c.N, c.p))
    assert n_out == st.offline_output_len(c.L, window_len=c.N, factor=c.f, pitch_multiple=c.p, channels=c.ch) == su.geometry(c)[2]
    w0, w1 = total // 3, 2 * total // 3
    assert w0 >= 2 and w1 > w0
    lo, hi = lu.range_span(step, c.N, par.hops_per_window, w0, w1, c.L)
    assert 0 < lo < hi < c.L  # (poison on both sides of the span, inside the row)


# ------------------------------------------------------------------ the three parts, on the stand-in
def _part_a(engine, c, offsets):
    """every (in_off, out_off): guards, finite, the contiguous run's bits -> {check: what}"""
    x = wu.white_input(c.ch, c.L)
    n_out = _geometry(c)[2]
    flat = Layout(c.ch, c.L, n_out, c.N, contiguous=True)
    want = lu.rows_of(StandIn(c.N, c.f, c.p)(lu.pack_input(x, flat), flat), flat)  # (the contiguous run is held to the
    failed = {}                                                                   # oracle in _contiguous below)
    for in_off, out_off in offsets:
        lay = Layout(c.ch, c.L, n_out, c.N, in_off, out_off)
        for k, v in lu.hostile_checks(engine(lu.pack_input(x, lay), lay), lay, want).items():
            failed.setdefault(k, f"({in_off}, {out_off}): {v}")
    return failed


def _part_b(engine, c, k=5):
    """L = k step + N + dL in layout (1, 1), against the oracle at that L"""
    step = su.geometry(c)[0]
    failed = {}
    for dL in (-1, 0, 1):
        L = k * step + c.N + dL
        x = wu.white_input(c.ch, L)
        lay = Layout(c.ch, L, _geometry(c, L)[2], c.N, *TAIL_OFFSETS)
        ref = wu.oracle_with_window(x, c.N, c.f, c.p, lu.oc.hanning(c.N), lu.SEED)
        for name, v in lu.oracle_checks(engine(lu.pack_input(x, lay), lay), lay, ref, c.N, c.f, c.p, f"dL={dL}").items():
            failed.setdefault(name, f"dL={dL}: {v}")
    return failed


def _part_c(engine, c, contiguous=False):
    """the middle third of the last channel from a buffer that holds its span alone, into one guarded row with a window
    of excess capacity; against the full job's bits"""
    step, total, n_out = _geometry(c)
    w0, w1 = total // 3, 2 * total // 3
    wout = lu.window_out_len(c.N, c.p)
    x = wu.white_input(c.ch, c.L)
    flat = Layout(c.ch, c.L, n_out, c.N, contiguous=True)
    full = lu.rows_of(StandIn(c.N, c.f, c.p)(lu.pack_input(x, flat), flat), flat)
    want = full[c.ch - 1:, w0 * wout:w1 * wout]
    if contiguous:  # what test_window_ranges_... does: the whole input is there, the output has room for the range alone
        out_lay = Layout(1, c.L, (w1 - w0) * wout, c.N, contiguous=True)
        got = engine.range(lu.pack_input(x, flat), flat, c.ch - 1, w0, w1, out_lay, (w1 - w0) * wout)
        return {} if lu.bits_equal(lu.rows_of(got, out_lay), want) else {"bits": "range != full job"}
    lay = Layout(c.ch, c.L, n_out, c.N, *RANGE_OFFSETS)
    lo, hi = lu.range_span(step, c.N, lu.hops_per_window(c.p), w0, w1, c.L)
    out_lay = Layout(1, c.L, (w1 - w0) * wout, c.N, *RANGE_OFFSETS)
    got = engine.range(lu.pack_input(x, lay, keep=(c.ch - 1, lo, hi)), lay, c.ch - 1, w0, w1, out_lay, (w1 - w0) * wout + c.N)
    return lu.hostile_checks(got, out_lay, want)


def _contiguous(engine, c):
    """What the suite had: fresh contiguous buffers, the result alone looked at - held to the oracle under the three
    gates, and a range to the full job."""
    from test_gpu_window_parity import _check

    x = wu.white_input(c.ch, c.L)
    flat = Layout(c.ch, c.L, _geometry(c)[2], c.N, contiguous=True)
    got = lu.rows_of(engine(lu.pack_input(x, flat), flat), flat)
    failed = {}
    try:
        assert np.isfinite(got).all()
        _check(got, wu.oracle_with_window(x, c.N, c.f, c.p, lu.oc.hanning(c.N), lu.SEED), c.N, c.f, c.p, su.case_id(c))
    except AssertionError as e:
        failed["parity"] = str(e)
    failed.update(_part_c(engine, c, contiguous=True))
    return failed


def _refusals(engine, c):
    parts = (("a", _part_a(engine, c, lu.OFFSETS)), ("b", _part_b(engine, c)), ("c", _part_c(engine, c)))
    return {f"{p}:{k}" for p, failed in parts for k in failed}


@pytest.mark.parametrize("c", SMALL, ids=su.case_id)
def test_the_stand_in_passes_every_check(c):
    engine = StandIn(c.N, c.f, c.p)
    lu.assert_none(_part_a(engine, c, lu.OFFSETS), "every base alignment")
    lu.assert_none(_part_a(engine, c, lu.SPECTRUM_OFFSETS), "the four layouts of the spectrum cases")
    lu.assert_none(_part_b(engine, c), "last full hop, first short hop")
    lu.assert_none(_part_b(engine, c, k=0), "a job of one hop")
    lu.assert_none(_part_c(engine, c), "a range reads only its span")
    lu.assert_none(_contiguous(engine, c), "contiguous")


# mutant -> the checks that refuse it, as part:check (a: every alignment, b: the last hops, c: a range). NaN that got
# into a row fails `finite` and with it `bits` / `parity`; a stray store fails `damage` alone: the rows are right.
_NAN_A, _NAN_B, _NAN_C = {"a:finite", "a:bits"}, {"b:finite", "b:parity"}, {"c:finite", "c:bits"}
REFUSED_BY = {
    "tail_reads_x[L]": _NAN_A | _NAN_B,                       # x[L] is POISON (the range of part c ends inside the row)
    "in_stride_is_L": _NAN_A | _NAN_B | _NAN_C,               # row 1 starts in row 0's trailing pad
    "out_stride_is_n_out": {"a:damage", "b:damage"} | _NAN_A | _NAN_B,  # row 1 lands behind row 0, GUARD stays in its place
    "store_past_end": {"a:damage", "b:damage", "c:damage"},
    "store_before_start": {"a:damage", "b:damage", "c:damage"},
    "in_base_8": _NAN_A | _NAN_B | _NAN_C,                    # at an odd offset the row starts one POISON early
    "out_base_8": {"a:damage", "b:damage", "c:damage"} | _NAN_A | _NAN_B | _NAN_C,  # ... and its last word stays GUARD
    "range_reads_lo-1": _NAN_C,
    "range_reads_hi": _NAN_C,
    "range_writes_out_cap": {"c:damage"},
}


@pytest.mark.parametrize("mutant", lu.MUTANTS)
@pytest.mark.parametrize("c", SMALL, ids=su.case_id)
def test_every_mutant_is_refused_in_hostile_buffers_and_passes_in_contiguous_ones(c, mutant):
    engine = StandIn(c.N, c.f, c.p, mutant)
    got = _refusals(engine, c)
    assert got, f"{mutant} passes every check"
    assert got == REFUSED_BY[mutant], (mutant, sorted(got))
    if mutant == "tail_reads_x[L]":
        # The one mutant contiguous buffers do not let through everywhere: x[L] of a row that another row follows is
        # that row's first sample, 0.9 at most under a window weight of a few percent, and the gates see it (1.6e-4
        # of the RMS at N = 64). The LAST row's x[L] is whatever lies behind the allocation - zeros in fresh memory -
        # so a mono job, and the last channel of any job, pass.
        assert set(_contiguous(engine, c)) == {"parity"}
        c = c._replace(ch=1)
    lu.assert_none(_contiguous(engine, c), f"{mutant} in contiguous, aligned buffers")


def test_the_list_of_mutants_is_the_table():
    assert sorted(REFUSED_BY) == sorted(lu.MUTANTS) and len(lu.MUTANTS) == 10
