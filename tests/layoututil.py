"""Helpers of the caller-buffer tests (tests/test_caller_buffers_host.py, tests/test_gpu_caller_buffers.py): device-form
jobs whose rows lie at float-aligned (not 8-byte-aligned) bases and odd strides inside one allocation, with a quiet NaN
in every input word that is no sample and another in every output word before the call; what the checks of the GPU
file are; the input span the header promises for the range form; and a numpy stand-in for the engine that reads and
writes such buffers by base and stride, so that the checks can be shown to pass and to bite on the CPU.
No GPU, no product import."""
import numpy as np

import windowutil as wu
from oracle import cbind as oc
from oracle import oracle_np as onp
from test_gpu_window_parity import _half_window, _reg  # the gates' own block length and regression bound

POISON = 0x7FC00BAD  # input padding: a quiet NaN no computation produces
GUARD = 0xFFC0DEAD   # output buffers before the call: another one
ALIGN = 256          # bytes: what the tests assert of an allocation's base
SLACK = ALIGN // 4   # floats an allocator leaves around a contiguous tensor (the model of the contiguous layout)
OFFSETS = [(i, o) for i in range(4) for o in range(4)]
SPECTRUM_OFFSETS = [(1, 2), (2, 3), (3, 1), (0, 0)]
SEED = 3


def _odd_at_least(n):
    return n | 1


def aligned_words(n, fill):
    """uint32 [n] whose first byte is 256-byte aligned, every word `fill`"""
    raw = np.empty(n + SLACK, np.uint32)
    a = raw[(-(raw.ctypes.data // 4)) % SLACK:][:n]
    assert a.ctypes.data % ALIGN == 0 and a.size == n
    a[:] = np.uint32(fill)
    return a


class Layout:
    """Where the rows of a [ch, L] -> [ch, n_out] job lie in two flat allocations of floats. Hostile: row c of the input
    starts N + in_off + c in_stride floats into its allocation, in_stride the smallest odd number >= L + N + 1, so
    rows alternate between 4 and 8 byte alignment and at least a window of padding lies on each side of every row, the
    last included; the output alike with out_off and n_out. contiguous=True is what every other GPU test hands over:
    stride == row length, an aligned first row, nothing between the rows - and SLACK floats the caller never looks at
    on both sides, which stand for whatever the allocator has there."""

    def __init__(self, ch, L, n_out, N, in_off=0, out_off=0, contiguous=False):
        assert 0 <= in_off <= 3 and 0 <= out_off <= 3 and ch >= 1
        self.ch, self.L, self.n_out, self.N, self.contiguous = ch, L, n_out, N, contiguous
        if contiguous:
            assert in_off == out_off == 0
            self.in_base = self.out_base = SLACK
            self.in_stride, self.out_stride = L, n_out
            self.in_words, self.out_words = 2 * SLACK + ch * L, 2 * SLACK + ch * n_out
        else:
            self.in_base, self.out_base = N + in_off, N + out_off
            self.in_stride, self.out_stride = _odd_at_least(L + N + 1), _odd_at_least(n_out + N + 1)
            self.in_words = self.in_base + ch * self.in_stride
            self.out_words = self.out_base + ch * self.out_stride

    def in_row(self, c):
        return self.in_base + c * self.in_stride

    def out_row(self, c):
        return self.out_base + c * self.out_stride


def pack_input(x, lay, keep=None):
    """uint32 [lay.in_words]: the rows of x (float32 [ch, L]) in their places, POISON in every other word (zeros in the
    slack of the contiguous layout: fresh memory). keep=(row, lo, hi): that row's samples [lo, hi) only, POISON in every
    other word of every row as well."""
    x = np.ascontiguousarray(x, np.float32)
    assert x.shape == (lay.ch, lay.L)
    buf = aligned_words(lay.in_words, 0 if lay.contiguous else POISON)
    for c in range(lay.ch):
        r = lay.in_row(c)
        if keep is None:
            buf[r:r + lay.L] = x[c].view(np.uint32)
        else:
            buf[r:r + lay.L] = np.uint32(POISON)
            if c == keep[0]:
                buf[r + keep[1]:r + keep[2]] = x[c, keep[1]:keep[2]].view(np.uint32)
    return buf


def blank_output(lay):
    return aligned_words(lay.out_words, GUARD)


def rows_of(buf, lay):
    """float32 [ch, n_out]: the output rows (a copy)"""
    buf = np.asarray(buf).view(np.uint32)
    assert buf.shape == (lay.out_words,)
    return np.stack([buf[lay.out_row(c):lay.out_row(c) + lay.n_out] for c in range(lay.ch)]).view(np.float32)


def first_damage(buf, lay):
    """None, or (row, offset) of the first word outside the rows that is no longer GUARD: offset -1 is the word in front
    of the row's first sample, +1 the word behind its last; a word between two rows goes to the nearer end."""
    buf = np.asarray(buf).view(np.uint32)
    assert buf.shape == (lay.out_words,)
    outside = np.ones(lay.out_words, bool)
    for c in range(lay.ch):
        outside[lay.out_row(c):lay.out_row(c) + lay.n_out] = False
    bad = np.flatnonzero(outside & (buf != np.uint32(GUARD)))
    if bad.size == 0:
        return None
    i = int(bad[0])
    best = None
    for c in range(lay.ch):
        a, b = lay.out_row(c), lay.out_row(c) + lay.n_out
        off = i - a if i < a else i - b + 1
        if best is None or abs(off) < abs(best[1]):
            best = (c, off)
    return best


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def hostile_checks(out_buf, lay, want_rows):
    """The checks of a run in a hostile layout -> the names of those that fail: guards (`damage`), `finite` rows, rows
    equal to `want_rows` bit for bit (`bits`). Each comes with what it saw."""
    failed = {}
    d = first_damage(out_buf, lay)
    if d is not None:
        failed["damage"] = f"stray store at row {d[0]} offset {d[1]:+d}"
    rows = rows_of(out_buf, lay)
    if not np.isfinite(rows).all():
        c, t = (int(v) for v in np.argwhere(~np.isfinite(rows))[0])
        failed["finite"] = f"{np.count_nonzero(~np.isfinite(rows))} samples not finite, first at row {c} sample {t}"
    if not bits_equal(rows, want_rows):
        bad = np.argwhere(rows.view(np.uint32) != np.ascontiguousarray(want_rows, np.float32).view(np.uint32))
        c, t = (int(v) for v in bad[0])
        failed["bits"] = f"{len(bad)} of {rows.size} samples differ, first at row {c} sample {t}"
    return failed


def oracle_checks(out_buf, lay, ref, N, f, p, what=""):
    """The checks of a run whose expected value is the oracle's `ref` (f64 [ch, n_out]): guards, `finite` rows, and
    `parity`: the contract and the regression gate per channel (windowutil.assert_parity with the project's _reg) and
    the per-block bound over half windows wherever the output holds a block. Prints the figures first."""
    failed = {}
    d = first_damage(out_buf, lay)
    if d is not None:
        failed["damage"] = f"stray store at row {d[0]} offset {d[1]:+d}"
    rows = rows_of(out_buf, lay)
    if not np.isfinite(rows).all():
        c, t = (int(v) for v in np.argwhere(~np.isfinite(rows))[0])
        failed["finite"] = f"{np.count_nonzero(~np.isfinite(rows))} samples not finite, first at row {c} sample {t}"
    block = _half_window(N, p)
    with np.errstate(invalid="ignore"):
        print(f"\nFIGURES {what}: rel {max(wu.rel_err(rows[c], ref[c]) for c in range(lay.ch)):.2e}")
        try:
            assert rows.shape == ref.shape, (rows.shape, ref.shape)
            for c in range(lay.ch):
                wu.assert_parity(rows[c], ref[c], f"{what} ch{c}", reg=_reg(N, f))
            if rows.shape[-1] >= block:
                wu.assert_blocks(rows, ref, block, what)
        except AssertionError as e:
            failed["parity"] = str(e)
    return failed


def assert_none(failed, what):
    assert not failed, f"{what}: " + "; ".join(f"{k}: {v}" for k, v in failed.items())


# ------------------------------------------------------------------ geometry, restated
def hops_per_window(p):
    return 2 * p if p >= 1 else 1  # ceil(S / (N - H)) with S = N p, or S = ceil(N / |p|) <= H


def window_out_len(N, p):
    return N if p >= 1 else (-(-N // -p) - 1) * -p


def total_windows(L, N, step, p):
    kd = (L - N) // step + 1 if L >= N else 0  # the first hop whose window runs past the input
    return kd // hops_per_window(p) + 1


def range_span(step, N, hpw, w0, w1, L):
    """[lo, hi) of the input that windows [w0, w1) read: include/rocoder_hip.h, "the one-hop overlap is recomputed
    locally" - the hops of the range and the one in front of them, cut at the end of the input."""
    return max(0, w0 * hpw - 1) * step, min(L, (w1 * hpw - 1) * step + N)


# ------------------------------------------------------------------ a numpy stand-in for the engine
MUTANTS = ["tail_reads_x[L]", "in_stride_is_L", "out_stride_is_n_out", "store_past_end", "store_before_start",
           "in_base_8", "out_base_8", "range_reads_lo-1", "range_reads_hi", "range_writes_out_cap"]


class StandIn:
    """(in_buf, layout) -> out_buf like rc_engine_stretch_device, and .range(...) like rc_engine_stretch_device_range:
    rows taken from the flat input by base and stride, the oracle (windowutil.oracle_with_window, default window),
    rows put into a GUARD-filled flat output by base and stride. `mutant` makes one of the addressing mistakes the
    checks are there for. A stray read is modelled by a value that ENTERS the arithmetic (times zero where the right
    result must not move): a read whose value is dropped is invisible to any test without a fault."""

    _memo = {}

    def __init__(self, N, f, p, mutant=None):
        assert mutant is None or mutant in MUTANTS
        self.N, self.f, self.p, self.mutant = N, f, p, mutant
        self.step = onp.derive(N, f, 1.0, p)["step"]
        self.hpw, self.wout = hops_per_window(p), window_out_len(N, p)

    def _oracle(self, x):
        key = (self.N, self.f, self.p, x.shape, x.tobytes())
        if key not in self._memo:
            y = wu.oracle_with_window(x, self.N, self.f, self.p, oc.hanning(self.N), SEED).astype(np.float32)
            y.setflags(write=False)
            self._memo[key] = y
        return self._memo[key]

    def _read_rows(self, in_buf, lay, length):
        m = self.mutant
        base = lay.in_base & ~1 if m == "in_base_8" else lay.in_base  # (the allocation is 256-byte aligned)
        stride = lay.L if m == "in_stride_is_L" else lay.in_stride
        return np.stack([in_buf[base + c * stride:][:length] for c in range(lay.ch)]).view(np.float32)

    def _write_rows(self, out, lay, rows, first_row=0):
        m = self.mutant
        base = lay.out_base & ~1 if m == "out_base_8" else lay.out_base
        stride = lay.n_out if m == "out_stride_is_n_out" else lay.out_stride
        words = np.ascontiguousarray(rows, np.float32).view(np.uint32)
        at = [base + (first_row + i) * stride for i in range(len(words))]
        for a, w in zip(at, words):  # (strays first: a neighbouring row is written over them "a moment later")
            if m == "store_past_end":
                out[a + w.size] = w[-1]
            if m == "store_before_start":
                out[a - 1] = w[0]
        for a, w in zip(at, words):
            out[a:a + w.size] = w
        return out

    def __call__(self, in_buf, lay):
        in_buf = np.asarray(in_buf).view(np.uint32)
        assert in_buf.shape == (lay.in_words,)
        n_in = lay.L + 1 if self.mutant == "tail_reads_x[L]" else lay.L  # (the zero padding starts one sample late)
        with np.errstate(invalid="ignore"):
            y = self._oracle(self._read_rows(in_buf, lay, n_in))[:, :lay.n_out]
        assert y.shape == (lay.ch, lay.n_out), (y.shape, lay.n_out)
        return self._write_rows(blank_output(lay), lay, y)

    def range(self, in_buf, lay, ch_first, w0, w1, out_lay, out_cap):
        """windows [w0, w1) of channel ch_first into the one row of out_lay; reads range_span of that row alone"""
        in_buf = np.asarray(in_buf).view(np.uint32)
        assert out_lay.ch == 1 and out_lay.n_out == (w1 - w0) * self.wout <= out_cap
        lo, hi = range_span(self.step, self.N, self.hpw, w0, w1, lay.L)
        base = lay.in_base & ~1 if self.mutant == "in_base_8" else lay.in_base
        stride = lay.L if self.mutant == "in_stride_is_L" else lay.in_stride
        row = in_buf[base + ch_first * stride:].view(np.float32)
        # (the channel index is part of the phase key: the oracle runs on all rows, the others silent)
        xs = np.zeros((lay.ch, lay.L), np.float32)
        xs[ch_first, lo:hi] = row[lo:hi]
        with np.errstate(invalid="ignore"):
            y = self._oracle(xs)[ch_first, w0 * self.wout:w1 * self.wout].copy()
            if self.mutant == "range_reads_lo-1" and lo > 0:
                y[0] += np.float32(0.0) * row[lo - 1]
            if self.mutant == "range_reads_hi":
                y[-1] += np.float32(0.0) * row[hi]
        if self.mutant == "range_writes_out_cap":
            y = np.concatenate([y, np.zeros(out_cap - y.size, np.float32)])
        return self._write_rows(blank_output(out_lay), out_lay, y[None, :])
