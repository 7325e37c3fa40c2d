"""GPU parity tests (-m gpu) of the device-form entries - rc_engine_stretch_device, rc_engine_stretch_device_range,
rc_multi_stretch_device, where the CALLER owns the buffers - in buffers no other test hands over: rows at every
float-aligned base (4 but not 8 bytes aligned included) and odd strides inside one allocation, a quiet NaN in every
input word that is no sample (POISON) and another in every output word before the call (GUARD). Every kernel path of
tests/signalutil.py: CASES, white input.

The hop kernels never bounds-check: which hops read the zero-padded tail copy, where a row starts and how much input a
range needs is host arithmetic. A read of x[L], a store one pair past a row, in_len where in_stride belongs or an
8-byte assumption about a base all stay inside a contiguous allocation and pass every other test
(tests/test_caller_buffers_host.py shows that on the CPU, and that the checks used here refuse each of them). Here
such a read turns the output into NaN and such a store breaks a guard word, named by row and offset
("Parity on the caller's buffers")."""
import numpy as np
import pytest

import layoututil as lu
import signalutil as su
import windowutil as wu
from layoututil import Layout
from oracle import cbind as oc
from test_gpu_window_parity import _check, _engine_mod

pytestmark = pytest.mark.gpu


def _engine(ra, c):
    return ra.Engine(window_len=c.N, factor=c.f, pitch_multiple=c.p, channels=c.ch, seed=su.SEED, **su.engine_kwargs(c))


def _to_device(words):
    """uint32 words -> one flat float32 device tensor with the same bits, at a 256-byte aligned base"""
    import torch

    t = torch.from_numpy(words.view(np.int32)).cuda().view(torch.float32)
    assert t.data_ptr() % lu.ALIGN == 0 and t.numel() == words.size
    return t


def _to_host(t):
    import torch

    return t.view(torch.int32).cpu().numpy().view(np.uint32)


def _views(fin, fout, lay):
    """the rows of a layout as strided views of the two flat tensors: data_ptr() and stride(0) are the layout's"""
    x = fin.as_strided((lay.ch, lay.L), (lay.in_stride, 1), lay.in_base)
    out = fout.as_strided((lay.ch, lay.n_out), (lay.out_stride, 1), lay.out_base)
    assert x.data_ptr() == fin.data_ptr() + 4 * lay.in_base and out.data_ptr() == fout.data_ptr() + 4 * lay.out_base
    assert (x.stride(0), out.stride(0)) == (lay.in_stride, lay.out_stride) and x.stride(1) == out.stride(1) == 1
    return x, out


def _run_in_layout(engine, x, lay):
    """x [ch, L] through engine.stretch_tensor (Engine or MultiEngine) in the layout -> the whole output allocation.
    stretch_tensor orders the call by hand on the legacy default stream (torch's stream synchronised before, the engine
    after) and raises unless the call returns RC_OK."""
    import torch

    fin, fout = _to_device(lu.pack_input(x, lay)), _to_device(lu.blank_output(lay))
    xv, ov = _views(fin, fout, lay)
    assert torch.cuda.current_stream().cuda_stream == 0
    got = engine.stretch_tensor(xv, out=ov)
    assert got.data_ptr() == ov.data_ptr()
    torch.cuda.synchronize()
    return _to_host(fout)


def _contiguous(e, x):
    import torch

    return e.stretch_tensor(torch.from_numpy(x).cuda()).cpu().numpy()


# ------------------------------------------------------------------ (a) every path at every base alignment
@pytest.mark.parametrize("c", su.CASES, ids=su.case_id)
def test_every_path_at_every_base_alignment(c):
    """The contiguous device-form run against the oracle under the three gates of tests/test_gpu_window_parity.py; then
    the same job with input and output rows at every offset of 0 .. 3 floats and odd strides (four of the sixteen
    layouts where a host kernel is a Python call per hop): RC_OK, every guard word intact, finite, and the contiguous
    run's bits - a sample's bits depend on neither launch, range nor tile, and an address is less than any of these."""
    ra = _engine_mod()
    x = su.make_input(c, "white")
    with _engine(ra, c) as e:
        base = _contiguous(e, x)
        _check(base, su.reference(c, "white"), c.N, c.f, c.p, su.case_id(c))
        for in_off, out_off in (lu.OFFSETS if c.spec is None else lu.SPECTRUM_OFFSETS):
            lay = Layout(c.ch, c.L, base.shape[1], c.N, in_off, out_off)
            lu.assert_none(lu.hostile_checks(_run_in_layout(e, x, lay), lay, base), f"{su.case_id(c)} at ({in_off}, {out_off})")


TABLE_WINDOW = [(512, 2.0, 5, 1, 9000, "skew"), (2048, 8.0, 1, 2, 30000, "skew"), (4096, 0.25, 1, 2, 100000, "ramp"),
                (8192, 2.0, 2, 3, 60001, "skew"), (16384, 8.0, 1, 2, su.L16, "ramp"), (16384, 8.0, 3, 2, su.L16, "ramp"),
                (32768, 8.0, 2, 2, 3 * 32768 + 777, "ramp"), (65536, 16.0, 1, 2, 3 * 65536 + 777, "skew")]


@pytest.mark.parametrize("N,f,p,ch,L,name", TABLE_WINDOW)
def test_table_window_instantiations_at_odd_alignment(N, f, p, ch, L, name):
    """CASES run the default window. With a caller's window the wave-local kernels, hop4 / hop2 and big5s / big5 are
    other instantiations, which load through plain pointers and store `v2f` pairs where the default ones use buffer
    accesses (tests/test_gpu_window_parity.py holds their contiguous result to the oracle, case by case): the four
    layouts of the spectrum cases, guards intact, finite, the contiguous run's bits."""
    ra = _engine_mod()
    x = wu.white_input(ch, L)
    with ra.Engine(window_len=N, factor=f, pitch_multiple=p, channels=ch, seed=su.SEED, window=wu.WINDOWS[name](N)) as e:
        base = _contiguous(e, x)
        assert np.isfinite(base).all() and base.shape == (ch, e.output_len(L))
        for in_off, out_off in lu.SPECTRUM_OFFSETS:
            lay = Layout(ch, L, base.shape[1], N, in_off, out_off)
            lu.assert_none(lu.hostile_checks(_run_in_layout(e, x, lay), lay, base), f"N={N} p={p} {name} at ({in_off}, {out_off})")


# ------------------------------------------------------------------ (b) the last full hop and the first short hop
def _one_per_family():
    seen = {}
    for c in su.CASES:
        if c.spec is None:
            seen.setdefault(c.path, c)
    assert sorted(seen) == ["16384", "chirpz", "generic", "long", "negative", "quarter", "wave"]
    return list(seen.values())


TAIL_CASES = [(c, 5) for c in su.CASES] + [(c, 0) for c in _one_per_family()]


@pytest.mark.parametrize("dL", [-1, 0, 1])
@pytest.mark.parametrize("c,k", TAIL_CASES, ids=[f"{su.case_id(c)}-k{k}" for c, k in TAIL_CASES])
def test_last_full_hop_and_first_short_hop(c, k, dL):
    """L = k step + N + dL: at dL = 0 hop k ends on the input's last sample and hop k + 1 is the first short one, at -1
    hop k is, at +1 one sample of hop k + 1 is real. Layout (1, 1), so x[L] is POISON: a last full hop that reads one
    sample too many, or a first short hop read from x instead of the tail copy, is NaN in the output. The expected
    value is the oracle's at that L (the engine's own contiguous run would share an off-by-one in the first short hop):
    the contract and the regression gate per channel, the block gate wherever the output holds a block."""
    ra = _engine_mod()
    step = su.geometry(c)[0]
    L = k * step + c.N + dL
    x = wu.white_input(c.ch, L)
    ref = wu.oracle_with_window(x, c.N, c.f, c.p, oc.hanning(c.N), su.SEED, kernel=su.oracle_kernel(c))
    what = f"{su.case_id(c)} L={L} (k={k}, dL={dL:+d})"
    with _engine(ra, c) as e:
        assert e.output_len(L) == ref.shape[1], what
        lay = Layout(c.ch, L, ref.shape[1], c.N, 1, 1)
        lu.assert_none(lu.oracle_checks(_run_in_layout(e, x, lay), lay, ref, c.N, c.f, c.p, what), what)


# ------------------------------------------------------------------ (c) a range reads only its span
RANGE_CASES = [c for c in su.CASES if c.spec != "host"]  # (a stateful apply() carries its tail: no hop is recomputed)


@pytest.mark.parametrize("c", RANGE_CASES, ids=su.case_id)
def test_a_range_reads_only_its_span(c):
    """The middle third of the LAST channel's windows from a buffer in which everything but layoututil.range_span of
    that row is POISON - the other channels' rows too - into one guarded row with a window of capacity to spare: the
    contiguous full job's bits, and the excess still GUARD. The header's promise for the range form ("the one-hop
    overlap is recomputed locally"), which is also how much input a remote device of rc_multi is sent."""
    import torch

    ra = _engine_mod()
    x = su.make_input(c, "white")
    with _engine(ra, c) as e:
        par = e.params
        step, hpw, wout = par.sample_step_len, par.hops_per_window, par.window_out_len
        full = _contiguous(e, x)
        total = full.shape[1] // wout
        w0, w1 = total // 3, 2 * total // 3
        assert w0 >= 2 and w1 > w0 and total * wout == full.shape[1]
        count = w1 - w0
        lo, hi = lu.range_span(step, c.N, hpw, w0, w1, c.L)
        lay = Layout(c.ch, c.L, full.shape[1], c.N, 1, 3)
        out_lay = Layout(1, c.L, count * wout, c.N, 1, 3)
        fin = _to_device(lu.pack_input(x, lay, keep=(c.ch - 1, lo, hi)))
        fout = _to_device(lu.blank_output(out_lay))
        torch.cuda.synchronize()
        e.stretch_device_range_ptr(fin.data_ptr() + 4 * lay.in_base, lay.in_stride, c.L, c.ch - 1, 1, w0, count,
                                   fout.data_ptr() + 4 * out_lay.out_base, out_lay.out_stride, count * wout + c.N)
        e.synchronize()
        lu.assert_none(lu.hostile_checks(_to_host(fout), out_lay, full[c.ch - 1:, w0 * wout:w1 * wout]),
                       f"{su.case_id(c)} windows [{w0}, {w1}) of {total}: input [{lo}, {hi}) of {c.L}")


# ------------------------------------------------------------------ (d) rc_multi
MULTI_CASES = [c for c in su.CASES if c.spec is None and (c.N, c.f, c.p, c.ch) in ((16384, 8.0, 1, 2), (1024, 4.0, 3, 1))]


@pytest.mark.parametrize("c", MULTI_CASES, ids=su.case_id)
def test_multi_device_form_in_hostile_buffers(c):
    """rc_multi_stretch_device on two and three shares of ONE device with forced staging, so that every share takes a
    remote device's path: its input span copied out of the caller's rows, its shard copied into them. Layout (3, 1):
    one engine's bits, every guard word intact."""
    ra = _engine_mod()
    assert len(MULTI_CASES) == 2
    x = su.make_input(c, "white")
    with _engine(ra, c) as e:
        one = _contiguous(e, x)
    lay = Layout(c.ch, c.L, one.shape[1], c.N, 3, 1)
    for ids in ([0, 0], [0, 0, 0]):
        with ra.MultiEngine(ids, window_len=c.N, factor=c.f, pitch_multiple=c.p, channels=c.ch, seed=su.SEED) as m:
            m.set_staging(True)
            lu.assert_none(lu.hostile_checks(_run_in_layout(m, x, lay), lay, one), f"{su.case_id(c)} on {ids}")
