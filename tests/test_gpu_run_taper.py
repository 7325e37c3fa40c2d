"""The tapered run plan of the fused N = 16384 kernel (hop4_kernel, HopParams::run_first). Where the run seams lie does not change a bit of the output - the
hand-over performs the same additions in the same order - so every check here is bit equality: with the same job
planned without the taper (the test-hook library's ROCODER_TAPER=-1), with the unsharded job, with the first launch."""
import ctypes as C

import numpy as np
import pytest

from oracle import cbind as oc
from oracle import oracle_np as onp
from test_gpu_parity import _engine_mod, assert_parity

pytestmark = pytest.mark.gpu

N, FACTOR, SEED = 16384, 8.0, 0x7A9E
# 7 000 hops per channel (the step is 1024 samples): runs of 10 hops, 1.8 rounds of the 768 workgroup slots at two
# channels - every XCD's span has a body and a taper
L_TAPER = 7_000 * 1024
L_PREFIX = 600_000
_inputs = {}


def _x(channels, length):
    for c in range(channels):
        if c not in _inputs or _inputs[c].size < length:
            _inputs[c] = onp.synth_input(c, max(length, L_TAPER))
    return np.stack([_inputs[c][:length] for c in range(channels)])


def _oracle(x, pitch, window):
    if window is None:
        return oc.stretch_offline(x, N, FACTOR, 1.0, pitch, seed=SEED)
    chans = []
    for c in range(x.shape[0]):
        st = oc.Stretcher(channels=x.shape[0], factor=FACTOR, pitch_multiple=pitch, window=window, seed=SEED, channel_index=c)
        st.send(x[c])
        st.close_input()
        wins = []
        while not st.is_done():
            wins.append(st.next_window())
        chans.append(np.concatenate(wins))
    return np.stack(chans)


def _plan(e):
    """(runs, body length, shortest run) of the engine's last launch (test-hook library)."""
    from rocoder_amd import _lib

    with _lib.hooks_library() as Lh:
        fn = Lh.rc_test_last_run_plan
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p] + [C.POINTER(C.c_uint32)] * 3
    r, b, s = C.c_uint32(), C.c_uint32(), C.c_uint32()
    assert fn(e._h, C.byref(r), C.byref(b), C.byref(s)) == 0
    return r.value, b.value, s.value


def _engines(monkeypatch, **kw):
    """A tapered engine and one planned without taper, both of the test-hook build (it alone reads ROCODER_TAPER)."""
    from rocoder_amd import _lib

    ra = _engine_mod()
    with _lib.hooks_library():
        monkeypatch.delenv("ROCODER_TAPER", raising=False)
        tapered = ra.Engine(window_len=N, factor=FACTOR, seed=SEED, **kw)
        monkeypatch.setenv("ROCODER_TAPER", "-1")
        plain = ra.Engine(window_len=N, factor=FACTOR, seed=SEED, **kw)
        monkeypatch.delenv("ROCODER_TAPER")
    return tapered, plain


def _check_taper(monkeypatch, channels, pitch=1, window=None):
    import torch

    x = _x(channels, L_TAPER)
    xt = torch.from_numpy(x).cuda()
    kw = dict(channels=channels, pitch_multiple=pitch)
    if window is not None:
        kw["window"] = window
    tapered, plain = _engines(monkeypatch, **kw)
    with tapered, plain:
        want = plain.stretch_tensor(xt).clone()
        torch.cuda.synchronize()
        runs0, body0, short0 = _plan(plain)
        assert short0 == body0, "the partner has runs of one length"
        for rep in range(2):  # (the second launch finds the counters as the first one left them)
            got = tapered.stretch_tensor(xt)
            torch.cuda.synchronize()
            runs, body, shortest = _plan(tapered)
            assert body == body0 and shortest < body and runs > runs0, (runs, body, shortest, runs0)
            assert torch.equal(got, want), f"launch {rep}"
        # the prefix job against the oracle, and the long job's output where the two jobs run the same hops
        ref = _oracle(x[:, :L_PREFIX], pitch, window)
        pre = tapered.stretch_tensor(torch.from_numpy(np.ascontiguousarray(x[:, :L_PREFIX])).cuda()).cpu().numpy()
        assert_parity(pre, ref, f"prefix job, {channels} channels, pitch {pitch}")
        same = ref.shape[1] // 2
        assert_parity(got[:, :same].cpu().numpy(), ref[:, :same], f"long job's first samples, {channels} channels, pitch {pitch}")


def test_two_channels_body_and_taper_on_every_span(monkeypatch):
    _check_taper(monkeypatch, 2)


@pytest.mark.parametrize("pitch", [1, 3])
def test_three_channels_a_channel_ends_inside_a_span(monkeypatch, pitch):
    _check_taper(monkeypatch, 3, pitch=pitch)


def test_callers_window(monkeypatch):
    w = (np.hanning(N) ** 1.5).astype(np.float32)  # (the table-window instantiation of the kernel, pitch 1)
    _check_taper(monkeypatch, 2, window=w)


def test_two_shards_of_one_channel_equal_the_unsharded_job(monkeypatch):
    import torch

    from rocoder_amd.distributed import Shard, engine_compute

    from rocoder_amd import _lib

    ra = _engine_mod()
    # one channel of 16 000 hops: the whole job (1 455 runs of 11 hops before the taper) and the second shard (14 000
    # hops from hop 2 000 on) each get a taper of their own, the first shard (one round) gets none
    xt = torch.from_numpy(_x(1, 16_000 * 1024)).cuda()
    with _lib.hooks_library(), ra.Engine(window_len=N, factor=FACTOR, channels=1, seed=SEED) as e:
        full = e.stretch_tensor(xt).clone()
        torch.cuda.synchronize()
        assert _plan(e)[2] < _plan(e)[1]
        wout = e.params.window_out_len
        nwin = full.shape[1] // wout
        comp = engine_compute(e, xt)
        out = torch.zeros_like(full)
        cut = nwin // 8
        for s, tapered in ((Shard(0, 0, 1, 0, cut), False), (Shard(1, 0, 1, cut, nwin - cut), True)):
            out[:, s.win_first * wout:(s.win_first + s.win_count) * wout] = comp(s)
            assert (_plan(e)[2] < _plan(e)[1]) == tapered
        torch.cuda.synchronize()
        assert torch.equal(out, full)


@pytest.mark.parametrize("hops", [256, 2])
def test_short_jobs_keep_their_plan(monkeypatch, hops):
    """2 x 256 hops and 2 x 2 hops: no table, no taper - the plan and the bits of the engine that never tapers."""
    import torch

    ra = _engine_mod()
    xt = torch.from_numpy(_x(2, {256: 270 * 1024, 2: 2 * 1024}[hops])).cuda()
    new, old = _engines(monkeypatch, channels=2)
    with old, new:
        assert new.output_len(xt.shape[1]) == hops * (N // 2)
        want = old.stretch_tensor(xt).clone()
        torch.cuda.synchronize()
        plan_old = _plan(old)
        for rep in range(3):
            got = new.stretch_tensor(xt)
            torch.cuda.synchronize()
            assert _plan(new) == plan_old and plan_old[1] == plan_old[2]
            assert torch.equal(got, want), f"launch {rep}"


def test_back_to_back_launches_and_two_engines_on_two_streams():
    """The ticket counters and the seam flags from launch to launch: twenty launches in a row on one stream, then two
    engines on two streams at the same time, each with its own counters - every launch gives the first one's bits."""
    import torch

    ra = _engine_mod()
    xt = torch.from_numpy(_x(2, 3_000_000)).cuda()
    with ra.Engine(window_len=N, factor=FACTOR, channels=2, seed=SEED) as e1, \
            ra.Engine(window_len=N, factor=FACTOR, channels=2, seed=SEED) as e2:
        ref = e1.stretch_tensor(xt).clone()
        torch.cuda.synchronize()
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        outs = [torch.empty_like(ref) for _ in range(20)]
        with torch.cuda.stream(s1):
            for o in outs:
                e1.stretch_tensor(xt, out=o)
        s1.synchronize()
        e1.synchronize()
        for i, o in enumerate(outs):
            assert torch.equal(o, ref), f"launch {i} of 20"
        o1, o2 = outs[0], outs[1]
        for rep in range(4):
            o1.fill_(float("nan"))
            o2.fill_(float("nan"))
            torch.cuda.synchronize()
            with torch.cuda.stream(s1):
                for _ in range(2 + rep % 2):
                    e1.stretch_tensor(xt, out=o1)
            with torch.cuda.stream(s2):
                for _ in range(3 - rep % 2):
                    e2.stretch_tensor(xt, out=o2)
            s1.synchronize()
            s2.synchronize()
            e1.synchronize()
            e2.synchronize()
            assert torch.equal(o1, ref) and torch.equal(o2, ref), f"repetition {rep}"
