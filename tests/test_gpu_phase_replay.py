"""GPU tests of the phase modes stage by stage ("Replay"): rc_test_phase_tap of the test-hook library copies out
the rows a phase-mode job holds in device memory between its launches - the analysis spectra, the composed maps and base
states, the rotated spectra, the y rows - and the verifiers of tests/phaseutil.py check every stage in float64 against the
stage in front of it as the GPU left it. The comparison does not depend on the conditioning of the definition, so any
input is admissible: white noise, clicks, silence, DC, a signal that stops, every window length 32 ... 16384 (every
instantiation of hop_kernel<LOG2N, MODE_RESYNTH_KEEP>), the factors whose H / step is no integer, 1 to 5 channels, a
caller's window, the edge lengths. A stage that fails names its kernel: S1 the analysis, S2 phase_prep / phase_scan /
phase_walk, S3 phase_apply, S4 the KEEP synthesis, S5 the overlap-add. tests/test_phase_host.py holds the verifiers to the
same cases first, and to the mutants each of them must catch."""
import numpy as np
import pytest

import phaseutil as pu

import rocoder_amd
from rocoder_amd import _lib

pytestmark = pytest.mark.gpu


def _job(eng, x):
    """a whole-job call; a device error ends the session (nothing more is launched on a device in that state)"""
    try:
        out = eng.stretch_host(x).copy()
        eng.synchronize()
    except rocoder_amd.RocoderError as err:
        if err.code == _lib.RC_EHIP:
            pytest.exit(f"stretch_host: {err}; no further launches on this device", returncode=3)
        raise
    return out


def _replay(c):
    """the case with the budget's chunk and with chunks of hops_per_window: (RANDOM's shape, the untapped output, [(output,
    Tap)] of the two tapped runs)"""
    x = pu.replay_input(c)
    g = pu.geometry(c.N, c.f, c.p, c.L)
    with _lib.hooks_library():
        H = pu.hooks()
        eng = rocoder_amd.Engine(window_len=c.N, factor=c.f, pitch_multiple=c.p, channels=c.ch, seed=7, window=pu.case_window(c.N, c.window))
        assert eng.params.hops_per_window == g["hpw"] and eng.params.sample_step_len == g["step"]
        shape = _job(eng, x).shape
        eng.set_phase_mode(c.mode)
        plain = _job(eng, x)
        runs = []
        for chunk in (0, g["hpw"]):
            assert H.rc_test_phase_chunk_hops(eng._h, chunk) == 0
            tap = pu.Tap(c.N, c.ch, g["hops"], chunk or g["hops"])
            _lib.check(tap.set(eng), H)
            out = _job(eng, x)
            _lib.check(pu.Tap.clear(eng), H)
            runs.append((out, tap))
        eng.close()
    return x, g, shape, plain, runs


@pytest.mark.parametrize("case", pu.REPLAY_CASES, ids=pu.replay_id)
def test_every_stage_replays(case):
    c = case
    x, g, shape, plain, runs = _replay(c)
    (whole, tap_whole), (cut, tap_cut) = runs
    # a defined result of RANDOM's shape, L = 0 included; the tap and the chunking change no bit of it
    assert plain.shape == shape and np.isfinite(plain).all()
    assert whole.tobytes() == plain.tobytes(), "the output with the tap set differs from the output without it"
    assert cut.tobytes() == plain.tobytes()
    assert len(tap_cut.table()) == g["hops"] // g["hpw"] and len(tap_whole.table()) >= 1  # seams and halo inside the signal
    rows, rows_whole = tap_cut.rows(cut), tap_whole.rows(whole)
    for name in ("X", "theta", "Z", "y"):
        assert getattr(rows, name).tobytes() == getattr(rows_whole, name).tobytes(), f"the {name} rows depend on the chunking"
    fig = pu.verify(rows, x, c.N, c.f, c.p, c.mode, window=pu.case_window(c.N, c.window), what=pu.replay_id(c))
    assert set(fig) == {"S1", "S2", "S3", "S4", "S5"}


def test_the_tap_refuses_a_job_that_does_not_fit_and_cuts_nothing_short():
    c = [c for c in pu.REPLAY_CASES if c.group == "factor" and c.f == 2.0 and c.mode == pu.PROPAGATE][0]
    x = pu.replay_input(c)
    g = pu.geometry(c.N, c.f, c.p, c.L)
    with _lib.hooks_library():
        H = pu.hooks()
        eng = rocoder_amd.Engine(window_len=c.N, factor=c.f, pitch_multiple=c.p, channels=c.ch, seed=7)
        eng.set_phase_mode(c.mode)
        want = _job(eng, x)
        tap = pu.Tap(c.N, c.ch, g["hops"], g["hops"])
        # what the job's one chunk takes: spectra, map words, base words (one block's at the least), rotated spectra, samples, rows
        rows, nb = c.ch * g["hops"], c.N // 2 + 1
        need = [rows * c.N * 2, rows * 2 * nb, c.ch * nb, rows * c.N * 2, rows * c.N, 1]
        full = [need[0], need[1], tap.base.size, need[3], need[4], 1]
        for short in range(6):
            caps = list(full)
            caps[short] = need[short] - 1
            _lib.check(tap.set(eng, caps), H)
            with pytest.raises(rocoder_amd.RocoderError) as ei:
                eng.stretch_host(x)
            assert ei.value.code == _lib.RC_EINVAL and "rc_test_phase_tap" in str(ei.value)
            assert int(tap.count[0]) == 0 and np.isnan(tap.spec).all() and np.isnan(tap.y).all()  # nothing was written
        _lib.check(tap.set(eng, full), H)  # exactly the job's rows: it fits
        assert _job(eng, x).tobytes() == want.tobytes() and int(tap.count[0]) == 1
        _lib.check(pu.Tap.clear(eng), H)
        assert _job(eng, x).tobytes() == want.tobytes()
        eng.close()
