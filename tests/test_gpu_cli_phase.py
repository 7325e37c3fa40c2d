"""GPU tests of the CLI's --phase (--frames-on-gpu): the run writes the file the Python API gives under the same mode, the
report line names the mode and the hops, --pitch-cents composes with it, and the flag is refused where it cannot work."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import ROOT  # noqa: E402
from wavutil import write_wav  # noqa: E402

import phaseutil as pu  # noqa: E402

pytestmark = pytest.mark.gpu
CLI = os.path.join(ROOT, "rocoder_amd", "bin", "rocoder")
RATE, W = 8000, 1024


@pytest.fixture(scope="module")
def tones(tmp_path_factory):
    """the stereo tonal input of the parity cases as an f32 file: (path, frames [n, 2])"""
    wav = str(tmp_path_factory.mktemp("phase") / "tones.wav")
    x = pu.case_input(W)
    write_wav(wav, x, RATE, "f32")
    return wav, np.ascontiguousarray(x.T)


def run(wav, out, *flags):
    return subprocess.run([CLI, "-i", wav, "-o", out, "--seed", "5", "-w", str(W), *flags], capture_output=True, text=True, timeout=300)


def data_of(path):
    raw = open(path, "rb").read()
    at = raw.index(b"data")
    n = int.from_bytes(raw[at + 4:at + 8], "little")
    return raw[at + 8:at + 8 + n]


@pytest.mark.parametrize("mode", ["locked", "propagate"])
def test_the_flag_writes_the_file_the_python_api_gives(tones, tmp_path, mode):
    import rocoder_amd

    wav, frames = tones
    out = str(tmp_path / "out.wav")
    r = run(wav, out, "--frames-on-gpu", "-f", "2", "--phase", mode)
    assert r.returncode == 0, r.stderr
    eng = rocoder_amd.Engine(window_len=W, factor=2.0, channels=2, seed=5, sample_rate=RATE)
    eng.set_phase_mode(mode)
    want = eng.stretch_frames(frames)
    hops = want.shape[0] // eng.params.window_out_len * eng.params.hops_per_window
    eng.close()
    assert data_of(out) == want.tobytes()
    m = re.search(r"^phase: (\w+), (\d+) hops$", r.stderr, re.M)
    assert m and m.group(1) == mode and int(m.group(2)) == hops, r.stderr


def test_random_is_the_default(tones, tmp_path):
    wav, _ = tones
    a, b = str(tmp_path / "a.wav"), str(tmp_path / "b.wav")
    ra = run(wav, a, "--frames-on-gpu", "-f", "2")
    rb = run(wav, b, "--frames-on-gpu", "-f", "2", "--phase", "random")
    assert ra.returncode == 0 and rb.returncode == 0, (ra.stderr, rb.stderr)
    assert open(a, "rb").read() == open(b, "rb").read()
    assert "phase:" not in rb.stderr


def test_pitch_cents_under_a_mode_writes_a_file(tones, tmp_path):
    wav, frames = tones
    out = str(tmp_path / "down.wav")
    r = run(wav, out, "--frames-on-gpu", "-f", "2", "--phase", "locked", "--pitch-cents", "-300", "--output-format", "i16")
    assert r.returncode == 0, r.stderr
    assert re.search(r"^phase: locked, \d+ hops$", r.stderr, re.M) and "resample" in r.stderr
    y = np.frombuffer(data_of(out), "<i2").reshape(-1, 2).astype(np.float64) / 32767
    assert abs(y.shape[0] - 2 * frames.shape[0]) <= 4 * W  # the duration is the factor's
    # ... and the three partials sit 300 cents lower: the strongest bin of the steady part moves by 2^(-300 / 1200)
    n = 8 * W
    mid = y.shape[0] // 2
    spec = np.abs(np.fft.rfft(y[mid - n // 2:mid + n // 2, 0] * np.hanning(n)))
    got = spec.argmax() / n * W  # in bins of a W-point transform, as phaseutil states its partials
    assert abs(got - 37.3 * 2.0 ** (-300 / 1200.0)) < 0.3, got


@pytest.mark.parametrize("flags,word", [
    (("--layer", "f=2"), "--layer"),
    (("--factor-curve", "0:2,1:3"), "--factor-curve"),
    (("--time-map", "nowhere.txt"), "--time-map"),
    (("--pitch-curve", "0:0,1:100"), "--pitch-curve"),
    (("--device-kernel", "gain:2"), "--device-kernel"),
    (("--device-kernel-src", "nowhere.hip"), "--device-kernel-src"),
    (("--freq-kernel", "nowhere.so"), "--freq-kernel"),
])
def test_the_flag_is_refused_beside_maps_layers_and_kernels(tones, tmp_path, flags, word):
    wav, _ = tones
    out = str(tmp_path / "no.wav")
    r = run(wav, out, "--frames-on-gpu", "-f", "2", "--phase", "locked", *flags)
    assert r.returncode != 0 and not os.path.exists(out)
    assert word in r.stderr, r.stderr


def test_the_flag_is_refused_where_no_mode_can_run(tones, tmp_path):
    wav, _ = tones
    out = str(tmp_path / "no.wav")
    r = run(wav, out, "-f", "2", "--phase", "locked")
    assert r.returncode != 0 and "--frames-on-gpu" in r.stderr and not os.path.exists(out)
    r = run(wav, out, "--frames-on-gpu", "-f", "2", "--phase", "coherent")
    assert r.returncode != 0 and "random, propagate or locked" in r.stderr and not os.path.exists(out)
    r = subprocess.run([CLI, "-i", wav, "-o", out, "-w", "1000", "--frames-on-gpu", "-f", "2", "--phase", "propagate"], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "propagate" in r.stderr and "power of two" in r.stderr and not os.path.exists(out)
