"""GPU tests of the CLI's --pitch-ratio, --pitch-cents and --output-rate (--frames-on-gpu): a 1000 Hz sine comes out at the
pitch asked for, with the frame count of the definition and the rate in the header."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rocoder_amd  # noqa: E402, F401
from conftest import ROOT  # noqa: E402
from rocoder_amd.stretcher import offline_output_len, resample_len  # noqa: E402
from wavutil import read_wav_f32, write_wav  # noqa: E402

pytestmark = pytest.mark.gpu
CLI = os.path.join(ROOT, "rocoder_amd", "bin", "rocoder")
RATE, N, FRAMES = 44100, 4096, 2 * 44100
WIDTH = 2 * RATE / N  # the Hann main lobe's half-width at the analysis window


@pytest.fixture(scope="module")
def sine(tmp_path_factory):
    wav = str(tmp_path_factory.mktemp("resample") / "sine.wav")
    t = np.arange(FRAMES) / RATE
    write_wav(wav, 0.5 * np.sin(2 * np.pi * 1000.0 * t)[None, :], RATE, "i16")
    return wav


def run(wav, out, *flags):
    return subprocess.run([CLI, "-i", wav, "-o", out, "--seed", "5", "-w", str(N), "-f", "2", *flags], capture_output=True, text=True, timeout=300)


def spectral_peak(y, rate):
    """the frequency of the largest bin of the Hann-windowed output, Hz"""
    spec = np.abs(np.fft.rfft(y * np.hanning(y.size)))
    return float(np.argmax(spec)) * rate / y.size


def test_pitch_ratio_moves_the_sine_and_keeps_the_duration(sine, tmp_path):
    out = str(tmp_path / "o.wav")
    r = run(sine, out, "--frames-on-gpu", "--pitch-ratio", "3/2")
    assert r.returncode == 0, r.stderr
    assert re.search(r"^resample 3/2 \(\+0\.0000 cents off 1\.5\), 96 taps$", r.stderr, re.M), r.stderr
    rate, y = read_wav_f32(out)
    assert rate == RATE and y.shape[0] == 1
    n = offline_output_len(FRAMES, window_len=N, factor=3.0, channels=1)
    assert y.shape[1] == resample_len(n, 3, 2)
    f = spectral_peak(y[0], rate)
    print(f"peak at {f:.2f} Hz")
    assert abs(f - 1500.0) <= WIDTH
    # the decimal form is the same ratio
    out2 = str(tmp_path / "o2.wav")
    r = run(sine, out2, "--frames-on-gpu", "--pitch-ratio", "1.5")
    assert r.returncode == 0 and open(out2, "rb").read() == open(out, "rb").read()


def test_output_rate_keeps_the_pitch_and_says_so_in_the_header(sine, tmp_path):
    out = str(tmp_path / "o.wav")
    r = run(sine, out, "--frames-on-gpu", "--output-rate", "48000")
    assert r.returncode == 0, r.stderr
    assert re.search(r"^resample 147/160 ", r.stderr, re.M), r.stderr
    rate, y = read_wav_f32(out)
    assert rate == 48000
    n = offline_output_len(FRAMES, window_len=N, factor=2.0, channels=1)
    assert y.shape[1] == resample_len(n, 147, 160)
    f = spectral_peak(y[0], rate)
    print(f"peak at {f:.2f} Hz")
    assert abs(f - 1000.0) <= WIDTH


def test_pitch_cents_prints_the_ratio(sine, tmp_path):
    out = str(tmp_path / "o.wav")
    r = run(sine, out, "--frames-on-gpu", "--pitch-cents", "100")
    assert r.returncode == 0, r.stderr
    m = re.search(r"^resample 1069/1009 \(([-+][0-9.]+) cents off ([0-9.]+)\), 68 taps$", r.stderr, re.M)
    assert m and abs(float(m.group(1))) < 0.01 and abs(float(m.group(2)) - 2 ** (1 / 12)) < 1e-8, r.stderr
    rate, y = read_wav_f32(out)
    assert abs(spectral_peak(y[0], rate) - 1000.0 * 2 ** (1 / 12)) <= WIDTH


@pytest.mark.parametrize("flags", [("--pitch-ratio", "3/2"), ("--pitch-cents", "100"), ("--output-rate", "48000")])
def test_each_flag_needs_frames_on_gpu(sine, tmp_path, flags):
    out = str(tmp_path / "o.wav")
    r = run(sine, out, *flags)
    assert r.returncode != 0 and "--frames-on-gpu" in r.stderr and not os.path.exists(out)
