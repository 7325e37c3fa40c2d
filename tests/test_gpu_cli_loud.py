"""GPU tests of the CLI's --loudness and --true-peak (--frames-on-gpu): the file written is the Python path's bytes, with and
without --output-rate (the rate passed on is the output file's), the printed line carries the engine's three values, and the
flags are refused where they cannot work."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rocoder_amd  # noqa: E402
from conftest import ROOT  # noqa: E402
from test_frames_pcm_host import check_header  # noqa: E402
from wavutil import write_wav  # noqa: E402

pytestmark = pytest.mark.gpu
CLI = os.path.join(ROOT, "rocoder_amd", "bin", "rocoder")
RATE = 44100


@pytest.fixture(scope="module")
def take(tmp_path_factory):
    """a stereo i16 file of noise, a quarter of it 20 dB down, and the bytes of its frames"""
    wav = str(tmp_path_factory.mktemp("loud") / "in.wav")
    x = np.random.default_rng(29).uniform(-0.5, 0.5, (2, 16000))
    x[:, :4000] *= 0.1
    write_wav(wav, x, RATE, "i16")
    return wav, np.frombuffer(open(wav, "rb").read(), np.uint8)[44:]


def run(wav, out, *flags):
    return subprocess.run([CLI, "-i", wav, "-o", out, "--seed", "5", "-w", "1024", "-f", "4", *flags], capture_output=True, text=True, timeout=300)


def python_path(body, target, ceiling, rate=RATE, step=None, limit=None, dither=None):
    with rocoder_amd.Engine(window_len=1024, factor=4.0, channels=2, seed=5, sample_rate=RATE) as eng:
        if step:
            eng.set_output_resample(*step)
        if limit:
            eng.set_output_limiter(*limit)
        if dither:
            eng.set_output_dither(*dither)
        got = eng.stretch_frames_loud(body, target, ceiling, fmt="i16", out_fmt="i16", sample_rate=rate)
        return got.tobytes(), eng.last_lufs, eng.last_true_peak, eng.last_gain, eng.last_clipped


def loud_line(stderr):
    lines = [re.fullmatch(r"loudness (\S+) LUFS, true peak (\S+) \((\S+) dBTP\), gain (\S+) \((\S+) dB\)", l) for l in stderr.splitlines()
             if l.startswith("loudness ")]
    assert len(lines) == 1 and lines[0], stderr
    return lines[0]


def check_line(m, lufs, tp, gain):
    for got, want in ((m.group(1), lufs), (m.group(2), tp), (m.group(4), gain)):
        assert np.float32(got).view(np.uint32) == np.float32(want).view(np.uint32), (got, want)
    assert abs(float(m.group(3)) - 20 * np.log10(float(tp))) <= 0.006 and abs(float(m.group(5)) - 20 * np.log10(float(gain))) <= 0.006


def test_the_file_is_the_python_paths_bytes_and_the_line_matches(take, tmp_path):
    wav, body = take
    want, lufs, tp, gain, clipped = python_path(body, -16.0, 0.0)
    assert np.isfinite(lufs) and gain != 1
    out = str(tmp_path / "o.wav")
    r = run(wav, out, "--loudness", "-16", "--output-format", "i16", "--frames-on-gpu")
    assert r.returncode == 0, r.stderr
    assert check_header(open(out, "rb").read(), "i16", 2, RATE) == want
    check_line(loud_line(r.stderr), lufs, tp, gain)
    assert bool([l for l in r.stderr.splitlines() if "clipped" in l]) == bool(clipped)


def test_true_peak_in_decibels_binds_and_composes_with_limit_and_dither(take, tmp_path):
    wav, body = take
    ceiling = np.float32(10.0 ** (float(np.float32(-6.0)) / 20.0))  # (the CLI reads the number as an f32 and forms 10^(dB / 20) in doubles)
    lookahead = int(np.float32(0.005) * np.float32(RATE))
    want, lufs, tp, gain, clipped = python_path(body, -3.0, ceiling, limit=(1.0, 0.9, lookahead), dither=("tpdf", 5))
    assert gain == np.float32(ceiling / tp)  # the ceiling binds: -3 LUFS asks for more
    out = str(tmp_path / "o.wav")
    r = run(wav, out, "--loudness", "-3", "--true-peak", "-6dB", "--limit", "0.9", "--dither", "tpdf", "--output-format", "i16", "--frames-on-gpu")
    assert r.returncode == 0, r.stderr
    assert check_header(open(out, "rb").read(), "i16", 2, RATE) == want
    check_line(loud_line(r.stderr), lufs, tp, gain)
    # the same ceiling, linear
    out2 = str(tmp_path / "o2.wav")
    r = run(wav, out2, "--loudness", "-3", "--true-peak", "%.9g" % ceiling, "--limit", "0.9", "--dither", "tpdf", "--output-format", "i16", "--frames-on-gpu")
    assert r.returncode == 0 and open(out2, "rb").read() == open(out, "rb").read()


def test_output_rate_is_the_rate_the_loudness_is_measured_at(take, tmp_path):
    wav, body = take
    want, lufs, tp, gain, _ = python_path(body, -20.0, 1.0, rate=48000, step=(147, 160))
    at_44k = python_path(body, -20.0, 1.0, rate=RATE, step=(147, 160))
    assert at_44k[1] != lufs  # (other coefficients, other sub-blocks: the rate matters)
    out = str(tmp_path / "o.wav")
    r = run(wav, out, "--loudness", "-20", "--true-peak", "1", "--output-rate", "48000", "--output-format", "i16", "--frames-on-gpu")
    assert r.returncode == 0, r.stderr
    assert check_header(open(out, "rb").read(), "i16", 2, 48000) == want
    check_line(loud_line(r.stderr), lufs, tp, gain)


@pytest.mark.parametrize("flags,word", [
    (("--loudness", "-16"), "--frames-on-gpu"),
    (("--true-peak", "0.9", "--frames-on-gpu"), "--loudness"),
    (("--loudness", "-16", "--normalize", "0.9", "--frames-on-gpu"), "--normalize"),
    (("--loudness", "loud", "--frames-on-gpu"), "--loudness"),
    (("--loudness", "inf", "--frames-on-gpu"), "--loudness"),
    (("--loudness", "-16", "--true-peak", "0", "--frames-on-gpu"), "--true-peak"),
    (("--loudness", "-16", "--true-peak", "-1dBTP", "--frames-on-gpu"), "--true-peak"),
])
def test_refused(take, tmp_path, flags, word):
    wav, _body = take
    out = str(tmp_path / "o.wav")
    r = run(wav, out, *flags)
    assert r.returncode != 0 and word in r.stderr and not os.path.exists(out), r.stderr
