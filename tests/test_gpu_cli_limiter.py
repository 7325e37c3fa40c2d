"""GPU tests of the CLI's --limit, --limit-drive and --limit-lookahead (--frames-on-gpu): the file written is the Python
path's bytes, the printed line carries the engine's stats, and the flags are refused where they cannot work."""
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
    """a stereo i16 file whose stretch at -a 6 overshoots full scale, and the bytes of its frames"""
    wav = str(tmp_path_factory.mktemp("limiter") / "in.wav")
    write_wav(wav, np.random.default_rng(23).uniform(-1, 1, (2, 6000)), RATE, "i16")
    return wav, np.frombuffer(open(wav, "rb").read(), np.uint8)[44:]


def run(wav, out, *flags):
    return subprocess.run([CLI, "-i", wav, "-o", out, "--seed", "5", "-w", "1024", "-f", "4", "-a", "6", *flags], capture_output=True,
                          text=True, timeout=300)


def python_path(body, drive, ceiling, lookahead, **kw):
    with rocoder_amd.Engine(window_len=1024, factor=4.0, channels=2, seed=5, amplitude=6.0) as eng:
        eng.set_output_limiter(drive, ceiling, lookahead)
        got = eng.stretch_frames(body, fmt="i16", out_fmt="i16", **kw)
        return got.tobytes(), got.shape[0], eng.last_limiter_stats, eng.last_clipped


def stats_line(stderr):
    lines = [re.fullmatch(r"limited (\d+) of (\d+) frames, lowest gain (\S+) \((\S+) dB\)", l) for l in stderr.splitlines() if l.startswith("limited ")]
    assert len(lines) == 1 and lines[0], stderr
    return lines[0]


def test_the_file_is_the_python_paths_bytes_and_the_line_matches_the_stats(take, tmp_path):
    wav, body = take
    lookahead = int(np.float32(0.005) * np.float32(RATE))  # duration_to_sample: 220 frames
    assert lookahead == 220
    want, n, (g, limited), clipped = python_path(body, 1.0, 0.9, lookahead)
    assert 0 < limited and g < 1 and clipped == 0
    out = str(tmp_path / "o.wav")
    r = run(wav, out, "--limit", "0.9", "--limit-lookahead", "0.005", "--output-format", "i16", "--frames-on-gpu")
    assert r.returncode == 0, r.stderr
    assert check_header(open(out, "rb").read(), "i16", 2, RATE) == want
    m = stats_line(r.stderr)
    assert (int(m.group(1)), int(m.group(2))) == (limited, n)
    assert np.float32(m.group(3)).view(np.uint32) == np.float32(g).view(np.uint32)
    assert abs(float(m.group(4)) - 20 * np.log10(float(g))) <= 0.05
    assert not [l for l in r.stderr.splitlines() if "clipped" in l]
    # the default look-ahead is those 5 ms
    out2 = str(tmp_path / "o2.wav")
    r = run(wav, out2, "--limit", "0.9", "--output-format", "i16", "--frames-on-gpu")
    assert r.returncode == 0 and open(out2, "rb").read() == open(out, "rb").read()


def test_decibels_drive_and_normalize_compose(take, tmp_path):
    wav, body = take
    # (the CLI reads the number as an f32 and forms 10^(dB / 20) in doubles)
    ceiling = np.float32(10.0 ** (float(np.float32(-0.3)) / 20.0))
    drive = np.float32(10.0 ** (6.0 / 20.0))
    want, n, (g, limited), clipped = python_path(body, drive, ceiling, 44, normalize=0.5)
    out = str(tmp_path / "o.wav")
    r = run(wav, out, "--limit", "-0.3dB", "--limit-drive", "6dB", "--limit-lookahead", "0.001", "--normalize", "0.5", "--output-format", "i16",
            "--frames-on-gpu")
    assert r.returncode == 0, r.stderr
    assert check_header(open(out, "rb").read(), "i16", 2, RATE) == want
    m = stats_line(r.stderr)
    assert (int(m.group(1)), int(m.group(2))) == (limited, n)
    assert re.search(r"^peak (\S+), gain ", r.stderr, re.M)


@pytest.mark.parametrize("flags,word", [
    (("--limit", "0.9"), "--frames-on-gpu"),
    (("--limit-drive", "2", "--frames-on-gpu"), "--limit"),
    (("--limit-lookahead", "0.001", "--frames-on-gpu"), "--limit"),
    (("--limit", "0", "--frames-on-gpu"), "--limit"),
    (("--limit", "loud", "--frames-on-gpu"), "--limit"),
    (("--limit", "0.9", "--limit-lookahead", "0.1", "--frames-on-gpu"), "--limit-lookahead"),  # 4410 frames
])
def test_refused(take, tmp_path, flags, word):
    wav, _body = take
    out = str(tmp_path / "o.wav")
    r = run(wav, out, *flags)
    assert r.returncode != 0 and word in r.stderr and not os.path.exists(out), r.stderr
