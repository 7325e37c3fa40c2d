"""GPU tests of the CLI's --factor-curve and --time-map (--frames-on-gpu): the file written is the one the Python mirror
computes for the same map, the printed line names the map, and the flags are refused where they cannot work."""
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
RATE, N, L = 44100, 1024, 22050


@pytest.fixture(scope="module")
def take(tmp_path_factory):
    """half a second of stereo i16 noise and the bytes of its frames"""
    wav = str(tmp_path_factory.mktemp("tm") / "in.wav")
    write_wav(wav, np.random.default_rng(31).uniform(-0.5, 0.5, (2, L)), RATE, "i16")
    return wav, np.frombuffer(open(wav, "rb").read(), np.uint8)[44:]


def run(wav, out, *flags):
    return subprocess.run([CLI, "-i", wav, "-o", out, "--seed", "5", "-w", str(N), *flags], capture_output=True, text=True, timeout=300)


def python_path(body, pos, factor=1.0, fade=None):
    with rocoder_amd.Engine(window_len=N, factor=factor, channels=2, seed=5, sample_rate=RATE) as eng:
        eng.set_time_map(pos)
        if fade is not None:
            eng.set_output_fade(*fade)
        return eng.stretch_frames(body, fmt="i16", out_fmt="i16").tobytes()


def check_line(stderr, pos):
    lines = [l for l in stderr.splitlines() if l.startswith("time map: ")]
    assert len(lines) == 1, stderr
    m = re.fullmatch(r"time map: (\d+) hops, (\d+) frames out, input positions \[(-?\d+), (-?\d+)\]", lines[0])
    assert m, lines[0]
    n_out = rocoder_amd.time_map_output_len(len(pos), window_len=N)
    assert [int(g) for g in m.groups()] == [len(pos), n_out, int(min(pos)), int(max(pos))]


def test_factor_curve_writes_the_python_mirrors_file(take, tmp_path):
    wav, body = take
    # 0 s -> 2x, 0.25 s -> 6x: the times in input frames, as the CLI forms them (ms / 1000 * rate in doubles)
    at = [0 / 1000.0 * RATE, 250 / 1000.0 * RATE]
    pos = rocoder_amd.time_map_curve(L, at, [2.0, 6.0], window_len=N)
    out = str(tmp_path / "o.wav")
    r = run(wav, out, "--frames-on-gpu", "--output-format", "i16", "--factor-curve", "0:2,0.25:6")
    assert r.returncode == 0, r.stderr
    assert check_header(open(out, "rb").read(), "i16", 2, RATE) == python_path(body, pos)
    check_line(r.stderr, pos)


def test_time_map_file_writes_the_python_mirrors_file(take, tmp_path):
    wav, body = take
    pos = [0, 300, 600, 600, 600, 600, 9000, 8000, 7000, -200, L - 100, L + 50]  # a hold, a reversed stretch, both ends
    path = str(tmp_path / "map.txt")
    with open(path, "w") as f:
        f.write("# a hand-made map\n\n" + "\n".join(f"{p}  # hop {k}" if k % 3 == 0 else f"  {p}" for k, p in enumerate(pos)) + "\n")
    out = str(tmp_path / "o.wav")
    r = run(wav, out, "--frames-on-gpu", "--output-format", "i16", "-f", "3", "--time-map", path)
    assert r.returncode == 0, r.stderr
    assert check_header(open(out, "rb").read(), "i16", 2, RATE) == python_path(body, pos, factor=3.0)
    check_line(r.stderr, pos)


def test_fade_output_under_a_map_ends_with_the_map(take, tmp_path):
    """-f 3 would put the fade-out in front of frame 3 L = 66150; the map's job has 6 windows of 1024 frames, and the fade-out
    runs into its last frame."""
    wav, body = take
    pos = [0, 300, 600, 600, 600, 600, 9000, 8000, 7000, -200, L - 100, L + 50]
    path = str(tmp_path / "map.txt")
    open(path, "w").write("\n".join(str(p) for p in pos) + "\n")
    n_out = rocoder_amd.time_map_output_len(len(pos), window_len=N)
    fade = int(np.float32(0.01) * np.float32(RATE))  # duration_to_sample, in f32 as the CLI forms it
    assert n_out == 6144 and fade == 441
    out = str(tmp_path / "o.wav")
    r = run(wav, out, "--frames-on-gpu", "--output-format", "i16", "-f", "3", "--time-map", path, "--fade-output", "-x", "0.01")
    assert r.returncode == 0, r.stderr
    assert f"fade in {fade} frames, out from {n_out - fade} over {fade}" in r.stderr, r.stderr
    want = python_path(body, pos, factor=3.0, fade=(fade, n_out - fade, fade))
    assert check_header(open(out, "rb").read(), "i16", 2, RATE) == want
    assert want != python_path(body, pos, factor=3.0)  # (the fade changed frames)


@pytest.mark.parametrize("flags,word", [
    (("--frames-on-gpu", "--factor-curve", "0:2", "--pitch-ratio", "3/2"), "--pitch-ratio"),
    (("--frames-on-gpu", "--time-map", "m.txt", "--pitch-cents", "100"), "--pitch-ratio"),
    (("--factor-curve", "0:2"), "--frames-on-gpu"),
    (("--time-map", "nowhere.txt"), "--frames-on-gpu"),
    (("--frames-on-gpu", "--factor-curve", "0:2", "-f", "3"), "-f"),
    (("--frames-on-gpu", "--factor-curve", "0:2", "--time-map", "m.txt"), "--time-map"),
    (("--frames-on-gpu", "--factor-curve", "0;2"), "--factor-curve"),
    (("--frames-on-gpu", "--factor-curve", "0:two"), "--factor-curve"),
    (("--frames-on-gpu", "--factor-curve", "0.2:2,0.1:3"), "--factor-curve"),
    (("--frames-on-gpu", "--factor-curve", "0:0"), "--factor-curve"),
    (("--frames-on-gpu", "--time-map", "nowhere.txt"), "nowhere.txt"),
])
def test_refused_flags(take, tmp_path, flags, word):
    wav, _body = take
    out = str(tmp_path / "o.wav")
    r = run(wav, out, *flags)
    assert r.returncode != 0 and word in r.stderr, r.stderr
    assert not os.path.exists(out)


def test_a_map_file_with_a_bad_line_or_a_bad_length_is_refused(take, tmp_path):
    wav, _body = take
    out = str(tmp_path / "o.wav")
    bad = str(tmp_path / "bad.txt")
    open(bad, "w").write("0\n12x\n")
    r = run(wav, out, "--frames-on-gpu", "--time-map", bad)
    assert r.returncode != 0 and "bad.txt:2" in r.stderr, r.stderr
    odd = str(tmp_path / "odd.txt")
    open(odd, "w").write("0\n100\n200\n")  # three hops: hops_per_window is 2
    r = run(wav, out, "--frames-on-gpu", "--time-map", odd)
    assert r.returncode != 0 and "hops_per_window" in r.stderr, r.stderr
    assert not os.path.exists(out)
