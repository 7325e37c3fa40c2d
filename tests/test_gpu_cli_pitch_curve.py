"""GPU tests of the CLI's --pitch-curve (--frames-on-gpu): a sine that glides down an octave while it is stretched lands where
the curve says, the output has the printed number of frames, and the flag is refused where it cannot work."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import ROOT  # noqa: E402
from test_frames_pcm_host import check_header  # noqa: E402
from wavutil import write_wav  # noqa: E402

pytestmark = pytest.mark.gpu
CLI = os.path.join(ROOT, "rocoder_amd", "bin", "rocoder")
RATE, N, SECONDS, TONE = 8000, 1024, 2.0, 1000.0


@pytest.fixture(scope="module")
def sine(tmp_path_factory):
    """a 1 kHz sine, 2 s at 8 kHz, mono i16"""
    wav = str(tmp_path_factory.mktemp("pc") / "sine.wav")
    t = np.arange(int(SECONDS * RATE)) / RATE
    write_wav(wav, 0.5 * np.sin(2 * np.pi * TONE * t)[None, :], RATE, "i16")
    return wav


def run(wav, out, *flags):
    return subprocess.run([CLI, "-i", wav, "-o", out, "--seed", "5", "-w", str(N), *flags], capture_output=True, text=True, timeout=300)


def peak_hz(x):
    """(centre, largest bin) of the spectral peak of the frames x under a Hann window: the power centroid of the bins within
    150 Hz of the largest one, and that bin's frequency. Inside 4096 frames the glide sweeps up to 80 Hz in steps of a hop,
    and the stretch gives every window phases of its own, so the largest single bin wanders over the swept band; the
    centre of the peak is the window-weighted mean of the frequencies the frames hold."""
    power = np.abs(np.fft.rfft(x * np.hanning(x.size))) ** 2
    f = np.arange(power.size) * RATE / x.size
    top = f[int(np.argmax(power))]
    near = np.abs(f - top) <= 150.0
    return float((f[near] * power[near]).sum() / power[near].sum()), float(top)


def curve_ratios(n_frames):
    """the ratio every output frame is read at, by the definition (the pure host helpers, no device): the CLI's curve - 24
    segments of 50 cents - its time map of f * r, and the anchors along that map's hops"""
    from rocoder_amd.stretcher import time_map_curve, time_map_output_len, warp_curve

    L, parts = int(SECONDS * RATE), 24
    at = [0.0 + (L - 0.0) * (k / parts) for k in range(parts + 1)]  # (the operations of the CLI's subdivision)
    ratio = [2.0 ** ((0.0 + (-1200.0 - 0.0) * (k / parts)) / 1200.0) for k in range(parts + 1)]
    kw = dict(window_len=N, factor=2.0, sample_rate=RATE)
    pos = time_map_curve(L, at, [2.0 * r for r in ratio], **kw)
    anchors, n_out = warp_curve(time_map_output_len(len(pos), **kw), at, ratio, hop_pos=pos, **kw)
    assert abs(n_out - n_frames) <= 64  # (exp2 and pow may differ in a last bit: a frame at the job's very end)
    per_frame = np.repeat(np.diff(anchors) / 2.0 ** 38, 64)
    return np.concatenate([per_frame, np.full(64, per_frame[-1])])[:n_frames]


def test_a_glide_down_an_octave_lands_where_the_curve_says(sine, tmp_path):
    out = str(tmp_path / "o.wav")
    r = run(sine, out, "--frames-on-gpu", "--output-format", "i16", "-f", "2", "--pitch-curve", "0:0,2:-1200")
    assert r.returncode == 0, r.stderr
    lines = [l for l in r.stderr.splitlines() if l.startswith("pitch curve: ")]
    assert len(lines) == 1, r.stderr
    m = re.fullmatch(r"pitch curve: (\d+) hops, (\d+) frames out, ratios \[([0-9.]+), ([0-9.]+)\], tiers (\d+) \.\.\. (\d+)", lines[0])
    assert m, lines[0]
    n_out = int(m.group(2))
    body = check_header(open(out, "rb").read(), "i16", 1, RATE)
    y = np.frombuffer(body, "<i2").astype(np.float64)
    assert y.size == n_out  # the output length is the printed n_out
    # the duration stays that of -f 2: the curve changes the pitch, not the speed
    assert abs(n_out - 2 * SECONDS * RATE) < 3 * N
    assert 0.49 < float(m.group(3)) < 0.52 and 0.99 < float(m.group(4)) <= 1.0 and (int(m.group(5)), int(m.group(6))) == (0, 0)
    # the first and the last 4096 frames: the centre of their peak lies within two 1024-point bins of 1000 * r at those
    # times - r of every frame of the segment, weighted as the Hann window weights the frame's power
    tol = 2 * RATE / 1024
    r_of = curve_ratios(n_out)
    w2 = np.hanning(4096) ** 2
    centres = {}
    for name, lo in (("first", 0), ("last", n_out - 4096)):
        want = TONE * float((r_of[lo:lo + 4096] * w2).sum() / w2.sum())
        got, top = peak_hz(y[lo:lo + 4096])
        centres[name] = got
        print(f"{name} 4096 frames: peak centred at {got:.1f} Hz (largest bin {top:.1f} Hz), the curve says {want:.1f} Hz "
              f"({TONE * r_of[lo]:.1f} ... {TONE * r_of[lo + 4095]:.1f} over the segment), tolerance {tol:.1f} Hz")
        assert abs(got - want) <= tol
    assert centres["first"] > 1.7 * centres["last"]  # most of an octave lies between them


def test_the_refusals(sine, tmp_path):
    out = str(tmp_path / "o.wav")
    for flags, word in ((("--pitch-curve", "0:0,2:-1200"), "--frames-on-gpu"),
                        (("--frames-on-gpu", "--pitch-curve", "0:0,2:-1200", "--pitch-cents", "100"), "--pitch-ratio"),
                        (("--frames-on-gpu", "--pitch-curve", "0:0,2:-1200", "--pitch-ratio", "3/2"), "--pitch-ratio"),
                        (("--frames-on-gpu", "--pitch-curve", "0:0,2:-1200", "--time-map", "nowhere.txt"), "--time-map"),
                        (("--frames-on-gpu", "--pitch-curve", "0:0,0:-1200"), "ascending"),
                        (("--frames-on-gpu", "--pitch-curve", "0:0,2:-4000"), "1/8"),
                        (("--frames-on-gpu", "--pitch-curve", "soon:low"), "t:c")):
        r = run(sine, out, *flags)
        assert r.returncode != 0 and word in r.stderr, (flags, r.stderr)
        assert not os.path.exists(out)
