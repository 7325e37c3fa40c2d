"""GPU tests of the CLI's --layer (--frames-on-gpu, -o): a three-layer run writes the file the Python API gives for the same
layers - an octave below, the original and a fifth above, each with its own entry, gain and fade - the report lines say what
was mixed, and the flag is refused where it cannot work."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import ROOT  # noqa: E402
from wavutil import write_wav  # noqa: E402

import mixutil as M  # noqa: E402

pytestmark = pytest.mark.gpu
CLI = os.path.join(ROOT, "rocoder_amd", "bin", "rocoder")
RATE, W, FRAMES = 8000, 1024, 6000


@pytest.fixture(scope="module")
def noise(tmp_path_factory):
    """stereo white noise, 0.75 s at 8 kHz, i16: (path, the file's frames as int16 [n, 2])"""
    wav = str(tmp_path_factory.mktemp("mix") / "noise.wav")
    x = np.random.default_rng(3).uniform(-0.5, 0.5, (2, FRAMES))
    write_wav(wav, x, RATE, "i16")
    raw = open(wav, "rb").read()
    at = raw.index(b"data") + 8
    return wav, np.frombuffer(raw[at:at + FRAMES * 4], "<i2").reshape(FRAMES, 2).copy()


def run(wav, out, *flags):
    return subprocess.run([CLI, "-i", wav, "-o", out, "--seed", "5", "-w", str(W), *flags], capture_output=True, text=True, timeout=300)


def data_of(path):
    raw = open(path, "rb").read()
    at = raw.index(b"data")
    n = int.from_bytes(raw[at + 4:at + 8], "little")
    return raw[at + 8:at + 8 + n]


def test_three_layers_write_the_file_the_python_api_gives(noise, tmp_path):
    import rocoder_amd
    from rocoder_amd.stretcher import Bus, resample_ratio

    wav, frames = noise
    out = str(tmp_path / "mix.wav")
    specs = ["f=4,p=-2,gain=-6dB,fade=0.5", "at=0.25,seed=9", "cents=700,a=0.5,at=1,fade=0.25,gain=0.8"]
    r = run(wav, out, "--frames-on-gpu", "-f", "4", "--output-format", "i16", "--normalize", "0.9", "--limit", "0.95", "--dither", "tpdf",
            *[v for s in specs for v in ("--layer", s)])
    assert r.returncode == 0, r.stderr
    ratio = 2.0 ** (700 / 1200.0)
    num, den = resample_ratio(ratio)
    layers = [dict(factor=4.0, pitch_multiple=-2, seed=5, amplitude=1.0, gain=np.float32(10.0 ** (-6 / 20.0)), at=0.0, fade=0.5, f=4.0),
              dict(factor=4.0, pitch_multiple=1, seed=9, amplitude=1.0, gain=np.float32(1.0), at=0.25, fade=None, f=4.0),
              dict(factor=float(np.float32(4.0 * ratio)), pitch_multiple=1, seed=5, amplitude=0.5, gain=np.float32(0.8), at=1.0, fade=0.25, f=4.0,
                   resample=(num, den))]
    engines, lens, offsets, keys = [], [], [], []
    for l in layers:
        e = rocoder_amd.Engine(window_len=W, factor=l["factor"], pitch_multiple=l["pitch_multiple"], seed=l["seed"], amplitude=l["amplitude"],
                               channels=2, sample_rate=RATE)
        if "resample" in l:
            e.set_output_resample(*l["resample"])
        engines.append(e)
        lens.append(e._host_output_len(FRAMES))
        offsets.append(M.dur_to_sample(l["at"], RATE))
        k = [(0, l["gain"])] if l["gain"] != 1 else None
        if l["fade"] is not None:
            k = [(f, np.float32(a) * l["gain"]) for f, a in M.fade_keys(l["fade"], int(np.float32(np.float32(FRAMES) * np.float32(l["f"]))), RATE)]
        keys.append(k)
    N = max(o + n for o, n in zip(offsets, lens))
    with Bus(2, N) as bus, rocoder_amd.Engine(window_len=W, factor=4.0, seed=5, channels=2, sample_rate=RATE) as master:
        mixed = [e.mix_frames(frames, bus, offset=o, keys=k) for e, o, k in zip(engines, offsets, keys)]
        master.set_output_limiter(1.0, 0.95, int(np.float32(np.float32(0.005) * np.float32(RATE))))
        master.set_output_dither("tpdf", 5)
        want, stats = master.bus_frames(bus, "i16", target_peak=0.9)
    for e in engines:
        e.close()
    assert data_of(out) == want.tobytes() and want.any()
    # the report
    err = r.stderr.splitlines()
    assert f"mix: 3 layers, {N} frames" in err, r.stderr
    got = [re.fullmatch(r"layer (\d): factor ([0-9.]+), ratio (\d+)/(\d+), offset (-?\d+), (\d+) frames mixed", ln) for ln in err if ln.startswith("layer ")]
    assert len(got) == 3 and all(got), r.stderr
    for i, m in enumerate(got):
        assert int(m.group(1)) == i and float(m.group(2)) == 4.0 and int(m.group(5)) == offsets[i] and int(m.group(6)) == mixed[i] == lens[i]
    assert (int(got[2].group(3)), int(got[2].group(4))) == (num, den) and (got[0].group(3), got[0].group(4)) == ("1", "1")
    assert any(ln.startswith("peak ") and f"gain {float(stats['gain']):.9g}" in ln for ln in err), r.stderr


@pytest.mark.parametrize("flags,needle", [
    (["--layer", "f=2"], "--layer needs --frames-on-gpu and -o"),
    (["--frames-on-gpu", "--layer", "f=2", "--loudness", "-14"], "--layer cannot be combined with --loudness"),
    (["--frames-on-gpu", "--layer", "f=2", "--pitch-curve", "0:0,1:100"], "--layer cannot be combined with --pitch-curve"),
    (["--frames-on-gpu", "--layer", "f=2", "--factor-curve", "0:2,1:3"], "--layer cannot be combined with --factor-curve"),
    (["--frames-on-gpu", "--layer", "f=2", "--time-map", "nofile"], "--layer cannot be combined with --time-map"),
    (["--frames-on-gpu", "--layer", "f=2,speed=3"], "--layer: bad speed=3"),
    (["--frames-on-gpu", "--layer", "f=2,cents=99999"], "--layer: bad cents=99999"),
    (["--frames-on-gpu", "--layer", "f=2,fade=30"], "is longer than the layer"),
    (["--frames-on-gpu", "--layer", "f=2,fade=1.5"], "with two amplitudes"),
])
def test_refusals(noise, tmp_path, flags, needle):
    out = str(tmp_path / "no.wav")
    r = run(noise[0], out, *flags)
    assert r.returncode != 0 and needle in r.stderr, r.stderr
    assert not os.path.exists(out)
