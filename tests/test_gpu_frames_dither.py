"""GPU tests of rc_engine_set_output_dither / Engine.set_output_dither / --dither: TPDF and high-passed TPDF dither in front
of the GPU's PCM quantiser. The yardstick is never the code under test: it is ref = eng.stretch_frames(raw), the f32 entry
(itself tied to stretch_host and to the oracle by tests/test_gpu_frames.py), quantised in numpy by the definition of
include/rocoder_hip.h (tests/ditherutil.py). Every comparison is of bytes, with no tolerance."""
import os
import subprocess

import numpy as np
import pytest

import ditherutil as D
import rocoder_amd
from conftest import ROOT
from rocoder_amd import _lib
from rocoder_amd.stretcher import pinned_empty
from test_frames_pcm_host import check_header, count_clipped
from test_gpu_frames_pcm import GUARD, SLOT_FLOATS, check_result, expected_bytes, noise_i16
from wavutil import write_wav

pytestmark = pytest.mark.gpu
CLI = os.path.join(ROOT, "rocoder_amd", "bin", "rocoder")
MODES = ["tpdf", "tpdf-hp"]
SEED = 9


def want_bytes(ref, fmt, mode, seed=SEED):
    return D.dithered_bytes(ref, fmt, mode, seed).tobytes()


@pytest.mark.parametrize("ch", [1, 2, 3, 8])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("fmt", D.DITHER_FORMATS)
def test_every_dithered_format_and_channel_count(fmt, mode, ch):
    """N = 1024, f = 2, 30001 frames: the odd length and the 3- and 9-byte frames put tile edges on every byte phase.
    One combination also into a target at each of the four byte phases between guard bytes."""
    a = noise_i16(30001, ch, 40 + ch)
    with rocoder_amd.Engine(window_len=1024, factor=2.0, channels=ch, seed=3) as eng:
        ref = eng.stretch_frames(a)
        n_out = eng.output_len(30001)
        eng.set_output_dither(mode, SEED)
        want = want_bytes(ref, fmt, mode)
        assert want != expected_bytes(ref, fmt), "the dither changes nothing: nothing is tested"
        check_result(eng.stretch_frames(a, out_fmt=fmt), want, fmt, n_out, ch)
        assert eng.last_clipped == count_clipped(ref)
        if (fmt, mode, ch) == ("i24", "tpdf-hp", 3):
            for offset in (0, 1, 2, 3):
                big = np.full(len(want) + 64, GUARD, np.uint8)
                lo = 16 + offset
                got = eng.stretch_frames(a, out=big[lo:lo + len(want)], out_fmt=fmt)
                check_result(got, want, fmt, n_out, ch)
                assert (big[:lo] == GUARD).all() and (big[lo + len(want):] == GUARD).all(), (offset, "guard bytes were written")
                assert eng.last_clipped == count_clipped(ref)


@pytest.mark.parametrize("fmt", ["i16", "i24"])
def test_more_channels_than_a_wave(fmt):
    """67 channels at N = 256, 3000 frames: the wide kernel, a second channel tile of three channels"""
    a = noise_i16(3000, 67, 5)
    with rocoder_amd.Engine(window_len=256, factor=2.0, channels=67, seed=5) as eng:
        ref = eng.stretch_frames(a)
        for mode in MODES:
            eng.set_output_dither(mode, SEED)
            check_result(eng.stretch_frames(a, out_fmt=fmt), want_bytes(ref, fmt, mode), fmt, ref.shape[0], 67)
            assert eng.last_clipped == count_clipped(ref)


@pytest.fixture(scope="module")
def chunked():
    """The chunked shape of tests/test_gpu_frames_pcm.py: N = 1024, f = 8, three channels, 1 200 000 frames, several
    pipeline chunks. The yardstick and its dithered bytes are computed once and never written to."""
    eng = rocoder_amd.Engine(window_len=1024, factor=8.0, channels=3, seed=21)
    a = noise_i16(1_200_000, 3, 4)
    ref = eng.stretch_frames(a)
    assert ref.shape[0] > 2 * SLOT_FLOATS
    mode = {"u8": "tpdf", "i24": "tpdf-hp"}
    want = {fmt: want_bytes(ref, fmt, mode[fmt]) for fmt in mode}
    clipped = count_clipped(ref)
    yield eng, a, mode, want, ref.shape[0], clipped
    eng.close()


@pytest.mark.parametrize("kind", ["pageable", "pinned"])
@pytest.mark.parametrize("fmt", ["u8", "i24"])
def test_several_pipeline_chunks_with_either_kind_of_memory(chunked, fmt, kind):
    """every chunk's launch starts at its own absolute frame: the bytes do not depend on the chunking"""
    eng, a, mode, want, n_out, clipped = chunked
    want = want[fmt]
    eng.set_output_dither(mode[fmt], SEED)
    if kind == "pageable":
        got = eng.stretch_frames(a, out_fmt=fmt)
    else:
        src = pinned_empty(a.shape, a.dtype)
        src[:] = a
        big = pinned_empty(len(want) + 32, np.uint8)
        big[:] = GUARD
        got = eng.stretch_frames(src, out=big[17:17 + len(want)], out_fmt=fmt)
        assert (big[:17] == GUARD).all() and (big[17 + len(want):] == GUARD).all(), "guard bytes were written"
    check_result(got, want, fmt, n_out, 3)
    assert eng.last_clipped == clipped


def test_formats_and_entries_that_take_no_dither_and_the_state():
    """i32 and f32 out, stretch_frames (f32) and stretch_host are what they are without a mode; "none" restores the
    undithered bytes; the same seed gives the same bytes, another seed other bytes; a rejected mode leaves the state."""
    a = noise_i16(30001, 2, 9)
    with rocoder_amd.Engine(window_len=1024, factor=2.0, channels=2, seed=3) as eng:
        ref = eng.stretch_frames(a)
        n_out = ref.shape[0]
        planar = np.ascontiguousarray((a.astype(np.float32) / np.float32(32767)).T)
        host = eng.stretch_host(planar)
        plain = {fmt: eng.stretch_frames(a, out_fmt=fmt).tobytes() for fmt in ("u8", "i16", "i24", "i32", "f32")}
        eng.set_output_dither("tpdf", SEED)
        for fmt in ("i32", "f32"):
            assert eng.stretch_frames(a, out_fmt=fmt).tobytes() == plain[fmt] == expected_bytes(ref, fmt)
        assert eng.stretch_frames(a).tobytes() == ref.tobytes()
        assert eng.stretch_host(planar).tobytes() == host.tobytes()
        first = eng.stretch_frames(a, out_fmt="i16").tobytes()
        assert first == want_bytes(ref, "i16", "tpdf") and first != plain["i16"]
        eng.set_output_dither("tpdf", SEED)
        assert eng.stretch_frames(a, out_fmt="i16").tobytes() == first
        eng.set_output_dither("tpdf", SEED + 1)
        other = eng.stretch_frames(a, out_fmt="i16").tobytes()
        assert other == want_bytes(ref, "i16", "tpdf", SEED + 1) and other != first
        with pytest.raises(ValueError):
            eng.set_output_dither("blue", SEED)
        assert _lib.lib().rc_engine_set_output_dither(eng._h, 3, SEED) == _lib.RC_EINVAL
        assert eng.stretch_frames(a, out_fmt="i16").tobytes() == other
        eng.set_output_dither("none")
        for fmt in ("u8", "i16", "i24"):
            check_result(eng.stretch_frames(a, out_fmt=fmt), plain[fmt], fmt, n_out, 2)
        eng.set_output_dither()
        assert eng.stretch_frames(a, out_fmt="i16").tobytes() == plain["i16"]


@pytest.mark.parametrize("mode", MODES)
def test_with_the_normalised_entry(mode):
    """the expected bytes: numpy on ref * gain, one f32 multiplication, with the gain the call reports"""
    a = noise_i16(30001, 2, 11)
    with rocoder_amd.Engine(window_len=1024, factor=2.0, channels=2, seed=3) as eng:
        ref = eng.stretch_frames(a)
        eng.set_output_dither(mode, SEED)
        for fmt in ("u8", "i16"):
            got = eng.stretch_frames(a, out_fmt=fmt, normalize=0.9)
            gain = np.float32(eng.last_gain)
            peak = np.abs(ref).max()
            assert np.float32(eng.last_peak) == peak and gain == np.float32(0.9) / peak
            z = (ref * gain).astype(np.float32)
            check_result(got, want_bytes(z, fmt, mode), fmt, ref.shape[0], 2)
            assert eng.last_clipped == count_clipped(z)


def test_with_a_fade_a_channel_map_and_a_host_frequency_kernel():
    a = noise_i16(30001, 2, 12)
    with rocoder_amd.Engine(window_len=1024, factor=2.0, channels=2, seed=3) as eng:
        n_out = eng.output_len(30001)
        eng.set_output_fade(5000, n_out - 7000, 7000)
        ref = eng.stretch_frames(a)  # (with the same fade)
        eng.set_output_dither("tpdf-hp", SEED)
        check_result(eng.stretch_frames(a, out_fmt="i16"), want_bytes(ref, "i16", "tpdf-hp"), "i16", n_out, 2)
        assert eng.last_clipped == count_clipped(ref)
        eng.set_output_fade()
        eng.set_channel_map([1, 0])
        ref = eng.stretch_frames(a)  # (with the same map: the dither is keyed by the job's row, not by the source channel)
        check_result(eng.stretch_frames(a, out_fmt="u8"), want_bytes(ref, "u8", "tpdf-hp"), "u8", n_out, 2)
    with rocoder_amd.Engine(window_len=1024, factor=2.0, channels=2, seed=3, kernel=lambda t, x: 2.0 * x, kernel_time_ms=1) as eng:
        ref = eng.stretch_frames(a)
        eng.set_output_dither("tpdf", SEED)
        check_result(eng.stretch_frames(a, out_fmt="i16"), want_bytes(ref, "i16", "tpdf"), "i16", ref.shape[0], 2)
        assert eng.last_clipped == count_clipped(ref)
        got = eng.stretch_frames(a, out_fmt="i24", normalize=0.5)
        z = (ref * np.float32(eng.last_gain)).astype(np.float32)
        check_result(got, want_bytes(z, "i24", "tpdf"), "i24", ref.shape[0], 2)


def run_cli(*args):
    r = subprocess.run([CLI, *args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return r


def test_cli_dither_on_the_gpu_and_on_the_host_write_the_same_file(tmp_path):
    """--output-format i16 --dither tpdf-hp --dither-seed 7 with and without --frames-on-gpu: one file, whose data chunk
    is the numpy definition on the f32 file of the same job; without --dither-seed the seed is --seed."""
    x = np.random.default_rng(17).uniform(-1, 1, (2, 5000))
    wav = str(tmp_path / "in.wav")
    write_wav(wav, x, 44100, "i16")
    common = ["-i", wav, "--seed", "5", "-w", "1024", "-f", "4"]
    f32 = str(tmp_path / "f32.wav")
    run_cli(*common, "-o", f32, "--frames-on-gpu")
    ref = np.frombuffer(check_header(open(f32, "rb").read(), "f32", 2, 44100), "<f4").reshape(-1, 2)
    files = []
    for k, extra in enumerate(([], ["--frames-on-gpu"])):
        out = str(tmp_path / f"o{k}.wav")
        run_cli(*common, "-o", out, "--output-format", "i16", "--dither", "tpdf-hp", "--dither-seed", "7", *extra)
        files.append(open(out, "rb").read())
    assert files[0] == files[1]
    assert check_header(files[0], "i16", 2, 44100) == want_bytes(ref, "i16", "tpdf-hp", 7)
    for k, extra in enumerate(([], ["--frames-on-gpu"])):
        out = str(tmp_path / f"s{k}.wav")
        run_cli(*common, "-o", out, "--output-format", "u8", "--dither", "tpdf", *extra)
        assert check_header(open(out, "rb").read(), "u8", 2, 44100) == want_bytes(ref, "u8", "tpdf", 5)
