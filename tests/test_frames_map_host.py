"""CPU tests (-m "not gpu") of the channel-map entries (rc_engine_set_channel_map, rc_engine_frames_channel_peaks,
rc_split_mono_map): rc_split_mono_map against the numpy restatement of the reference's auto_split_mono
(tests/splitmonoutil.py) on every pattern of silent and live channels, for NaN and inf peaks and for its status codes; the
symbols in the header, the ctypes table and the Rust block; what the engine entries reject before they touch a device; the
CLI's argument checks for --channel-map and --split-mono."""
import ctypes as C
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import splitmonoutil as sm
from conftest import ROOT
from rocoder_amd import _lib, split_mono_map
from wavutil import write_wav

NAMES = ("rc_engine_set_channel_map", "rc_engine_frames_channel_peaks", "rc_split_mono_map")
EINVAL = _lib.RC_EINVAL
CLI = os.environ.get("ROCODER_CLI") or os.path.join(ROOT, "rocoder_amd", "bin", "rocoder")
U32P, F32P = C.POINTER(C.c_uint32), C.POINTER(C.c_float)


def split(peaks, channels=None):
    """rc_split_mono_map itself: (status, map, found); the map starts as 99s and found as 13"""
    peaks = np.ascontiguousarray(peaks, np.float32)
    n = peaks.size if channels is None else channels
    out = np.full(max(peaks.size, 1) + 1, 99, np.uint32)
    found = C.c_int(13)
    rc = _lib.lib().rc_split_mono_map(peaks.ctypes.data_as(F32P), n, out.ctypes.data_as(U32P), C.byref(found))
    assert out[peaks.size:].tolist() == [99] * (out.size - peaks.size)  # nothing behind the map
    return rc, out[:peaks.size].tolist(), found.value


def test_the_restatement_on_the_references_cases():
    """the yardstick itself: one live channel among silent ones is copied; anything else is left alone"""
    assert sm.split_mono_map([0.0, 0.5]) == ([1, 1], True) and sm.split_mono_map([0.5, 0.0]) == ([0, 0], True)
    assert sm.split_mono_map([0.5, 0.5]) == ([0, 1], False) and sm.split_mono_map([0.0, 0.0]) == ([0, 1], False)
    assert sm.split_mono_map([0.25]) == ([0], True) and sm.split_mono_map([0.0]) == ([0], False)
    assert sm.split_mono_map([-0.0, np.nan, 0.0]) == ([1, 1, 1], True)
    x = np.array([[0.0, -0.0, np.nan], [-2.0, 0.0, 1.0], [1.0, -0.0, np.inf], [1e-45, 0.0, 3.0]], np.float32)
    assert sm.channel_peaks(x).view(np.uint32).tolist() == [0x40000000, 0, 0x7FC00000]
    assert sm.channel_peaks(x[1:]).view(np.uint32).tolist() == [0x40000000, 0, 0x7F800000]
    assert sm.channel_peaks(x[:0]).view(np.uint32).tolist() == [0, 0, 0]
    assert sm.raw_channel_peaks(bytes([0, 255, 128, 128]), "u8", 2).tolist() == [np.float32(128) / np.float32(127), 1.0]


VALUES = (0.0, -0.0, 0.5, np.float32(1e-45), np.inf, np.nan)


@pytest.mark.parametrize("channels", [1, 2, 3, 4])
def test_split_mono_map_on_every_pattern(channels):
    """every pattern of silent and live channels, the live ones finite, denormal, inf or NaN, the silent ones +-0"""
    seen = {True: 0, False: 0}
    for pattern in itertools.product(VALUES, repeat=channels):
        want_map, want_found = sm.split_mono_map(pattern)
        assert split(pattern) == (0, want_map, int(want_found)), pattern
        assert split_mono_map(pattern) == (want_map, want_found), pattern
        seen[want_found] += 1
    assert seen[True] >= channels and seen[False] >= 1


def test_split_mono_map_five_channels():
    for live in range(5):
        peaks = np.zeros(5, np.float32)
        peaks[live] = 0.125
        assert split(peaks) == (0, [live] * 5, 1)
        peaks[(live + 2) % 5] = 1.0
        assert split(peaks) == (0, [0, 1, 2, 3, 4], 0)
    assert split(np.zeros(5, np.float32)) == (0, [0, 1, 2, 3, 4], 0)
    assert split(np.full(5, np.nan, np.float32)) == (0, [0, 1, 2, 3, 4], 0)


def test_split_mono_map_status_codes():
    peaks = np.array([0.0, 1.0], np.float32)
    assert split(peaks, channels=0) == (EINVAL, [99, 99], 13)
    L = _lib.lib()
    out = np.full(2, 99, np.uint32)
    found = C.c_int(13)
    p, m = peaks.ctypes.data_as(F32P), out.ctypes.data_as(U32P)
    assert L.rc_split_mono_map(None, 2, m, C.byref(found)) == EINVAL
    assert L.rc_split_mono_map(p, 2, None, C.byref(found)) == EINVAL
    assert L.rc_split_mono_map(p, 2, m, None) == EINVAL
    assert out.tolist() == [99, 99] and found.value == 13
    with pytest.raises(_lib.RocoderError):
        split_mono_map([])


def test_the_symbols_are_in_the_header_the_ctypes_table_and_the_rust_block():
    h = open(os.path.join(ROOT, "include", "rocoder_hip.h")).read()
    rust = open(os.path.join(ROOT, "integration", "rust", "hip_engine.rs")).read()
    for name in NAMES:
        assert re.search(r"^int %s\(" % name, h, re.M), name
        assert name in _lib.SYMBOLS and hasattr(_lib.lib(), name)
        assert re.search(r"pub fn %s\(" % name, rust), name
    assert int(re.search(r"#define RC_ABI_VERSION (\d+)", h).group(1)) == 5


def test_the_engine_entries_reject_a_null_engine_and_write_nothing():
    L = _lib.lib()
    out = np.full(4, 7.0, np.float32)
    rc = L.rc_engine_frames_channel_peaks(None, C.c_void_p(out.ctypes.data), 1, _lib.RC_PCM_F32, out.ctypes.data_as(F32P), 4)
    assert rc == EINVAL and (out == 7).all()
    m = np.array([1, 0], np.uint32)
    assert L.rc_engine_set_channel_map(None, m.ctypes.data_as(U32P), 2) == EINVAL and m.tolist() == [1, 0]
    assert L.rc_engine_set_channel_map(None, None, 0) == EINVAL


# ---- the CLI's argument checks -----------------------------------------------------------------------------------------
def cli(tmp_path, *args, wav=None):
    out = str(tmp_path / "o.wav")
    src = str(tmp_path / "missing.wav") if wav is None else wav
    r = subprocess.run([CLI, "-i", src, "-o", out, *args], capture_output=True, text=True, timeout=60)
    assert not os.path.exists(out) and not os.path.exists(out + ".part")
    assert r.returncode != 0 and len(r.stderr.strip().splitlines()) == 1, (r.returncode, r.stderr)
    return r


def test_each_flag_needs_frames_on_gpu(tmp_path):
    assert "--channel-map needs --frames-on-gpu" in cli(tmp_path, "--channel-map", "1,0").stderr
    assert "--split-mono needs --frames-on-gpu" in cli(tmp_path, "--split-mono").stderr


@pytest.mark.parametrize("v", ["", "1,", ",1", "1,,0", "a,b", "1;0", "-1,0", "0x1,0", "1.0,0", "70000,0", "1 0"])
def test_a_malformed_list(tmp_path, v):
    r = cli(tmp_path, "--frames-on-gpu", "--channel-map", v)
    assert "--channel-map takes a list of channel indices" in r.stderr


def test_a_valid_list_reaches_the_input(tmp_path):
    assert "cannot open" in cli(tmp_path, "--frames-on-gpu", "--channel-map", "1,0", "--split-mono").stderr


@pytest.fixture()
def stereo(tmp_path):
    path = str(tmp_path / "stereo.wav")
    write_wav(path, np.zeros((2, 64)), 44100, "i16")
    return path


@pytest.mark.parametrize("v,what", [("0", "1 entries"), ("0,1,0", "3 entries"), ("0,2", "names channel 2"), ("2,2", "names channel 2"),
                                    ("65535,0", "names channel 65535")])
def test_a_list_that_does_not_fit_the_file(tmp_path, stereo, v, what):
    """the wrong count or an index out of range: one error line and exit status 2, once the file's header is read and
    before any engine work (no device is needed to get there)"""
    r = cli(tmp_path, "--frames-on-gpu", "--channel-map", v, wav=stereo)
    assert r.returncode == 2 and "--channel-map" in r.stderr and what in r.stderr


def test_usage_names_the_flags():
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60)
    text = r.stdout + r.stderr
    assert "--channel-map" in text and "--split-mono" in text
    # under --frames-on-gpu the rotation is spelled --channel-map
    assert "--channel-map 1,0" in text and "(c + C - 1) % C" in text
