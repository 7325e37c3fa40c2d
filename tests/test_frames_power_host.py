"""CPU tests (-m "not gpu") of the autocrop entries (rc_frames_power_bins, rc_engine_frames_power, rc_autocrop_points):
the numpy statement of the definition (tests/autocroputil.py) against the reference's own known answers
(tests/golden/autocrop_known_answers.json), which checks the yardstick; rc_autocrop_points against those answers, against
the restatement on seeded random lists and for its status codes; the bin count; the symbols in the header, the ctypes table
and the Rust block; what rc_engine_frames_power rejects before it touches a device."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import autocroputil as au
from conftest import ROOT
from rocoder_amd import _lib, autocrop_points

NAMES = ("rc_frames_power_bins", "rc_engine_frames_power", "rc_autocrop_points")
EINVAL = _lib.RC_EINVAL


@pytest.fixture(scope="module")
def known():
    with open(os.path.join(ROOT, "tests", "golden", "autocrop_known_answers.json")) as f:
        return json.load(f)


def points(peaks, bin_frames, n_frames, percentile):
    """rc_autocrop_points itself: (status, start, end, found); the out-words start as 11, 12, 13"""
    peaks = np.ascontiguousarray(peaks, np.float32)
    start, end, found = C.c_uint64(11), C.c_uint64(12), C.c_int(13)
    rc = _lib.lib().rc_autocrop_points(peaks.ctypes.data_as(C.POINTER(C.c_float)), peaks.size, bin_frames, n_frames, percentile,
                                       C.byref(start), C.byref(end), C.byref(found))
    return rc, start.value, end.value, found.value


def test_the_restatement_reproduces_the_references_known_answers(known):
    k = known["autocrop_points"]
    assert au.crop_bins(k["amplitudes"], k["percentile"]) == (k["start"], k["end"])
    k = known["autocrop_points_none"]
    assert au.crop_bins(k["amplitudes"], k["percentile"]) is None
    k = known["noise_threshold"]
    for p, want in zip(k["percentiles"], k["thresholds"]):
        assert au.noise_threshold(k["amplitudes"], p) == np.float32(want)
    k = known["relative_decibels"]
    want = np.array(k["decibels"], np.float32)  # (the reference compares f32 values: -99999999.0 is -1e8 there)
    assert au.decibels(k["amplitudes"])[0] == want[0] == au.MIN_DECIBELS
    assert np.abs(au.decibels(k["amplitudes"]).astype(np.float64) - want).max() <= k["tolerance"]
    k = known["chunked_audio_power"]
    x = np.array(k["channels"], np.float32).T
    peaks = au.bin_peaks(x, k["bin_frames"])
    assert peaks.dtype == np.float32 and peaks.tolist() == [np.float32(0.3), np.float32(0.9), np.float32(0.7)]
    assert list(range(0, x.shape[0], k["bin_frames"])) == k["bin_starts"]
    assert np.abs(au.decibels(peaks).astype(np.float64) - np.array(k["decibels"])).max() <= k["tolerance"]
    k = known["autocrop_audio"]
    x = np.array(k["channels"], np.float32).T
    start, end = au.autocrop_points(au.bin_peaks(x, k["bin_frames"]), k["bin_frames"], k["percentile"])
    assert x[start:end].T.tolist() == np.array(k["cropped"], np.float32).tolist()


def test_the_restatements_decode_and_peaks():
    """the corners of the definition in the yardstick itself: u8's 128/127, INT32_MIN, NaN skipped, -0.0, inf, a ragged bin"""
    assert au.decode(bytes([0, 255, 128]), "u8", 1)[:, 0].tolist() == [np.float32(-128) / np.float32(127), np.float32(1), 0]
    x = au.decode(np.array([-2 ** 31, 2 ** 31 - 1, 2 ** 24 + 1], "<i4").tobytes(), "i32", 1)[:, 0]
    assert x.tolist() == [-1.0, 1.0, np.float32(2 ** 24) / np.float32(2 ** 31)]
    assert au.decode(bytes([0, 0, 0x80, 0xff, 0xff, 0x7f]), "i24", 2).tolist() == [[-1.0, np.float32(8388607) / np.float32(8388608)]]
    f = np.array([[np.nan, -0.0], [np.nan, np.nan], [-3.0, 2.0], [-np.inf, 1.0], [1e-45, 0.0]], np.float32)
    got = au.bin_peaks(f, 1)
    assert got.view(np.uint32).tolist() == np.array([0, 0, 3, np.inf, 1e-45], np.float32).view(np.uint32).tolist()
    assert au.bin_peaks(f, 2).tolist() == [0.0, np.inf, np.float32(1e-45)] and au.bin_peaks(f[:0], 3).size == 0


def test_autocrop_points_agrees_with_the_known_answers(known):
    k = known["autocrop_points"]
    n = len(k["amplitudes"])
    assert points(k["amplitudes"], 1, n, k["percentile"]) == (0, k["start"], k["end"], 1)
    assert points(k["amplitudes"], 4410, n * 4410 - 17, k["percentile"]) == (0, k["start"] * 4410, k["end"] * 4410, 1)
    assert autocrop_points(k["amplitudes"], 1, n, k["percentile"]) == (k["start"], k["end"])
    k = known["autocrop_points_none"]
    assert points(k["amplitudes"], 5, 13, k["percentile"]) == (0, 0, 13, 0)
    assert autocrop_points(k["amplitudes"], 5, 13, k["percentile"]) is None
    k = known["autocrop_audio"]
    x = np.array(k["channels"], np.float32).T
    rc, start, end, found = points(au.bin_peaks(x, 1), 1, x.shape[0], k["percentile"])
    assert (rc, found) == (0, 1) and x[start:end].T.tolist() == np.array(k["cropped"], np.float32).tolist()


def random_lists():
    """A few hundred seeded lists of 1 ... 64 bins. Every value is +0, +inf or a rung of a ladder whose neighbours are 2 %
    apart: any two bins are bit-equal or differ by at least 1 % (0.086 dB), four orders above what a log10f can round away."""
    rng = np.random.default_rng(20261018)
    ladder = (1e-4 * 1.02 ** np.arange(600)).astype(np.float32)  # 1e-4 ... 14.5
    out = []
    for i in range(400):
        n = int(rng.integers(1, 65))
        kind = i % 8
        v = ladder[rng.integers(0, ladder.size, n)].copy()
        if kind == 0:
            v[:] = v[0]  # all equal
        elif kind == 1:
            v[-1] = ladder[-1]  # the last bin is the loudest: the quirk
        elif kind == 2:
            v[rng.random(n) < 0.5] = 0
        elif kind == 3:
            v[rng.random(n) < 0.2] = np.inf
        elif kind == 4:
            v[:] = 0
        elif kind == 5:
            v = ladder[rng.integers(0, 3, n)].copy()  # many ties
        out.append((v, int(rng.integers(0, 100)), int(rng.integers(1, 50000))))
    return out


def test_autocrop_points_agrees_with_the_restatement_on_random_lists():
    seen = {"none": 0, "quirk": 0, "inf": 0, "equal": 0}
    for v, percentile, bin_frames in random_lists():
        pos = np.unique(v[(v > 0) & np.isfinite(v)]).astype(np.float64)
        assert 1 <= v.size <= 64 and 0 <= percentile <= 99 and (pos[1:] >= 1.01 * pos[:-1]).all()
        n_frames = (v.size - 1) * bin_frames + 1 + (percentile * 7919) % bin_frames  # a ragged or a whole last bin
        want = au.autocrop_points(v, bin_frames, percentile)
        got = points(v, bin_frames, n_frames, percentile)
        assert got == ((0, 0, n_frames, 0) if want is None else (0, want[0], want[1], 1)), (v.tolist(), percentile, bin_frames)
        seen["none"] += want is None
        seen["quirk"] += want is not None and v.size > 1 and au.decibels(v)[-1] > au.noise_threshold(au.decibels(v), percentile)
        seen["inf"] += bool(np.isinf(v).any())
        seen["equal"] += bool((v == v[0]).all())
    assert min(seen.values()) >= 10, seen


def test_autocrop_points_status_codes():
    peaks = np.array([0.0, 0.1, 1.0, 0.4, 0.8, 1.0, 0.1, 0.0], np.float32)
    assert points(peaks, 1, 8, 25)[0] == 0
    untouched = (EINVAL, 11, 12, 13)
    assert points(peaks[:0], 1, 0, 25) == untouched          # no bins
    assert points(peaks, 1, 8, 100) == untouched             # the index leaves the array
    assert points(peaks, 1, 8, 2 ** 32 - 1) == untouched
    assert points(peaks, 0, 8, 25) == untouched              # bin_frames == 0
    assert points(peaks, 1, 7, 25) == untouched and points(peaks, 1, 9, 25) == untouched and points(peaks, 2, 8, 25) == untouched
    bad = peaks.copy()
    bad[3] = np.nan
    assert points(bad, 1, 8, 25) == untouched
    assert points(peaks, 1, 8, 99)[0] == 0
    L = _lib.lib()
    a, b, f = C.c_uint64(0), C.c_uint64(0), C.c_int(0)
    p = peaks.ctypes.data_as(C.POINTER(C.c_float))
    assert L.rc_autocrop_points(None, 8, 1, 8, 25, C.byref(a), C.byref(b), C.byref(f)) == EINVAL
    assert L.rc_autocrop_points(p, 8, 1, 8, 25, None, C.byref(b), C.byref(f)) == EINVAL
    assert L.rc_autocrop_points(p, 8, 1, 8, 25, C.byref(a), None, C.byref(f)) == EINVAL
    assert L.rc_autocrop_points(p, 8, 1, 8, 25, C.byref(a), C.byref(b), None) == EINVAL
    with pytest.raises(_lib.RocoderError):
        autocrop_points(peaks, 1, 8, 100)


def test_frames_power_bins():
    bins = _lib.lib().rc_frames_power_bins
    assert [bins(n, 4410) for n in (0, 1, 4409, 4410, 4411, 8820, 8821)] == [0, 1, 1, 1, 2, 2, 3]
    assert bins(5, 1) == 5 and bins(5, 0) == 0 and bins(0, 0) == 0 and bins(5, 2 ** 64 - 1) == 1
    assert bins(2 ** 64 - 1, 2) == 2 ** 63 and bins(2 ** 64 - 1, 1) == 2 ** 64 - 1


def test_the_symbols_are_in_the_header_the_ctypes_table_and_the_rust_block():
    h = open(os.path.join(ROOT, "include", "rocoder_hip.h")).read()
    rust = open(os.path.join(ROOT, "integration", "rust", "hip_engine.rs")).read()
    for name in NAMES:
        assert re.search(r"^(?:int|size_t) %s\(" % name, h, re.M), name
        assert name in _lib.SYMBOLS and hasattr(_lib.lib(), name)
        assert re.search(r"pub fn %s\(" % name, rust), name
    assert int(re.search(r"#define RC_ABI_VERSION (\d+)", h).group(1)) == 5


def test_frames_power_rejects_before_it_touches_a_device():
    """without an engine there is one check to reach: a null engine is RC_EINVAL and nothing is written"""
    out = np.full(4, 7.0, np.float32)
    n = C.c_size_t(99)
    rc = _lib.lib().rc_engine_frames_power(None, C.c_void_p(out.ctypes.data), 4, _lib.RC_PCM_F32, 1,
                                           out.ctypes.data_as(C.POINTER(C.c_float)), 4, C.byref(n))
    assert rc == EINVAL and n.value == 99 and (out == 7).all()
