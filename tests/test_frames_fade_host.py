"""CPU tests (-m "not gpu") of the output fade (rc_engine_set_output_fade, --fade-output): the numpy statement of the
definition (tests/fadeutil.py) against the reference's own known answers (tests/golden/fade_known_answers.json) and
against exact arithmetic; the symbol in the header, the ctypes table and the Rust block; status codes without a device;
the engine's cut of every pipeline chunk with the fade ranges under AddressSanitizer over the HIP stub
(tests/c/engine_host_driver_frames_fade.cpp + tests/c/hip_stub_frames_fade.cpp, a stand-alone program); the CLI's
argument checks. The tests of tests/fadeutil.py alone (the known answers, the rounding of long frame counts, the edges)
check the yardstick, not the feature: they are what makes the GPU tests' byte comparisons mean something."""
import ctypes as C
import json
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from conftest import ROOT
from fadeutil import NONE, apply_fade, sq
from rocoder_amd import _lib

CLI = os.environ.get("ROCODER_CLI") or os.path.join(ROOT, "rocoder_amd", "bin", "rocoder")
NAME = "rc_engine_set_output_fade"


@pytest.fixture(scope="module")
def known():
    with open(os.path.join(ROOT, "tests", "golden", "fade_known_answers.json")) as f:
        return json.load(f)


def test_the_definition_reproduces_the_references_known_answers(known):
    """fade_in_at_sample(3, 4) zeroes the frames in front of its start and fades from there; the engine's fade-in starts
    at frame 0, so the start offset is a slice: frames 3 ... 9 through a fade-in of 4. fade_out_at_sample(3, 4) is the
    engine's (0, 3, 4) as it stands."""
    x = np.array(known["input"], np.float32)
    s, d, tol = known["start"], known["dur"], known["tolerance"]
    want_in = np.array(known["fade_in_at_sample"], np.float64)
    want_out = np.array(known["fade_out_at_sample"], np.float64)
    assert not want_in[:s].any()
    got_in = apply_fade(x[s:], in_len=d)
    got_out = apply_fade(x, out_start=s, out_len=d)
    assert np.abs(got_in - want_in[s:]).max() <= tol and np.abs(got_out - want_out).max() <= tol
    # the interior values exactly: r = 0.25, 0.5, 0.75 hand 0.25, 0.5, 0.75 to the square root
    exact = [np.float32(0.5), np.sqrt(np.float32(0.5)), np.sqrt(np.float32(0.75))]
    assert got_in[0] == 0 and list(got_in[1:d]) == exact and (got_in[d:] == 1).all()
    assert got_out[s] == 1 and list(got_out[s + 1:s + d]) == exact[::-1] and (got_out[:s] == 1).all()
    assert got_out[s + d:].view(np.uint32).tolist() == [0, 0, 0]
    assert got_in.dtype == np.float32 and got_out.dtype == np.float32


def f32_of(q):
    """the float32 nearest to the Fraction q > 0, ties to even, by exact arithmetic (normal range)"""
    e = 0
    while q >= 2 ** 24:
        q, e = q / 2, e + 1
    while q < 2 ** 23:
        q, e = q * 2, e - 1
    n, rest = divmod(q, 1)
    n = int(n) + (1 if rest > Fraction(1, 2) or (rest == Fraction(1, 2) and int(n) % 2) else 0)
    return np.float32(n * 2.0 ** e)


def test_frame_counts_above_2_to_24_are_rounded_to_nearest_even():
    """(float)p and (float)d of the definition, and their quotient, against exact arithmetic"""
    d = 2 ** 24 + 1 + 3
    for p in (0, 1, 2 ** 24 - 1, 2 ** 24, 2 ** 24 + 1, 2 ** 24 + 2, 2 ** 24 + 3, d - 1):
        pf, df = f32_of(Fraction(p)) if p else np.float32(0), f32_of(Fraction(d))
        assert float(df) == 2 ** 24 + 4 and float(pf) in (p, p - 1, p + 1)
        r = f32_of(Fraction(float(pf)) / Fraction(float(df))) if p else np.float32(0)
        b = np.float32(r * np.float32(2) - np.float32(1))
        for falling in (False, True):
            want = np.sqrt(np.float32(0.5) * (np.float32(1) + max(-b if falling else b, np.float32(-1))))
            assert sq([p], d, falling)[0] == want, (p, falling)
    assert np.array([2 ** 24 + 1, 2 ** 24 + 3, 2 ** 63 + 2 ** 39], np.uint64).astype(np.float32).tolist() == \
        [2.0 ** 24, 2.0 ** 24 + 4, 2.0 ** 63]


def test_the_definition_on_its_edges():
    y = np.array([[1.0, -2.0], [np.nan, 3.0], [-0.0, -5.0], [np.inf, 1e-40], [np.nan, -7.0], [-1.0, np.nan]], np.float32)
    assert apply_fade(y).tobytes() == y.tobytes() and apply_fade(y, 0, 6, 0).tobytes() == y.tobytes()
    z = apply_fade(y, 0, 4, 0)  # a hard cut: +0.0 for NaN, for negative values, for everything
    assert z[:4].tobytes() == y[:4].tobytes() and not z[4:].view(np.uint32).any()
    z = apply_fade(y, 2, NONE, 0)  # p = 0 silences the first frame; NaN stays NaN
    assert z[0].tolist() == [0.0, -0.0] and np.isnan(z[1, 0]) and z[1, 1] == np.float32(3) * np.sqrt(np.float32(0.5))
    assert z[2:].tobytes() == y[2:].tobytes()
    z = apply_fade(y, 4, 2, 3)  # both ranges on frames 2 and 3: two multiplications, the fade-in's first
    up, down = sq(np.arange(4), 4, False), sq(np.arange(3), 3, True)
    assert z[2, 1] == (np.float32(-5) * up[2]) * down[0] and z[3, 1] == (np.float32(1e-40) * up[3]) * down[1]
    assert z[4, 1] == np.float32(-7) * down[2] and z[5].view(np.uint32).tolist() == [0, 0]
    assert apply_fade(y.T, 4, 2, 3, axis=1).tobytes() == z.T.tobytes()  # planar rows: the same envelope on every row
    with pytest.raises(AssertionError):
        apply_fade(y, 7)
    with pytest.raises(AssertionError):
        apply_fade(y, 0, 5, 2)


def test_the_symbol_is_declared_in_every_binding():
    assert NAME in _lib.SYMBOLS
    assert _lib.SYMBOLS[NAME] == (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64])
    assert _lib.RC_FADE_NONE == NONE
    assert hasattr(_lib.lib(), NAME)
    h = open(os.path.join(ROOT, "include", "rocoder_hip.h")).read()
    m = re.search(r"\nint rc_engine_set_output_fade\(([^;]*)\);", h)
    assert m and re.sub(r"\s+", " ", m.group(1)) == "rc_engine *e, uint64_t in_len, uint64_t out_start, uint64_t out_len"
    assert "#define RC_FADE_NONE UINT64_MAX" in h
    for s in ("fade_in_at_sample", "fade_out_at_sample", "sqrt_interp", "+0.0f", "rc_multi", "round to\n *          nearest even"):
        assert s in h, s
    rust = open(os.path.join(ROOT, "integration", "rust", "hip_engine.rs")).read()
    m = re.search(r"pub fn rc_engine_set_output_fade\(([^;]*)\) -> c_int;", rust)
    assert m and m.group(1) == "e: *mut RcEngine, in_len: u64, out_start: u64, out_len: u64"
    assert _lib.lib().rc_abi_version() == 5
    from rocoder_amd.stretcher import Engine

    assert callable(Engine.set_output_fade)


def test_the_setter_and_the_engine_bookkeeping_under_asan():
    """The stand-alone driver over the HIP stub, under ASan + UBSan. It is also the only place where an engine exists
    without a device, so it holds the setter's codes - clearing is RC_OK, a wrapping sum is RC_EINVAL - and prints them.
    All four whole-job host-form entries, several pipeline chunks, a host kernel, fades at every edge: every sample of a
    fade range through the fade launcher exactly once, in front of the peak launch and the pack launch or download that
    read it, no other sample, and nothing at all on an error."""
    from test_engine_host_sanitized import _build

    assert _lib.lib().rc_engine_set_output_fade(None, 0, NONE, 0) == _lib.RC_EINVAL  # (no engine: no fade to set)
    exe = _build("engine_frames_fade_asan")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    lines = r.stdout.splitlines()
    assert lines[0] == f"setter: clear {_lib.RC_OK}, wrap {_lib.RC_EINVAL}, none with a length {_lib.RC_EINVAL}, " \
                       f"null engine {_lib.RC_EINVAL}", lines[0]
    assert lines[-1] == "engine_host_driver_frames_fade: ok"


def test_python_wrapper_checks_the_counts_before_it_touches_an_engine():
    from rocoder_amd.stretcher import Engine

    eng = object.__new__(Engine)  # (no engine behind it: the check comes first)
    for bad in ((-1, None, 0), (0, -5, 0), (0, 3, 2 ** 64), (2 ** 64, None, 0)):
        with pytest.raises(ValueError, match="unsigned 64-bit"):
            Engine.set_output_fade(eng, *bad)


def run(*args):
    return subprocess.run([CLI, *args], capture_output=True, text=True, timeout=60)


def test_cli_names_the_flag_and_needs_frames_on_gpu(tmp_path):
    r = run("--help")
    assert r.returncode == 0 and "--fade-output" in r.stderr
    out = str(tmp_path / "o.wav")
    r = run("-i", "a.wav", "-o", out, "--fade-output", "-x", "0.01")
    assert r.returncode != 0 and "--fade-output" in r.stderr and "--frames-on-gpu" in r.stderr, r.stderr
    assert not os.path.exists(out)
    assert "--fade-output" in open(os.path.join(ROOT, "README.md")).read()
