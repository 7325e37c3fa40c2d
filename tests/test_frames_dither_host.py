"""CPU tests (-m "not gpu") of the dither in front of the PCM quantiser (rc_engine_set_output_dither, --dither): the symbol in
the header, the ctypes table and the Rust block; the status code without an engine; the numpy definition of
tests/ditherutil.py against the pinned known answers (tests/golden/dither_known_answers.json) and against the library's
rc_phase_key / rc_phase_hash; the properties that make it a dither, on fixed inputs; the CLI's host quantiser
(--encode-pcm-dither) against the numpy definition, byte for byte; the CLI's flag checks; the engine's side of the feature
under AddressSanitizer over the HIP stub (tests/c/engine_host_driver_frames_dither.cpp + tests/c/hip_stub_frames_dither.cpp)."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

import ditherutil as D
from conftest import ROOT
from rocoder_amd import _lib
from test_frames_pcm_host import count_clipped, edge_values, quantise
from wavutil import write_wav

CLI = os.environ.get("ROCODER_CLI") or os.path.join(ROOT, "rocoder_amd", "bin", "rocoder")
KNOWN = json.load(open(os.path.join(ROOT, "tests", "golden", "dither_known_answers.json")))
MODES = ["tpdf", "tpdf-hp"]


def test_symbol_in_header_ctypes_table_and_rust_block():
    import ctypes as C

    assert _lib.SYMBOLS["rc_engine_set_output_dither"] == (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint64])
    assert (_lib.RC_DITHER_NONE, _lib.RC_DITHER_TPDF, _lib.RC_DITHER_TPDF_HP) == (0, 1, 2)
    h = open(os.path.join(ROOT, "include", "rocoder_hip.h")).read()
    assert re.search(r"\nint rc_engine_set_output_dither\(rc_engine \*e, uint32_t mode, uint64_t seed\);", h)
    for name, v in (("RC_DITHER_NONE", 0), ("RC_DITHER_TPDF", 1), ("RC_DITHER_TPDF_HP", 2)):
        assert re.search(r"\n#define %s %d\n" % (name, v), h), name
    for s in ("0xFFFFFFFFFF", "(int)(h >> 16) - (int)(h & 0xFFFF)", "not contracted into an fma", "does not give the same bytes"):
        assert s in h, s
    rust = open(os.path.join(ROOT, "integration", "rust", "hip_engine.rs")).read()
    assert re.search(r"pub fn rc_engine_set_output_dither\(e: \*mut RcEngine, mode: u32, seed: u64\) -> c_int;", rust)
    for name, v in (("RC_DITHER_NONE", 0), ("RC_DITHER_TPDF", 1), ("RC_DITHER_TPDF_HP", 2)):
        assert re.search(r"pub const %s: u32 = %d;" % (name, v), rust), name
    assert _lib.lib().rc_abi_version() == 5


def test_setter_returns_einval_without_an_engine():
    L = _lib.lib()
    for mode in (0, 1, 2, 3):
        assert L.rc_engine_set_output_dither(None, mode, 1) == _lib.RC_EINVAL
    assert L.rc_last_error()


def test_numpy_definition_meets_the_pinned_known_answers_and_the_library_draws_the_same():
    L = _lib.lib()
    seed, ts = KNOWN["seed"], KNOWN["t"]
    assert KNOWN["hop"] == 2 ** 40 - 1 == D.DITHER_HOP and ts == [0, 1, 2, 3, 2 ** 32 - 1, 2 ** 32, 2 ** 40 + 3]
    assert KNOWN["keys"] == {"0": "0x9325d380e9db2d08", "1": "0x33b323d83c6543ec"}
    for c in (0, 1):
        k = D.key(seed, c)
        assert k == int(KNOWN["keys"][str(c)], 16) == L.rc_phase_key(seed, c, 0xFFFFFFFFFF)
        h = [L.rc_phase_hash(k, t % 2 ** 32) for t in ts]
        hb = [L.rc_phase_hash(k, (t - 1) % 2 ** 32) for t in ts]
        assert [(a >> 16) - (a & 0xFFFF) for a in h] == KNOWN["i"][f"tpdf/{c}"] == D.draws_i("tpdf", seed, c, ts).tolist()
        assert [(a >> 16) - (b >> 16) for a, b in zip(h, hb)] == KNOWN["i"][f"tpdf-hp/{c}"] == D.draws_i("tpdf-hp", seed, c, ts).tolist()
    assert KNOWN["i"]["tpdf/0"] == [41036, -9767, 14429, -24918, 46879, 41036, -24918]
    assert KNOWN["i"]["tpdf-hp/1"] == [-13317, 33572, -53286, 34990, -1366, -13317, 34990]
    ka = KNOWN["i16_tpdf_seed1_channel0"]
    x = np.array([int(b, 16) for b in ka["x_bits"]], np.uint32).view(np.float32)
    want_x = np.array([1, -1, 1 - 2.0 ** -24, np.nan, np.inf, -np.inf, 0, -0.0], np.float32)
    assert x.tobytes() == want_x.tobytes()
    assert ka["codes"] == [32767, -32767, 32767, 0, 32767, -32768, 1, 0]
    assert D.quantise_dithered(x[:, None], "i16", "tpdf", 1)[:, 0].tolist() == ka["codes"]


@pytest.mark.parametrize("channel", [0, 1, 5])
@pytest.mark.parametrize("mode", MODES)
def test_the_draws_are_a_triangle_of_the_stated_colour(mode, channel):
    """Fixed inputs (seed 1, t = 0 ... 65535): the figures cannot flake. Measured for these seeds and channels: |mean| at
    most 0.0011, variance within 0.0013 of 1/6, lag-1 autocorrelation within 0.003 of 0 (tpdf) and of -0.5 (tpdf-hp)."""
    d = D.dither(mode, 1, channel, np.arange(65536)).astype(np.float64)
    mean, var = d.mean(), d.var()
    e = d - mean
    rho = float((e[1:] * e[:-1]).mean() / var)
    print(f"{mode} channel {channel}: mean {mean:.5f}, var - 1/6 {var - 1 / 6:.5f}, lag-1 autocorrelation {rho:.5f}")
    assert abs(mean) < 0.01
    assert abs(var - 1 / 6) < 0.005
    assert abs(rho - (0.0 if mode == "tpdf" else -0.5)) < 0.02
    assert np.abs(d).max() < 1


@pytest.mark.parametrize("channel", [0, 1, 5])
@pytest.mark.parametrize("mode", MODES)
def test_what_the_dither_is_for(mode, channel):
    """i16 of a constant of 0.3 LSB and of a sine of 0.4 LSB, period 64: undithered both are all zeros; dithered, the mean
    is 0.3 and the sine comes back at 0.4 (measured: within 0.002 of both)."""
    n = 65536
    const = np.full((n, 1), np.float32(0.3) / np.float32(32767), np.float32)
    assert not quantise(const, "i16").any()
    q = D.quantise_dithered(const, "i16", mode, 1, channel0=channel)
    print(f"{mode} channel {channel}: mean code of 0.3 LSB {q.mean():.5f}")
    assert abs(q.mean() - 0.3) < 0.01
    s = np.sin(2 * np.pi * np.arange(n) / 64)
    sine = (np.float32(0.4) * s.astype(np.float32) / np.float32(32767)).astype(np.float32)[:, None]
    assert not quantise(sine, "i16").any()
    q = D.quantise_dithered(sine, "i16", mode, 1, channel0=channel)[:, 0]
    amp = 2 * float((q * s).mean())  # the amplitude of the component in phase with the sine
    print(f"{mode} channel {channel}: 0.4 LSB sine comes back at {amp:.5f}")
    assert abs(amp - 0.4) < 0.02


@pytest.mark.parametrize("t0", [0, 2 ** 32 - 7])
@pytest.mark.parametrize("ch", [1, 3])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("fmt", D.DITHER_FORMATS)
def test_cli_host_quantiser_equals_the_numpy_definition(tmp_path, fmt, mode, ch, t0):
    x = edge_values()
    x = x[:x.size // ch * ch].reshape(-1, ch)
    src, dst = str(tmp_path / "x.f32"), str(tmp_path / "y.raw")
    x.tofile(src)
    r = subprocess.run([CLI, "--encode-pcm-dither", fmt, mode, "1", str(ch), str(t0), src, dst], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    assert r.stdout.split() == [str(x.shape[0]), str(count_clipped(x))]
    got = np.frombuffer(open(dst, "rb").read(), np.uint8)
    want = D.dithered_bytes(x, fmt, mode, 1, t0=t0)
    assert got.size == want.size
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (fmt, mode, ch, t0, bad.size, bad[:8].tolist())
    # and it is a dither: the bytes differ from the undithered ones
    assert (want != D.dithered_bytes(x, fmt, "none", 1)).any()


def test_cli_hook_with_mode_none_is_the_undithered_quantiser(tmp_path):
    x = edge_values()[:, None]
    src, dst, und = str(tmp_path / "x.f32"), str(tmp_path / "y.raw"), str(tmp_path / "u.raw")
    x.tofile(src)
    for fmt in D.DITHER_FORMATS:
        assert subprocess.run([CLI, "--encode-pcm-dither", fmt, "none", "1", "1", "0", src, dst], capture_output=True, timeout=60).returncode == 0
        assert subprocess.run([CLI, "--encode-pcm", fmt, src, und], capture_output=True, timeout=60).returncode == 0
        assert open(dst, "rb").read() == open(und, "rb").read()


@pytest.mark.parametrize("extra", [["--output-format", "f32"], ["--output-format", "i32"], []])
def test_cli_refuses_dither_without_an_8_16_or_24_bit_output_format(tmp_path, extra):
    wav, out = str(tmp_path / "in.wav"), str(tmp_path / "out.wav")
    write_wav(wav, np.zeros((1, 2000)), 44100, "i16")
    r = subprocess.run([CLI, "-i", wav, "-o", out, "-w", "1024", "--dither", "tpdf", *extra], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "--dither" in r.stderr and "--output-format" in r.stderr, (r.returncode, r.stderr)
    assert not os.path.exists(out)
    r = subprocess.run([CLI, "-i", wav, "-o", out, "-w", "1024", "--dither", "blue", "--output-format", "i16"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "--dither" in r.stderr


def test_help_and_readme_name_the_flags():
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60)
    text = r.stdout + r.stderr
    assert "--dither <mode>" in text and "--dither-seed" in text and "tpdf-hp" in text
    assert "--dither" in open(os.path.join(ROOT, "README.md")).read()


def test_engine_frames_dither_is_clean_under_asan():
    """Several pipeline chunks with every byte marked by its absolute frame, targets at all four byte phases, both entries,
    formats that do and do not dither, a host frequency kernel, the setter's errors, jobs of 0 and 1 frames. A stand-alone
    program: nothing is loaded into python."""
    from test_engine_host_sanitized import _build

    exe = _build("engine_frames_dither_asan")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert r.stdout.splitlines()[-1] == "engine_host_driver_frames_dither: ok"
