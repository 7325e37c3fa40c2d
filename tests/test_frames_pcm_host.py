"""CPU tests (-m "not gpu") of integer PCM output (rc_engine_stretch_frames_pcm, --output-format): the symbol in the
header, the ctypes table and the Rust block; status codes without a device; the engine's arithmetic on the output block
under AddressSanitizer over the HIP stub (tests/c/engine_host_driver_frames_pcm.cpp + tests/c/hip_stub_frames_pcm.cpp);
the CLI's host quantiser against the numpy formula of include/rocoder_hip.h on a table of edge values; the WAV header of
every format."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from rocoder_amd import _lib

CLI = os.environ.get("ROCODER_CLI") or os.path.join(ROOT, "rocoder_amd", "bin", "rocoder")

# format -> (S, LO, HI, bytes): the table of include/rocoder_hip.h
PCM = {"u8": (127, -128, 127, 1), "i16": (32767, -32768, 32767, 2), "i24": (8388608, -8388608, 8388607, 3),
       "i32": (2147483647, -2147483648, 2147483647, 4)}


def quantise(x, fmt):
    """The definition: one f32 multiplication, rint (ties to even), NaN -> 0, clamp. Returns int64."""
    s, lo, hi, _ = PCM[fmt]
    with np.errstate(invalid="ignore", over="ignore"):
        t = (np.asarray(x, np.float32) * np.float32(s)).astype(np.float32)
        r = np.where(np.isnan(t), 0, np.rint(t))
    return np.clip(r.astype(np.float64), lo, hi).astype(np.int64)


def pcm_bytes(q, fmt):
    """int64 samples -> the little-endian bytes of the file"""
    q = np.asarray(q, np.int64).reshape(-1)
    if fmt == "u8":
        return (q + 128).astype(np.uint8).tobytes()
    if fmt == "i16":
        return q.astype("<i2").tobytes()
    if fmt == "i32":
        return q.astype("<i4").tobytes()
    return (q & 0xFFFFFF).astype("<u4").view(np.uint8).reshape(-1, 4)[:, :3].tobytes()


def count_clipped(x):
    with np.errstate(invalid="ignore"):
        return int(np.count_nonzero(~(np.abs(np.asarray(x, np.float32)) <= 1)))


def test_the_symbol_is_declared_in_every_binding():
    assert "rc_engine_stretch_frames_pcm" in _lib.SYMBOLS
    assert len(_lib.SYMBOLS["rc_engine_stretch_frames_pcm"][1]) == 9
    h = open(os.path.join(ROOT, "include", "rocoder_hip.h")).read()
    m = re.search(r"\nint rc_engine_stretch_frames_pcm\(([^;]*)\);", h)
    assert m and m.group(1).count(",") == 8, "header: nine arguments"
    assert "uint64_t *clipped" in m.group(1) and "uint32_t out_format" in m.group(1) and "void *out_frames" in m.group(1)
    for s in ("S 127 ", "S 32767 ", "S 8388608 ", "S 2147483647 ", "ties to even", "no dither"):
        assert s in h, s
    rust = open(os.path.join(ROOT, "integration", "rust", "hip_engine.rs")).read()
    m = re.search(r"pub fn rc_engine_stretch_frames_pcm\(([^;]*)\) -> c_int;", rust)
    assert m and m.group(1).count(",") == 8 and "clipped: *mut u64" in m.group(1)
    assert _lib.lib().rc_abi_version() == 5


def test_entry_point_returns_status_codes_without_an_engine():
    L = _lib.lib()
    src = np.zeros(64, np.uint8)
    out = np.zeros(64, np.uint8)
    n = C.c_size_t(7)
    clipped = C.c_uint64(9)
    for fmt in range(7):
        for ofmt in range(7):
            assert L.rc_engine_stretch_frames_pcm(None, src.ctypes.data, 4, fmt, out.ctypes.data, 16, ofmt, C.byref(n),
                                                  C.byref(clipped)) == _lib.RC_EINVAL
    assert L.rc_engine_stretch_frames_pcm(None, None, 4, 2, out.ctypes.data, 16, 2, None, None) == _lib.RC_EINVAL
    assert L.rc_engine_stretch_frames_pcm(None, src.ctypes.data, 0, 2, None, 0, 2, None, None) == _lib.RC_EINVAL
    assert n.value == 7 and clipped.value == 9 and not out.any()
    assert L.rc_last_error()


def test_engine_frames_pcm_arithmetic_is_clean_under_asan():
    """Every output format, targets at all four byte phases, several chunks whose edges fall inside a dword, 0 and 1
    frames; the output buffer exactly as long as the call says, every byte of it checked."""
    from test_engine_host_sanitized import _build

    exe = _build("engine_frames_pcm_asan")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert r.stdout.startswith("engine_host_driver_frames_pcm: ok")


def edge_values():
    v = [0.0, -0.0, 1.0, -1.0, 1.0 + 2.0 ** -23, -(1.0 + 2.0 ** -23), 1e-40, -1e-40, np.inf, -np.inf, np.nan, 3.7, -3.7]
    for s, _lo, _hi, _b in PCM.values():  # ties: x * S lands on k + 0.5 exactly
        for k in (0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 100.5, -101.5):
            v.append(np.float32(k) / np.float32(s))
    v += list(np.random.default_rng(11).uniform(-1.2, 1.2, 4000))
    return np.array(v, np.float32)


@pytest.mark.parametrize("fmt", ["u8", "i16", "i24", "i32", "f32"])
def test_cli_host_quantiser_equals_the_numpy_formula(tmp_path, fmt):
    x = edge_values()
    src, dst = str(tmp_path / "x.f32"), str(tmp_path / "y.raw")
    x.tofile(src)
    r = subprocess.run([CLI, "--encode-pcm", fmt, src, dst], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    assert r.stdout.split() == [str(x.size), str(count_clipped(x))]
    got = open(dst, "rb").read()
    want = x.tobytes() if fmt == "f32" else pcm_bytes(quantise(x, fmt), fmt)
    if got != want:
        b = 4 if fmt == "f32" else PCM[fmt][3]
        bad = [i for i in range(x.size) if got[i * b:(i + 1) * b] != want[i * b:(i + 1) * b]]
        raise AssertionError((fmt, [(float(x[i]), got[i * b:(i + 1) * b].hex(), want[i * b:(i + 1) * b].hex()) for i in bad[:8]]))


@pytest.mark.parametrize("fmt", ["u8", "i16", "i24"])
def test_the_cli_quantiser_round_trips_what_the_reader_gives(tmp_path, fmt):
    """S is the reader's divisor: what the reader decodes from a sample n, n / S in one f32 division, the CLI's quantiser
    (--encode-pcm) encodes as n again - every u8 and i16 sample, a spread of i24 with both ends."""
    s, lo, hi, _ = PCM[fmt]
    n = np.arange(lo, hi + 1, 1 if fmt != "i24" else 97, dtype=np.int64)
    n = np.append(n, hi)
    x = (n.astype(np.float32) / np.float32(s)).astype(np.float32)
    src, dst = str(tmp_path / "x.f32"), str(tmp_path / "y.raw")
    x.tofile(src)
    r = subprocess.run([CLI, "--encode-pcm", fmt, src, dst], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    assert r.stdout.split() == [str(x.size), str(count_clipped(x))]
    assert open(dst, "rb").read() == pcm_bytes(n, fmt)


def parse_header(b):
    assert b[:4] == b"RIFF" and b[8:12] == b"WAVE" and b[12:16] == b"fmt " and struct.unpack("<I", b[16:20])[0] == 40
    tag, ch, rate, byte_rate, align, bits, cb, valid, mask = struct.unpack("<HHIIHHHHI", b[20:44])
    assert b[60:64] == b"data"
    return dict(riff=struct.unpack("<I", b[4:8])[0], tag=tag, ch=ch, rate=rate, byte_rate=byte_rate, align=align, bits=bits,
                cb=cb, valid=valid, mask=mask, guid=b[44:60], data=struct.unpack("<I", b[64:68])[0])


GUID_TAIL = bytes([0x00, 0x00, 0x00, 0x00, 0x10, 0x00, 0x80, 0x00, 0x00, 0xAA, 0x00, 0x38, 0x9B, 0x71])


def check_header(b, fmt, ch, rate):
    """An extensible header with the PCM (or float) subformat; returns the data chunk."""
    sb = 4 if fmt == "f32" else PCM[fmt][3]
    h = parse_header(b)
    assert (h["tag"], h["ch"], h["rate"], h["cb"], h["mask"]) == (0xFFFE, ch, rate, 22, 0)
    assert (h["bits"], h["valid"], h["align"], h["byte_rate"]) == (8 * sb, 8 * sb, ch * sb, rate * ch * sb)
    assert h["guid"] == bytes([3 if fmt == "f32" else 1, 0]) + GUID_TAIL
    assert h["data"] % (ch * sb) == 0
    pad = h["data"] & 1
    assert len(b) == 68 + h["data"] + pad and h["riff"] == len(b) - 8
    if pad:
        assert b[-1] == 0
    return b[68:68 + h["data"]]


@pytest.mark.parametrize("fmt,ch,frames", [("u8", 1, 1001), ("u8", 3, 1001), ("i16", 2, 1000), ("i24", 1, 1001), ("i24", 3, 333),
                                           ("i32", 2, 500), ("f32", 2, 500), ("u8", 1, 0)])
def test_wav_header_fields_of_every_format(tmp_path, fmt, ch, frames):
    """bits, block_align and byte_rate follow the format, the subformat is PCM (float for f32), an odd data chunk is
    followed by a pad byte that the RIFF size counts, and the data chunk is the quantised samples, frame-major."""
    x = np.random.default_rng(5).uniform(-1.1, 1.1, (ch, frames)).astype(np.float32)
    src, dst = str(tmp_path / "x.f32"), str(tmp_path / "y.wav")
    x.tofile(src)
    r = subprocess.run([CLI, "--encode-wav", fmt, str(ch), "22050", src, dst], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    assert r.stdout.split() == [str(frames), str(count_clipped(x))]
    data = check_header(open(dst, "rb").read(), fmt, ch, 22050)
    assert data == (x.T.tobytes() if fmt == "f32" else pcm_bytes(quantise(x.T, fmt), fmt))
    if frames:  # the project's own reader takes the file back: what it decodes is what was quantised
        raw = str(tmp_path / "back.f32")
        r = subprocess.run([CLI, "--decode-wav", dst, raw], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0 and r.stdout.split() == [str(ch), "22050", str(frames)], (r.stdout, r.stderr)
        back = np.fromfile(raw, np.float32).reshape(ch, frames)
        if fmt == "f32":
            assert np.array_equal(back, x)
        else:
            assert np.array_equal(back, (quantise(x, fmt).astype(np.float32) / np.float32(PCM[fmt][0])).astype(np.float32))


def test_cli_names_the_flag_and_refuses_an_unknown_format(tmp_path):
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--output-format" in r.stderr
    r = subprocess.run([CLI, "-i", "a.wav", "-o", str(tmp_path / "o.wav"), "--output-format", "i20"], capture_output=True,
                       text=True, timeout=60)
    assert r.returncode != 0 and "--output-format" in r.stderr and not os.path.exists(tmp_path / "o.wav")
