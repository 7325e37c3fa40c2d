"""GPU tests of rc_engine_stretch_frames / Engine.stretch_frames: interleaved PCM frames in, interleaved f32 frames out,
both format changes on the device. The yardstick is the host form: raw frames R decoded with numpy exactly as
tests/wavutil.py decodes them into planar x must give stretch_frames(R) == stretch_host(x).T under np.array_equal - the
rows the hops see are the same rows, so there is no tolerance. One case is tied to the oracle as well."""
import os
import subprocess

import numpy as np
import pytest

import rocoder_amd
from conftest import ROOT
from oracle import cbind as oc
from oracle import oracle_np as onp
from rocoder_amd import _lib
from rocoder_amd.stretcher import pinned_empty
from wavutil import write_wav

pytestmark = pytest.mark.gpu
CLI = os.path.join(ROOT, "rocoder_amd", "bin", "rocoder")
KERNELS = os.path.join(ROOT, "examples", "kernels")

INT_FORMATS = {"u8": (-128, 127, 127.0), "i16": (-32768, 32767, 32767.0), "i24": (-8388608, 8388607, 8388608.0),
               "i32": (-2147483648, 2147483647, 2147483647.0)}
FORMATS = ["u8", "i16", "i24", "i32", "f32"]


def make_frames(fmt, ch, n, seed):
    """(what to hand to stretch_frames, the raw bytes, the planar float32 rows the reader decodes from them). Full-scale
    noise; the first and the last frame hold the format's extreme values (f32: -0.0, a denormal, +-1)."""
    rng = np.random.default_rng(seed)
    if fmt == "f32":
        a = rng.uniform(-1.0, 1.0, (n, ch)).astype("<f4")
        special = np.array([-0.0, 1e-40, 1.0, -1.0], "<f4")
        if n:
            a[0, :] = special[np.arange(ch) % 4]
            a[-1, :] = special[(np.arange(ch) + 2) % 4]
        return a, a.tobytes(), a.T.copy()
    lo, hi, k = INT_FORMATS[fmt]
    q = rng.integers(lo, hi + 1, (n, ch), dtype=np.int64)
    if n:
        q[0, :] = np.where(np.arange(ch) % 2 == 0, lo, hi)
        q[-1, :] = np.where(np.arange(ch) % 2 == 0, hi, lo)
    dec = (q.astype(np.float32) / np.float32(k)).astype(np.float32).T.copy()  # tests/wavutil.py
    if fmt == "u8":
        a = (q + 128).astype(np.uint8)
    elif fmt == "i16":
        a = q.astype("<i2")
    elif fmt == "i32":
        a = q.astype("<i4")
    else:
        raw = (q & 0xFFFFFF).astype("<u4").view(np.uint8).reshape(-1, 4)[:, :3].tobytes()
        return raw, raw, dec
    return a, a.tobytes(), dec


def both(eng, fmt, ch, n, seed=1):
    arg, raw, dec = make_frames(fmt, ch, n, seed)
    ref = eng.stretch_host(dec).T
    got = eng.stretch_frames(arg, fmt="i24" if fmt == "i24" else None)
    assert got.shape == ref.shape == (eng.output_len(n), ch) and got.dtype == np.float32
    assert np.array_equal(got, ref), (fmt, ch, n, int(np.sum(got != ref)))
    return raw, ref


@pytest.mark.parametrize("ch", [1, 2, 3, 5, 8])
@pytest.mark.parametrize("fmt", FORMATS)
def test_every_format_and_channel_count_equals_the_host_form(fmt, ch):
    """The odd length, and 9- and 15-byte frames, put tile and chunk edges on every byte phase; the first and last
    frames hold the extreme values. The explicit-format form on the same bytes from an odd address gives the same."""
    with rocoder_amd.Engine(window_len=1024, factor=2.0, channels=ch, seed=3) as eng:
        raw, ref = both(eng, fmt, ch, 30001)
        buf = np.empty(len(raw) + 1, np.uint8)
        buf[1:] = np.frombuffer(raw, np.uint8)
        assert np.array_equal(eng.stretch_frames(buf[1:], fmt=fmt), ref)
        assert np.array_equal(eng.stretch_frames(raw, fmt=fmt), ref)


@pytest.mark.parametrize("fmt", ["i16", "i24"])
def test_more_channels_than_a_wave(fmt):
    with rocoder_amd.Engine(window_len=256, factor=2.0, channels=67, seed=5) as eng:
        both(eng, fmt, 67, 3000)


@pytest.fixture(scope="module")
def chunked():
    """N = 1024, f = 8, three channels of i24, 1 200 000 frames: 9.6 M output samples per channel against 4 M per
    staging slot, so several pipeline chunks. The reference is computed once and never written to."""
    eng = rocoder_amd.Engine(window_len=1024, factor=8.0, channels=3, seed=21)
    _arg, raw, dec = make_frames("i24", 3, 1_200_000, 4)
    ref = np.ascontiguousarray(eng.stretch_host(dec).T)
    ref.flags.writeable = False
    assert ref.shape[0] > 2 * (16 << 20) // 4
    yield eng, raw, ref
    eng.close()


@pytest.mark.parametrize("src_kind,out_kind", [("pageable", "pageable"), ("pinned", "pinned"), ("pageable", "pinned"),
                                               ("pinned", "pageable"), ("offset1", "spare")])
def test_several_pipeline_chunks_with_either_kind_of_memory(chunked, src_kind, out_kind):
    eng, raw, ref = chunked
    n_out = ref.shape[0]
    if src_kind == "pinned":
        src = pinned_empty(len(raw), np.uint8)
        src[:] = np.frombuffer(raw, np.uint8)
    elif src_kind == "offset1":  # the source at byte offset 1 of a larger buffer
        big = np.zeros(len(raw) + 64, np.uint8)
        big[1:1 + len(raw)] = np.frombuffer(raw, np.uint8)
        src = big[1:1 + len(raw)]
    else:
        src = raw
    if out_kind == "pageable":
        got = eng.stretch_frames(src, fmt="i24")
    else:
        spare = 5 if out_kind == "spare" else 0
        out = pinned_empty((n_out + spare, 3)) if out_kind == "pinned" else np.empty((n_out + spare, 3), np.float32)
        out[:] = np.nan
        got = eng.stretch_frames(src, fmt="i24", out=out)
        assert got.base is not None and np.shares_memory(got, out)
        assert np.isnan(out[n_out:]).all(), "rows behind the output were written"
    assert np.array_equal(got, ref)


@pytest.mark.parametrize("kw,fmt,ch,n", [
    (dict(window_len=16384, factor=8.0), "i16", 2, 400_000),
    (dict(window_len=65536, factor=32.0), "f32", 2, 300_000),
    (dict(window_len=3000, factor=4.0), "u8", 1, 30_001),
    (dict(window_len=2048, factor=2.0, pitch_multiple=-2), "i32", 2, 30_001),
    (dict(window_len=4096, factor=0.3), "i16", 2, 3_000_000),  # more input than output
])
def test_the_other_window_paths(kw, fmt, ch, n):
    with rocoder_amd.Engine(channels=ch, seed=8, **kw) as eng:
        both(eng, fmt, ch, n)


def test_with_a_curated_device_kernel():
    with rocoder_amd.Engine(window_len=1024, factor=2.0, channels=2, seed=3, device_kernel=("gain", 0.5)) as eng:
        both(eng, "i16", 2, 30001)


@pytest.mark.parametrize("name,history,cross", [("blur.hip", 3, False), ("duck.hip", 2, True), ("mid_side.hip", 0, True)])
def test_with_a_user_device_kernel(name, history, cross):
    """A declared RC_HISTORY makes the spans of the chunks reach further back; under RC_CROSS_CHANNEL every channel's
    input is read by every channel's hops."""
    from rocoder_amd.stretcher import compile_device_kernel, device_kernel_cross_channel, device_kernel_history

    code = compile_device_kernel(open(os.path.join(KERNELS, name)).read(), name)
    assert device_kernel_history(code) == history and device_kernel_cross_channel(code) == cross
    with rocoder_amd.Engine(window_len=1024, factor=8.0, channels=2, seed=3) as eng:
        eng.load_device_kernel(code)
        both(eng, "i24", 2, 700_001)  # 5.6 M output samples per channel: two chunks


def test_with_a_host_frequency_kernel():
    with rocoder_amd.Engine(window_len=1024, factor=2.0, channels=2, seed=3, kernel=lambda t, x: 2.0 * x,
                            kernel_time_ms=1) as eng:
        both(eng, "i16", 2, 30001)


@pytest.mark.parametrize("n", [0, 1, 1023, 1024])
def test_small_lengths(n):
    with rocoder_amd.Engine(window_len=1024, factor=2.0, channels=3, seed=3) as eng:
        for fmt in ("i24", "u8", "f32"):
            both(eng, fmt, 3, n)


def test_status_codes_and_python_argument_checks():
    L = _lib.lib()
    with rocoder_amd.Engine(window_len=1024, factor=2.0, channels=2, seed=3) as eng:
        a = np.zeros((5000, 2), np.int16)
        n_out = eng.output_len(5000)
        out = np.empty((n_out, 2), np.float32)
        import ctypes as C

        fp = out.ctypes.data_as(C.POINTER(C.c_float))
        for fmt in (0, 6, 255):
            assert L.rc_engine_stretch_frames(eng._h, a.ctypes.data, 5000, fmt, fp, n_out, None) == _lib.RC_EINVAL
        assert L.rc_engine_stretch_frames(eng._h, None, 5000, 2, fp, n_out, None) == _lib.RC_EINVAL
        assert L.rc_engine_stretch_frames(eng._h, a.ctypes.data, 5000, 2, None, n_out, None) == _lib.RC_EINVAL
        assert L.rc_engine_stretch_frames(eng._h, a.ctypes.data, 5000, 2, fp, n_out - 1, None) == _lib.RC_ECAPACITY
        assert L.rc_engine_stretch_frames(eng._h, a.ctypes.data, 5000, 2, fp, n_out, None) == _lib.RC_OK
        with pytest.raises(ValueError):
            eng.stretch_frames(a, out=np.empty((n_out - 1, 2), np.float32))
        with pytest.raises(ValueError):
            eng.stretch_frames(a, out=np.empty((2, n_out), np.float32))
        with pytest.raises(ValueError):
            eng.stretch_frames(np.zeros((5000, 3), np.int16))
        with pytest.raises(ValueError):
            eng.stretch_frames(np.zeros((5000, 2), np.float64))
        with pytest.raises(ValueError):
            eng.stretch_frames(b"\0" * 13, fmt="i24")
        with pytest.raises(ValueError):
            eng.stretch_frames(a, fmt="i20")


def test_oracle_anchor(tmp_path):
    """i16 stereo at N = 1024, f = 4: the bytes of a WAV data chunk (44 bytes into the file) against the oracle on the
    decoded samples, with the tolerances of tests/test_gpu_cli.py::check - the new path is tied to the oracle and not
    only to its sibling."""
    from test_gpu_cli import check

    x = np.stack([onp.synth_input(c, 30000) for c in range(2)])
    wav = str(tmp_path / "in.wav")
    dec = write_wav(wav, x, 44100, "i16")
    body = np.frombuffer(open(wav, "rb").read(), np.uint8)[44:]
    with rocoder_amd.Engine(window_len=1024, factor=4.0, channels=2, seed=77) as eng:
        got = eng.stretch_frames(body, fmt="i16")
        assert np.array_equal(got, eng.stretch_host(dec).T)
    check(got.T, oc.stretch_offline(dec, seed=77, window_len=1024, factor=4.0))


@pytest.mark.parametrize("fmt,ch,extra", [
    ("i16", 2, ["-w", "1024", "-f", "4"]),
    ("i24", 3, ["-w", "2048", "-f", "2", "-p", "-2"]),
    ("f32", 2, ["-w", "16384", "-f", "8", "-s", "0.5", "-d", "2"]),
])
def test_cli_frames_on_gpu_writes_the_same_file(tmp_path, fmt, ch, extra):
    x = np.stack([onp.synth_input(c, 150000) for c in range(ch)])
    wav = str(tmp_path / "in.wav")
    write_wav(wav, x, 44100, fmt)
    outs = []
    for name, flag in (("default", []), ("frames", ["--frames-on-gpu"])):
        out = str(tmp_path / f"{name}.wav")
        r = subprocess.run([CLI, "-i", wav, "-o", out, "--seed", "5", *extra, *flag], capture_output=True, text=True,
                           timeout=300)
        assert r.returncode == 0, r.stderr
        assert not os.path.exists(out + ".part")
        outs.append(open(out, "rb").read())
    assert outs[0] == outs[1]
    assert len(outs[0]) > 44 + ch * 4 * 44100


def test_cli_frames_on_gpu_with_a_curated_device_kernel(tmp_path):
    x = np.stack([onp.synth_input(c, 60000) for c in range(2)])
    wav = str(tmp_path / "in.wav")
    write_wav(wav, x, 44100, "i16")
    outs = []
    for name, flag in (("default", []), ("frames", ["--frames-on-gpu"])):
        out = str(tmp_path / f"{name}.wav")
        r = subprocess.run([CLI, "-i", wav, "-o", out, "--seed", "5", "-w", "1024", "-f", "2", "--device-kernel",
                            "gain:0.5", *flag], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        outs.append(open(out, "rb").read())
    assert outs[0] == outs[1]
