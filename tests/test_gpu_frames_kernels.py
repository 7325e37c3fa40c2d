"""GPU tests of the kernels of rc_frames.hip through their launchers (rc_frames.h), called directly by way of the
test-hook entries rc_test_frames_* (tests/frameskernelutil.py): the planar samples, the raw bytes, the peak word and the
launch ranges are chosen here, which no public entry allows - there the input of these kernels is a stretcher's output.

Every comparison is of bytes or of bits against the numpy statements of the definitions - test_frames_pcm_host.quantise /
pcm_bytes / count_clipped, test_frames_norm_host.normalise, fadeutil.apply_fade, frameskernelutil.decode_ints - with no
tolerance. The one licence: where the definition names an IEEE multiplication (the gain, the fade) and the expected float
is a NaN, a NaN of any payload is accepted, since the standard leaves the payload open; where no arithmetic stands
between input and output (f32 out without a gain, f32 in, the interleave, the frames a fade does not name) NaN payloads
are compared too. Every target lies inside a larger buffer filled with a guard byte, and what lies outside the launch's
range is asserted unchanged. The values come from tests/test_frames_kernels_host.py, which asserts what they contain."""
import numpy as np
import pytest

import fadeutil
import frameskernelutil as K
from test_frames_kernels_host import F, INT_FORMATS, corner_set, decode_codes, f32, fade_abs, random_patterns, specials
from test_frames_norm_host import normalise
from test_frames_pcm_host import count_clipped, pcm_bytes, quantise

pytestmark = pytest.mark.gpu
SENTINEL = F(-123.25)  # what the gain word holds in front of a launch
WIDTHS = ["narrow", "wide"]


def ceil16(n):
    return (int(n) + 15) // 16 * 16


def first_bad(got, want):
    bad = np.nonzero(np.asarray(got) != np.asarray(want))[0]
    return f"{bad.size} of {np.asarray(want).size} differ, the first at {bad[:8].tolist()}"


def gain_of_word(word, target_peak):
    """the numpy gain of a peak word: normalise on the one-sample job whose peak it is"""
    return normalise(f32([word]), target_peak)[2]


def encoded(z, fmt):
    """rows z[C, n] -> the bytes of the frame-major block"""
    zt = np.ascontiguousarray(z.T)
    return np.frombuffer(zt.tobytes() if fmt == "f32" else pcm_bytes(quantise(zt, fmt), fmt), np.uint8)


def run_pack_pcm(fmt, x, phase, pad=0, base=0, tbase=0, word=None, target_peak=1.0, store_gain=1, clipped0=3):
    """One pack launch of the rows x[C, n] into a guarded target, held to the definition: the bytes, the guard bytes on
    both sides, the clipped counter (it starts at clipped0), the two norm words, the planar rows left as they were.
    word: the peak word (then the launch is pack_pcm_gain). Returns the bytes of the block."""
    ch, n = x.shape
    stride = n + pad
    host, _ = K.planar_host(x, stride, base)
    planar = K.DevBuf(host)
    nb = n * ch * K.BYTES[fmt]
    off = 16 + 4 * tbase
    lo = off + phase
    target = K.DevBuf(K.guarded(ceil16(lo + nb + 16)))
    clipped = K.DevBuf(np.array([clipped0], np.uint64))
    z, norm, gain = x, None, None
    if word is not None:
        gain = gain_of_word(word, target_peak)
        with np.errstate(invalid="ignore", over="ignore", under="ignore"):
            z = (x * gain).astype(np.float32)
        norm = K.DevBuf(K.norm_words(word, SENTINEL))
    rc = K.pack_pcm(fmt, planar, base, stride, target, off, phase, ch, n, clipped, norm, target_peak, store_gain)
    assert rc == 0, rc
    got = target.read()
    what = (fmt, ch, n, phase, pad, base, tbase, word)
    assert (got[:lo] == K.GUARD).all() and (got[lo + nb:] == K.GUARD).all(), (what, "guard bytes were written")
    want = encoded(z, fmt)
    if fmt == "f32" and word is not None:
        assert K.same_floats(got[lo:lo + nb].view("<f4"), want.view("<f4"), nan_payloads=False), what
    else:
        assert np.array_equal(got[lo:lo + nb], want), (what, first_bad(got[lo:lo + nb], want))
    assert int(clipped.read().view(np.uint64)[0]) == clipped0 + count_clipped(z), (what, "clipped")
    if norm is not None:
        w = norm.read().view(np.uint32)
        assert int(w[0]) == word, (what, "the peak word was written")
        assert int(w[1]) == int(K.bits(gain if store_gain else SENTINEL)[()]), (what, "the gain word", hex(int(w[1])))
    assert np.array_equal(planar.read(), host), (what, "the planar rows were written")
    return got[lo:lo + nb]


def run_unpack(fmt, data, phase, ch, frame0, n, pad=0, base=0, chan_map=None):
    """One unpack launch of the frames [frame0, frame0 + n) of the block `data` (bytes of frame0 + n frames, put `phase`
    bytes into a 16-byte aligned buffer) into guarded planar rows: the floats of the range bit for bit, everything else -
    the frames in front, the padding of the rows, the floats around them - left as it was."""
    b = K.BYTES[fmt]
    rows_len = frame0 + n
    data = np.asarray(data, np.uint8).reshape(-1)
    assert data.size == rows_len * ch * b
    host = K.guarded(ceil16(phase + data.size))
    host[phase:phase + data.size] = data
    raw = K.DevBuf(host)
    stride = rows_len + pad
    planar = K.DevBuf(K.guarded(4 * (base + (ch - 1) * stride + rows_len + 8)))
    dmap = None if chan_map is None else K.DevBuf(np.asarray(chan_map, np.uint32))
    if chan_map is not None:
        assert len(chan_map) == ch and max(chan_map) < ch
    rc = K.unpack(fmt, raw, phase, ch, frame0, n, planar, base, stride, dmap)
    assert rc == 0, rc
    rows, outside = K.rows_of(planar.read(), ch, rows_len, stride, base)
    what = (fmt, ch, n, phase, frame0, pad, base, None if chan_map is None else "map")
    assert (outside == K.GUARD_WORD).all(), (what, "floats outside the rows were written")
    assert (K.bits(rows[:, :frame0]) == K.GUARD_WORD).all(), (what, "frames in front of frame0 were written")
    want = K.decode_bytes(data, fmt).reshape(rows_len, ch).T
    if chan_map is not None:
        want = want[np.asarray(chan_map)]
    got = K.bits(rows[:, frame0:]).reshape(-1)
    assert np.array_equal(got, K.bits(want[:, frame0:]).reshape(-1)), (what, first_bad(got, K.bits(want[:, frame0:]).reshape(-1)))
    assert np.array_equal(raw.read(), host), (what, "the block was written")


def run_pack_f32(x, foff, pad=0, base=0):
    """One interleave launch (launch_frames_pack) of the rows x[C, n] to `frames`, foff floats off a 16-byte boundary"""
    ch, n = x.shape
    stride = n + pad
    host, _ = K.planar_host(x, stride, base)
    planar = K.DevBuf(host)
    lo = 4 + foff
    frames = K.DevBuf(K.guarded(4 * (lo + n * ch + 8)))
    rc = K.pack(planar, base, stride, frames, lo, n, ch)
    assert rc == 0, rc
    got = frames.read().view(np.uint32)
    what = (ch, n, foff, pad, base)
    assert (got[:lo] == K.GUARD_WORD).all() and (got[lo + n * ch:] == K.GUARD_WORD).all(), (what, "guard floats were written")
    want = K.bits(np.ascontiguousarray(x.T)).reshape(-1)
    assert np.array_equal(got[lo:lo + n * ch], want), (what, first_bad(got[lo:lo + n * ch], want))


def uniform(seed, shape, amp=1.2):
    return np.random.default_rng(seed).uniform(-amp, amp, shape).astype(np.float32)


# ------------------------------------------------------------------------------------------------ the quantiser's values
@pytest.fixture(scope="module")
def corner_rows():
    """per format: the corner set as 9 rows, each rotated so that the chosen values lie across frame 1024 - an edge of
    the narrow tile and of the wide one - at another offset in every channel. Built once, never written to."""
    out = {}
    for fmt in K.FORMATS:
        row = corner_set(fmt)
        n_special = row.size - random_patterns().size
        rows = np.stack([np.roll(row, 1024 - n_special // 2 + 17 * c) for c in range(9)])
        rows.setflags(write=False)
        out[fmt] = rows
    return out


@pytest.mark.parametrize("fmt", K.FORMATS)
def test_quantiser_on_the_corner_set(corner_rows, fmt):
    """ties, +-1 and its neighbours, HI / S and LO / S, zeros, denormals, FLT_MAX, infinities, NaNs, 2^31 and 65 536
    random bit patterns through pack_pcm at 1, 3 and 9 channels and every byte phase: the bytes, and the clipped count
    on top of a counter that does not start at 0"""
    rows = corner_rows[fmt]
    u = K.bits(rows[0])
    assert ((u & 0x7FFFFFFF) > 0x7F800000).any() and (((u & 0x7F800000) == 0) & ((u & 0x007FFFFF) != 0)).any()
    for ch in (1, 3, 9):
        for phase in range(4):
            block = run_pack_pcm(fmt, rows[:ch], phase, clipped0=1000 + phase)
            if fmt == "f32":  # NaN payloads and denormals come out bit for bit
                assert np.array_equal(block.view(np.uint32), K.bits(np.ascontiguousarray(rows[:ch].T)).reshape(-1))


WORDS = [(0, 1.0), (1, 1.0), (int(K.bits(F(2))[()]), 1.0), (int(K.bits(F(3))[()]), 1.0), (int(K.bits(F(0.7))[()]), 0.5)]


@pytest.mark.parametrize("fmt", K.FORMATS)
def test_gain_from_a_chosen_peak_word(fmt):
    """pack_pcm_gain with the peak word written by the test: no peak (gain 1), the smallest denormal (the quotient
    overflows: gain 1), 2 and 3 at target 1, 0.7 at target 0.5; store_gain 1 stores numpy's gain, store_gain 0 leaves
    the sentinel; the chosen values of the format and uniform noise at 2 channels (narrow kernel) and 9 (wide)"""
    sp = specials(fmt if fmt != "f32" else "i32")
    for ch in (2, 9):
        x = uniform(60 + ch, (ch, 1200), 3.5)
        for c in range(ch):
            x[c, 40 * c + 3:40 * c + 3 + sp.size] = sp
        x[0, 0] = F(1e-40)
        for i, (word, target) in enumerate(WORDS):
            for store in (1, 0):
                block = run_pack_pcm(fmt, x, (i + store) % 4, pad=(0, 1, 3)[i % 3], base=i % 4, tbase=(i + 1) % 4, word=word,
                                     target_peak=target, store_gain=store)
                if fmt == "f32" and word == WORDS[2][0]:  # 1e-40 * 0.5 is the denormal, not 0
                    assert int(block.view(np.uint32)[0]) == int(K.bits(F(1e-40))[()]) // 2 != 0


# --------------------------------------------------------------------------------------------------- the byte layout sweep
@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("fmt", K.FORMATS)
def test_layout_pack_pcm(fmt, width):
    """pack_pcm, and pack_pcm_gain at the gain 1 / 3, over frameskernelutil.layout_cases: every channel count, frame
    count, byte phase, row stride, row base and target dword of the list"""
    word = WORDS[3][0]
    for i, c in enumerate(K.layout_cases(width)):
        x = uniform(1000 + i, (c["channels"], c["n_frames"]))
        run_pack_pcm(fmt, x, c["phase"], c["pad"], c["base"], c["tbase"])
        run_pack_pcm(fmt, x * F(2.5), c["phase"], c["pad"], c["base"], c["tbase"], word=word, store_gain=i & 1)


@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("fmt", K.FORMATS)
def test_layout_unpack(fmt, width):
    """unpack, and unpack_map with the reverse map and with a random one (channels that feed several rows, and none)"""
    rng = np.random.default_rng(7)
    for c in K.layout_cases(width):
        ch, n, f0 = c["channels"], c["n_frames"], c["frame0"]
        data = rng.integers(0, 256, (f0 + n) * ch * K.BYTES[fmt], dtype=np.uint8)
        run_unpack(fmt, data, c["phase"], ch, f0, n, c["pad"], c["base"])
        run_unpack(fmt, data, c["phase"], ch, f0, n, c["pad"], c["base"], chan_map=list(range(ch))[::-1])
        run_unpack(fmt, data, c["phase"], ch, f0, n, c["pad"], c["base"], chan_map=rng.integers(0, ch, ch).tolist())


@pytest.mark.parametrize("width", WIDTHS)
def test_layout_pack_f32(width):
    """the f32 interleave on random bit patterns, NaNs included, compared as uint32; `frames` 0 to 3 floats off a
    16-byte boundary (the case's phase): both branches of the kernel's alignment test"""
    pat = np.concatenate([random_patterns(), random_patterns(99)])
    for i, c in enumerate(K.layout_cases(width)):
        ch, n = c["channels"], c["n_frames"]
        x = np.resize(np.roll(pat, 31 * i), ch * n).reshape(ch, n)
        run_pack_f32(x, c["phase"], c["pad"], c["base"])


# ---------------------------------------------------------------------------------------------------------- decode values
def check_decode(fmt, codes, ch, phase):
    data = K.int_bytes(codes, fmt)
    run_unpack(fmt, data, phase, ch, 0, codes.size // ch)


def test_decode_every_u8_code():
    codes = decode_codes("u8")
    for phase in range(4):
        check_decode("u8", codes, 1, phase)
        check_decode("u8", np.resize(codes, 256 * 9), 9, phase)


def test_decode_every_i16_code():
    codes = decode_codes("i16")
    for phase in range(4):
        check_decode("i16", codes, 1, phase)
        check_decode("i16", codes, 8, phase)


def test_decode_every_i24_code():
    """one mono launch of all 2^24 codes at phase 0"""
    check_decode("i24", decode_codes("i24"), 1, 0)


@pytest.mark.parametrize("phase", [1, 2, 3])
def test_decode_i24_slice_at_a_byte_phase(phase):
    """70 000 codes around the step from 0x7fffff to 0x800000"""
    check_decode("i24", np.arange(-35000, 35000, dtype=np.int64) % 2 ** 24 - 2 ** 23, 1, phase)


def test_decode_the_i32_set():
    codes = decode_codes("i32")
    for phase in range(4):
        check_decode("i32", codes, 1, phase)
    check_decode("i32", codes[:codes.size // 9 * 9], 9, 1)


def test_decode_f32_keeps_the_bits():
    x = corner_set("f32")
    assert np.isnan(x).any()
    for phase in range(4):
        run_unpack("f32", x.view(np.uint8), phase, 1, 0, x.size)
    n = x.size // 9
    run_unpack("f32", x[:9 * n].view(np.uint8), 3, 9, 0, n)


# -------------------------------------------------------------------------------------------------------------------- peak
PEAK_LENS = [1, 2, 3, 4, 5, 8191, 8192, 8193, 16385]


def peak_positions(n, base):
    head = min((4 - base) % 4, n)  # single samples in front of the first 16-byte group
    tail = (n - head) % 4 if n <= 8192 else 0
    pos = {0, n - 1, head + 5, 8189, 8190, 8191, 8192, 8193} | set(range(head)) | {n - 1 - k for k in range(max(tail, 3))}
    return sorted(p for p in pos if 0 <= p < n)


def run_peak(rows, base, pad, start_word):
    ch, n = rows.shape
    host, _ = K.planar_host(rows, n + pad, base)
    planar = K.DevBuf(host)
    norm = K.DevBuf(K.norm_words(start_word, SENTINEL))
    assert K.peak(planar, base, n + pad, n, ch, norm) == 0
    w = norm.read().view(np.uint32)
    assert int(w[1]) == int(K.bits(SENTINEL)[()]), "the gain word was written"
    assert np.array_equal(planar.read(), host)
    return int(w[0])


@pytest.mark.parametrize("ch", [1, 3])
def test_peak_finds_one_large_sample_wherever_it_lies(ch):
    """rows of small values, one large one placed in turn at the first sample, each head sample in front of the first
    16-byte group, inside the body, each tail sample, 8191 / 8192 / 8193 and the last sample, with either sign; a NaN
    and both infinities, larger than everything, are skipped; the word starts at 0, below the peak, or above it"""
    below, above = int(K.bits(F(0.3))[()]), int(K.bits(F(0.9))[()])
    case = 0
    for n in PEAK_LENS:
        quiet = uniform(n, (ch, n), 0.01)
        for base in range(4):
            for pos in peak_positions(n, base):
                case += 1
                rows = quiet.copy()
                if n >= 5:
                    other = rows[(case + 1) % ch]
                    other[(pos + 1) % n], other[(pos + 2) % n], other[(pos + 3) % n] = f32(0x7FC01234), F(np.inf), F(-np.inf)
                large = F(0.5 + 0.001 * (case % 100)) * F(-1 if case & 1 else 1)
                rows[case % ch, pos] = large
                start = (0, below, above)[case % 3]
                want_peak = normalise(rows, 1.0)[1]
                assert want_peak == abs(large)
                got = run_peak(rows, base, (0, 1, 3)[case % 3], start)
                assert got == max(start, int(K.bits(want_peak)[()])), (ch, n, base, pos, hex(got), float(large), hex(start))
    assert case > 150


def test_peak_leaves_the_word_where_nothing_finite_and_non_zero_is_seen():
    rows = np.zeros((3, 8200), np.float32)
    rows[0, ::2] = f32(0x7FC00000)
    rows[1, 1::3] = f32(0xFF800001)
    rows[2, 5], rows[2, 8195], rows[1, 0] = F(np.inf), F(-np.inf), F(-0.0)
    assert normalise(rows, 1.0)[1] == 0
    for start in (0, 123, int(K.bits(F(0.25))[()])):
        for base in range(4):
            assert run_peak(rows, base, 1, start) == start


# -------------------------------------------------------------------------------------------------------------------- fade
FADE_T = 8400


@pytest.fixture(scope="module")
def fade_rows():
    """two rows of 8400 frames: uniform noise, with the chosen values of two formats where the fades of the tests below
    rise, fall and end. Never written to."""
    y = uniform(5, (2, FADE_T), 1.0)
    for c, fmt in enumerate(("i16", "i32")):
        sp = specials(fmt)
        for at in (0, 100, 3500, 4090, 6600, 6960, 7100, 8180):
            y[c, at + 7 * c:at + 7 * c + sp.size] = sp
    assert np.isnan(y[:, :5000]).any() and np.isnan(y[:, 3000:7000]).any() and np.isnan(y[:, 7000:]).any()
    y.setflags(write=False)
    return y


def run_fade(y, in_len, out_start, out_len, t0, t1, base, pad, want_range=None, t_abs=0):
    """One fade launch on the frames [t0, t1) of rows y[C, T] whose frame 0 is absolute frame t_abs: inside the range the
    definition (a NaN the multiplication made: any payload; a frame no line of the definition names: its bits as they
    were), outside it and around the rows nothing written."""
    ch, total = y.shape
    stride = total + pad
    host, _ = K.planar_host(y, stride, base)
    planar = K.DevBuf(host)
    rc = K.fade(planar, base + t0, stride, ch, in_len, out_start, out_len, t_abs + t0, t_abs + t1)
    assert rc == 0, rc
    rows, outside = K.rows_of(planar.read(), ch, total, stride, base)
    what = (in_len, out_start, out_len, t0, t1, base, pad, t_abs)
    assert (outside == K.GUARD_WORD).all(), (what, "floats outside the rows were written")
    assert np.array_equal(K.bits(rows[:, :t0]), K.bits(y[:, :t0])) and np.array_equal(K.bits(rows[:, t1:]), K.bits(y[:, t1:])), \
        (what, "frames outside [t0, t1) were written")
    if want_range is None:
        want_range = fadeutil.apply_fade(y, in_len, out_start, out_len, axis=1)[:, t0:t1]
    got = rows[:, t0:t1]
    assert K.same_floats(got, want_range, nan_payloads=False), (what, first_bad(K.bits(got).reshape(-1), K.bits(want_range).reshape(-1)))
    t = t_abs + np.arange(t0, t1, dtype=np.uint64)
    unnamed = ~((t < np.uint64(in_len)) | (t >= np.uint64(out_start)))
    assert np.array_equal(K.bits(got[:, unnamed]), K.bits(y[:, t0:t1][:, unnamed])), (what, "a frame no line names changed")
    tail = (t >= np.uint64(out_start)) & (t - np.uint64(out_start) >= np.uint64(out_len)) if out_start != fadeutil.NONE else np.zeros(t.size, bool)
    assert (K.bits(got[:, tail]) == 0).all(), (what, "behind the fade-out: +0.0")
    return int(tail.sum())


FADES = [  # in_len, out_start, out_len, the launch ranges [t0, t1)
    (5000, fadeutil.NONE, 0, [(0, 5000), (3, 4999), (4097, 5003), (0, FADE_T)]),                       # fade-in only
    (0, 3000, 4000, [(3000, FADE_T), (3001, 6999), (6990, 7013), (7001, 8399), (2990, 3010)]),         # fade-out only
    (6000, 2000, 5000, [(0, FADE_T), (2500, 5500), (0, 8191), (0, 8192), (0, 8193), (5, 8198)]),       # overlapping
    (100, 4001, 0, [(3990, FADE_T), (4001, 4002), (0, 4001)]),                                          # out_len == 0
    (FADE_T, 0, FADE_T, [(0, FADE_T), (8191, 8193)]),                                                   # both over everything
]


@pytest.mark.parametrize("which", range(len(FADES)))
def test_fade_on_chosen_values(fade_rows, which):
    in_len, out_start, out_len, ranges = FADES[which]
    i = 0
    for t0, t1 in ranges:
        for base in range(4):
            run_fade(fade_rows, in_len, out_start, out_len, t0, t1, base, (0, 1, 3)[i % 3])
            i += 1


def test_fade_tail_is_plus_zero_where_a_group_straddles_its_start(fade_rows):
    """out_start + out_len at every float of a 16-byte group, for every row base: +0.0 from there on whatever was there
    (NaNs, infinities, -0.0 lie at 6960 ... and 7100 ...), the samples of the same group in front of it faded"""
    assert np.isnan(fade_rows[:, 7000:7200]).any() and np.isinf(fade_rows[:, 7000:7200]).any()
    for out_len in (4000, 4001, 4002, 4003):
        for base in range(4):
            n_tail = run_fade(fade_rows, 0, 3000, out_len, 6990, 7300, base, 1)
            assert n_tail == 7300 - 3000 - out_len


@pytest.mark.parametrize("t_abs", [2 ** 24 + 3, 2 ** 40 + 1])
def test_fade_far_into_a_job(fade_rows, t_abs):
    """t0 beyond the integers f32 holds exactly, and beyond 32 bits: `planar` is relative to t0, so a small buffer will
    do. The yardstick is fadeutil.sq on the absolute positions (test_frames_kernels_host.fade_abs, held to apply_fade
    there)."""
    for in_len, out_start, out_len in ((t_abs + 5000, fadeutil.NONE, 0), (0, t_abs + 2000, 4000), (t_abs + 6000, t_abs + 1000, 7000),
                                       (t_abs + 3, t_abs - 1000, 2 ** 33)):
        want = fade_abs(fade_rows, t_abs, in_len, out_start, out_len)
        for base, (t0, t1) in enumerate(((0, FADE_T), (1, 8200), (4999, 6003), (2, 8195))):
            run_fade(fade_rows, in_len, out_start, out_len, t0, t1, base, base % 3, want_range=want[:, t0:t1], t_abs=t_abs)


# ------------------------------------------------------------------------------------------- more than one launch per job
BIG_N = 2 ** 27 + 1029
BIG_CHUNK = 2 ** 24


def big_chunks():
    """(a, b, k) over the job: k_i = (7 i) mod 255 - 127 as an int64 tensor on the device"""
    import torch

    for a in range(0, BIG_N, BIG_CHUNK):
        b = min(a + BIG_CHUNK, BIG_N)
        i = torch.arange(a, b, dtype=torch.int64, device=K.DEVICE)
        yield a, b, (7 * i) % 255 - 127


@pytest.mark.parametrize("kind", ["pack_pcm", "pack_pcm_gain", "unpack"])
def test_a_job_of_more_than_one_launch(kind):
    """2^27 + 1029 frames of u8, mono, at byte phase 1: the launcher cuts the job into two launches, the second of which
    starts inside a dword of the block. Samples and expected bytes are built on the device with integer arithmetic and a
    table of the 255 floats fl(k / 127) made by numpy (test_frames_kernels_host holds quantise(fl(k / 127)) == k);
    neither comes from a kernel under test."""
    import torch

    ks = np.arange(-127, 128, dtype=np.int64)
    table = torch.from_numpy(K.decode_ints(ks, "u8") * (F(2) if kind == "pack_pcm_gain" else F(1))).to(K.DEVICE)
    lo = 16 + 1
    if kind == "unpack":
        raw_t = torch.full((ceil16(1 + BIG_N),), K.GUARD, dtype=torch.uint8, device=K.DEVICE)
        for a, b, k in big_chunks():
            raw_t[1 + a:1 + b] = (k + 128).to(torch.uint8)
        out_t = torch.full((4 * (4 + BIG_N + 4),), K.GUARD, dtype=torch.uint8, device=K.DEVICE)
        rc = K.unpack("u8", K.DevBuf.wrap(raw_t), 1, 1, 0, BIG_N, K.DevBuf.wrap(out_t), 4, BIG_N)
        assert rc == 0, rc
        words = out_t.view(torch.int32)
        guard = int(np.array([K.GUARD_WORD], np.uint32).view(np.int32)[0])
        assert bool((words[:4] == guard).all()) and bool((words[4 + BIG_N:] == guard).all()), "guard floats were written"
        got = out_t.view(torch.float32)[4:4 + BIG_N]
        for a, b, k in big_chunks():
            assert torch.equal(got[a:b], table[k + 127]), (a, b)
        return
    x_t = torch.empty(4 * BIG_N, dtype=torch.uint8, device=K.DEVICE)
    for a, b, k in big_chunks():
        x_t.view(torch.float32)[a:b] = table[k + 127]
    target_t = torch.full((ceil16(lo + BIG_N + 16),), K.GUARD, dtype=torch.uint8, device=K.DEVICE)
    clipped = K.DevBuf(np.array([11], np.uint64))
    norm = K.DevBuf(K.norm_words(int(K.bits(F(2))[()]), SENTINEL)) if kind == "pack_pcm_gain" else None
    rc = K.pack_pcm("u8", K.DevBuf.wrap(x_t), 0, BIG_N, K.DevBuf.wrap(target_t), 16, 1, 1, BIG_N, clipped, norm, 1.0, 1)
    assert rc == 0, rc
    assert bool((target_t[:lo] == K.GUARD).all()) and bool((target_t[lo + BIG_N:] == K.GUARD).all()), "guard bytes were written"
    for a, b, k in big_chunks():
        assert torch.equal(target_t[lo + a:lo + b], (k + 128).to(torch.uint8)), (a, b)
    assert int(clipped.read().view(np.uint64)[0]) == 11
    if norm is not None:  # stored by the first launch; the peak word as it was
        w = norm.read().view(np.uint32)
        assert (int(w[0]), int(w[1])) == (int(K.bits(F(2))[()]), int(K.bits(F(0.5))[()]))
