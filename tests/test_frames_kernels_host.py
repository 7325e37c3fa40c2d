"""CPU tests (-m "not gpu") behind tests/test_gpu_frames_kernels.py, which calls the launchers of rc_frames.h directly on
values of its own choosing: the corner set of every integer format and the decode sets are built here, their contents are
asserted (so that no GPU test can pass vacuously), and the numpy yardsticks - test_frames_pcm_host.quantise / pcm_bytes /
count_clipped, test_frames_norm_host.normalise, frameskernelutil.decode_ints - are held to hand-written known answers
on them, every tie included."""
import numpy as np
import pytest

import fadeutil
import frameskernelutil as K
from test_frames_norm_host import normalise
from test_frames_pcm_host import PCM, count_clipped, pcm_bytes, quantise

F = np.float32
INT_FORMATS = ["u8", "i16", "i24", "i32"]
# ties t = k + 0.5 and what rint (ties to even) makes of them, written by hand
TIE_K = [0, 1, 2, 3, 100, 101, -1, -2, -3, -4, -101, -102]
TIE_ROUNDED = [0, 2, 2, 4, 100, 102, 0, -2, -2, -4, -100, -102]
QNAN, SNAN = 0x7FC00000, 0x7F800001
NAN_BITS = [QNAN, QNAN | 0x1234, QNAN | 0x80000000, 0xFFC54321, SNAN, 0x7F812345, SNAN | 0x80000000, 0xFFA00001, 0x7FFFFFFF]
N_RANDOM = 65536


def f32(bits_):
    return np.array(bits_, np.uint32).view(np.float32)


def step(x, n):
    """the float n places above (below: n < 0) the finite float x in the order of the values"""
    for _ in range(abs(n)):
        x = np.nextafter(F(x), F(np.inf) if n > 0 else F(-np.inf))
    return F(x)


def scale(fmt):
    return F(PCM[fmt][0])  # (i32: 2147483647 rounds to 2^31, the kernel's (float)S)


def ties(fmt):
    """(x, k) with fl(x * S) == k + 0.5 exactly. i24 and i32: S is a power of two and x = (k + 0.5) / S is exact. u8 and
    i16: a search over the floats next to (k + 0.5) / S, keeping those whose f32 product is the tie."""
    s = scale(fmt)
    out = []
    for k in TIE_K:
        t = F(k + 0.5)
        x0 = F(t / s)
        for d in range(-8, 9) if fmt in ("u8", "i16") else (0,):
            x = step(x0, d)
            if F(x * s) == t:
                out.append((x, k))
                break
    return out


def full_scale_edges(fmt):
    """HI / S and LO / S with two neighbours on either side, and values beyond both"""
    s, lo, hi, _ = PCM[fmt]
    v = []
    for e in (F(hi) / scale(fmt), F(lo) / scale(fmt)):
        v += [step(e, d) for d in (-2, -1, 0, 1, 2)]
    return v + [F(1.5), F(-1.5), F(3.7), F(-3.7), F(1e9), F(-1e9), F(hi + 0.5) / scale(fmt), F(lo - 0.5) / scale(fmt)]


def specials(fmt):
    """the chosen values of one integer format (float32, by bits)"""
    v = [x for x, _ in ties(fmt)]
    for one in (F(1), F(-1)):
        v += [step(one, -1), one, step(one, 1)]
    v += full_scale_edges(fmt)
    v += [F(0.0), F(-0.0)]
    v += list(f32([0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0x00800000, 0x80800000]))  # denormals, the smallest normal
    fmax = np.finfo(np.float32).max
    v += [fmax, -fmax, F(np.inf), F(-np.inf)]
    v += list(f32(NAN_BITS))
    if fmt == "i32":  # what gives 2^31 in float, and its neighbours
        v += [F(1) - F(2.0 ** -24), -(F(1) - F(2.0 ** -24)), step(F(1), -2), step(F(-1), 2), step(F(1), 2), step(F(-1), -2)]
    return np.array(v, np.float32).view(np.uint32).copy().view(np.float32)


def random_patterns(seed=1234):
    return np.random.default_rng(seed).integers(0, 2 ** 32, N_RANDOM, dtype=np.uint64).astype(np.uint32).view(np.float32)


def corner_set(fmt):
    """specials(fmt) - for "f32" those of every integer format - followed by 65 536 random f32 bit patterns"""
    sp = np.concatenate([specials(f) for f in INT_FORMATS]) if fmt == "f32" else specials(fmt)
    return np.concatenate([sp, random_patterns()])


def decode_codes(fmt):
    """the integer samples the decode tests run: every code of u8, i16 and i24; for i32 chosen values, both ends, random"""
    lo, hi = PCM[fmt][1], PCM[fmt][2]
    if fmt != "i32":
        return np.arange(lo, hi + 1, dtype=np.int64)
    v = [0, 1, -1, 127, -127, 128, -128, 2 ** 24 - 1, 2 ** 24, 2 ** 24 + 1, -(2 ** 24) - 1, -(2 ** 24) + 1, hi, lo]
    v += list(range(hi - 63, hi + 1)) + list(range(lo, lo + 64))  # the 64 values at either end
    v += list(np.random.default_rng(77).integers(lo, hi + 1, N_RANDOM, dtype=np.int64))
    return np.array(v, np.int64)


def has_bits(x, b):
    return bool((K.bits(x) == np.uint32(b)).any())


# ----------------------------------------------------------------------------------------------------------- the tests
@pytest.mark.parametrize("fmt", INT_FORMATS)
def test_corner_set_holds_every_class_of_value(fmt):
    s = scale(fmt)
    tk = ties(fmt)
    ks = [k for _, k in tk]
    assert len(tk) >= 8, ks
    for sign in (1, -1):
        for parity in (0, 1):
            assert any((k >= 0) == (sign > 0) and k % 2 == parity for k in ks), (fmt, sign, parity, ks)
    for x, k in tk:
        assert F(x * s) == F(k + 0.5) and float(F(x * s)) - k == 0.5
        if fmt in ("i24", "i32"):
            assert float(x) == (k + 0.5) / float(s)  # exact: S is a power of two
    if fmt in ("i24", "i32"):
        assert ks == TIE_K
    c = corner_set(fmt)
    assert c.dtype == np.float32 and c.size >= N_RANDOM + 50
    for x, _ in tk:
        assert has_bits(c, K.bits(x)[()])
    for one in (1.0, -1.0):
        for d in (-1, 0, 1):
            assert has_bits(c, K.bits(step(F(one), d))[()]), (one, d)
    _, lo, hi, _ = PCM[fmt]
    for e in (F(hi) / s, F(lo) / s):
        for d in (-1, 0, 1):
            assert has_bits(c, K.bits(step(e, d))[()])
    with np.errstate(invalid="ignore", over="ignore"):
        assert (c[np.isfinite(c)] * s > hi + 1).any() and (c[np.isfinite(c)] * s < lo - 1).any(), "values beyond both ends"
    for b in (0x00000000, 0x80000000, 0x00000001, 0x007FFFFF, 0x00800000, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F800000, 0xFF800000):
        assert has_bits(c, b), hex(b)
    for b in NAN_BITS:
        assert has_bits(c, b), hex(b)
    u = K.bits(c)
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    quiet = (u & 0x00400000) != 0
    for neg in (False, True):
        for q in (False, True):
            m = nan & (((u >> 31) == 1) == neg) & (quiet == q) & ((u & 0x003FFFFF) != 0)
            assert m[:c.size - N_RANDOM].any(), ("a NaN with a payload", neg, q)
    if fmt == "i32":
        assert has_bits(c, 0x3F7FFFFF) and float(F(f32(0x3F7FFFFF)) * s) == 2.0 ** 31 - 128
        assert has_bits(c, 0x3F800001) and has_bits(c, 0xBF800001) and has_bits(c, 0x3F7FFFFE) and has_bits(c, 0xBF7FFFFE)
    assert np.array_equal(K.bits(c[-N_RANDOM:]), K.bits(random_patterns())) and np.unique(K.bits(c[-N_RANDOM:])).size > 65000
    assert np.array_equal(K.bits(corner_set(fmt)), u), "the set is the same on every call"


def test_f32_corner_set_is_the_union():
    c = K.bits(corner_set("f32"))
    for fmt in INT_FORMATS:
        assert np.isin(K.bits(specials(fmt)), c).all()


@pytest.mark.parametrize("fmt", INT_FORMATS)
def test_quantise_on_hand_written_answers(fmt):
    s, lo, hi, _ = PCM[fmt]
    tk = ties(fmt)
    for x, k in tk:  # every tie goes to the even neighbour
        want = TIE_ROUNDED[TIE_K.index(k)]
        assert want % 2 == 0 and abs(want - (k + 0.5)) == 0.5
        assert quantise([x], fmt)[0] == want, (fmt, k)
    one = {"u8": 127, "i16": 32767, "i24": 8388607, "i32": 2147483647}[fmt]      # 1.0: S, clamped to HI
    minus = {"u8": -127, "i16": -32767, "i24": -8388608, "i32": -2147483648}[fmt]  # -1.0: -S, inside [LO, HI]
    fmax = np.finfo(np.float32).max
    table = [(1.0, one), (-1.0, minus), (0.0, 0), (-0.0, 0), (np.inf, hi), (-np.inf, lo), (fmax, hi), (-fmax, lo),
             (1.5, hi), (-1.5, lo), (3.7, hi), (-3.7, lo), (f32(0x00000001), 0), (f32(0x807FFFFF), 0), (f32(0x00800000), 0),
             (F(hi) / scale(fmt), hi), (F(lo) / scale(fmt), lo), (0.5, {"u8": 64, "i16": 16384, "i24": 4194304, "i32": 2 ** 30}[fmt]),
             (-0.25, {"u8": -32, "i16": -8192, "i24": -2097152, "i32": -(2 ** 29)}[fmt])]
    # (0.5 * 127 = 63.5 -> 64 and 0.5 * 32767 = 16383.5 -> 16384: ties again; -0.25 * 127 = -31.75, -0.25 * 32767 = -8191.75)
    for b in NAN_BITS:
        table.append((f32(b), 0))
    if fmt == "i32":
        table += [(f32(0x3F7FFFFF), 2147483520), (f32(0xBF7FFFFF), -2147483520), (f32(0x3F800001), hi), (f32(0xBF800001), lo),
                  (2.0 ** -31, 1), (-(2.0 ** -31), -1), (1.5 * 2.0 ** -31, 2), (2.5 * 2.0 ** -31, 2)]
    if fmt == "i24":
        table += [(8388606.5 / 8388608, 8388606), (8388607.5 / 8388608, 8388607), (-8388607.5 / 8388608, -8388608)]
    assert len(table) + len(tk) >= 24
    for x, want in table:
        assert quantise(np.array([x], np.float32), fmt)[0] == want, (fmt, float(x), want)


def test_pcm_bytes_and_count_clipped_on_hand_written_answers():
    assert pcm_bytes([-128, -1, 0, 127], "u8") == bytes([0x00, 0x7F, 0x80, 0xFF])
    assert pcm_bytes([-32768, -2, 258], "i16") == bytes([0x00, 0x80, 0xFE, 0xFF, 0x02, 0x01])
    assert pcm_bytes([-8388608, -1, 0x010203, 8388607], "i24") == bytes([0, 0, 0x80, 0xFF, 0xFF, 0xFF, 3, 2, 1, 0xFF, 0xFF, 0x7F])
    assert pcm_bytes([-2147483648, 0x01020304], "i32") == bytes([0, 0, 0, 0x80, 4, 3, 2, 1])
    for fmt in INT_FORMATS:  # frameskernelutil's packer and its inverse
        n = decode_codes(fmt)[:70000]
        assert K.int_bytes(n, fmt).tobytes() == pcm_bytes(n, fmt)
        assert np.array_equal(K.bytes_ints(K.int_bytes(n, fmt), fmt), n)
    x = np.concatenate([[F(1), F(-1), step(F(1), -1), step(F(-1), 1), F(0), f32(0x00000001)],          # not clipped: 6
                        [step(F(1), 1), step(F(-1), -1), F(np.inf), F(-np.inf), F(1.5)], f32(NAN_BITS)])  # clipped: 5 + 9
    assert count_clipped(x) == 14 and count_clipped(x[:6]) == 0
    for i in range(6, x.size):
        assert count_clipped(x[i:i + 1]) == 1, i


def test_u8_round_trip_of_the_big_launch_pattern():
    """quantise(fl(k / 127), "u8") == k for every k in [-127, 127]: the job of more than one launch is built from these"""
    k = np.arange(-127, 128, dtype=np.int64)
    x = (k.astype(np.float32) / F(127)).astype(np.float32)
    assert np.array_equal(quantise(x, "u8"), k) and count_clipped(x) == 0
    assert np.array_equal(quantise((x * F(2)) * F(0.5), "u8"), k)  # doubled, then the gain of peak 2 at target 1
    assert np.array_equal(K.decode_ints(k, "u8"), x)
    i = np.arange(0, 3000, dtype=np.int64)
    assert set(((7 * i) % 255 - 127).tolist()) == set(k.tolist())  # the pattern k_i = (7 i) mod 255 - 127 takes every k


def test_decode_sets_and_the_decode_yardstick():
    assert decode_codes("u8").size == 256 and decode_codes("i16").size == 65536 and decode_codes("i24").size == 2 ** 24
    c = decode_codes("i32")
    hi, lo = 2 ** 31 - 1, -(2 ** 31)
    for v in (0, 1, -1, 127, -127, 128, -128, 2 ** 24 + 1, 2 ** 24 - 1, hi, lo):
        assert (c == v).any(), v
    assert np.isin(np.arange(hi - 63, hi + 1), c).all() and np.isin(np.arange(lo, lo + 64), c).all()
    assert c.size >= N_RANDOM + 128 and c.min() == lo and c.max() == hi
    # hand-written answers: (float)n / K in f32
    assert K.decode_ints([-128, 0, 127, -127], "u8").tolist() == [float(F(-128) / F(127)), 0.0, 1.0, -1.0]
    assert K.bits(K.decode_ints([-128], "u8"))[0] == 0xBF810204  # -1.007874...: -128 / 127 rounded to nearest
    assert K.decode_ints([-32768, 32767, 1], "i16").tolist() == [float(F(-32768) / F(32767)), 1.0, float(F(1) / F(32767))]
    assert K.bits(K.decode_ints([-32768], "i16"))[0] == 0xBF800100  # -(1 + 2^-15 + 2^-30 ...) -> 1 + 2^-15 in 24 bits
    assert K.decode_ints([-8388608, 8388607, 1], "i24").tolist() == [-1.0, 1.0 - 2.0 ** -23, 2.0 ** -23]
    # i32: the integer is rounded to f32 first (2^24 + 1 -> 2^24, 2^31 - 1 -> 2^31), K = 2147483647 is 2^31 in f32
    assert K.decode_ints([lo, hi, 2 ** 24 + 1, 2 ** 24 - 1, -1], "i32").tolist() == [-1.0, 1.0, 2.0 ** -7, (2.0 ** 24 - 1) / 2.0 ** 31, -(2.0 ** -31)]
    assert np.array_equal(K.decode_bytes(np.array([0x00, 0xFF, 0x80], np.uint8), "u8"), K.decode_ints([-128, 127, 0], "u8"))
    assert K.decode_bytes(np.array([0xFF, 0xFF, 0xFF, 0x00, 0x00, 0x80], np.uint8), "i24").tolist() == [-(2.0 ** -23), -1.0]


def test_gain_yardstick_on_the_words_the_gpu_tests_write():
    """the gain the pack launch forms from a peak word: test_frames_norm_host.normalise on a one-sample job"""
    g = lambda word, target: normalise(f32([word]), target)[2]
    assert g(0, 1.0) == 1 and g(0x00000001, 1.0) == 1                # no peak; the quotient overflows
    assert g(K.bits(F(2))[()], 1.0) == F(0.5)
    assert K.bits(g(K.bits(F(3))[()], 1.0))[()] == 0x3EAAAAAB        # 1 / 3 rounded to nearest
    assert g(K.bits(F(0.7))[()], 0.5) == F(0.5) / F(0.7)
    z = normalise(np.array([2.0, 1e-40], np.float32), 1.0)[0]
    assert z[1] != 0 and K.bits(z[1:])[0] == K.bits(F(1e-40))[()] // 2  # the denormal, halved exactly (its bits are even)


def fade_abs(y, t0, in_len, out_start, out_len):
    """fadeutil.apply_fade for rows y[C, n] whose first frame is absolute frame t0 (fadeutil.sq on absolute positions):
    what the launches far into a job are held to, where apply_fade itself would need the whole job in memory"""
    z = np.array(y, np.float32, copy=True)
    t = t0 + np.arange(z.shape[1], dtype=np.uint64)
    with np.errstate(invalid="ignore"):
        m = t < np.uint64(in_len)
        if m.any():
            z[:, m] = z[:, m] * fadeutil.sq(t[m], in_len, False)
        if out_start != fadeutil.NONE:
            m = (t >= np.uint64(out_start)) & (t < np.uint64(out_start + out_len))
            if m.any():
                z[:, m] = z[:, m] * fadeutil.sq(t[m] - np.uint64(out_start), out_len, True)
            z[:, t >= np.uint64(out_start + out_len)] = F(0)
    return z


def test_fade_abs_is_apply_fade():
    y = np.stack([corner_set("i16")[:9000], corner_set("u8")[100:9100]])
    for in_len, out_start, out_len in ((0, fadeutil.NONE, 0), (5000, fadeutil.NONE, 0), (0, 3000, 4000), (6000, 2000, 5000),
                                       (100, 8000, 0), (9000, 0, 9000)):
        want = fadeutil.apply_fade(y, in_len, out_start, out_len, axis=1)
        assert K.same_floats(fade_abs(y, 0, in_len, out_start, out_len), want, nan_payloads=False)
        for t0 in (1, 2999, 7001):
            assert K.same_floats(fade_abs(y[:, t0:], t0, in_len, out_start, out_len), want[:, t0:], nan_payloads=False)


@pytest.mark.parametrize("width", ["narrow", "wide"])
def test_layout_sweep_keeps_every_value_and_every_pair(width):
    cases = K.layout_cases(width)
    want = {"channels": [c for c in K.CHANNELS if (c <= 8) == (width == "narrow")], "n_frames": K.FRAMES[width],
            "phase": [0, 1, 2, 3], "frame0": K.FRAME0[width], "pad": [0, 1, 3], "base": [0, 1, 2, 3], "tbase": [0, 1, 2, 3]}
    assert sorted(K.CHANNELS) == [1, 2, 3, 5, 7, 8, 9, 10, 63, 64, 65, 67, 128, 129, 130]
    for a in K.AXES:
        assert sorted({c[a] for c in cases}) == sorted(want[a]), a
        for b in K.AXES:
            if a < b:
                seen = {(c[a], c[b]) for c in cases}
                assert len(seen) == len(want[a]) * len(want[b]), (a, b, "a pair of values is never run")
    assert cases == K.layout_cases(width)
