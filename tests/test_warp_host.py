"""CPU tests (-m "not gpu") of the output warp's host side (include/rocoder_hip_warp.h): the tier constants against exact
arithmetic, rc_warp_table against the f64 definition of tests/warputil.py and against rc_resample_table's rows, the error of
the linear interpolation between 256 phases against a bound taken from the f64 prototype, rc_warp_curve against its Python
twin bit for bit - and the gate of the GPU kernel test itself, asserted on a CPU f32 implementation and refused for eight
mutants."""
import ctypes as C
import os
import re
import sys
from fractions import Fraction

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
rocoder_amd = pytest.importorskip("rocoder_amd")
from rocoder_amd import _lib  # noqa: E402
from rocoder_amd.stretcher import (derive_params, make_config, resample_len, resample_table, time_map_curve, warp_curve,  # noqa: E402
                                   warp_table)

import warputil as Wp  # noqa: E402

_tables = {}


def table(t):
    if t not in _tables:
        _tables[t] = warp_table(t)
        _tables[t].flags.writeable = False
    return _tables[t]


def test_symbols_agree_in_header_ctypes_and_libraries():
    h = open(os.path.join(ROOT, "include", "rocoder_hip_warp.h")).read()
    assert '#include "rocoder_hip_warp.h"' in open(os.path.join(ROOT, "include", "rocoder_hip.h")).read()
    assert re.search(r"\nint rc_engine_set_output_warp\(rc_engine \*e, const int64_t \*anchor, size_t n_anchors, size_t n_out\);", h)
    assert re.search(r"\nint rc_warp_table\(uint32_t tier, float \*table, size_t cap, uint32_t \*rows, uint32_t \*taps\);", h)
    assert "\nint rc_warp_curve(const rc_config *cfg, const int64_t *hop_pos, size_t n_hops, const double *at, const double *ratio," in h
    for name in ("rc_engine_set_output_warp", "rc_warp_table", "rc_warp_curve"):
        assert name in _lib.WARP_SYMBOLS and hasattr(_lib.lib(), name), name
    assert _lib.lib().rc_abi_version() == 5
    assert b"rc_test_frames_warp" not in open(_lib.LIB_PATH, "rb").read()
    with _lib.hooks_library() as H:
        assert hasattr(H, "rc_test_frames_warp")


def test_the_thirteen_tiers_are_the_exact_values():
    h = open(os.path.join(ROOT, "include", "rocoder_hip_warp.h")).read()
    d_list = re.search(r"#define RC_WARP_D_LIST(.*?)\n/\*", h, re.S).group(1)
    w_list = re.search(r"#define RC_WARP_W_LIST(.*)", h).group(1)
    assert [int(v) for v in re.findall(r"(\d+)LL", d_list)] == Wp.D
    assert [int(v) for v in re.findall(r"\d+", w_list)] == Wp.W
    for t in range(Wp.TIERS):
        d, w = Wp.D[t], Wp.W[t]
        # d = floor(2^(t/4) * 2^38)  <=>  d^4 <= 2^t * 2^152 < (d + 1)^4;  w = ceil(32 * 2^(t/4))  <=>  (w - 1)^4 < 32^4 2^t <= w^4
        assert Fraction(d) ** 4 <= Fraction(2) ** (t + 152) < Fraction(d + 1) ** 4, t
        assert Fraction(w - 1) ** 4 < Fraction(32) ** 4 * 2 ** t <= Fraction(w) ** 4, t
        assert Wp.tier_of(d) == t and (t == Wp.TIERS - 1 or Wp.tier_of(d + 1) == t + 1)
    assert Wp.D[0] == 2 ** 38 and Wp.D[12] == Wp.D_MAX == 2 ** 41 and Wp.tier_of(Wp.D_MIN) == 0
    assert sum(Wp.ROWS * 2 * w for w in Wp.W) == 743244


@pytest.mark.parametrize("t", range(Wp.TIERS))
def test_table_is_the_f64_definition_rounded_once(t):
    """every coefficient within 2^-24 absolute: an f32 rounding of a value <= 1, plus one flip at a rounding boundary where
    libm and numpy differ in the last f64 bit; 257 rows of 2 W taps"""
    got, ref = table(t), Wp.table_f64(t)
    assert got.shape == (Wp.ROWS, 2 * Wp.W[t]) == ref.shape and got.dtype == np.float32
    err = np.abs(got.astype(np.float64) - ref).max()
    print(f"tier {t}: T = {2 * Wp.W[t]}, max |h - h64| = {err * 2 ** 24:.3f} * 2^-24")
    assert err <= 2.0 ** -24
    assert (got[256, 1:] == got[0, :-1]).all() and got[256, 0] == 0.0  # row 256 is row 0 one tap on


def test_table_sizes_and_refusals():
    L = _lib.lib()
    u32p = C.POINTER(C.c_uint32)
    rows, taps = C.c_uint32(0), C.c_uint32(0)
    assert L.rc_warp_table(3, None, 0, C.byref(rows), C.byref(taps)) == 0 and (rows.value, taps.value) == (257, 108)
    buf = np.full(257 * 108, 7.0, np.float32)
    fp = buf.ctypes.data_as(C.POINTER(C.c_float))
    assert L.rc_warp_table(3, fp, buf.size - 1, C.byref(rows), C.byref(taps)) == _lib.RC_ECAPACITY and (buf == 7.0).all()
    assert L.rc_warp_table(3, fp, buf.size, C.byref(rows), C.byref(taps)) == 0 and np.array_equal(buf.reshape(257, 108), table(3))
    assert L.rc_warp_table(13, None, 0, C.byref(rows), C.byref(taps)) == _lib.RC_EINVAL
    assert L.rc_warp_table(0, None, 0, u32p(), C.byref(taps)) == _lib.RC_EINVAL


@pytest.mark.parametrize("num,den,t", [(1, 2, 0), (1, 4, 0), (3, 4, 0), (3, 8, 0), (1, 8, 0), (1, 1, 0), (2, 1, 4), (4, 1, 8), (8, 1, 12)])
def test_tables_hold_the_rational_resamplers_rows(num, den, t):
    """at these constant steps the warp IS the rational resampler: the same rows, bit for bit, at p * 256 / den"""
    r = resample_table(num, den)
    assert Wp.tier_of(num * 2 ** 38 // den) == t and r.shape == (den, 2 * Wp.W[t])
    assert np.array_equal(r.view(np.uint32), table(t)[np.arange(den) * 256 // den].view(np.uint32))


@pytest.mark.parametrize("t", range(Wp.TIERS))
def test_interpolation_between_phases_stays_within_the_second_derivative_bound(t):
    """|(1 - a) h[p][j] + a h[p + 1][j] - h(u - a / 256)| <= max |h''| / (8 * 256^2) + 2^-24 |h| at a = 1/4, 1/2, 3/4, every
    row and tap: the error of linear interpolation over a step of 1/256 plus the f32 rounding of the two entries. max |h''|
    is the largest second difference of the f64 prototype on a grid of 1/1024 inside its support - not of the code under
    test. The bound is Taylor's, and holds where h is smooth between the two entries. The prototype of DESIGN 6h is not
    smooth at the ends of its support: a Kaiser window of beta = 9 ends at 1 / I0(9) = 9.1e-4, not at zero, so h steps from
    c sinc(c W) / I0(9) (4.8e-6 at tier 0, 3.0e-7 at tier 12) to zero at |u| = W. The two pairs of a row that straddle
    that step (tap 0 of rows 255 / 256, the last tap of rows 0 / 1) get the step added to their bound, and only they."""
    got = table(t).astype(np.float64)
    w = Wp.W[t]
    g = 1.0 / 1024
    u = np.arange(-w + 2 * g, w - g, g)
    h2 = np.abs(Wp.prototype(t, u - g) - 2 * Wp.prototype(t, u) + Wp.prototype(t, u + g)).max() / g ** 2
    edge = abs(float(Wp.prototype(t, np.nextafter(float(w), 0.0))))
    j = np.arange(2 * w, dtype=np.float64)[None, :]
    p = np.arange(256, dtype=np.float64)[:, None]
    worst_db = -np.inf
    for a in (0.25, 0.5, 0.75):
        uu = j - (w - 1) - (p + a) / 256
        true = Wp.prototype(t, uu)
        lin = (1 - a) * got[:256] + a * got[1:]
        err = np.abs(lin - true)
        straddles = (np.abs(j - (w - 1) - p / 256) >= w) | (np.abs(j - (w - 1) - (p + 1) / 256) >= w)
        bound = h2 / (8 * 256 ** 2) + 2.0 ** -24 * np.abs(true) + np.where(straddles, edge, 0.0)
        rows_db = 20 * np.log10(err.sum(axis=1).max())
        worst_db = max(worst_db, rows_db)
        print(f"tier {t} a = {a}: max tap error {err.max():.3e} (bound {bound[err == err.max()].max():.3e}), "
              f"largest row sum {rows_db:.1f} dB, max |h''| = {h2:.3f}")
        assert (err <= bound).all()
    assert worst_db < -90.0  # at the level of the filter's own stop band


# ---- rc_warp_curve against the twin ------------------------------------------------------------------------------------
KW = dict(window_len=1024, factor=2.0)


def both(n, at, ratio, hop_pos=None, n_hops=None, **kw):
    kw = kw or KW
    par = derive_params(**kw)
    got, got_out = warp_curve(n, at, ratio, hop_pos=hop_pos, n_hops=n_hops, **kw)
    want, want_out = Wp.warp_curve(par, hop_pos, len(hop_pos) if hop_pos is not None else n_hops, at, ratio, n)
    assert np.array_equal(got, want) and got_out == want_out
    d = np.diff(got)
    assert got[0] == 0 and (d >= Wp.D_MIN).all() and (d <= Wp.D_MAX).all()
    assert got[-1] >> 32 >= n and (got.size < 2 or got[-2] >> 32 < n)
    assert got_out == sum(1 for m in range(max(0, Wp.BLOCK * (got.size - 3)), Wp.BLOCK * (got.size - 1))
                          if Wp.position(got, m)[0] >> 32 < n) + max(0, Wp.BLOCK * (got.size - 3))
    return got, got_out


def test_curve_of_a_ramp_is_the_twins():
    a, n_out = both(40000, [0.0, 9000.0, 15000.0], [0.5, 2.2, 1.3], n_hops=80)
    assert len(set(np.diff(a).tolist())) > 10 and 0 < n_out <= 64 * (a.size - 1)


def test_curve_of_one_point_and_the_constant_ratios():
    a, n_out = both(12345, [0.0], [1.0], n_hops=40)
    assert np.array_equal(a, np.arange(a.size, dtype=np.int64) << 38) and n_out == 12345
    for n in (1, 63, 64, 65, 12345):
        a, n_out = both(n, [100.0], [0.75], n_hops=40)
        assert n_out == resample_len(n, 3, 4) and (np.diff(a) == 3 << 36).all()
    a, n_out = both(0, [0.0], [1.0], n_hops=4)
    assert a.tolist() == [0] and n_out == 0


def test_curve_whose_clamp_engages():
    """r * 2^38 + 0.5 floors to 2^35 - 1 ... below the lowest step and above the highest: both ends are clamped"""
    lo = 0.125 * (1 + 2.0 ** -40)
    a, _ = both(3000, [0.0, 4000.0], [0.125, 8.0], n_hops=30)
    d = np.diff(a)
    assert d[0] == Wp.D_MIN
    a, _ = both(9000, [0.0], [8.0], n_hops=30)
    assert (np.diff(a) == Wp.D_MAX).all()
    a, _ = both(900, [0.0], [lo], n_hops=30)
    assert (np.diff(a) == Wp.D_MIN).all()


def test_curve_over_a_reversed_map():
    kw = dict(window_len=1024, factor=4.0)
    hop_pos = time_map_curve(30000, [0.0, 30000.0], [2.0, 6.0], **kw)[::-1].copy()
    par = derive_params(**kw)
    n = hop_pos.size // par.hops_per_window * par.window_out_len
    a, n_out = both(n, [0.0, 10000.0, 30000.0], [2.0, 0.5, 1.0], hop_pos=hop_pos, **kw)
    r = np.diff(a) / 2.0 ** 38
    # the ratio follows the INPUT position, which runs backwards: the output ends where the input begins, at a ratio of 2
    assert r[-1] == 2.0 and r[0] < 1.0 and r.min() < 0.7 and n_out > 0


def test_curve_capacity_idiom_and_refusals():
    L = _lib.lib()
    cfg, _keep = make_config(**KW)
    dp, ip, sp = C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_size_t)
    at, ratio = (C.c_double * 2)(0.0, 5000.0), (C.c_double * 2)(0.5, 2.0)
    na, no = C.c_size_t(0), C.c_size_t(0)

    def call(n_hops=50, at=at, ratio=ratio, n_points=2, n=20000, anchor=None, cap=0, pna=C.byref(na), pno=C.byref(no), pos=None):
        return L.rc_warp_curve(C.byref(cfg), pos, n_hops, at, ratio, n_points, n, anchor, cap, pna, pno)

    assert call() == _lib.RC_ECAPACITY and na.value > 2 and no.value > 0
    A = na.value
    buf = np.full(A, -7, np.int64)
    assert call(anchor=buf.ctypes.data_as(ip), cap=A - 1) == _lib.RC_ECAPACITY and (buf == -7).all()
    assert call(anchor=buf.ctypes.data_as(ip), cap=A) == 0 and na.value == A and buf[0] == 0 and (np.diff(buf) > 0).all()
    assert call(n_hops=0) == _lib.RC_EINVAL
    assert call(n_points=0) == _lib.RC_EINVAL
    assert call(at=dp()) == _lib.RC_EINVAL and call(ratio=dp()) == _lib.RC_EINVAL
    assert call(pna=sp()) == _lib.RC_EINVAL and call(pno=sp()) == _lib.RC_EINVAL
    assert call(cap=3) == _lib.RC_EINVAL  # a capacity without a buffer
    assert call(n=2 ** 29 + 1) == _lib.RC_EINVAL
    assert call(at=(C.c_double * 2)(5.0, 5.0)) == _lib.RC_EINVAL and call(at=(C.c_double * 2)(-1.0, 5.0)) == _lib.RC_EINVAL
    for bad in (0.1249, 8.001, float("nan"), float("inf")):
        assert call(ratio=(C.c_double * 2)(1.0, bad)) == _lib.RC_EINVAL
    bad_cfg, _k = make_config(window_len=1024, factor=2.0)
    bad_cfg.window_len = 7
    assert L.rc_warp_curve(C.byref(bad_cfg), None, 50, at, ratio, 2, 100, None, 0, C.byref(na), C.byref(no)) != 0


# ---- the gate of tests/test_gpu_frames_warp_kernel.py, on a CPU implementation and its mutants --------------------------
@pytest.fixture(scope="module")
def glide():
    """the rows and the anchors of the GPU kernel test; the outputs looked at are whole blocks of every tier the glide
    reaches, neighbours of different tiers among them, and every output that reads row 256"""
    rows = Wp.white_rows()
    anchors, n_out = Wp.glide_case()
    tiers = [Wp.tier_of(int(d)) for d in np.diff(anchors)]
    assert set(tiers) == set(range(7)) and any(a > b for a, b in zip(tiers, tiers[1:]))
    tables = {t: table(t) for t in set(tiers)}
    picked = [b for b in range(len(tiers) - 1) if b in (0, 7, 13, 19, 20, 26, 27, 28)]
    ranges = [(64 * b, min(64 * b + 64, n_out)) for b in picked]
    last_rows = [m for m in range(n_out) if Wp.split(Wp.position(anchors, m)[0])[1] == 255]
    assert {tiers[b] for b in picked} == set(range(7)) and len(last_rows) >= 3
    ranges += [(m, m + 1) for m in last_rows if not any(a <= m < b for a, b in ranges)]
    want = [Wp.warp_f64(rows, tables, anchors, n_out, m0=a, m1=b) for a, b in ranges]
    return rows, anchors, n_out, tables, ranges, want


def worst(glide, **mut):
    rows, anchors, n_out, tables, ranges, want = glide
    tables = {**{t: table(t) for t in range(8)}, **tables}  # (a mutant may pick a tier the glide does not use)
    ratio = 0.0
    for (a, b), (y, bound) in zip(ranges, want):
        got = Wp.warp_f32(rows, tables, anchors, n_out, m0=a, m1=b, **mut)
        ratio = max(ratio, (np.abs(got.astype(np.float64) - y) / bound).max())
    return ratio


def test_the_gate_passes_a_cpu_f32_implementation(glide):
    r = worst(glide)
    print(f"honest f32: {r:.3f} of the bound")
    assert r <= 1.0


@pytest.mark.parametrize("mutant", [dict(drop_a=True), dict(tier_shift=1), dict(tier_shift=-1), dict(wrap_row=True), dict(wrap32=True),
                                    dict(next_shift=1), dict(k0_shift=1), dict(k0_shift=-1)],
                         ids=lambda m: "-".join(f"{k}{v}" for k, v in m.items()))
def test_the_gate_refuses_the_mutants(glide, mutant):
    r = worst(glide, **mutant)
    print(f"{mutant}: {r:.1f} times the bound")
    assert r > 1.0
