"""GPU tests of the launchers of rocoder_amd/csrc/rc_phase.h, called through the test-hook entries rc_test_phase_*
(rc_phase_hooks.hip, librocoder_hip_hooks.so only), against the numpy twin of the definition (tests/phaseutil.py): bit for
bit wherever the definition is in integers. Every call asserts on the host, before it launches, that the rows it hands
over have the sizes the launcher reads and writes."""
import numpy as np
import pytest

import phaseutil as pu

import rocoder_amd  # noqa: F401

pytestmark = pytest.mark.gpu


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def _spec_rows(X, N):
    """[ch, rows, H + 1] complex bins -> the float32 [ch, rows, N, 2] rows the analysis writes (Hermitian above H)"""
    X = np.asarray(X)
    H = N // 2
    full = np.concatenate([X, np.conj(X[..., 1:H][..., ::-1])], axis=-1)
    return np.stack([full.real, full.imag], axis=-1).astype(np.float32)


def run_prep(spec, N, step, locked, halo):
    """spec: float32 [ch, halo + hops, N, 2] -> (P, e) as int64 [ch, hops, H + 1]"""
    import torch

    ch, rows = spec.shape[:2]
    hops, nb = rows - halo, N // 2 + 1
    assert spec.shape == (ch, rows, N, 2) and spec.dtype == np.float32 and hops >= 1 and halo in (0, 1)
    d_spec = _dev(spec)
    pe = torch.full((ch, hops, 2, nb), 0xA5A5A5A5 - (1 << 32), dtype=torch.int32, device="cuda")
    pu.done("rc_test_phase_prep", pu.hooks().rc_test_phase_prep(d_spec.data_ptr(), pe.data_ptr(), N, step, int(locked), ch, halo, hops))
    out = pe.cpu().numpy().astype(np.int64) & pu.MASK
    return out[:, :, 0], out[:, :, 1]


def run_scan(P, e, theta0, N, block):
    """P, e: [ch, hops, H + 1]; theta0: [ch, H + 1] -> (theta of every hop [ch, hops, H + 1], the carried state [ch, H + 1])"""
    import torch

    ch, hops, nb = P.shape
    assert nb == N // 2 + 1 and e.shape == P.shape and theta0.shape == (ch, nb) and block >= 1
    assert P.min() >= 0 and P.max() < nb  # the launcher gathers through P unchecked
    n_blocks = (hops + block - 1) // block
    pe = _dev(np.stack([P, e], axis=2).astype(np.uint32).view(np.int32))
    base = torch.full((ch, n_blocks, nb), -1, dtype=torch.int32, device="cuda")
    theta = _dev(theta0.astype(np.uint32).view(np.int32))
    pu.done("rc_test_phase_scan", pu.hooks().rc_test_phase_scan(pe.data_ptr(), base.data_ptr(), theta.data_ptr(), N, ch, block, hops))
    qs = pe.cpu().numpy().astype(np.int64) & pu.MASK
    b = base.cpu().numpy().astype(np.int64) & pu.MASK
    Q, s = qs[:, :, 0], qs[:, :, 1]
    assert Q.max() < nb
    blk = np.arange(hops) // block
    th = np.stack([(np.take_along_axis(b[c][blk], Q[c], axis=1) + s[c]) & pu.MASK for c in range(ch)])
    return th, theta.cpu().numpy().astype(np.int64) & pu.MASK, (qs, b)


def run_apply(spec, theta, N, halo=0, block=4):
    """spec float32 [ch, halo + hops, N, 2], theta [ch, hops, H + 1] -> Z float32 [ch, hops, N, 2]; the rotation goes in
    as (Q, s) = (identity, theta) over zero base states"""
    import torch

    ch, rows = spec.shape[:2]
    hops, nb = rows - halo, N // 2 + 1
    assert spec.shape == (ch, rows, N, 2) and theta.shape == (ch, hops, nb)
    Q = np.broadcast_to(np.arange(nb), theta.shape)
    pe = _dev(np.stack([Q, theta], axis=2).astype(np.uint32).view(np.int32))
    base = torch.zeros((ch, (hops + block - 1) // block, nb), dtype=torch.int32, device="cuda")
    out = torch.full((ch, hops, N, 2), float("nan"), dtype=torch.float32, device="cuda")
    d_spec = _dev(spec)
    pu.done("rc_test_phase_apply", pu.hooks().rc_test_phase_apply(d_spec.data_ptr(), out.data_ptr(), pe.data_ptr(), base.data_ptr(), N, ch, halo, block, hops))
    return out.cpu().numpy()


# ------------------------------------------------------------------------------------------------ phase_prep
def _int_spectra(rng, ch, rows, N, lo=-40, hi=41):
    """small-integer components: m2 and its comparisons are exact in f32, ties included"""
    nb = N // 2 + 1
    return rng.integers(lo, hi, (ch, rows, nb)) + 1j * rng.integers(lo, hi, (ch, rows, nb))


def _hand_spectra(N):
    """the hand cases of tests/test_phase_host.py as hops of one channel (a first hop in front: the halo)"""
    H = N // 2
    rows = []

    def hop(peaks_at, base=1.0, top=3.0):
        m = np.full(H + 1, base)
        for j, v in (peaks_at.items() if isinstance(peaks_at, dict) else ((j, top) for j in peaks_at)):
            m[j] = v
        rows.append(m * (1 + 0j))

    hop([])                                        # the halo hop
    hop({1: 2.0, 2: 3.0, H - 2: 3.0, H - 1: 2.0})  # peaks at 2 and H - 2; 1 and H - 1 lose
    hop([1, H - 1])                                # the edge bins as peaks
    hop([0, H])                                    # bins 0 and H are never peaks
    hop({6: 3.0, 7: 3.0})                          # a plateau
    hop({6: 3.0, 8: 3.0})                          # equal at distance 2
    hop([5])                                       # one peak
    hop([4, 10])                                   # an equidistant bin
    rows.append(np.zeros(H + 1, complex))          # a silent hop
    return np.stack(rows)[None]


@pytest.mark.parametrize("N", [32, 512, 16384])
def test_prep_owner_is_the_twins(N):
    rng = np.random.default_rng(N)
    X = np.concatenate([_hand_spectra(N), _int_spectra(rng, 1, 64, N, -6, 7)], axis=1)  # (a narrow range: many ties)
    X = np.concatenate([X, np.concatenate([_int_spectra(rng, 1, X.shape[1] - 8, N), X[:, :8]], axis=1)])  # a second channel
    P, _e = run_prep(_spec_rows(X, N), N, N // 8, True, 1)
    for c in range(2):
        for k in range(1, X.shape[1]):
            m2 = X[c, k].real ** 2 + X[c, k].imag ** 2
            assert list(P[c, k - 1]) == list(pu.owners(m2, True)), (c, k)
    # PROPAGATE: the identity; a first hop without a halo: the identity and no increment
    P1, _ = run_prep(_spec_rows(X, N), N, N // 8, False, 1)
    assert (P1 == np.arange(N // 2 + 1)).all()
    P0, e0 = run_prep(_spec_rows(X, N), N, N // 8, True, 0)
    assert (P0[:, 0] == np.arange(N // 2 + 1)).all() and not e0[:, 0].any()
    assert (P0[:, 1:] == P[:, :]).all()


def _turns_from_gpu(X, N):
    """a[j] as the kernel forms it, read back through e: behind a hop of ones (a_prev == 0) at H / step == 2,
    e = -a + ((j & 1) << 31) + 2 (a - expect) exactly, whatever the wrap of dev"""
    ch, hops, nb = X.shape
    H, step = N // 2, N // 4
    pair = np.stack([np.ones_like(X), X], axis=2).reshape(ch * hops, 2, nb)
    _P, e = run_prep(_spec_rows(pair, N), N, step, False, 1)
    j = np.arange(nb)
    expect = ((j * step) % N) * ((1 << 32) // N)
    return ((e[:, 0] - ((j & 1) << 31) + 2 * expect) & pu.MASK).reshape(ch, hops, nb)


@pytest.mark.parametrize("N", [32, 512, 16384])
def test_prep_turns_are_within_the_bound_and_increments_exact_given_them(N):
    rng = np.random.default_rng(100 + N)
    hops = 64 if N < 16384 else 8
    X = _int_spectra(rng, 1, hops + 1, N)
    X[0, 1, :4] = [1, -1, 1j, -1j]  # the axes: 0, half a turn, a quarter, three quarters
    X[0, 2, :3] = [0, -3 + 0j, complex(-3, -0.0)]  # atan2(0, 0) == 0; the two signs of zero at half a turn
    a = _turns_from_gpu(X, N)
    want = pu.turns(X)
    d = (a - want) & pu.MASK
    d = np.minimum(d, (1 << 32) - d)
    # 2^-22 turn = 2^10 units: atan2f within 6 ulp (of pi: half a turn) + the two roundings, at half a turn
    print(f"N={N}: a is within {d.max()} units of 2^-32 turn")
    assert d.max() <= 1 << 10
    assert list(a[0, 1, :4]) == [0, 1 << 31, 1 << 30, 3 << 30]
    assert a[0, 2, 0] == 0 and a[0, 2, 1] == 1 << 31 and a[0, 2, 2] == 1 << 31
    for step in (N // 2, N // 4, N // 16, 5, N // 2 - 1, N // 3, 3 * N // 4 + 1):
        _P, e = run_prep(_spec_rows(X, N), N, step, True, 1)
        for k in range(1, hops + 1):
            assert list(e[0, k - 1]) == list(pu.increments(a[0, k - 1], a[0, k], N, step)), (step, k)


# ------------------------------------------------------------------------------------------------ phase_scan
def _maps(rng, kind, ch, hops, nb):
    j = np.arange(nb)
    if kind == "identity":
        return np.broadcast_to(j, (ch, hops, nb)).copy()
    if kind == "reversal":
        return np.broadcast_to(j[::-1], (ch, hops, nb)).copy()
    if kind == "constant":
        return np.broadcast_to(rng.integers(0, nb, (ch, hops, 1)), (ch, hops, nb)).copy()
    if kind == "nearest":  # what prep makes: piecewise constant, idempotent
        P = np.empty((ch, hops, nb), np.int64)
        for c in range(ch):
            for k in range(hops):
                P[c, k] = pu.owners(rng.integers(0, 5, nb).astype(float), True)
        return P
    return rng.integers(0, nb, (ch, hops, nb))  # arbitrary


def _scan_case(N, block, hops, kind, seed):
    rng = np.random.default_rng(seed)
    nb, ch = N // 2 + 1, 2
    P = _maps(rng, kind, ch, hops, nb)
    e = rng.integers(0, 1 << 32, (ch, hops, nb))
    th0 = rng.integers(0, 1 << 32, (ch, nb))  # a carried state that is not zero
    th, carried, _raw = run_scan(P, e, th0, N, block)
    for c in range(ch):
        want = pu.scan_sequential(P[c], e[c], th0[c])
        assert (th[c] == want).all(), (N, block, hops, kind, c, np.argwhere(th[c] != want)[:3])
        assert (carried[c] == want[-1]).all(), (N, block, hops, kind, c)


@pytest.mark.parametrize("kind", ["arbitrary", "constant", "reversal", "identity", "nearest"])
@pytest.mark.parametrize("which", ["shipped", 1, 2])
def test_scan_is_the_sequential_definition(which, kind):
    # shipped: the block the engine takes for a chunk of that many hops, from the shortest chunk to the longest
    blocks = sorted({int(pu.hooks().rc_test_phase_scan_block(h)) for h in (1, 2600, 10000, 32767)}) if which == "shipped" else [which]
    assert blocks[0] >= 1 and (which != "shipped" or blocks == [16, 32, 64, 128])
    for B in blocks:
        for i, hops in enumerate(sorted({1, max(1, B - 1), B, B + 1, 3 * B + 2})):
            _scan_case(32, B, hops, kind, 1000 * B + i)
        _scan_case(512, B, 3 * B + 2, kind, 7 + B)


@pytest.mark.parametrize("block,hops", [(2, 7), ("shipped", None)])
def test_scan_at_the_longest_window(block, hops):
    """N = 16384: 1024 threads, nine bins each, the last of them past H"""
    B = int(pu.hooks().rc_test_phase_scan_block(2600)) if block == "shipped" else block  # (a chunk of this window's job)
    _scan_case(16384, B, hops or B + 1, "arbitrary", 5)
    _scan_case(16384, B, hops or B + 1, "nearest", 6)


# ------------------------------------------------------------------------------------------------ phase_apply
@pytest.mark.parametrize("N", [32, 512, 16384])
def test_apply(N):
    rng = np.random.default_rng(200 + N)
    H, nb, hops = N // 2, N // 2 + 1, 6
    spec = rng.standard_normal((2, hops + 1, N, 2)).astype(np.float32)  # (not Hermitian: apply reads bins 0 ... H alone)
    spec[0, 1, 3] = [0.0, -0.0]
    spec[0, 1, 4] = [-0.0, 2.5]
    theta = np.zeros((2, hops, nb), np.int64)
    theta[:, 1] = 1 << 30           # a quarter turn
    theta[:, 2] = 1 << 31           # half a turn
    theta[:, 3] = 3 << 30           # three quarters
    theta[:, 4:] = rng.integers(0, 1 << 32, (2, hops - 4, nb))
    theta[0, 4, :6] = [1, (1 << 32) - 1, (1 << 29), (1 << 29) - 1, 0xE0000000, 0xDFFFFFFF]  # the edges of the quarter reduction
    Z = run_apply(spec, theta, N, halo=1)
    X = spec[:, 1:]
    # theta == 0: the bits of bins 0 ... H, exact conjugates above
    assert Z[:, 0, :nb].tobytes() == X[:, 0, :nb].tobytes()
    up = Z[:, :, nb:][:, :, ::-1]  # bins N - 1 ... H + 1 reversed: the partners of bins 1 ... H - 1
    assert up[..., 0].tobytes() == np.ascontiguousarray(Z[:, :, 1:H, 0]).tobytes()
    assert np.ascontiguousarray(up[..., 1]).tobytes() == np.ascontiguousarray(-Z[:, :, 1:H, 1]).tobytes()
    Zc = Z[..., 0].astype(np.float64) + 1j * Z[..., 1]
    Xc = X[..., 0].astype(np.float64) + 1j * X[..., 1]
    mag = np.abs(Xc[:, :, :nb])
    # the quarter turns are swaps and signs of v_cos(0) == 1, v_sin(0) == 0: exact
    for k, rot in ((1, 1j), (2, -1), (3, -1j)):
        assert (Zc[:, k, :nb] == Xc[:, k, :nb] * rot).all(), k
    # any rotation to 2^-22 of the bin's magnitude: the products' and the sum's roundings (3 x 2^-24), the argument's
    # conversion (2 pi 2^-28) and v_sin / v_cos within an eighth of a turn
    want = Xc[:, :, :nb] * np.exp(2j * np.pi * theta / 2.0 ** 32)
    err = np.abs(Zc[:, :, :nb] - want) / np.maximum(mag, 1e-30)
    print(f"N={N}: rotation error {err.max():.3e} of the magnitude (2^-22 = {2.0 ** -22:.3e})")
    assert err.max() <= 2.0 ** -22
