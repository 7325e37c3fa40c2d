"""GPU tests of the dithered PCM pack kernels of rc_frames.hip through their launchers, called directly by way of the
test-hook entry rc_test_frames_pack_pcm_dither (tests/ditherutil.py): the planar samples, the launch's t0 and channel0 and
the way a range is cut into launches are chosen here, which no public entry allows.

Every comparison is of bytes against the numpy definition of tests/ditherutil.py applied to rows built on the host, with no
tolerance. Every target lies inside a larger buffer filled with a guard byte, and what lies outside the launch's range is
asserted unchanged. The shapes are the smallest with a tile edge inside a dword - 1- and 3-byte frames, odd phases - where a
tile quantises samples in front of its own range a second time: those must get the dither of their own frame and channel."""
import numpy as np
import pytest

import ditherutil as D
import frameskernelutil as K
from test_frames_pcm_host import count_clipped, edge_values

pytestmark = pytest.mark.gpu
SEED = 1
KEY_CHANNELS = 80  # the key table of every launch here: channel0 + channels <= 5 + 67
T0S = [0, 2 ** 32 - 7, 2 ** 40 + 3]  # (2^32 - 7: a launch of 14 frames or more runs across the counter's wrap)
CHANNEL0S = [0, 5]
MODES = ["tpdf", "tpdf-hp"]
PEAK_WORD, GAIN = 0x40000000, np.float32(0.5)  # the peak word of 2.0f under target_peak 1: a gain of exactly 0.5


def ceil16(n):
    return (int(n) + 15) // 16 * 16


@pytest.fixture(scope="module")
def keys():
    return K.DevBuf(D.keys_host(SEED, KEY_CHANNELS))


def rows(kind, ch, n):
    """x[C, n]: zeros (the output is rint(d): the dither's indexing alone), or the edge-value table, cycled"""
    if kind == "zeros":
        return np.zeros((ch, n), np.float32)
    e = edge_values()
    return np.resize(e, ch * n).reshape(ch, n).copy()


def launch(fmt, mode, x, phase, t0, channel0, keys, gain=False, tbase=0, target=None, frame0=0, n=None, lo=None):
    """One launch over the frames [frame0, frame0 + n) of the rows x[C, .] at absolute frame t0 + frame0. Without `target`,
    into a fresh guarded target, which is returned read back together with the block's first byte; with one (a DevBuf and
    `lo`, the byte where frame 0 of the rows lies), into its place there."""
    ch, total = x.shape
    n = total - frame0 if n is None else n
    B = K.BYTES[fmt]
    host, _ = K.planar_host(x, total, 0)
    planar = K.DevBuf(host)
    fresh = target is None
    if fresh:
        lo = 16 + 4 * tbase + phase
        target = K.DevBuf(K.guarded(ceil16(lo + total * ch * B + 16)))
    at = lo + frame0 * ch * B
    clipped = K.DevBuf(np.array([3], np.uint64))
    norm = K.DevBuf(K.norm_words(PEAK_WORD, -123.25)) if gain else None
    D.pack_pcm_dither(fmt, planar, frame0, total, target, at & ~3, at & 3, ch, n, clipped, D.MODES[mode], (t0 + frame0) % 2 ** 64, channel0,
                      keys, norm=norm)
    z = (x * GAIN).astype(np.float32) if gain else x
    assert int(clipped.read().view(np.uint64)[0]) == 3 + count_clipped(z[:, frame0:frame0 + n])
    if gain:
        assert norm.read().view(np.uint32).tolist() == [PEAK_WORD, int(K.bits(GAIN)[()])]
    assert planar.read().tobytes() == host.tobytes(), "the planar rows were written"
    return target, lo, z


def check_block(target, lo, z, fmt, mode, t0, channel0, what):
    """the whole target: guard bytes, the block by the numpy definition, guard bytes"""
    want = D.dithered_bytes(np.ascontiguousarray(z.T), fmt, mode, SEED, t0=t0, channel0=channel0)
    got = target.read()
    bad = np.nonzero(got[lo:lo + want.size] != want)[0]
    assert bad.size == 0, (what, f"{bad.size} of {want.size} bytes differ, the first at {bad[:8].tolist()}")
    assert (got[:lo] == K.GUARD).all() and (got[lo + want.size:] == K.GUARD).all(), (what, "guard bytes were written")
    return got[lo:lo + want.size]


def sweep(fmt, mode, channels, frames, keys):
    """channels x frames x byte phase x values x channel0 crossed in full. t0, the gain and the target's dword take turns
    on a running count of the launches, with periods (3, 6, 20) that share no cycle with the four launches of a phase or
    the sixteen of a shape: each of their values meets every phase, every kind of values and both channel0."""
    j = 0
    for ch in channels:
        for n in frames:
            for phase in range(4):
                for kind in ("zeros", "edges"):
                    for channel0 in CHANNEL0S:
                        t0 = T0S[j % 3]
                        gain = bool((j // 3) % 2)
                        tbase = (j // 5) % 4
                        j += 1
                        x = rows(kind, ch, n)
                        target, lo, z = launch(fmt, mode, x, phase, t0, channel0, keys, gain=gain, tbase=tbase)
                        check_block(target, lo, z, fmt, mode, t0, channel0, (fmt, mode, ch, n, phase, kind, channel0, t0, gain))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("fmt", D.DITHER_FORMATS)
def test_narrow_tiles(fmt, mode, keys):
    sweep(fmt, mode, [1, 2, 3, 8], [1, 5, 1023, 1025, 2049], keys)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("fmt", D.DITHER_FORMATS)
def test_wide_tiles(fmt, mode, keys):
    sweep(fmt, mode, [9, 65, 67], [1, 63, 65, 129], keys)


@pytest.mark.parametrize("mode", MODES)
def test_the_dither_is_there_and_depends_on_frame_channel_and_mode(mode, keys):
    """zeros in: the codes are rint(d), not all zero, and other frames, channels and modes give other codes"""
    x = rows("zeros", 2, 2049)
    a = check_block(*launch("i16", mode, x, 0, 0, 0, keys), "i16", mode, 0, 0, "base")
    assert K.bytes_ints(a, "i16").any()
    assert set(np.unique(K.bytes_ints(a, "i16")).tolist()) == {-1, 0, 1}
    b = check_block(*launch("i16", mode, x, 0, 1, 0, keys), "i16", mode, 1, 0, "t0 + 1")
    c = check_block(*launch("i16", mode, x, 0, 0, 5, keys), "i16", mode, 0, 5, "channel0 5")
    other = [m for m in MODES if m != mode][0]
    d = check_block(*launch("i16", other, x, 0, 0, 0, keys), "i16", other, 0, 0, "other mode")
    assert (a != b).any() and (a != c).any() and (a != d).any()
    assert (a[4:] == b[:-4]).all()  # frame t of the first launch is frame t - 1 of the second


@pytest.mark.parametrize("k", [1, 1023, 1024, 1029])
@pytest.mark.parametrize("fmt,ch", [("u8", 3), ("i24", 1)])
@pytest.mark.parametrize("mode", MODES)
def test_split_invariance(mode, fmt, ch, k, keys):
    """One launch over [0, n) and launches over [0, k) and [k, n), the second with t0 + k, write the same bytes: the
    samples in front of a tile that it quantises again take the dither of their own frame. Phase 1, so that the cut lies
    inside a dword."""
    n, t0 = 2049, 2 ** 32 - 1030
    x = rows("edges", ch, n)
    target, lo, z = launch(fmt, mode, x, 1, t0, 5, keys)
    one = check_block(target, lo, z, fmt, mode, t0, 5, "one launch")
    two = K.DevBuf(K.guarded(target.nbytes))
    launch(fmt, mode, x, 1, t0, 5, keys, target=two, lo=lo, frame0=0, n=k)
    head = two.read()
    nb = k * ch * K.BYTES[fmt]
    assert (head[lo:lo + nb] == one[:nb]).all() and (head[:lo] == K.GUARD).all() and (head[lo + nb:] == K.GUARD).all()
    launch(fmt, mode, x, 1, t0, 5, keys, target=two, lo=lo, frame0=k, n=n - k)
    both = check_block(two, lo, z, fmt, mode, t0, 5, ("two launches", k))
    assert (both == one).all()


@pytest.mark.parametrize("mode", MODES)
def test_the_launchers_own_split_advances_t0(mode, keys):
    """u8 x 1 channel, 2^27 + 1025 frames: the launcher cuts the job at 2^27 frames, and the second launch starts at
    t0 + 2^27. The planar zeros and the target live on the device alone; the windows [0, 4096) and
    [2^27 - 2048, 2^27 + 1025) of the target and the guard bytes around the block are brought back and compared."""
    import torch

    n, phase, t0, channel0 = (1 << 27) + 1025, 1, 2 ** 40 + 3, 5
    lo = 16 + phase
    planar = K.DevBuf.wrap(torch.zeros(4 * n, dtype=torch.uint8, device=K.DEVICE))
    target = K.DevBuf.wrap(torch.full((ceil16(lo + n + 16),), K.GUARD, dtype=torch.uint8, device=K.DEVICE))
    clipped = K.DevBuf(np.array([0], np.uint64))
    D.pack_pcm_dither("u8", planar, 0, n, target, 16, phase, 1, n, clipped, D.MODES[mode], t0, channel0, keys)
    assert int(clipped.read().view(np.uint64)[0]) == 0
    for a, b in ((0, 4096), ((1 << 27) - 2048, n)):
        got = target.t[lo + a:lo + b].cpu().numpy()
        want = D.dithered_bytes(np.zeros((b - a, 1), np.float32), "u8", mode, SEED, t0=t0 + a, channel0=channel0)
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, (a, b, bad.size, bad[:8].tolist())
    assert (target.t[:lo].cpu().numpy() == K.GUARD).all() and (target.t[lo + n:].cpu().numpy() == K.GUARD).all()
