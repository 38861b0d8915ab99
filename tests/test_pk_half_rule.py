"""The argument behind search_pkp_kernel's shorter end of row (search_pk.hip, EOR), in numpy on
the CPU: the lazy pair step that also records which lane half of a block holds a new minimum,
and the two-level rescan of that half's 16 rows, against a brute-force NoDuplicates argmin.

The model keeps per col0 what the kernel keeps per distance field: the running minimum R, the
tie marker M (0 = a second column at the running minimum), the block base and the half of the
last strict drop. A block's 32 rows belong to the halves as the MFMA accumulator lays them out:
register r of lane half h holds row rrow(r, h) = (r & 3) + 8 (r >> 2) + 4 h. On a strict drop
with equal minima in both halves the marker becomes 0 at once ("equal halves on a drop => tie");
otherwise the half with the smaller minimum is recorded and only its 16 rows are rescanned:
first ham_lo (descriptor words 0 and 1) against the minimum, then the full distance of the
candidates. Blocks are visited in the kernel's order (tools/reach_sim.py order_current), the
partial last block of a chunk first, its columns past the row padded.
"""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.reach_sim import order_current  # noqa: E402

WORDS = 4
MASK = np.array([0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0x3FFFFFFF], np.uint32)
PAD = 1 << 20
WAVE_COLS = 128          # col0 per wave: two wide tiles
WAVES = 2                # per workgroup in the model
CHUNK = 128              # col1 per chunk in the model: several chunks, the order wraps
POP8 = np.array([bin(i).count("1") for i in range(256)], np.int32)


def rrow(r, h):
    return (r & 3) + 8 * (r >> 2) + 4 * h


def half_of_row(row):
    return (row >> 2) & 1


def popc(x):
    return POP8[np.ascontiguousarray(x).view(np.uint8)].reshape(x.shape + (4,)).sum(axis=-1)


def distances(a, b):
    """(ham_lo, ham) [W, W] of left descriptors a and right descriptors b ([W, 4] uint32)."""
    x = popc(a[:, None, :] ^ b[None, :, :])
    return x[:, :, :2].sum(axis=-1), x.sum(axis=-1)


def brute_force(ham):
    """NoDuplicates: the column of the minimum, -1 where the minimum occurs twice."""
    m = ham.min(axis=1)
    return np.where((ham == m[:, None]).sum(axis=1) == 1, ham.argmin(axis=1), -1)


def lazy_half_search(ham_lo, ham, stats=None):
    """The kernel's end result per col0 from the model described in the module docstring."""
    W = ham.shape[0]
    out = np.full(W, -2, np.int64)
    rows = np.arange(32)
    in_half = [half_of_row(rows) == 0, half_of_row(rows) == 1]
    per_wg = WAVE_COLS * WAVES
    for c0_wave in range(0, W, WAVE_COLS):
        hi = min(W, c0_wave + WAVE_COLS)
        n = hi - c0_wave
        wg_hi = (c0_wave // per_wg + 1) * per_wg - 1
        R = np.full(n, PAD, np.int64)
        M = np.full(n, 0xFFFF, np.int64)
        Cb = np.zeros(n, np.int64)
        Ch = np.zeros(n, np.int64)
        for B in order_current(c0_wave, wg_hi, W, CHUNK):
            blk = np.full((n, 32), PAD, np.int64)
            w = min(32, W - B)
            blk[:, :w] = ham[c0_wave:hi, B:B + w]
            m0 = blk[:, in_half[0]].min(axis=1)
            m1 = blk[:, in_half[1]].min(axis=1)
            comb = np.minimum(m0, m1)
            diff = comb - R
            drop = diff < 0
            M = np.where(drop, (m0 != m1).astype(np.int64) * 0x7FFF, np.minimum(M, diff))
            R = np.where(drop, comb, R)
            Cb = np.where(drop, B, Cb)
            Ch = np.where(drop, (m1 < m0).astype(np.int64), Ch)
        for i in range(n):
            c0 = c0_wave + i
            if M[i] == 0:
                out[c0] = -1
                if stats is not None:
                    stats["no_rescan"] = stats.get("no_rescan", 0) + 1
                    stats.setdefault("no_rescan_cols", set()).add(c0)
                continue
            B0 = Cb[i] + 4 * Ch[i]
            offs = np.array([(k & 3) + 8 * (k >> 2) for k in range(16)])
            cols1 = B0 + offs
            cols1 = cols1[cols1 < W]
            cand = cols1[ham_lo[c0, cols1] <= R[i]]
            eq = cand[ham[c0, cand] == R[i]]
            if stats is not None:
                stats["trips"] = max(stats.get("trips", 0), len(cand))
            out[c0] = eq.min() if len(eq) == 1 else -1
            assert len(eq) >= 1, "the recorded half holds the minimum"
    return out


def check(a, b, stats=None):
    lo, ham = distances(a, b)
    got = lazy_half_search(lo, ham, stats)
    ref = brute_force(ham)
    bad = np.nonzero(got != ref)[0]
    assert bad.size == 0, (bad[:8], got[bad[:8]], ref[bad[:8]])
    return ref


def _rand(rng, W):
    return rng.integers(0, 2 ** 32, size=(W, WORDS), dtype=np.uint64).astype(np.uint32) & MASK


WIDTHS = [33, 47, 64, 65, 96, 100, 127, 128, 129, 160, 191, 200, 255, 256, 257, 289, 300]


def test_rows_map_to_halves():
    for h in (0, 1):
        rows = sorted(rrow(r, h) for r in range(16))
        assert rows == [x for x in range(32) if half_of_row(x) == h]
        # the rescan's 16 rows from B0 = base + 4 h
        assert rows == [4 * h + (k & 3) + 8 * (k >> 2) for k in range(16)]
    assert sorted(rrow(r, h) for r in range(16) for h in (0, 1)) == list(range(32))


@pytest.mark.parametrize("W", WIDTHS)
def test_random_rows(W):
    rng = np.random.default_rng(W)
    ref = check(_rand(rng, W), _rand(rng, W))
    assert (ref >= 0).any()


@pytest.mark.parametrize("W", WIDTHS)
@pytest.mark.parametrize("bits", [1, 2, 4])
def test_low_entropy_rows(W, bits):
    """Few distinct descriptors: minima repeat within a half, across halves and across blocks."""
    rng = np.random.default_rng(1000 * bits + W)
    table = _rand(rng, 1 << bits)
    table[:, 2:] = table[0, 2:] ^ (table[:, 2:] & 0x3)      # ham_lo decides little, ham_hi too
    a = table[rng.integers(0, 1 << bits, W)]
    b = table[rng.integers(0, 1 << bits, W)]
    stats = {}
    ref = check(a, b, stats)
    assert (ref < 0).any() and stats.get("no_rescan", 0) > 0


@pytest.mark.parametrize("W", WIDTHS)
def test_shifted_rows_with_noise(W):
    """A stereo-like row: the match at col0 + 3 a few bits away, so the match's row sweeps
    all 32 rows of a block and both halves."""
    rng = np.random.default_rng(7 * W)
    a = _rand(rng, W)
    flips = _rand(rng, W) & _rand(rng, W) & _rand(rng, W) & _rand(rng, W)
    b = a[np.roll(np.arange(W), 3)] ^ flips
    ref = check(a, b)
    assert (ref[:W - 3] == np.arange(W - 3) + 3).mean() > 0.9


def _planted(W, seed):
    rng = np.random.default_rng(seed)
    a = _rand(rng, W)
    b = a[np.roll(np.arange(W), 3)].copy()
    return a, b


@pytest.mark.parametrize("W", [100, 200, 300])
@pytest.mark.parametrize("r1,r2,expect", [
    (0, 1, "invalid"), (8, 11, "invalid"),        # the same half of the final block
    (0, 4, "tie"), (3, 31, "tie"),                # the other half: a tie without a rescan
])
def test_planted_second_column_in_the_block(W, r1, r2, expect):
    a, b = _planted(W, 31 * W + r1)
    c0, B = 70, 32                                # col0 70, its block 32..63
    b[:] ^= np.uint32(0x0F0F0F0F) & MASK          # every column far away
    b[B + r1] = a[c0] ^ np.array([1, 0, 0, 0], np.uint32)
    b[B + r2] = a[c0] ^ np.array([0, 0, 2, 0], np.uint32)
    stats = {}
    ref = check(a, b, stats)
    assert ref[c0] == -1
    # equal halves on the drop => the tie marker, no rescan; the same half => the rescan counts
    assert (c0 in stats["no_rescan_cols"]) == (expect == "tie")
    assert (half_of_row(r1) != half_of_row(r2)) == (expect == "tie")


@pytest.mark.parametrize("W", [200, 300])
def test_other_half_duplicate_then_a_better_column_behind_the_wrap(W):
    a, b = _planted(W, 99 + W)
    b[:] ^= np.uint32(0x0F0F0F0F) & MASK
    c0 = 40
    b[3] = a[c0] ^ np.array([1, 0, 0, 0], np.uint32)       # rows 3 and 31 of block 0: distance 1
    b[31] = a[c0] ^ np.array([0, 0, 0, 1], np.uint32)
    better = W - 40                                        # visited after the wrap: distance 0
    b[better] = a[c0]
    ref = check(a, b)
    assert ref[c0] == better


@pytest.mark.parametrize("W", [200, 300])
def test_tie_in_a_later_block(W):
    a, b = _planted(W, 5 + W)
    b[:] ^= np.uint32(0x0F0F0F0F) & MASK
    c0 = 100
    b[101] = a[c0] ^ np.array([4, 0, 0, 0], np.uint32)
    b[20] = a[c0] ^ np.array([0, 0, 8, 0], np.uint32)
    assert check(a, b)[c0] == -1


@pytest.mark.parametrize("W", [100, 300])
def test_candidates_with_small_ham_lo(W):
    """ham_lo = 0, ham_hi = 62 beside the match, and ham_lo = hm, ham_hi = 0: the candidate
    loop takes several trips and keeps the one column."""
    a, b = _planted(W, 77 + W)
    b[:] ^= np.uint32(0x0F0F0F0F) & MASK
    c0 = 72
    hi62 = np.array([0, 0, 0xFFFFFFFF, 0x3FFFFFFF], np.uint32)
    b[64] = a[c0] ^ np.array([0, 3, 0, 0], np.uint32)       # the match: ham_lo = hm = 2
    b[65] = a[c0] ^ hi62                                    # ham_lo 0, distance 62
    b[66] = a[c0] ^ hi62 ^ np.array([1, 0, 0, 0], np.uint32)
    stats = {}
    ref = check(a, b, stats)
    assert ref[c0] == 64 and stats["trips"] >= 3


@pytest.mark.parametrize("W,row", [(44, 2), (44, 9), (108, 5), (300, 6)])
def test_partial_last_block(W, row):
    """The final block is the row's partial last block; the match in half 0 / half 1 of it."""
    a, b = _planted(W, 3 * W + row)
    b[:] ^= np.uint32(0x0F0F0F0F) & MASK
    B = W // 32 * 32
    assert B + row < W
    c0 = W // 2
    b[B + row] = a[c0] ^ np.array([0, 0, 1, 0], np.uint32)
    assert check(a, b)[c0] == B + row
    b[B + (row ^ 1)] = a[c0] ^ np.array([1, 0, 0, 0], np.uint32)    # the same half, twice
    assert check(a, b)[c0] == -1
