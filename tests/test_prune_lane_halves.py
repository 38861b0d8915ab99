"""The pruned search's per-block reach test seen from the lane halves (search_mx.hip block_pr):
each lane half holds 16 rows of a block for both tiles of a pair, the two block minima are
brought to the tiles' home halves and compared with a per-pair threshold that is renewed after
every reaching block. What any form of that test can get wrong is WHICH lane half, or which tile
of a pair, sees a reaching key, and which tile's minimum and |a_hi| a renewed threshold is built
from -- so these scenes place every reach by hand. (Written with the variant that keeps both
tiles' thresholds in every lane and drops the exchange; it measured slower and is not the one
built, DESIGN.md s9. The scenes hold for the exchange as well, and for the block loop's order:
the wrapping block index and the fallback's windows.)

The descriptors are crafted so that pruning stays active and every reach is a known one. The
right row holds every left descriptor at col1 = col0 - 3 (wrapping) with 6 bits flipped, 3 of
them in bits 0..63: each col0 finds its minimum, cost 6, in the first blocks of its scan, and
every other col1 is random (partial cost about 32: far from reach). A site then plants, for one
col0, ONE col1 far away that comes within reach: the col0's descriptor with `lo` bits flipped
in bits 0..63 and `hi` in bits 64..127. A plant of cost 6 ties the minimum (NoDuplicates:
invalid) and one of cost 5 replaces it, so a block skipped by mistake changes the result.
Accumulator register r of lane l holds col1 = B + (r & 3) + 8 (r >> 2) + 4 (l >> 5): a plant in
an even 4-row group of its block is seen by lanes 0-31 only, one in an odd group by lanes 32-63.

Every case is compared bit for bit with the CPU oracle and with the unpruned loop of the same
library (BICOS_MX_PRUNE=0, read once per process: one child process computes them all).
"""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests.test_search_stream import gpu_search, same  # noqa: E402
from tests.test_search_prune import HI62, WIDE  # noqa: E402

pytestmark = pytest.mark.gpu

NODUPES = 1
INVALID = -32768
ROWS = 3
WIDTHS = [64, 128, 1056, 2081]  # 2 tiles per wave; 1056, 2081: streamed stages, 2081: + tail
PARTIAL_W = 1056 + 7            # the last block holds 7 columns
HI_KINDS = ["random", "extreme"]
TIE, NEW = (6, 0), (2, 3)       # (lo, hi) flips: cost 6 with partial cost 6 = the threshold
                                # exactly; cost 5


def _noise(c):
    """6 bits of column c's copy: 3 in words 0, 1 and 3 in bits 64..125."""
    n = np.zeros(4, np.uint32)
    n[0] = 1 << (c % 32)
    n[1] = (1 << (c * 7 % 32)) | (1 << ((c * 7 + 13) % 32))
    n[2] = 1 << (c % 32)
    n[3] = (1 << (c * 5 % 30)) | (1 << ((c * 5 + 11) % 30))
    return n


def base_pair(H, W, seed, hi_kind):
    """Left descriptors random -- hi_kind "extreme": words 2, 3 all ones over bits 64..125
    (|a_hi| = 62) or all zeros (|a_hi| = 0) over alternating runs of 32 columns, so the two
    tiles of every pair stand at the two ends, in either order by the row's parity. Right: the
    copy of col0 at col1 = col0 - 3 (wrapping), 6 bits flipped."""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 2 ** 32, size=(H, W, 4), dtype=np.uint64).astype(np.uint32)
    if hi_kind == "extreme":
        ones = ((np.arange(W)[None, :] // 32 + np.arange(H)[:, None]) % 2 == 0)
        for w in (2, 3):
            a[..., w] = np.where(ones, HI62[w - 2], np.uint32(0))
    noise = np.stack([_noise(c) for c in range(W)])
    b = np.empty_like(a)
    b[:, (np.arange(W) - 3) % W] = a ^ noise[(np.arange(W) - 3) % W][None]
    return a, b


def plant(a, b, sites):
    """sites: (row, col0, [(col1, lo, hi), ...]). b[row, col1] becomes a[row, col0] with `lo`
    bits of word 0 and `hi` bits of word 2 flipped; the col0 whose copy stood there (col1 + 3)
    gets a new descriptor, 6 bits from the planted one, so that it keeps a minimum nearby and
    its wave keeps pruning."""
    W = a.shape[1]
    used = {}
    for r, c, plants in sites:
        cols = [c, (c - 3) % W] + [p for p, _, _ in plants] + [(p + 3) % W for p, _, _ in plants]
        for x in cols:
            assert (r, x) not in used, (r, c, x, used[(r, x)])
            used[(r, x)] = c
    for i, (r, c, plants) in enumerate(sites):
        for k, (p, lo, hi) in enumerate(plants):
            d = a[r, c].copy()
            for n in range(lo):
                d[0] ^= np.uint32(1 << ((5 * i + 3 * k + n) % 32))
            for n in range(hi):
                d[2] ^= np.uint32(1 << ((7 * i + k + n) % 32))
            b[r, p] = d
            a[r, (p + 3) % W] = d ^ _noise(p)


def row_in_group(g, i):
    """A row of a block in an even (g = 0: lanes 0-31) or odd (g = 1) 4-row group."""
    return 8 * (i % 4) + 4 * g + i % 3


def lane_sites(W, rows, G):
    """Tile of the pair x lane half of the planted row x tie / new minimum: 8 sites, in waves
    spread over the row (G col0 per wave), the plant 3 + i blocks below the col0's own."""
    out = []
    nbf = W // 32
    for i in range(8):
        u, g, kind = i & 1, (i >> 1) & 1, (i >> 2) & 1
        wb = (5 * i + 1) * G % (W // G * G)
        c = wb + 64 * (i % (G // 64)) + 32 * u + (7 * i + 3) % 32
        p = 32 * ((c // 32 - 3 - i) % nbf) + row_in_group(g, i)
        out.append((rows[i % len(rows)], c, [(p,) + (TIE if kind == 0 else NEW)]))
    return out


def pair_sites(W, rows, G):
    """Both tiles of a pair reach in the same block (one plant per lane half), and the
    renewal: tile A takes a new minimum in block k, then tile B of the same pair -- the same
    lane of the other tile -- has a tie at exactly its old threshold in block k - 1, the next
    one visited. Both ways round."""
    out = []
    wb = (W // 2) // G * G  # a wave in the middle of the row; its blocks k, k - 1 share a stage
    k = wb // 32 - 4 if wb >= 256 else wb // 32 - 1
    if k < 1:
        return out
    r0, r1, r2 = rows[0], rows[1 % len(rows)], rows[2 % len(rows)]
    out.append((r0, wb + 5, [(32 * k + 2, *NEW)]))          # tile A, lanes 0-31
    out.append((r0, wb + 32 + 20, [(32 * k + 21, *TIE)]))   # tile B, lanes 32-63: same block
    out.append((r1, wb + 9, [(32 * k + 9, *NEW)]))          # A lowers its minimum in block k
    out.append((r1, wb + 32 + 9, [(32 * (k - 1) + 14, *TIE)]))  # B ties in block k - 1
    out.append((r2, wb + 32 + 17, [(32 * k + 30, *NEW)]))   # B lowers
    out.append((r2, wb + 17, [(32 * (k - 1) + 1, *TIE)]))   # A ties
    return out


def partial_sites():
    """1063 columns: the wave of col0 1024.. visits the partial block 1056..1062 first. The
    first col0 of a tile takes a new minimum there (cost 5), which a plant far away ties at
    partial cost 5 = the threshold renewed after the partial block."""
    return [(0, 1024, [(1058, *NEW), (700, 5, 0)]),
            (1, 1056, [(1061, *NEW), (300, 5, 0)]),
            (2, 1024, [(1057, 1, 3)])]


def cases():
    out = []
    for hk in HI_KINDS:
        for W in WIDTHS:
            out.append(("w%d_%s" % (W, hk), ROWS, W, hk))
        out.append(("partial_%s" % hk, ROWS, PARTIAL_W, hk))
        out.append(("wide_%s" % hk, WIDE[0], WIDE[1], hk))
    return out


def build_case(name, H, W, hk):
    """(left, right, sites) -- `wide`: 4 tiles per wave (two pairs of 64 col0 per wave)."""
    G = 128 if name.startswith("wide") else 64
    rows = [0, 1, 2] if H == ROWS else [0, H // 2, H - 1]
    a, b = base_pair(H, W, 4242 + W + (H if H != ROWS else 0), hk)
    if name.startswith("partial"):
        sites = partial_sites()
    else:
        sites = pair_sites(W, rows, G)
        taken = {(r, c) for r, c, _ in sites}
        shifted = [rows[1 % len(rows)], rows[2 % len(rows)], rows[0]]
        sites += [s for s in lane_sites(W, shifted if sites else rows, G) if (s[0], s[1]) not in taken]
    plant(a, b, sites)
    return a, b, sites


def expected(sites):
    """The disparity (col0 - col1) the sites must show: a tie is invalid, the lowest plant wins."""
    out = []
    for r, c, plants in sites:
        costs = sorted((lo + hi, p) for p, lo, hi in plants) + [(6, c - 3)]
        costs.sort()
        tie = costs[0][0] == costs[1][0]
        out.append((r, c, INVALID if tie else c - costs[0][1]))
    return out


def run_all(eng):
    out = {}
    for name, H, W, hk in cases():
        a, b, _ = build_case(name, H, W, hk)
        out[name] = gpu_search(eng, a, b)
    return out


@pytest.fixture(scope="module")
def unpruned(gpu, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("mx_halves") / "unpruned.npz")
    env = dict(os.environ, BICOS_MX_PRUNE="0")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", path], env=env,
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("name,H,W,hk", cases(), ids=[c[0] for c in cases()])
def test_lane_halves_equal_oracle_and_unpruned(gpu, oracle, unpruned, name, H, W, hk):
    a, b, sites = build_case(name, H, W, hk)
    ref = oracle.search(a, b, NODUPES)
    for r, c, want in expected(sites):  # the scene is what it was built to be
        assert ref[r, c] == want, (name, r, c, want, ref[r, c])
    got = gpu_search(gpu, a, b)
    same(got, ref)
    same(got, unpruned[name])


if __name__ == "__main__":
    # child of the `unpruned` fixture: every case through this process's library switch
    assert sys.argv[1] == "--child" and os.environ.get("BICOS_MX_PRUNE") == "0"
    from libbicos_amd import device
    np.savez(sys.argv[2], **run_all(device.Engine(0)))
