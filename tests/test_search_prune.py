"""The pruned second K-step of the 128-bit NoDuplicates search (search_mx.hip search_mx_kernel
PRUNE): per block of 32 col1 a tile pair multiplies descriptor bits 0..63 first, and bits
64..127 only if the lower bound x_lo - |a_hi| of some col0 comes within reach (<=) of that
col0's running minimum cost; a wave whose blocks nearly all reach falls back to the unpruned
loop for the rest of its row.

Every case is compared bit for bit with the CPU oracle (reference bicos.hpp:50-113), with the
unpruned loop of the same library (BICOS_MX_PRUNE=0) and with the pruned chunk loop
(BICOS_MX_STREAM=0, prune on); both switches are read once per process, so one child process
per setting computes every case. Widths: one chunk and less (64, 96, 1024: no streaming), the
chunk and stage boundaries with and without a partial last block, 2081 (tail launch behind
the main one) and four chunks. The descriptor kinds are chosen for where pruning can go wrong
(see search_case).
"""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests.test_search_stream import (  # noqa: E402
    MATCH_THRESHOLD, _random_pair, _ties_pair, gpu_match, gpu_search, match_case, same)

pytestmark = pytest.mark.gpu

WORDS = 4
NODUPES = 1
INVALID = -32768
ROWS = 3
WIDTHS = [64, 96, 1024, 1025, 1056, 1537, 2048, 2049, 2081, 3073]
KINDS = ["clean", "random", "half", "bound_ones", "bound_zeros", "ties", "planted", "lo_const",
         "hi_const"]
IDLE_WIDTHS = [1100, 2081]  # the row's last main workgroup: waves without col0, col0 past cols
WIDE = (176, 2081)          # enough workgroups for 4 tiles per wave + the tail launch
MATCH_WIDTHS = [1536, 2048, 2049, 3840]
HI62 = (np.uint32(0xFFFFFFFF), np.uint32(0x3FFFFFFF))  # descriptor bits 64..125


def _rand(rng, H, W, words=WORDS):
    return rng.integers(0, 2 ** 32, size=(H, W, words), dtype=np.uint64).astype(np.uint32)


def sites(W, H=ROWS):
    """(row, col0, first col1, second col1) of planted equal minima. The two col1 lie in
    different blocks always, in different stages from 1056 columns and in different chunks from
    1025 (rows 0 and 2: the first in the lower half of chunk 0; row 1: in its upper half); the
    fourth site of a row (W >= 1024) has both in one chunk, the second in a block visited
    after the first."""
    out = []
    for r in range(H):
        for i, c in enumerate((7, W // 2, W - 3)):
            out.append((r, c, (517 if r == 1 and W >= 1024 else 5) + 13 * i, W - 1 - 13 * i))
        if W >= 1024:
            out.append((r, 700, 690, 600))
    return out


def _clean_pair(H, W, seed):
    a = _rand(np.random.default_rng(seed), H, W)
    # right = left rolled by 3: col0's copy at col1 = col0 - 3, where the scan starts
    return a, np.ascontiguousarray(a[:, np.roll(np.arange(W), -3)])


def _half_pair(H, W, seed):
    # the left half of the right row a clean copy, its right half random: one scan runs the
    # pruned loop and the fallback
    a, b = _clean_pair(H, W, seed)
    b[:, W // 2:] = _rand(np.random.default_rng(seed + 1), H, W - W // 2)
    return a, b


def _bound_pair(H, W, seed, ones):
    """The bound x >= x_lo - |a_hi| attained. Left words 2, 3: bits 64..125 all ones (|a_hi| =
    62) or all zeros (|a_hi| = 0: partial = full); right words 2, 3 the complement (62 bits of
    cost) except at the planted col1, where they equal the left's: x_hi = -|a_hi| there. Words
    0, 1 random; each planted col1 carries the col0's with one bit flipped, so the cost 1 comes
    twice per site and the second ties the running minimum."""
    rng = np.random.default_rng(seed)
    a, b = _rand(rng, H, W), _rand(rng, H, W)
    for w in (2, 3):
        a[..., w] = HI62[w - 2] if ones else 0
        b[..., w] = 0 if ones else HI62[w - 2]
    for i, (r, c, p1, p2) in enumerate(sites(W, H)):
        for k, p in enumerate((p1, p2)):
            b[r, p] = a[r, c]
            b[r, p, k] ^= np.uint32(1 << (i % 5 + 9 * k))
    return a, b


def _planted_pair(H, W, seed):
    """Random descriptors with pairs of equal minima (cost 1 twice). One of the two col1 has
    its flipped bit in the high 64 bits, so its low 64 bits equal the col0's: its partial cost
    is 0 and its whole cost sits in the second K-step (the second col1 at even sites, the first
    at odd ones)."""
    rng = np.random.default_rng(seed)
    a, b = _rand(rng, H, W), _rand(rng, H, W)
    for i, (r, c, p1, p2) in enumerate(sites(W, H)):
        lo, hi = (p1, p2) if i % 2 == 0 else (p2, p1)
        b[r, lo] = a[r, c]
        b[r, lo, 0] ^= np.uint32(1 << (i % 3))
        b[r, hi] = a[r, c]
        b[r, hi, 3] ^= np.uint32(1 << (7 + i % 3))
    return a, b


def _const_pair(H, W, seed, words):
    # a shifted copy with 1 bit in 16 flipped, `words` of both sides constant over the row
    a, b = _random_pair(H, W, seed)
    for w in words:
        a[..., w] = b[..., w] = np.uint32(0x5A5A3C0F + w)
    return a, b


def search_case(kind, W, H=ROWS):
    seed = 9000 + W
    if kind == "clean":        # nearly every block is pruned
        return _clean_pair(H, W, seed)
    if kind == "random":       # every block reaches: the fallback
        rng = np.random.default_rng(seed + 1)
        return _rand(rng, H, W), _rand(rng, H, W)
    if kind == "half":
        return _half_pair(H, W, seed + 2)
    if kind == "bound_ones":
        return _bound_pair(H, W, seed + 3, True)
    if kind == "bound_zeros":
        return _bound_pair(H, W, seed + 4, False)
    if kind == "ties":         # few distinct descriptors: most minima repeated
        return _ties_pair(H, W, seed + 5)
    if kind == "planted":
        return _planted_pair(H, W, seed + 6)
    if kind == "lo_const":     # partial cost 0 everywhere: never prunes
        return _const_pair(H, W, seed + 7, (0, 1))
    if kind == "hi_const":     # all information in K-step 0
        return _const_pair(H, W, seed + 8, (2, 3))
    raise ValueError(kind)


def search_cases():
    cases = [(k, W, ROWS) for W in WIDTHS for k in KINDS]
    cases += [(k, W, ROWS) for W in IDLE_WIDTHS for k in ("clean", "random") if W not in WIDTHS]
    cases += [(k, WIDE[1], WIDE[0]) for k in ("clean", "random", "half", "planted")]
    return cases


def run_all(eng):
    """Every case's maps, keyed by name: what a child process computes under its switches."""
    out = {}
    for kind, W, H in search_cases():
        out["search_%s_%d_%d" % (kind, W, H)] = gpu_search(eng, *search_case(kind, W, H))
    for W in MATCH_WIDTHS:
        d, c = gpu_match(eng, *match_case(W))
        out["match_d_%d" % W] = d
        out["match_c_%d" % W] = c
    return out


def _child(tmp_path_factory, name, **switches):
    path = str(tmp_path_factory.mktemp("mx_prune") / (name + ".npz"))
    env = dict(os.environ, **switches)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", path], env=env,
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def others(gpu, tmp_path_factory):
    """The same inputs through the unpruned loop and through the pruned chunk loop."""
    return (_child(tmp_path_factory, "unpruned", BICOS_MX_PRUNE="0"),
            _child(tmp_path_factory, "pruned_chunk_loop", BICOS_MX_STREAM="0"))


def _check_search(gpu, oracle, others, kind, W, H=ROWS):
    a, b = search_case(kind, W, H)
    ref = oracle.search(a, b, NODUPES)
    if kind in ("bound_ones", "bound_zeros", "planted"):
        for r, c, p1, p2 in sites(W, H):  # the same minimum twice: invalid
            assert ref[r, c] == INVALID, (r, c, p1, p2, ref[r, c])
    if kind == "clean":
        assert (ref[:, 3:] == 3).all()
    got = gpu_search(gpu, a, b)
    same(got, ref)
    for o in others:
        same(got, o["search_%s_%d_%d" % (kind, W, H)])


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("W", WIDTHS)
def test_pruned_search_equals_oracle_and_unpruned(gpu, oracle, others, W, kind):
    _check_search(gpu, oracle, others, kind, W)


@pytest.mark.parametrize("kind", ["clean", "random"])
@pytest.mark.parametrize("W", IDLE_WIDTHS)
def test_pruned_search_idle_waves(gpu, oracle, others, W, kind):
    """Waves without col0 and left columns past the image in the row's last workgroup."""
    _check_search(gpu, oracle, others, kind, W)


@pytest.mark.parametrize("kind", ["clean", "random", "half", "planted"])
def test_pruned_search_four_tiles_per_wave(gpu, oracle, others, kind):
    """Enough rows for the full frames' shape (4 tiles = 2 pairs per wave), the last 33 columns
    in the (unpruned) tail launch."""
    _check_search(gpu, oracle, others, kind, WIDE[1], WIDE[0])


@pytest.mark.parametrize("W", MATCH_WIDTHS)
def test_pruned_fused_match_equals_oracle(gpu, oracle, others, W):
    from libbicos_amd import _lib
    L, R = match_case(W)
    d, c = gpu_match(gpu, L, R, _lib.PLAN_AGREE_IN_SEARCH)  # (asserts the fused plan)
    rd, rc = oracle.match(L, R, oracle.OracleConfig(nxcorr_threshold=MATCH_THRESHOLD))
    same(d, rd)
    same(c, rc)
    for o in others:
        same(d, o["match_d_%d" % W])
        same(c, o["match_c_%d" % W])


if __name__ == "__main__":
    # child of the `others` fixture: every case through this process's library switches
    assert sys.argv[1] == "--child"
    assert os.environ.get("BICOS_MX_PRUNE") == "0" or os.environ.get("BICOS_MX_STREAM") == "0"
    from libbicos_amd import device
    np.savez(sys.argv[2], **run_all(device.Engine(0)))
