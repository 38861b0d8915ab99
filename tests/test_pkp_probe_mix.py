"""Which 32 bits the packed pruned search's one-product probe tests (search_pk.hip pkp_mix,
search_plan.hpp pkp_dword_word): the kernel's four matrix products partition the 128 descriptor
bits into groups of 32; products 0 and 1 take words 0 and 1 by alternate dwords of their FP4
expansion (16 bits of each word), products 2 and 3 are words 2 and 3. A block of 32 col1 is
probed with product 0 alone (ham'_0), a wave that falls back with products 0 and 1, which are
words 0 and 1 whole, so BICOS_PKP_PROBE=2 tests what it always did. The map is asked of the
library (bicos_search_packed_product); nothing here restates it except the model that checks it.

CPU (numpy, no GPU):
  the query       every product holds 32 bits; products 2 and 3 are words 2 and 3; products 0
                  and 1 together are bits 0-63 with 16 bits of each of words 0 and 1
  the model       expand_bits (the v_perm byte table) and the dword selection as the kernel makes
                  it, on one-hot descriptors, give the same map, the same K position in both
                  operands; tools/prune_sim.py --mix 2 simulates the same map
  the distances   the four products of the FP4 operands of random descriptors give the popcount
                  distances over the query's bits, their sum the popcount distance, products 0
                  and 1 the distance over words 0 and 1
  the edge kind   is what it says (below), checked with a model of the wave's scan

GPU: one child process per switch setting computes every case of its shapes; every case asserts
through bicos_search_packed that the packed pruned form runs and is compared byte for byte with
the CPU oracle and with the BICOS_PKP_PROBE=2 child.
Shapes, 256 rows (the fewest the packed plan takes): 1057 columns (a partial block, and a second
chunk with one full block), 2016 (a stage of 480 columns), and 1088 with BICOS_MX_STREAM=0 (the
chunk loop, which shares put_col).
Kinds: stereo, random (every wave falls back) and tie of tests/test_search_packed_prune.py, and
  edge   every left descriptor matches right column col0 - 3 within one bit, so every other block
         is pruned at depth 1. For planted col0 in both wide tiles and both lane halves of a
         wave, the left descriptor equals right column c1 but for k bits that all lie in
         products 1-3 (ham'_0 = 0, ham = k); a second column c2, in a block visited later,
         differs in k bits that all lie in product 0: its probe distance EQUALS the running
         minimum, it must reach -- a tie, invalid -- or in k + 1 such bits: pruned, the result is
         c1. k = 0, 1, 31, 32 by row (32: all of product 0; one more bit cannot lie in product 0,
         so the second outcome there is 32 bits of product 0 and one of another product -- it
         reaches and loses). Where k + 1 >= 32 the other columns of c2's block are planted too
         (k + 1 bits of product 0), or the planted col0 would reach that block through them. c1
         and c2 lie on either side of a stage or chunk boundary, of the first block boundary, or
         in the row's first and last column.
  edge2  the same once at depth 2 (1057 columns): k bits of products 2-3 against k or k + 1 bits
         of products 0-1
"""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests.test_pkp_block_loop import CHUNK, column_pairs, visit_order  # noqa: E402
from tests.test_search_packed_prune import (BITS, INVALID, MASK, NODUPES, WORDS, _rand,  # noqa: E402
                                            gpu_search, search_case, tie_sites)
from tests.test_search_stream import same  # noqa: E402

SHAPES = [(256, 1057, True), (256, 2016, True), (256, 1088, False)]     # (rows, columns, streamed)
KINDS = ["stereo", "random", "tie", "edge"]
EDGE2 = (256, 1057, True)
KS = (0, 1, 31, 32)
LANE_OFFSETS = (5, 40, 77, 110)     # col0 of a wave: tile 0 P / Q lanes, tile 1 P / Q lanes
PRUNE_WINDOW = 8                    # search_plan.hpp
INF = 0x7BFF - 0x4B00               # the running minimum's start, PK_PAD, as a distance
LUT_PA = 0xAAA22A22                 # search_pk.hip: right, bit 0 -> +1.0 (0x2), 1 -> -1.0 (0xA)
LUT_PB = 0x11199199                 # left, bit 0 -> -0.5 (0x9), 1 -> +0.5 (0x1)
FP4 = {0x2: 1.0, 0xA: -1.0, 0x9: -0.5, 0x1: 0.5}


# ---- the query ---------------------------------------------------------------------------------

_PRODUCT = []


def products():
    """[128] the product of every descriptor bit, from the library"""
    if not _PRODUCT:
        from libbicos_amd import _lib
        if not os.path.exists(_lib.LIB_PATH):
            _lib.build()
        L = _lib.lib()
        _PRODUCT.append(np.array([L.bicos_search_packed_product(b) for b in range(128)]))
    return _PRODUCT[0]


def product_mask(prods):
    """the 4-word mask of the bits the given products hold"""
    x = np.zeros(WORDS, np.uint32)
    for b in np.flatnonzero(np.isin(products(), prods)):
        x[b // 32] |= np.uint32(1) << np.uint32(b % 32)
    return x


def test_query_partitions_the_bits(blib):
    P = products()
    assert blib.bicos_search_packed_product(-1) == -1 and blib.bicos_search_packed_product(128) == -1
    assert [int((P == k).sum()) for k in range(4)] == [32, 32, 32, 32]
    assert (P[64:96] == 2).all() and (P[96:] == 3).all()
    assert set(P[:64]) == {0, 1}
    for w in (0, 1):
        assert (P[32 * w:32 * w + 32] == 0).sum() == 16 and (P[32 * w:32 * w + 32] == 1).sum() == 16


# ---- the model: expand_bits and the dword selection ------------------------------------------

def expand_bits(x, lut):
    """search_mx_common.hpp expand_bits: dword m = v_perm of the byte table by the bit pairs
    (x >> 2m) & 3 of every byte of x"""
    out = []
    for m in range(4):
        sel = (x >> (2 * m)) & 0x03030303
        out.append(sum(((lut >> (8 * ((sel >> (8 * q)) & 0xFF))) & 0xFF) << (8 * q) for q in range(4)))
    return out


def operands(desc, lut):
    """[4 products][4 dwords] of one descriptor (4 words): product 0 = {E(w0)[0], E(w1)[1],
    E(w0)[2], E(w1)[3]}, product 1 = {E(w1)[0], E(w0)[1], E(w1)[2], E(w0)[3]}, products 2 and 3
    the expansions of words 2 and 3"""
    E = [expand_bits(int(w), lut) for w in desc]
    return [[E[0][0], E[1][1], E[0][2], E[1][3]], [E[1][0], E[0][1], E[1][2], E[0][3]], E[2], E[3]]


def nibbles(op):
    """[4 dwords] -> the 32 FP4 codes along K"""
    return [(d >> (4 * i)) & 0xF for d in op for i in range(8)]


def test_model_of_expansion_and_selection_gives_the_querys_map():
    P = products()
    zero = {lut: operands([0, 0, 0, 0], lut) for lut in (LUT_PA, LUT_PB)}
    for b in range(128):
        desc = [0, 0, 0, 0]
        desc[b // 32] = 1 << (b % 32)
        where = []
        for lut in (LUT_PA, LUT_PB):
            ops = operands(desc, lut)
            diff = [(k, i) for k in range(4) for i, (x, y) in
                    enumerate(zip(nibbles(ops[k]), nibbles(zero[lut][k]))) if x != y]
            assert len(diff) == 1, (b, diff)       # one K position of one product
            where.append(diff[0])
        assert where[0] == where[1]                 # the same one in both operands
        assert where[0][0] == P[b], (b, where, P[b])


def test_prune_sim_mix_2_is_the_querys_map():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import prune_sim
    assert [prune_sim.mix_product(b, 2) for b in range(128)] == list(products())
    assert [prune_sim.mix_product(b, 1) for b in range(128)] == [b // 32 for b in range(128)]
    for K in (3, 4):
        assert sorted(prune_sim.mix_order(K)) == list(range(128))
        assert [sum(prune_sim.mix_product(b, K) == k for b in range(128)) for k in range(4)] == [32] * 4


def pop(x):
    return int(np.unpackbits(np.ascontiguousarray(x).view(np.uint8)).sum())


def test_products_sum_to_the_popcount_distance():
    rng = np.random.default_rng(17)
    masks = [product_mask([k]) for k in range(4)]
    for _ in range(200):
        a, b = _rand(rng, WORDS) & MASK, _rand(rng, WORDS) & MASK
        if rng.random() < 0.2:
            b = a ^ (_rand(rng, WORDS) & _rand(rng, WORDS) & _rand(rng, WORDS) & MASK)
        A, B = operands(b, LUT_PA), operands(a, LUT_PB)     # right, left
        # K positions sum to ham - K / 2 (search_pk.hip mfma_pk)
        hams = [sum(FP4[x] * FP4[y] for x, y in zip(nibbles(A[k]), nibbles(B[k]))) + 16 for k in range(4)]
        assert hams == [pop((a ^ b) & masks[k]) for k in range(4)]
        assert sum(hams) == pop(a ^ b)
        assert hams[0] + hams[1] == pop((a ^ b)[:2])


# ---- the edge kinds ------------------------------------------------------------------------------

def chunk_order(W, c):
    """Block bases in the order the wave of col0 c visits them in the chunk loop
    (BICOS_MX_STREAM=0): chunks downwards from the workgroup's, wrapping; in every chunk the
    partial block first, then the full blocks downwards from the one holding the wave's highest
    col0 (clamped), wrapping."""
    tile, c0_wave = c // CHUNK, c // 128 * 128
    nchunks = (W + CHUNK - 1) // CHUNK
    cstart = min(W - 1, (tile + 1) * CHUNK - 1) // CHUNK
    order = []
    for k in range(nchunks):
        base = (cstart - k) % nchunks * CHUNK
        ncols = min(CHUNK, W - base)
        nfull = ncols // 32
        if ncols & 31:
            order.append(base + 32 * nfull)
        sb0 = max(0, min(nfull - 1, (min(W - 1, c0_wave + 127) - base) // 32))
        order += [base + 32 * ((sb0 - i) % nfull) for i in range(nfull)]
    assert sorted(order) == list(range(0, W, 32))
    return order


def order_of(W, c, streamed):
    return visit_order(W, c) if streamed else chunk_order(W, c)


def _flip(rng, k, prods):
    """A 4-word mask of k distinct used bits of the given products"""
    pool = np.array([b for b in np.flatnonzero(np.isin(products(), prods)) if b < BITS])
    x = np.zeros(WORDS, np.uint32)
    for p in rng.choice(pool, size=k, replace=False):
        x[p // 32] |= np.uint32(1) << np.uint32(p % 32)
    return x


def _matched_pair(H, W, seed):
    """Random 126-bit descriptors; left column c equals right column c - 3 but for at most one
    bit: once a col0 has met its match its running minimum is <= 1, and no random column comes
    that close in 32 bits."""
    rng = np.random.default_rng(seed)
    a = _rand(rng, (H, W, WORDS)) & MASK
    b = a[:, np.roll(np.arange(W), -3)].copy()
    bit = rng.integers(0, BITS, size=(H, W))
    on = rng.random((H, W)) < 0.5
    for w in range(WORDS):
        b[:, :, w] ^= np.where(on & (bit // 32 == w), np.uint32(1) << (bit % 32).astype(np.uint32),
                               np.uint32(0)).astype(np.uint32)
    return a, b


_EDGE = {}


def edge_case(H, W, streamed, depth=1):
    """(left, right, sites): sites = [(row, col0, c1, c2, k, tie, expected disparity)]. depth: the
    probe the boundary is planted for -- product 0 against products 1-3, or (2) products 0-1
    against products 2-3."""
    key = (H, W, streamed, depth)
    if key not in _EDGE:
        probe, rest = ((0,), (1, 2, 3)) if depth == 1 else ((0, 1), (2, 3))
        nprobe = int(np.isin(products()[:BITS], probe).sum())
        a, b = _matched_pair(H, W, 17000 + W + depth)
        rng = np.random.default_rng(17500 + W + depth)
        pairs = column_pairs(W)
        # (waves whose col0 lose their matches to the planted columns reach in every block:
        # the planted col0 live in the others)
        waves = [w for w in range((W - 4) // 128) if w % 4 in (1, 2)]
        sites = []
        for r in range(H):
            k, tie = KS[r % 4], (r // 4) % 2 == 0
            fill = not tie and 32 <= k + 1 <= nprobe    # c2's whole block is planted (below)
            # (the row's first and last column share block 0 with the first block boundary)
            prs = [p for p in pairs if p != (0, W - 1)] if fill else pairs
            for i in range(min(4, len(prs))):
                c = 128 * waves[(r + i) % len(waves)] + LANE_OFFSETS[(i + r // 8) % 4]
                p, q = prs[(r // 32 + i) % len(prs)]
                order = order_of(W, c, streamed)
                rank = lambda x: order.index(x // 32 * 32)  # noqa: E731
                assert rank(p) != rank(q)
                c1, c2 = (p, q) if rank(p) < rank(q) else (q, p)
                b[r, c - 3] = ~a[r, c] & MASK
                b[r, c1] = a[r, c] ^ _flip(rng, k, rest)
                if tie:
                    b[r, c2] = a[r, c] ^ _flip(rng, k, probe)
                elif k + 1 <= nprobe:       # pruned
                    if fill:                # ... if the block's other columns do not reach either
                        for x in range(c2 // 32 * 32, min(W, c2 // 32 * 32 + 32)):
                            b[r, x] = a[r, c] ^ _flip(rng, k + 1, probe) ^ _flip(rng, 8, rest)
                    b[r, c2] = a[r, c] ^ _flip(rng, k + 1, probe)
                else:                       # the probe's bits all differ: it reaches, and loses
                    b[r, c2] = a[r, c] ^ _flip(rng, k, probe) ^ _flip(rng, 1, rest)
                sites.append((r, c, c1, c2, k, tie, INVALID if tie else c - c1))
        _EDGE[key] = (a, b, sites)
    a, b, sites = _EDGE[key]
    return a.copy(), b.copy(), sites


POP8 = np.array([bin(i).count("1") for i in range(256)], np.int32)


def ham(a, b, mask):
    """[n, 4] x [W, 4] uint32 -> [n, W] Hamming distances over the mask's bits"""
    x = ((a[:, None, :] ^ b[None, :, :]) & mask).copy().view(np.uint8)
    return POP8[x].sum(axis=-1)


def scan_until(a, b, W, c, order, depth0, stop):
    """A model of the scan of col0 c's wave (search_pk.hip block_pr and the window rule) over one
    row, up to the probe of the block at col1 `stop`: -> (probe depth there, does c's wide tile
    reach, does it reach through another col0 than c, c's running minimum there)"""
    c0 = c // 128 * 128
    full = np.array([0xFFFFFFFF] * WORDS, np.uint32)
    Hp = {1: ham(a[c0:c0 + 128], b, product_mask([0])), 2: ham(a[c0:c0 + 128], b, product_mask([0, 1]))}
    Hf = ham(a[c0:c0 + 128], b, full)
    R = np.full(128, INF)
    depth, wb, wr = depth0, 0, 0
    for B in order:
        e = min(W, B + 32)
        d = depth if e - B == 32 else 0      # the partial last block never prunes
        reach = [True, True]
        if d:
            lb = Hp[d][:, B:e].min(axis=1) <= R
            if B == stop:
                t = (c - c0) // 64
                others = lb[64 * t:64 * t + 64].copy()
                others[c - c0 - 64 * t] = False
                return d, bool(lb[64 * t:64 * t + 64].any()), bool(others.any()), int(R[c - c0])
            reach = [bool(lb[:64].any()), bool(lb[64:].any())]
        for t in (0, 1):
            if reach[t]:
                s = slice(64 * t, 64 * t + 64)
                R[s] = np.minimum(R[s], Hf[s, B:e].min(axis=1))
        if d:
            wb += 1
            wr += sum(reach)
            if wb == PRUNE_WINDOW:
                if 8 * wr >= 7 * PRUNE_WINDOW * 2:
                    depth = 2 if depth == 1 else 0
                wb = wr = 0
    raise AssertionError("block %d not probed" % stop)


@pytest.mark.parametrize("H,W,streamed,depth", [s + (1,) for s in SHAPES] + [EDGE2 + (2,)])
def test_edge_case_is_what_it_says(blib, H, W, streamed, depth):
    """The planted distances over the probe's bits and over all bits, every k with both outcomes
    at all four lane positions, no two sites of a row on one column; and by the model of the
    wave's scan, for the sites of the first 16 rows: c2's block is probed at the planted depth
    with the running minimum k, a tie reaches through the planted col0 alone, and k + 1 bits
    are pruned."""
    a, b, sites = edge_case(H, W, streamed, depth)
    probe = product_mask([0] if depth == 1 else [0, 1])
    nprobe = pop(probe & MASK)
    assert nprobe == 32 * depth
    seen, cols = set(), set()
    for r, c, c1, c2, k, tie, want in sites:
        d = a[r, c] ^ b[r]
        assert pop(d[c - 3]) > 100
        assert (pop(d[c1]), pop(d[c1] & probe)) == (k, 0)
        if tie:
            assert (pop(d[c2]), pop(d[c2] & probe)) == (k, k) and want == INVALID
        elif k + 1 <= nprobe:
            assert (pop(d[c2]), pop(d[c2] & probe)) == (k + 1, k + 1) and want == c - c1
        else:
            assert (pop(d[c2]), pop(d[c2] & probe)) == (k + 1, k) and want == c - c1
        seen.add((k, tie, (c % 128) // 32))
        for x in (c - 3, c1, c2):
            assert (r, x) not in cols
            cols.add((r, x))
        if r < 16 and c2 // 32 * 32 + 32 <= W:     # (the partial last block is never probed)
            at, reaches, others, run = scan_until(a[r], b[r], W, c, order_of(W, c, streamed), depth,
                                                  c2 // 32 * 32)
            assert at == depth and run == k and not others, (r, c, at, run, others)
            assert reaches == (tie or k + 1 > nprobe), (r, c, k, tie)
    assert len(seen) == len(KS) * 2 * 4


# ---- GPU ---------------------------------------------------------------------------------------

def case(kind, H, W, streamed):
    """(left, right, stated bits)"""
    if kind in ("edge", "edge2"):
        return edge_case(H, W, streamed, 1 if kind == "edge" else 2)[:2] + (BITS,)
    return search_case(kind, H, W)


def cases(streamed):
    out = [(H, W, kind) for H, W, s in SHAPES if s == streamed for kind in KINDS]
    return out + [EDGE2[:2] + ("edge2",)] if streamed == EDGE2[2] else out


def run_all(eng, streamed):
    out = {}
    for H, W, kind in cases(streamed):
        a, b, bits = case(kind, H, W, streamed)
        assert eng.search_packed(H, W, WORDS, bits)
        out["%s_%d" % (kind, W)] = gpu_search(eng, a, b, bits)
    return out


@pytest.fixture(scope="module")
def children(gpu, tmp_path_factory):
    """{(streamed, start depth): results}: the two-product probe on the streamed shapes, and the
    chunk loop at both start depths; one child process each, side by side."""
    d = tmp_path_factory.mktemp("pkp_probe_mix")
    runs = {}
    for streamed, depth in ((True, 2), (False, 1), (False, 2)):
        env = dict(os.environ, BICOS_PKP_PROBE=str(depth))
        if not streamed:
            env["BICOS_MX_STREAM"] = "0"
        path = str(d / ("s%d_d%d.npz" % (streamed, depth)))
        runs[streamed, depth] = (path, subprocess.Popen(
            [sys.executable, os.path.abspath(__file__), "--child", path], env=env, cwd=ROOT,
            stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    out = {}
    for key, (path, p) in runs.items():
        log = p.communicate(timeout=600)[0]
        assert p.returncode == 0, log[-4000:]
        with np.load(path) as z:
            out[key] = {k: z[k] for k in z.files}
    return out


def _check(gpu, oracle, children, H, W, streamed, kind):
    a, b, bits = case(kind, H, W, streamed)
    assert gpu.search_packed(H, W, WORDS, bits)
    ref = oracle.search(a, b, NODUPES)
    if kind == "tie":       # the same minimum twice: invalid (valid if the reach test were "<")
        for c, p2 in tie_sites(W):
            assert (ref[:, c] == INVALID).all(), (c, p2, ref[0, c])
    if kind in ("edge", "edge2"):
        for r, c, c1, c2, k, tie, want in edge_case(H, W, streamed, 1 if kind == "edge" else 2)[2]:
            assert ref[r, c] == want, (r, c, c1, c2, k, tie, want, ref[r, c])
    name = "%s_%d" % (kind, W)
    here = gpu_search(gpu, a, b, bits)      # this process: the default, streamed
    same(here, ref)
    one = here if streamed else children[False, 1][name]
    same(one, ref)
    same(one, children[streamed, 2][name])


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("H,W,streamed", SHAPES)
def test_probe_mix_search_equals_oracle_and_two_product_probe(gpu, oracle, children, H, W, streamed, kind):
    _check(gpu, oracle, children, H, W, streamed, kind)


@pytest.mark.gpu
def test_probe_mix_depth2_edge_equals_oracle_and_two_product_probe(gpu, oracle, children):
    _check(gpu, oracle, children, *EDGE2, "edge2")


if __name__ == "__main__":
    # child of the `children` fixture: every case of this process's switches
    assert sys.argv[1] == "--child" and os.environ.get("BICOS_PKP_PROBE") in ("1", "2")
    from libbicos_amd import device
    np.savez(sys.argv[2], **run_all(device.Engine(0), os.environ.get("BICOS_MX_STREAM") != "0"))
