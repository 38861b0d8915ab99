"""The packed pruned search's block loop (search_pk.hip search_pkp_kernel, round 13): one
carried LDS address per lane with the other words of a block at immediate offsets, and the
reach test as a saturating subtraction against R + 33.

CPU (numpy, no GPU):
  reach predicate  the sign-bit test against R + 32 and the saturating test against R + 33
                   decide alike for every value the kernel can hold, one field and both packed
  address walk     the carried address, stepped by the scalar delta, visits the blocks of a
                   step downwards from the start block, wrapping, each once, and every read
                   (the unused prefetch behind the last block too) stays inside the step

GPU: every case asserts through bicos_search_packed that the packed form runs and is compared
byte for byte with the CPU oracle and with the chunk loop of the same library
(BICOS_MX_STREAM=0, read once per process: one child process computes every case; the runner of
tests/test_search_packed_prune.py starts that file, so this one has a copy for itself).
Rows: 256, at 3968 columns 128 -- with 64 rows fewer bicos_search_packed says no (below 4 tiles
per wave: test_rows_are_the_fewest_packed). Widths, chunks of 1024 columns streamed in stages of 512:
  1025  the second chunk holds one column: nfull = 0, only the partial block runs there
  1057  nfull = 1: the wrap lands on the same block; and a partial block
  1088  nfull = 2
  2016  a stage of 480 columns
  3968  the widest row the packed plan takes (3969 is refused: a query only)
Kinds: stereo, random (every wave falls back: the unpruned loop on the carried address) and tie
of tests/test_search_packed_prune.py, and edge: on a near pair (every col0 c matches col1 c + 3
about 8 bits away, made far here for the planted col0), for col0 in both wide tiles and both
lane halves of a wave, the left descriptor equals right column c1 but for k bits of words 2-3
(ham_lo = 0, ham = k) and a second column c2, in a block visited later, differs by k bits of
words 0-1 (ham_lo = k = the running minimum: it reaches, a tie, invalid) or by k + 1 (pruned:
the result is c1); k = 0, 1, 31 by row; c1 and c2 lie on either side of a stage or chunk
boundary of the width (the last column of one block, the first of the next), of the first
block boundary, or in the row's first and last column.

The streamed instantiations are built for the default geometry's 1024-column chunk alone. A
tuned engine (fewer waves, a smaller stage) gets chunks of 512 or 256 columns, which
mx_streamable would stream as well: the plan gives the packed search of such a geometry the
chunk loop (a host-only probe of the plan, tests/cpp/pkp_stream_plan.cpp), and three such
geometries run on the GPU against the oracle.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests.test_search_packed_prune import (BITS, INVALID, MASK, NODUPES, WORDS, _near_pair,  # noqa: E402
                                            gpu_search, search_case, tie_sites)
from tests.test_search_stream import same  # noqa: E402

WIDTHS = [1025, 1057, 1088, 2016, 3968]
ROWS = {1025: 256, 1057: 256, 1088: 256, 2016: 256, 3968: 128}
KINDS = ["stereo", "random", "tie", "edge"]
CHUNK = 1024            # search_pk.hip PKP_ST_CHUNK
HALF = CHUNK // 2       # a streamed stage
KS = (0, 1, 31)
LANE_OFFSETS = (3, 40, 77, 110)     # col0 of a wave: tile 0 P / Q lanes, tile 1 P / Q lanes


# ---- CPU: the reach predicate -------------------------------------------------------------

R_FIELDS = np.array(list(range(0x4B00, 0x4B80)) + [0x7BFF], np.uint32)
M_FIELDS = np.array(list(range(0x4B20, 0x4B61)) + [0x7BFF], np.uint32)


def _fields(x):
    return (x >> np.uint32(16)).astype(np.uint16), (x & np.uint32(0xFFFF)).astype(np.uint16)


def reach_sign(R, m):
    """as it was: (thr - m) & 0x80008000 != 0x80008000 with thr = R + 0x00200020 (one 32-bit
    add, v_pk_sub_i16 wrapping per field)"""
    thr = (R + np.uint32(0x00200020)).astype(np.uint32)
    out = np.zeros(R.shape, bool)
    for t, f in zip(_fields(thr), _fields(m)):
        d = (t - f).astype(np.uint16)       # wraps
        out |= (d & np.uint16(0x8000)) == 0
    return out


def reach_sat(R, m):
    """v_pk_sub_u16 clamp of thr1 = R + 0x00210021 and m, then != 0 on the 32 bits"""
    thr = (R + np.uint32(0x00210021)).astype(np.uint32)
    out = np.zeros(R.shape, bool)
    for t, f in zip(_fields(thr), _fields(m)):
        d = np.where(t > f, t - f, np.uint16(0)).astype(np.uint16)
        out |= d != 0
    return out


def test_reach_predicate_one_field():
    R, m = np.meshgrid(R_FIELDS, M_FIELDS, indexing="ij")
    for sh in (0, 16):      # the other field never reaches: R = 0x4B00 against the pad
        Rp = (R << np.uint32(sh)) | np.uint32(0x4B00 << (16 - sh))
        mp = (m << np.uint32(sh)) | np.uint32(0x7BFF << (16 - sh))
        old, new = reach_sign(Rp, mp), reach_sat(Rp, mp)
        assert np.array_equal(old, new)
        assert np.array_equal(new, m <= R + 0x20)     # a tie reaches, one more is pruned
    tie = np.uint32(0x4B10 + 0x20) | np.uint32(0x7BFF << 16)
    Rt = np.uint32(0x4B10) | np.uint32(0x4B00 << 16)
    assert reach_sat(np.array([Rt]), np.array([tie]))[0]
    assert not reach_sat(np.array([Rt]), np.array([tie + np.uint32(1)]))[0]


def test_reach_predicate_both_fields_packed():
    Rl, ml = (x.ravel() for x in np.meshgrid(R_FIELDS, M_FIELDS, indexing="ij"))
    low_R, low_m = Rl.astype(np.uint32), ml.astype(np.uint32)
    want_low = low_m <= low_R + 0x20
    for Rh in R_FIELDS:
        for mh in M_FIELDS:
            R = (np.uint32(Rh) << np.uint32(16)) | low_R
            m = (np.uint32(mh) << np.uint32(16)) | low_m
            old, new = reach_sign(R, m), reach_sat(R, m)
            assert np.array_equal(old, new), (hex(Rh), hex(mh))
            assert np.array_equal(new, want_low | (mh <= Rh + 0x20))


# ---- CPU: the address walk ----------------------------------------------------------------

def walk(nfull, sb0, b0, j, lds0=0):
    """The pruned loop's reads of one step as the kernel issues them: [(block visited,
    [addresses of words 1-3], address of the word-0 prefetch behind it)]; 32-bit unsigned
    arithmetic, the delta a signed scalar.

    A transcription of search_pk.hip search_pkp_kernel, from `int so = 512 * sb0;` ("The visiting
    order as one carried address") to the end of the pruned loop, and of block_pr's reads and
    its `ad += d`: a model, which cannot see the kernel diverge from it -- the GPU cases below
    do that. Change the two together."""
    u32 = 0xFFFFFFFF
    so = 512 * sb0
    wrap = 512 * (nfull - 1)
    ad = (lds0 + 16 * (32 * b0 + j) + so) & u32
    first = ad
    out = []
    for _ in range(nfull):
        d = -512 if so > 0 else wrap
        words = [ad + w * CHUNK * 16 for w in (1, 2, 3)]
        blk = so // 512
        ad = (ad + d) & u32
        so += d
        out.append((blk, words, ad))
    return first, out


def test_address_walk_visits_every_block_once_inside_the_step():
    assert 3 * CHUNK * 16 < 1 << 16     # the largest word offset fits the ds_read offset field
    for nfull in range(1, 65):
        for b0 in (0, 16):
            lo, hi = 16 * 32 * b0, 16 * 32 * (b0 + nfull)   # word-0 bytes of the step's columns
            for sb0 in range(nfull):
                for j in (0, 31):
                    first, steps = walk(nfull, sb0, b0, j)
                    assert first == 16 * (32 * (b0 + sb0) + j)
                    assert [s[0] for s in steps] == [(sb0 - i) % nfull for i in range(nfull)]
                    cur = first
                    for blk, words, nxt in steps:
                        assert cur == 16 * (32 * (b0 + blk) + j)
                        for w, x in zip((1, 2, 3), words):
                            assert x - w * CHUNK * 16 == cur and lo <= cur < hi
                        assert lo <= nxt < hi and (nxt - 16 * j) % 512 == 0
                        cur = nxt
                    # behind the last block: the wrapped address, the block before sb0's turn
                    assert cur == 16 * (32 * (b0 + (sb0 - nfull) % nfull) + j)


# ---- the visiting order of one col0 (the edge kind places its columns by it) ----------------

def visit_order(W, c):
    """Block bases (col1) in the order the wave of col0 c visits them: its workgroup's chunk,
    then the other chunks downwards (wrapping) in stages of half a chunk, upper half first; in
    every step the partial block first, then the full blocks downwards from the one holding
    the wave's highest col0 (clamped), wrapping."""
    tile, c0_wave = c // CHUNK, c // 128 * 128
    nchunks = (W + CHUNK - 1) // CHUNK
    cstart = min(W - 1, (tile + 1) * CHUNK - 1) // CHUNK
    steps = [(cstart * CHUNK, min(CHUNK, W - cstart * CHUNK))]
    for s in range(2 * (nchunks - 1)):
        ci = (cstart - 1 - (s >> 1)) % nchunks
        sbase = ci * CHUNK + (0 if s & 1 else HALF)
        steps.append((sbase, max(0, min(HALF, W - sbase))))
    order = []
    for sbase, ncols in steps:
        nfull = ncols // 32
        if ncols & 31:
            order.append(sbase + 32 * nfull)
        sb0 = max(0, min(nfull - 1, (min(W - 1, c0_wave + 127) - sbase) // 32))
        order += [sbase + 32 * ((sb0 - i) % nfull) for i in range(nfull)]
    assert sorted(order) == list(range(0, W, 32))
    return order


def test_visit_order_covers_the_row():
    for W in WIDTHS:
        for c in (0, 127, 128, 1023, 1024, W - 1):
            visit_order(W, c)


# ---- the edge kind ---------------------------------------------------------------------------

def column_pairs(W):
    """Pairs of right columns on either side of every stage / chunk boundary, of the first
    block boundary, and the row's first and last column; no column twice."""
    pairs = [(m - 1, m) for m in range(HALF, W, HALF)] + [(31, 32), (0, W - 1)]
    used, out = set(), []
    for p in pairs:
        if not (set(p) & used):
            out.append(p)
            used |= set(p)
    return out


def _bits(rng, k, lo_words):
    """A 4-word mask of k distinct bits in words 0-1 (lo_words) or in the used bits of 2-3."""
    pos = rng.choice(64 if lo_words else 62, size=k, replace=False) + (0 if lo_words else 64)
    x = np.zeros(WORDS, np.uint32)
    for p in pos:
        x[p // 32] |= np.uint32(1) << np.uint32(p % 32)
    return x


_EDGE = {}


def edge_case(H, W):
    """(left, right, {(row, col0): expected disparity})"""
    if (H, W) in _EDGE:
        a, b, want = _EDGE[H, W]
        return a.copy(), b.copy(), want
    a, b = _near_pair(H, W, 13000 + W)
    rng = np.random.default_rng(13500 + W)
    pairs = column_pairs(W)
    nwaves = (W - 4) // 128
    want = {}
    for r in range(H):
        k = KS[r % 3]
        c0_wave = 128 * ((5 * r + r // 7) % nwaves)
        for i in range(min(4, len(pairs))):
            c = c0_wave + LANE_OFFSETS[(i + r // 6) % 4]
            p, q = pairs[(r // 24 + i) % len(pairs)]
            order = visit_order(W, c)
            rank = lambda x: order.index(x // 32 * 32)  # noqa: E731
            assert rank(p) != rank(q)
            c1, c2 = (p, q) if rank(p) < rank(q) else (q, p)
            tie = (r // 3 + i) % 2 == 0
            b[r, c + 3] = ~a[r, c] & MASK
            b[r, c1] = a[r, c] ^ _bits(rng, k, False)
            b[r, c2] = a[r, c] ^ _bits(rng, k if tie else k + 1, True)
            want[r, c] = INVALID if tie else c - c1
    _EDGE[H, W] = (a, b, want)
    return a.copy(), b.copy(), want


def case(kind, H, W):
    """(left, right, stated bits)"""
    if kind == "edge":
        return edge_case(H, W)[:2] + (BITS,)
    return search_case(kind, H, W)


def test_edge_case_is_what_it_says():
    """ham_lo / ham of the planted columns, sites of every k, both outcomes and all four lane
    positions in every width, and no two sites of a row on one column."""
    pop = lambda x: np.unpackbits(x.view(np.uint8)).sum()  # noqa: E731
    for W in WIDTHS:
        a, b, want = edge_case(ROWS[W], W)
        seen = set()
        for (r, c), v in want.items():
            k = KS[r % 3]
            assert pop(a[r, c] ^ b[r, c + 3]) > 100
            ham = sorted(((int(pop(a[r, c] ^ b[r, x])), int(pop(a[r, c, :2] ^ b[r, x, :2]))), x)
                         for p in column_pairs(W) for x in p)     # ((ham, ham_lo), column)
            assert ham[0][0] == (k, 0) and ham[1][0] == ((k, k) if v == INVALID else (k + 1, k + 1))
            assert v == INVALID or v == c - ham[0][1]
            assert ham[2][0][0] > 32     # (the other sites' columns: random, about 63)
            seen.add((k, v == INVALID, (c % 128) // 32))
        assert len(seen) == 3 * 2 * 4, W


# ---- GPU ---------------------------------------------------------------------------------------

def run_all(eng):
    out = {}
    for W in WIDTHS:
        for kind in KINDS:
            a, b, bits = case(kind, ROWS[W], W)
            out["%s_%d" % (kind, W)] = gpu_search(eng, a, b, bits)
    return out


@pytest.fixture(scope="module")
def chunk_loop(gpu, tmp_path_factory):
    """The same inputs through the chunk loop of the same library (runtime chunk, no stages)."""
    path = str(tmp_path_factory.mktemp("pkp_block_loop") / "chunk_loop.npz")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", path],
                       env=dict(os.environ, BICOS_MX_STREAM="0"), cwd=ROOT, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("W", WIDTHS)
def test_block_loop_search_equals_oracle_and_chunk_loop(gpu, oracle, chunk_loop, W, kind):
    a, b, bits = case(kind, ROWS[W], W)
    assert gpu.search_packed(ROWS[W], W, WORDS, bits)
    ref = oracle.search(a, b, NODUPES)
    if kind == "tie":
        for c, p2 in tie_sites(W):
            assert (ref[:, c] == INVALID).all(), (c, p2, ref[0, c])
    if kind == "edge":
        for (r, c), v in edge_case(ROWS[W], W)[2].items():
            assert ref[r, c] == v, (r, c, v, ref[r, c])
    got = gpu_search(gpu, a, b, bits)
    same(got, ref)
    same(got, chunk_loop["%s_%d" % (kind, W)])


def test_rows_are_the_fewest_packed(blib):
    """The packed form needs 4 tiles per wave, which 64 rows fewer do not get at these widths
    (a query without an engine: 256 CUs); 3969 columns are not packed at any count."""
    q = lambda rows, cols: blib.bicos_search_packed(None, rows, cols, WORDS, BITS, 0, 0)  # noqa: E731
    if os.environ.get("BICOS_MX_PACKED") == "0" or os.environ.get("BICOS_MX_PRUNE") == "0":
        return
    for W in WIDTHS:
        assert q(ROWS[W], W) == 1 and q(ROWS[W] - 64, W) == 0, W
    assert q(128, 3969) == 0 and q(256, 3969) == 0 and q(1024, 3969) == 0


# ---- geometries with another chunk than the streamed instantiations' -----------------------------
# mx_streamable (search_plan.cpp) allows any chunk of two columns per thread; the packed
# kernel's streamed instantiations are built for PKP_ST_CHUNK = 1024 alone (8 waves over a 64
# KiB stage). An engine tuned to fewer waves and a smaller stage (bicos_engine_tune(64, tiles,
# waves, stage KiB)) plans 512- or 256-column chunks: the packed search then runs its chunk loop.

# (rows, cols, tiles per wave, waves, stage KiB)
TUNED = [(512, 1536, 4, 4, 32), (512, 1984, 0, 4, 32), (1024, 900, 0, 2, 16)]
HIPCC = "/opt/rocm/bin/hipcc"


def test_plan_streams_the_packed_search_at_one_chunk_only(tmp_path):
    """tests/cpp/pkp_stream_plan.cpp, linked with the host-only planning source alone."""
    csrc = os.path.join(ROOT, "libbicos_amd", "csrc")
    exe = str(tmp_path / "pkp_stream_plan")
    src = os.path.join(ROOT, "tests", "cpp", "pkp_stream_plan.cpp")
    subprocess.run([HIPCC, "-O1", "-std=c++17", "-I" + csrc, src, os.path.join(csrc, "search_plan.cpp"),
                    "-o", exe], check=True, capture_output=True)
    env = {k: v for k, v in os.environ.items() if not k.startswith("BICOS_")}

    def plan(rows, cols, T, waves, kib, bits):
        arg = "%d,%d,%d,%d,%d,%d" % (rows, cols, T, waves, kib, bits)
        out = subprocess.run([exe, arg], check=True, capture_output=True, text=True, env=env).stdout
        ok, stream, prune, packed, chunk, block, lds = (int(x) for x in out.split(":")[1].split())
        assert ok and prune
        return stream, packed, chunk, block

    assert plan(256, 2048, 0, 0, 64, 125) == (1, 1, 1024, 512)      # the default geometry streams
    assert plan(1536, 2048, 0, 0, 64, 125) == (1, 1, 1024, 512)     # cfg2
    for (rows, cols, T, waves, kib), chunk in zip(TUNED, (512, 512, 256)):
        # packed: the chunk loop; the one-product kernel (bits unknown) streams at any chunk
        assert plan(rows, cols, T, waves, kib, 125) == (0, 1, chunk, 64 * waves)
        assert plan(rows, cols, T, waves, kib, 0) == (1, 0, chunk, 64 * waves)
    sweep = subprocess.run([exe, "sweep"], check=True, capture_output=True, text=True, env=env).stdout.split()
    counts = dict(zip(sweep[::2], (int(x) for x in sweep[1::2])))
    assert counts["packed"] > counts["streamed"] > 100 and counts["other"] == 0, counts


@pytest.mark.gpu
@pytest.mark.parametrize("rows,cols,T,waves,kib", TUNED)
@pytest.mark.parametrize("kind", ["stereo", "random"])
def test_tuned_geometry_runs_packed_and_equals_oracle(gpu, oracle, rows, cols, T, waves, kib, kind):
    a, b, bits = search_case(kind, rows, cols)
    ref = oracle.search(a, b, NODUPES)
    try:
        gpu.tune(64, T, waves, kib)
        assert gpu.search_packed(rows, cols, WORDS, bits)
        got = gpu_search(gpu, a, b, bits)
    finally:
        gpu.tune(0, 0, 0, 0)
    same(got, ref)


if __name__ == "__main__":
    # child of the chunk_loop fixture: every case through this process's library switch
    assert sys.argv[1] == "--child" and os.environ.get("BICOS_MX_STREAM") == "0"
    from libbicos_amd import device
    eng = device.Engine(0)
    for W in WIDTHS:
        assert eng.search_packed(ROWS[W], W, WORDS, BITS)
    np.savez(sys.argv[2], **run_all(eng))
