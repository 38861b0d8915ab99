"""The packed pruned search's probe depth (search_pk.hip search_pkp_kernel, block_pr): a block
of 32 col1 is probed with descriptor word 0 alone (2 scaled MFMAs per wave), and a wide tile
(64 col0) takes words 1-3 only where ham_0 of some col0 comes within reach (<=) of that col0's
running minimum. A wave whose wide-tile-blocks nearly all reach over a window goes on with the
two-word probe (ham_lo, words 0 and 1) for the rest of its row, and from there, by the same
rule, to the unpruned loop; it never goes back up. BICOS_PKP_PROBE=2 starts every wave at the
two-word probe (read once per process).

CPU (numpy, no GPU):
  reach predicate  after word 0 a key field holds 0x4B00 + 48 + ham_0; the saturated R + 0x31 -
                   key is non-zero exactly where ham_0 <= R - 0x4B00, for every R and ham_0 the
                   kernel can hold, one field and both packed, and no field of R + 0x31 wraps
  pruned scan      a model of the lazy scan of one row in the kernel's visiting order that skips
                   every wide-tile-block whose probe minimum lies above the running minimum, at
                   either start depth and whatever the windows decide, gives the full scan's
                   minimum, "duplicate" verdict and first column

GPU: one child process per BICOS_PKP_PROBE setting computes every case; every case asserts
through bicos_search_packed that the packed form runs; the default (depth 1) is compared byte
for byte with the CPU oracle and with the BICOS_PKP_PROBE=2 child.
Shapes: 256 x 1056 (streamed, one short stage), 512 x 1024 (the chunk loop), 256 x 1100 (a
partial last block, a workgroup with idle waves). Kinds: stereo, flip10, random and tie of
tests/test_search_packed_prune.py, and
  w0const  word 0 identical in every column, words 1-3 of the stereo frame: ham_0 = 0
           everywhere, every wide-tile-block reaches at depth 1 and few at depth 2 -- every wave
           takes the 1 -> 2 step and stays pruned there
  w0only   words 1-3 identical, word 0 random, the right row the left moved by 3 columns with
           a few bits flipped, and planted exact duplicates: ham_0 = ham, so every tie sits
           exactly on the threshold, and a tie must never be pruned
and one fused case: 64 rows of the cfg2 frame through the match (search + agree launch).
"""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests.test_search_packed_prune import (BITS, HINT, INVALID, MASK, N, NODUPES, WORDS, _rand,  # noqa: E402
                                            _stereo, gpu_match, gpu_search, search_case, tie_sites)
from tests.test_search_stream import _dev_stack, same  # noqa: E402

SHAPES = [(256, 1056), (512, 1024), (256, 1100)]
KINDS = ["stereo", "flip10", "random", "tie", "w0const", "w0only"]
FUSED_ROWS = 64
PRUNE_WINDOW = 8        # search_plan.hpp


# ---- CPU: the depth-1 reach predicate ---------------------------------------------------------

R_FIELDS = np.array(list(range(0x4B00, 0x4B80)) + [0x7BFF], np.uint32)
HAM0 = np.arange(33, dtype=np.uint32)
KEYS1 = HAM0 + np.uint32(0x4B00 + 48)        # what a field holds after the MFMA of word 0
THR1 = 0x00310031                           # search_pk.hip PKP_THR1


def _fields(x):
    return (x >> np.uint32(16)).astype(np.uint16), (x & np.uint32(0xFFFF)).astype(np.uint16)


def reach1(R, key):
    """thr = R + 0x00310031 (one 32-bit add), v_pk_sub_u16 clamp of thr and key, != 0"""
    thr = (R.astype(np.uint64) + THR1)
    assert (thr < 1 << 32).all()
    thr = thr.astype(np.uint32)
    out = np.zeros(R.shape, bool)
    for t, f in zip(_fields(thr), _fields(key)):
        d = np.where(t > f, t - f, np.uint16(0)).astype(np.uint16)
        out |= d != 0
    return out


def test_threshold_does_not_wrap():
    assert int(R_FIELDS.max()) + 0x31 < 1 << 16         # PK_PAD + 0x31 stays in its field
    for Rh in R_FIELDS:
        R = (np.uint32(Rh) << np.uint32(16)) | R_FIELDS
        th, tl = _fields((R + np.uint32(THR1)).astype(np.uint32))
        assert (tl.astype(np.uint32) == R_FIELDS + 0x31).all() and (th == Rh + 0x31).all()


def test_depth1_reach_predicate_one_field():
    R, k = np.meshgrid(R_FIELDS, KEYS1, indexing="ij")
    ham0 = k - np.uint32(0x4B00 + 48)
    for sh in (0, 16):      # the other field never reaches: R = 0x4B00 against the pad
        Rp = (R << np.uint32(sh)) | np.uint32(0x4B00 << (16 - sh))
        kp = (k << np.uint32(sh)) | np.uint32(0x7BFF << (16 - sh))
        assert np.array_equal(reach1(Rp, kp), ham0 <= R - 0x4B00)
    # a tie reaches, one more is pruned
    Rt = np.array([np.uint32(0x4B10) | np.uint32(0x4B00 << 16)])
    pad = np.uint32(0x7BFF << 16)
    assert reach1(Rt, np.array([np.uint32(0x4B00 + 48 + 0x10) | pad]))[0]
    assert not reach1(Rt, np.array([np.uint32(0x4B00 + 48 + 0x11) | pad]))[0]


def test_depth1_reach_predicate_both_fields_packed():
    Rl, kl = (x.ravel().astype(np.uint32) for x in np.meshgrid(R_FIELDS, KEYS1, indexing="ij"))
    want_low = kl - (0x4B00 + 48) <= Rl - 0x4B00
    for Rh in R_FIELDS:
        for kh in KEYS1:
            R = (np.uint32(Rh) << np.uint32(16)) | Rl
            k = (np.uint32(kh) << np.uint32(16)) | kl
            want = want_low | (int(kh) - (0x4B00 + 48) <= int(Rh) - 0x4B00)
            assert np.array_equal(reach1(R, k), want), (hex(Rh), hex(kh))


# ---- CPU: the pruned scan against the full scan --------------------------------------------------

POP = np.array([bin(i).count("1") for i in range(256)], np.int32)
KEY_OFF = {1: 48, 2: 32}        # what the skipped words' share of C leaves in a partial key
INF = 0x7BFF - 0x4B00           # the running minimum's start, PK_PAD, as a distance


def ham(a, b, nw):
    """[W0, 4] x [W1, 4] uint32 -> [W0, W1] Hamming distances over the first nw words"""
    x = (a[:, None, :nw] ^ b[None, :, :nw]).copy().view(np.uint8)
    return POP[x].sum(axis=-1)


def wave_order(W, c0_wave):
    """Block bases in the wave's visiting order (one step: the row fits a chunk): the partial
    last block, then the full blocks downwards from the one holding the wave's highest col0."""
    nfull = W // 32
    order = [32 * nfull] if W % 32 else []
    sb0 = max(0, min(nfull - 1, min(W - 1, c0_wave + 127) // 32))
    return order + [32 * ((sb0 - i) % nfull) for i in range(nfull)]


def pruned_scan(a, b, depth0, outcome, window):
    """The lazy scan of search_pkp_kernel for one row, per wave of two wide tiles: running
    minimum R, tie marker and block of the last drop per col0, the pair step with a skipped
    tile's partial keys where the other tile reaches, the end of row's count inside the
    recorded block. outcome(window index, reaching, tested) -> bool decides every window (the
    kernel's rule is one such function). -> (minimum, duplicate, first column) per col0"""
    W = a.shape[0]
    H = ham(a, b, 4)
    Hd = {1: ham(a, b, 1), 2: ham(a, b, 2)}
    mins, dup, col = np.zeros(W, np.int64), np.zeros(W, bool), np.zeros(W, np.int64)
    skipped = 0
    for c0_wave in range(0, W, 128):
        tiles = [(lo, min(W, lo + 64)) for lo in (c0_wave, c0_wave + 64) if lo < W]
        R = {t: np.full(t[1] - t[0], INF) for t in tiles}
        tie = {t: np.zeros(t[1] - t[0], bool) for t in tiles}
        Cb = {t: np.zeros(t[1] - t[0], np.int64) for t in tiles}
        depth, wb, wr, nwin = depth0, 0, 0, 0
        for B in wave_order(W, c0_wave):
            e = min(W, B + 32)
            d = depth if e - B == 32 else 0      # the partial last block never prunes
            keys, reach = {}, {}
            for t in tiles:
                reach[t] = True
                if d:
                    probe = Hd[d][t[0]:t[1], B:e].min(axis=1)
                    reach[t] = bool((probe <= R[t]).any())
                    keys[t] = probe + KEY_OFF[d]
                if reach[t]:
                    keys[t] = H[t[0]:t[1], B:e].min(axis=1)
                skipped += not reach[t]
            if any(reach.values()):
                for t in tiles:
                    k = keys[t]
                    if not reach[t]:
                        assert (k > R[t]).all()         # partial keys never decide anything
                    drop = k < R[t]
                    tie[t] = np.where(drop, False, tie[t] | (k == R[t]))
                    Cb[t] = np.where(drop, B, Cb[t])
                    R[t] = np.minimum(R[t], k)
            if d:
                wr += sum(reach.values())
                wb += 1
                if wb == window:
                    if outcome(nwin, wr, window * 2):
                        depth = 2 if depth == 1 else 0
                    nwin += 1
                    wb = wr = 0
        for t in tiles:
            for i, c in enumerate(range(t[0], t[1])):
                blk = H[c, Cb[t][i]:Cb[t][i] + 32]
                at = np.flatnonzero(blk == R[t][i])
                mins[c] = R[t][i]
                dup[c] = tie[t][i] or len(at) > 1
                col[c] = Cb[t][i] + at[0]
    return mins, dup, col, skipped


def full_scan(a, b):
    H = ham(a, b, 4)
    m = H.min(axis=1)
    return m, (H == m[:, None]).sum(axis=1) > 1, H.argmin(axis=1)


def small_row(rng, W, kind):
    a = _rand(rng, (W, WORDS)) & MASK
    if kind == "random":
        return a, _rand(rng, (W, WORDS)) & MASK
    flips = MASK.copy()
    for _ in range(7):
        flips = flips & _rand(rng, (W, WORDS))
    b = a[np.roll(np.arange(W), 3)] ^ flips      # col0 c matches col1 c + 3, about 1 bit away
    if kind == "w0only":                         # ham_0 = ham: ties sit on the threshold
        a[:, 1:] = a[0, 1:]
        b[:, 1:] = a[0, 1:]
    if kind in ("dup", "w0only"):                # exact duplicates of some matches, any block
        for c in rng.choice(W - 3, size=6, replace=False):
            b[(c + 3 + rng.integers(1, W)) % W] = b[c + 3]
    return a, b


def kernel_rule(_, reaching, tested):
    return 8 * reaching >= 7 * tested


@pytest.mark.parametrize("kind", ["near", "dup", "w0only", "random"])
def test_pruned_scan_equals_full_scan(kind):
    rng = np.random.default_rng({"near": 1, "dup": 2, "w0only": 3, "random": 4}[kind])
    total = 0
    for W in (64, 100, 160, 255, 256):
        for _ in range(2):
            a, b = small_row(rng, W, kind)
            want = full_scan(a, b)
            if kind in ("dup", "w0only"):
                assert want[1].sum() >= 4
            pattern = rng.random(64) < 0.5
            for depth0 in (1, 2):
                for window in (1, 2, PRUNE_WINDOW):
                    for outcome in (kernel_rule, lambda *_: False, lambda *_: True,
                                    lambda i, *_: bool(pattern[i % 64])):
                        m, d, c, skipped = pruned_scan(a, b, depth0, outcome, window)
                        assert np.array_equal(m, want[0])
                        assert np.array_equal(d, want[1])
                        assert np.array_equal(c[~d], want[2][~d])
                        total += skipped
    assert (total > 0) == (kind != "random")     # the planted rows do prune; random ones never


# ---- GPU ---------------------------------------------------------------------------------------

def _w0const_pair(H, W):
    a, b = _stereo(H, W)
    a[:, :, 0] = np.uint32(0x5A5A3C0F)
    b[:, :, 0] = np.uint32(0x5A5A3C0F)
    return a, b


def w0only_sites(W):
    """(col0, second col1): right columns col0 + 3 and second col1 are made exact copies of
    the left descriptor -- the second in a block further down, behind the wrap, and in the
    row's last column."""
    return [(700, 650), (40, W - 60), (W // 2, W - 1)]


def _w0only_pair(H, W, seed):
    rng = np.random.default_rng(seed)
    a = np.empty((H, W, WORDS), np.uint32)
    a[:] = np.array([0, 0x12345678, 0x9ABCDEF0, 0x0F0F0F0F], np.uint32) & MASK
    a[:, :, 0] = _rand(rng, (H, W))
    b = a[:, np.roll(np.arange(W), 3)].copy()
    b[:, :, 0] ^= _rand(rng, (H, W)) & _rand(rng, (H, W)) & _rand(rng, (H, W)) & _rand(rng, (H, W))
    for c, p2 in w0only_sites(W):     # (distance 0 twice: no other column can come closer)
        b[:, c + 3] = a[:, c]
        b[:, p2] = a[:, c]
    return a, b


def case(kind, H, W):
    """(left, right, stated bits)"""
    if kind == "w0const":
        return _w0const_pair(H, W) + (HINT,)
    if kind == "w0only":
        return _w0only_pair(H, W, 15000 + W) + (BITS,)
    return search_case(kind, H, W)


def test_planted_kinds_are_what_they_say():
    pop = lambda x: int(np.unpackbits(np.ascontiguousarray(x).view(np.uint8)).sum())  # noqa: E731
    for H, W in SHAPES:
        a, b, _ = case("w0const", H, W)
        assert (a[:, :, 0] == a[0, 0, 0]).all() and (b[:, :, 0] == a[0, 0, 0]).all()
        assert ((a & ~MASK) == 0).all() and ((b & ~MASK) == 0).all()
        a, b, _ = case("w0only", H, W)
        assert (a[:, :, 1:] == a[0, 0, 1:]).all() and (b[:, :, 1:] == a[0, 0, 1:]).all()
        for c, p2 in w0only_sites(W):
            assert (b[:, p2] == a[:, c]).all() and (b[:, c + 3] == a[:, c]).all() and p2 != c + 3
        assert pop(a[0, 100] ^ b[0, 103]) <= 8


def fused_rows():
    from tests.golden.make_frames import FRAMES, frame_stacks
    return frame_stacks(FRAMES["cfg2"], 0, FUSED_ROWS)


def fused_match(eng, L, R):
    """64 rows take two tiles per wave by default (a narrow band); tuned to four, as the
    whole frame runs, they go through the packed fused launch."""
    try:
        eng.tune(64, 4, 0, 0)
        assert eng.search_packed(FUSED_ROWS, L.shape[2], WORDS, HINT, N, fused=True)
        return gpu_match(eng, L, R)
    finally:
        eng.tune(0, 0, 0, 0)


def run_all(eng):
    out = {}
    for H, W in SHAPES:
        for kind in KINDS:
            a, b, bits = case(kind, H, W)
            assert eng.search_packed(H, W, WORDS, bits)
            out["%s_%d_%d" % (kind, H, W)] = gpu_search(eng, a, b, bits)
    out["match_d"], out["match_c"] = fused_match(eng, *fused_rows())
    return out


def _child(tmp_path_factory, depth):
    path = str(tmp_path_factory.mktemp("pkp_probe") / ("depth%d.npz" % depth))
    env = dict(os.environ, BICOS_PKP_PROBE=str(depth))
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", path], env=env,
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def depths(gpu, tmp_path_factory):
    """Every case at start depth 1 (the default) and 2, one child process each."""
    return _child(tmp_path_factory, 1), _child(tmp_path_factory, 2)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("H,W", SHAPES)
def test_probe_depth_search_equals_oracle_and_two_word_probe(gpu, oracle, depths, H, W, kind):
    a, b, bits = case(kind, H, W)
    assert gpu.search_packed(H, W, WORDS, bits)
    ref = oracle.search(a, b, NODUPES)
    if kind == "tie":
        for c, p2 in tie_sites(W):
            assert (ref[:, c] == INVALID).all(), (c, p2, ref[0, c])
    if kind == "w0only":    # the same minimum twice: invalid (valid if the reach test were "<")
        for c, p2 in w0only_sites(W):
            assert (ref[:, c] == INVALID).all(), (c, p2, ref[0, c])
        assert (ref != INVALID).mean() > 0.5
    one, two = (d["%s_%d_%d" % (kind, H, W)] for d in depths)
    same(one, ref)
    same(one, two)
    same(gpu_search(gpu, a, b, bits), ref)      # this process: the default


@pytest.mark.gpu
def test_probe_depth_fused_match_equals_two_word_probe(gpu, depths):
    from libbicos_amd import _lib
    from libbicos_amd.device import MatchConfig
    one, two = depths
    same(one["match_d"], two["match_d"])
    same(one["match_c"], two["match_c"])
    L, R = fused_rows()
    try:
        gpu.tune(64, 4, 0, 0)
        assert gpu.plan(_dev_stack(L), _dev_stack(R), MatchConfig(nxcorr_threshold=0.96)) & \
            _lib.PLAN_AGREE_IN_SEARCH
    finally:
        gpu.tune(0, 0, 0, 0)
    d, c = fused_match(gpu, L, R)
    same(d, one["match_d"])
    same(c, one["match_c"])


if __name__ == "__main__":
    # child of the `depths` fixture: every case at this process's start depth
    assert sys.argv[1] == "--child" and os.environ.get("BICOS_PKP_PROBE") in ("1", "2")
    from libbicos_amd import device
    np.savez(sys.argv[2], **run_all(device.Engine(0)))
