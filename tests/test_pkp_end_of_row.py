"""The pruned packed search's end of row (search_pk.hip search_pkp_kernel, EOR): a lazy drop
records the lane half of its block that holds the new minimum (equal halves: a tie at once),
the rescan visits that half's 16 rows in two levels (ham_lo, then the candidates' full
distance), and the raw right row and the left descriptors are requested before the barrier
behind the scan. tests/test_pk_half_rule.py holds the argument as a CPU model; here the kernel
itself, byte for byte against the CPU oracle, against the end of row as it was
(BICOS_PKP_EOR=0: rescans of all 32 rows), against the chunk loop (BICOS_MX_STREAM=0) and
against both together, and at match level against the separate agree launch
(BICOS_FUSE_AGREE=0). The switches are read once per process: one child process per setting
computes every case.

Shapes: 256 rows (4 tiles per wave planned) x 1056, 1100 (a partial last block of 12 columns;
its last 76 col0 go to the tail launch, another kernel), 1612 (the same partial block, and no
tail: the last workgroup of this kernel holds 588 col0 -- idle waves and a wave that ends
inside the row), 2048 and 2080 columns; 126-bit descriptors, the used bits stated (HINT for
transform descriptors, BITS for made-up ones). Match level: 2048 and 1612 run the fused launch
(asserted); 1100 columns plan a tail, so that match runs the search and the agree separately
and is compared all the same.

Planted sites (sites()): on top of a base pair, for some col0 c the right row gets columns at
distance 0..2 from a[c] -- everything else lies about 8 (the near pair's own match at c + 3),
12 (flip10) or 63 bits away:
  same half    two columns at the minimum in rows 0/1 and 8/11 of one block: the rescan counts 2
  other half   rows 0/4 and 3/31: equal halves on the drop, invalid without a rescan
  then better  the other-half pair at distance 2, and one column at distance 1 in a block that
               is visited later, behind the wrap of the wave's block order: valid there
  later tie    a unique minimum, then the same distance in another block
  candidates   the match with ham_lo = hm, ham_hi = 0; in its half a column with ham_lo = 0,
               ham_hi = 62, one with ham_lo = 1, ham_hi = 62 and one with ham_lo = hm, ham_hi = 1
  partial      (1100, 1612 columns) the final block is the row's last 12 columns: a match in its
               half 0, one in its half 1, a same-half pair and an other-half pair
The bases: the near pair (pruned), random descriptors and the 10 %-flipped stereo frame (every
wave falls back to the unpruned loop, whose pair step records the half as well).
"""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests.test_search_packed_prune import (BITS, HI62, HINT, INVALID, MASK, N, NODUPES, WORDS,  # noqa: E402
                                            _flipped, _near_pair, _rand, _stereo, gpu_search)
from tests.test_search_stream import _dev_stack, _ties_pair, same  # noqa: E402

ROWS = 256
WIDTHS = [1056, 1100, 1612, 2048, 2080]
KINDS = ["stereo", "ties", "near_planted", "random_planted", "flip10_planted"]
MATCH_WIDTHS = [2048, 1612, 1100]
FUSED_WIDTHS = [2048, 1612]
THRESHOLD = 0.96


def _w(*words):
    return np.array(words, np.uint32)


def sites(W):
    """[(col0, [(col1, xor of a[col0]) ...], expected disparity)] -- see the module docstring."""
    out = []
    for o in ([0, 1024] if W >= 2048 else [0]):
        out += [
            (o + 200, [(o + 192, _w(1, 0, 0, 0)), (o + 193, _w(0, 0, 1, 0))], INVALID),
            (o + 264, [(o + 264, _w(2, 0, 0, 0)), (o + 267, _w(0, 0, 0, 2))], INVALID),
            (o + 330, [(o + 320, _w(0, 4, 0, 0)), (o + 324, _w(0, 0, 4, 0))], INVALID),
            (o + 400, [(o + 387, _w(8, 0, 0, 0)), (o + 415, _w(0, 0, 0, 8))], INVALID),
            (o + 460, [(o + 451, _w(3, 0, 0, 0)), (o + 479, _w(0, 0, 0, 3)), (o + 900, _w(0, 0, 16, 0))], -440),
            (o + 530, [(o + 533, _w(32, 0, 0, 0)), (o + 100, _w(0, 0, 32, 0))], INVALID),
            (o + 600, [(o + 592, _w(0x41, 0, 0, 0)), (o + 593, HI62), (o + 594, HI62 ^ _w(0, 1, 0, 0)),
                       (o + 600, _w(0, 0x82, 1, 0))], 8),
        ]
    if W % 32:
        B = W // 32 * 32
        assert W - B == 12
        out += [
            (1000, [(B + 2, _w(1, 0, 0, 0))], 1000 - (B + 2)),
            (1010, [(B + 5, _w(0, 0, 0, 1))], 1010 - (B + 5)),
            (1020, [(B + 1, _w(0, 2, 0, 0)), (B + 9, _w(0, 0, 2, 0))], INVALID),
            (1030, [(B + 0, _w(4, 0, 0, 0)), (B + 6, _w(0, 0, 0, 4))], INVALID),
        ]
    return out


def _plant(a, b, W):
    b = b.copy()
    for c, cols1, _ in sites(W):
        b[:, c + 3] = ~a[:, c] & MASK   # (the near pair's own match, 0..2 bits away in some rows)
        for c1, x in cols1:
            b[:, c1] = a[:, c] ^ x
    return a, b


def search_case(kind, W):
    """(left, right, stated bits, whether the planted sites' results are known)"""
    seed = 12000 + W
    if kind == "stereo":
        return _stereo(ROWS, W) + (HINT, False)
    if kind == "ties":          # few distinct descriptors: equal halves and repeated minima
        a, b = _ties_pair(ROWS, W, seed)
        return a & MASK, b & MASK, BITS, False
    if kind == "near_planted":
        return _plant(*_near_pair(ROWS, W, seed + 1), W) + (BITS, True)
    if kind == "random_planted":
        rng = np.random.default_rng(seed + 2)
        return _plant(_rand(rng, (ROWS, W, WORDS)) & MASK, _rand(rng, (ROWS, W, WORDS)) & MASK, W) + (BITS, True)
    if kind == "flip10_planted":
        return _plant(*_flipped(ROWS, W, 10, seed + 3), W) + (HINT, False)
    raise ValueError(kind)


_MATCH = {}


def match_case(W):
    if W not in _MATCH:
        from libbicos_amd.synthetic import stereo_stack
        L, R = stereo_stack(N, ROWS, W, np.uint8, dmin=3, drange=40, seed=W)
        L[:, 1, 200:260] = 9    # a flat patch: NaN / low-variance correlations
        _MATCH[W] = (L, R)
    return _MATCH[W]


def gpu_match(eng, L, R):
    from libbicos_amd.device import MatchConfig
    d, c = eng.match(_dev_stack(L), _dev_stack(R), MatchConfig(nxcorr_threshold=THRESHOLD))
    return d.cpu().numpy(), c.cpu().numpy()


def run_all(eng):
    """Every case's maps, keyed by name: what a child process computes under its switch."""
    out = {}
    for W in WIDTHS:
        for kind in KINDS:
            a, b, bits, _ = search_case(kind, W)
            out["search_%s_%d" % (kind, W)] = gpu_search(eng, a, b, bits)
    for W in MATCH_WIDTHS:
        out["match_d_%d" % W], out["match_c_%d" % W] = gpu_match(eng, *match_case(W))
    return out


def _child(tmp_path_factory, name, **switches):
    path = str(tmp_path_factory.mktemp("pkp_eor") / (name + ".npz"))
    env = dict(os.environ, **switches)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", path], env=env,
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def others(gpu, tmp_path_factory):
    """The same inputs with the end of row as it was, through the chunk loop, with both (the
    shared end of row behind the pruned kernel's chunk loop: search_pkp_kernel<AG, false,
    false>), and with the separate agree launch."""
    return {"eor0": _child(tmp_path_factory, "eor0", BICOS_PKP_EOR="0"),
            "chunk_loop": _child(tmp_path_factory, "chunk_loop", BICOS_MX_STREAM="0"),
            "eor0_chunk_loop": _child(tmp_path_factory, "eor0_chunk_loop", BICOS_PKP_EOR="0",
                                      BICOS_MX_STREAM="0"),
            "agree_launch": _child(tmp_path_factory, "agree_launch", BICOS_FUSE_AGREE="0")}


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("W", WIDTHS)
def test_end_of_row_search_equals_oracle_and_parent_form(gpu, oracle, others, W, kind):
    a, b, bits, known = search_case(kind, W)
    assert gpu.search_packed(ROWS, W, WORDS, bits)
    ref = oracle.search(a, b, NODUPES)
    if known:
        for c, cols1, want in sites(W):
            assert (ref[:, c] == want).all(), (c, want, ref[0, c])
    got = gpu_search(gpu, a, b, bits)
    same(got, ref)
    for o in others.values():
        same(got, o["search_%s_%d" % (kind, W)])


@pytest.mark.gpu
@pytest.mark.parametrize("W", MATCH_WIDTHS)
def test_end_of_row_fused_match_equals_oracle_and_agree_launch(gpu, oracle, others, W):
    from libbicos_amd import _lib
    from libbicos_amd.device import MatchConfig
    L, R = match_case(W)
    if W in FUSED_WIDTHS:
        assert gpu.plan(_dev_stack(L), _dev_stack(R), MatchConfig(nxcorr_threshold=THRESHOLD)) & \
            _lib.PLAN_AGREE_IN_SEARCH
        assert gpu.search_packed(ROWS, W, WORDS, HINT, N, fused=True)
    d, c = gpu_match(gpu, L, R)
    rd, rc = oracle.match(L, R, oracle.OracleConfig(nxcorr_threshold=THRESHOLD))
    same(d, rd)
    same(c, rc)
    for o in others.values():
        same(d, o["match_d_%d" % W])
        same(c, o["match_c_%d" % W])


if __name__ == "__main__":
    # child of the `others` fixture: every case through this process's library switches (one of
    # them, or BICOS_PKP_EOR and BICOS_MX_STREAM together)
    assert sys.argv[1] == "--child"
    assert "0" in (os.environ.get("BICOS_PKP_EOR"), os.environ.get("BICOS_MX_STREAM"),
                   os.environ.get("BICOS_FUSE_AGREE"))
    from libbicos_amd import device
    eng = device.Engine(0)
    assert eng.search_packed(ROWS, 2048, WORDS, HINT)
    np.savez(sys.argv[2], **run_all(eng))
