"""The pruned 128-bit NoDuplicates search on packed keys (search_pk.hip search_pkp_kernel):
two Hamming distances per accumulator register; per block of 32 col1 a wide tile (64 col0)
multiplies descriptor words 0 and 1 first, and words 2 and 3 only if ham_lo of some col0 comes
within reach (<=) of that col0's running minimum; a wave whose wide-tile-blocks nearly all
reach falls back to the unpruned packed loop for the rest of its row. The right row is
streamed through LDS as in the one-product kernel.

Every case first asserts through bicos_search_packed that the packed form is what runs, and
is compared byte for byte with the CPU oracle (reference bicos.hpp:50-113), with the
one-product kernel of the same library (BICOS_MX_PACKED=0), with the unpruned loop
(BICOS_MX_PRUNE=0) and with the packed kernel's chunk loop (BICOS_MX_STREAM=0: still packed, the
non-streamed instantiations on every width); the switches are read once per process, so one
child process per setting computes every case.

Shapes: 256 rows, so that 4 tiles per wave are planned with at least two workgroups per row;
widths 1056 (one short stage), 1536, 2048, 2080 (a 32-column last chunk behind two full ones;
its last 32 col0 go to the tail launch), 2081 and 1100 (a partial last block; 2081's last 33
col0 in the tail launch, 1100's last workgroup with idle waves), 3840 at 128 rows (the LDS
stage of the lazy rescans nearly full), and 1024 at 512 rows (one chunk: 4 tiles per wave
without streaming, what the default plan runs for such rows). Descriptors: see search_case.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests.test_search_stream import _dev, _dev_stack, _pack, same  # noqa: E402

WORDS = 4
NODUPES = 1
INVALID = -32768
N = 33
BITS = 126                      # LIMITED n = 33 writes 4n - 6 bits
HINT = 4 * N - 5                # what the match states for them (used_bits)
MASK = np.array([0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0x3FFFFFFF], np.uint32)
LO62 = np.array([0xFFFFFFFF, 0x3FFFFFFF, 0, 0], np.uint32)
HI62 = np.array([0, 0, 0xFFFFFFFF, 0x3FFFFFFF], np.uint32)
SHAPES = [(256, 1056), (256, 1536), (256, 2048), (256, 2080), (256, 2081), (256, 1100), (128, 3840),
          (512, 1024)]
KINDS = ["stereo", "flip2", "flip10", "random", "const", "far", "tie", "mixed"]
MATCH_ROWS = 256


def _rand(rng, shape):
    return rng.integers(0, 2 ** 32, size=shape, dtype=np.uint64).astype(np.uint32)


_STEREO = {}


def _stereo(H, W):
    """LIMITED n = 33 descriptors of the planted stereo frame (the oracle's transform)."""
    if (H, W) not in _STEREO:
        from libbicos_amd.synthetic import stereo_stack
        from oracle import oracle as O
        O.build()
        L, R = stereo_stack(N, H, W)
        _STEREO[H, W] = (O.transform(L, 0, WORDS), O.transform(R, 0, WORDS))
    a, b = _STEREO[H, W]
    return a.copy(), b.copy()


def _flipped(H, W, percent, seed):
    a, b = _stereo(H, W)
    rng = np.random.default_rng(seed)
    flips = np.zeros(b.shape, np.uint32)
    for bit in range(32):
        flips |= (rng.random(b.shape) < percent / 100.0).astype(np.uint32) << np.uint32(bit)
    return a, b ^ (flips & MASK)


def _near_pair(H, W, seed):
    """Random 126-bit descriptors, the right row the left moved by 3 columns with 1 bit in 16
    flipped: every col0 c has its match at col1 c + 3, about 8 bits away, and every other
    column about 63."""
    rng = np.random.default_rng(seed)
    a = _rand(rng, (H, W, WORDS)) & MASK
    flips = _rand(rng, (H, W, WORDS)) & _rand(rng, (H, W, WORDS)) & _rand(rng, (H, W, WORDS)) & \
        _rand(rng, (H, W, WORDS)) & MASK
    return a, a[:, np.roll(np.arange(W), 3)] ^ flips


def tie_sites(W):
    """(col0, second col1): the match of col0 c at c + 3 is made ham_hi = 0, ham = ham_lo = 2;
    the second col1 gets exactly the same distance, again all of it in words 0 and 1, so its
    partial key EQUALS the running minimum when its block is probed. It lies at least 16
    blocks later in the visiting order (downwards from col0, wrapping): below col0 by 600,
    behind the wrap for a low col0 -- and, where the row has one, in the partial last block."""
    sites = [(700, 100), (W - 200, W - 800), (40, W - 50 - (W % 32))]
    if W % 32:
        sites.append((W // 2, W - 1))
    return sites


def _tie_pair(H, W, seed):
    a, b = _near_pair(H, W, seed)
    for i, (c, p2) in enumerate(tie_sites(W)):
        b[:, c + 3] = a[:, c]
        b[:, c + 3, 0] ^= np.uint32(0x5 << i)        # two bits of word 0
        b[:, p2] = a[:, c]
        b[:, p2, 1] ^= np.uint32(0x900 << i)         # two bits of word 1
    return a, b


def mixed_sites(W):
    return [(300, 900), (W - 100, 200)]


def _mixed_pair(H, W, seed):
    """Beside each other, for col0 c: a column with ham_lo = 0 and ham_hi = 62 (its probe says
    0, its distance is 62) and one with ham_lo = 62 and ham_hi = 0 (the largest partial key
    that is final); the match at c + 3 beats both."""
    a, b = _near_pair(H, W, seed)
    for c, p in mixed_sites(W):
        b[:, p] = a[:, c] ^ HI62
        b[:, p + 1] = a[:, c] ^ LO62
    return a, b


def search_case(kind, H, W):
    """(left, right, stated bits)"""
    seed = 11000 + W
    if kind == "stereo":        # nearly every block is pruned
        return _stereo(H, W) + (HINT,)
    if kind == "flip2":         # 2 % of the right bits flipped: still pruned (prune_sim: 0.11)
        return _flipped(H, W, 2, seed) + (HINT,)
    if kind == "flip10":        # 10 %: past the fallback cliff (0.98 of blocks reach)
        return _flipped(H, W, 10, seed + 1) + (HINT,)
    if kind == "random":        # every wave falls back
        rng = np.random.default_rng(seed + 2)
        return _rand(rng, (H, W, WORDS)) & MASK, _rand(rng, (H, W, WORDS)) & MASK, BITS
    if kind == "const":         # a constant row: all ties
        a = np.empty((H, W, WORDS), np.uint32)
        a[:] = np.array([0x5A5A3C0F, 0x12345678, 0x9ABCDEF0, 0x0F0F0F0F], np.uint32) & MASK
        return a, a.copy(), BITS
    if kind == "far":           # every distance is 126: the largest partial sums
        a = np.empty((H, W, WORDS), np.uint32)
        a[:] = MASK
        return a, np.zeros_like(a), BITS
    if kind == "tie":
        return _tie_pair(H, W, seed + 3) + (BITS,)
    if kind == "mixed":
        return _mixed_pair(H, W, seed + 4) + (BITS,)
    raise ValueError(kind)


def gpu_search(eng, a, b, bits):
    return eng.search(_dev(_pack(a)), _dev(_pack(b)), a.shape[1], WORDS, NODUPES, bits=bits).cpu().numpy()


def cfg2_rows():
    from tests.golden.make_frames import FRAMES, frame_stacks
    return frame_stacks(FRAMES["cfg2"], 0, MATCH_ROWS)


def gpu_match(eng, L, R):
    from libbicos_amd.device import MatchConfig
    d, c = eng.match(_dev_stack(L), _dev_stack(R), MatchConfig(nxcorr_threshold=0.96))
    return d.cpu().numpy(), c.cpu().numpy()


def run_all(eng):
    """Every case's maps, keyed by name: what a child process computes under its switches."""
    out = {}
    for H, W in SHAPES:
        for kind in KINDS:
            a, b, bits = search_case(kind, H, W)
            out["search_%s_%d_%d" % (kind, H, W)] = gpu_search(eng, a, b, bits)
    d, c = gpu_match(eng, *cfg2_rows())
    out["match_d"], out["match_c"] = d, c
    return out


def _child(tmp_path_factory, name, **switches):
    path = str(tmp_path_factory.mktemp("pk_prune") / (name + ".npz"))
    env = dict(os.environ, **switches)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", path], env=env,
                       cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def others(gpu, tmp_path_factory):
    """The same inputs through the one-product kernel, the unpruned loop and the packed
    kernel's chunk loop."""
    return (_child(tmp_path_factory, "one_product", BICOS_MX_PACKED="0"),
            _child(tmp_path_factory, "unpruned", BICOS_MX_PRUNE="0"),
            _child(tmp_path_factory, "packed_chunk_loop", BICOS_MX_STREAM="0"))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("H,W", SHAPES)
def test_packed_pruned_search_equals_oracle_and_one_product(gpu, oracle, others, H, W, kind):
    a, b, bits = search_case(kind, H, W)
    assert gpu.search_packed(H, W, WORDS, bits)
    ref = oracle.search(a, b, NODUPES)
    if kind == "tie":       # the same minimum twice: invalid (valid if the reach test were "<")
        for c, p2 in tie_sites(W):
            assert (ref[:, c] == INVALID).all(), (c, p2, ref[0, c])
    if kind == "mixed":
        for c, p in mixed_sites(W):
            assert (ref[:, c] == -3).all(), (c, p, ref[0, c])
    if kind in ("const", "far"):
        assert (ref == INVALID).all()
    got = gpu_search(gpu, a, b, bits)
    same(got, ref)
    for o in others:
        same(got, o["search_%s_%d_%d" % (kind, H, W)])


@pytest.mark.gpu
def test_packed_pruned_fused_match_equals_cfg2_bands(gpu, others):
    """Rows 0..255 of the cfg2 frame through the fused search + agree launch against the
    whole-frame fixture's first four 64-row band hashes."""
    from libbicos_amd import _lib
    from libbicos_amd.device import MatchConfig
    from tests.golden.make_frames import band_hashes
    rec = json.load(open(os.path.join(ROOT, "tests", "golden", "frames.json")))["cfg2"]
    L, R = cfg2_rows()
    W = L.shape[2]
    assert gpu.plan(_dev_stack(L), _dev_stack(R), MatchConfig(nxcorr_threshold=0.96)) & \
        _lib.PLAN_AGREE_IN_SEARCH
    assert gpu.search_packed(MATCH_ROWS, W, WORDS, HINT, N, fused=True)
    d, c = gpu_match(gpu, L, R)
    nb = MATCH_ROWS // rec["band_rows"]
    assert band_hashes(d, rec["band_rows"]) == rec["disparity_bands"][:nb]
    assert band_hashes(c, rec["band_rows"]) == rec["corrmap_bands"][:nb]
    for o in others:
        same(d, o["match_d"])
        same(c, o["match_c"])


def test_packed_query_conditions(blib):
    """bicos_search_packed without an engine (256 CUs): the packed form needs the used bits
    stated and <= 127, 4 tiles per wave, and the raw right row inside the LDS stage."""
    q = lambda rows, cols, words, bits, n=0, fused=0: blib.bicos_search_packed(  # noqa: E731
        None, rows, cols, words, bits, n, fused)
    if os.environ.get("BICOS_MX_PACKED") == "0" or os.environ.get("BICOS_MX_PRUNE") == "0":
        assert q(256, 2048, 4, 127) == 0
        return
    for rows, cols in SHAPES:
        assert q(rows, cols, 4, BITS) == 1 and q(rows, cols, 4, HINT) == 1, (rows, cols)
    assert q(1536, 2048, 4, HINT, N, 1) == 1    # cfg2's fused launch
    assert q(2160, 3840, 4, HINT, N, 1) == 1    # cfg5's
    assert q(256, 2048, 4, 0) == 0              # bits unknown
    assert q(256, 2048, 4, 128) == 0            # 128 used bits: a distance needs 8 bits
    assert q(192, 2048, 4, HINT) == 0           # 2 tiles per wave (a narrow row band)
    assert q(192, 2048, 4, HINT, N, 1) == 0
    assert q(256, 3968, 4, HINT) == 1           # the widest row whose raw words fit
    assert q(256, 4000, 4, HINT) == 0           # too wide for the rescans' LDS stage
    assert q(256, 2048, 8, HINT) == 0 and q(256, 2048, 2, 60) == 0   # other widths
    assert q(256, 2048, 4, HINT, 8, 1) == 0     # no fused launch for this stack depth


if __name__ == "__main__":
    # child of the `others` fixture: every case through this process's library switches
    assert sys.argv[1] == "--child"
    off = os.environ.get("BICOS_MX_PACKED") == "0" or os.environ.get("BICOS_MX_PRUNE") == "0"
    assert off or os.environ.get("BICOS_MX_STREAM") == "0"
    from libbicos_amd import device
    eng = device.Engine(0)
    assert eng.search_packed(256, 2048, WORDS, HINT) == (not off)
    assert eng.search_packed(MATCH_ROWS, 2048, WORDS, HINT, N, fused=True) == (not off)
    np.savez(sys.argv[2], **run_all(eng))
