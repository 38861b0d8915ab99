"""The streamed right row of the 128-bit NoDuplicates search (search_mx.hip search_mx_kernel
ST): a workgroup expands its own 1024-column chunk whole and takes the rest of the row in
512-column stages that alternate between the two halves of the chunk region, the raw
descriptors of the next stage prefetched into registers.

Every case is compared bit for bit with the CPU oracle (reference bicos.hpp:50-113) and with
the chunk loop of the same library (BICOS_MX_STREAM=0, read once per process: one child
process computes all of them).  Widths: around the chunk and stage boundaries (1024-column
chunks, 512-column stages), with and without a partial last block, rows of 2, 3, 4 and 5
chunks, and 3208 / 2081, whose last columns go to the tail launch.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

WORDS = 4
NODUPES = 1
INVALID = -32768
ROWS = 3
WIDTHS = [1024, 1025, 1056, 1535, 1536, 1537, 2047, 2048, 2049, 2081, 2560, 3073, 3208, 4097]
KINDS = ["random", "ties", "planted", "planted_removed"]
IDLE_W = 1100        # 2 tiles per wave: the row's third workgroup holds 76 col0, 6 waves idle
WIDE = (176, 2081)   # enough workgroups for 4 tiles per wave (the full frames' kernel) + tail
MATCH_N, MATCH_ROWS, MATCH_THRESHOLD = 33, 4, 0.96
MATCH_WIDTHS = [1536, 2048, 2049, 3840]


def _random_pair(H, W, seed):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 2 ** 32, size=(H, W, WORDS), dtype=np.uint64).astype(np.uint32)
    flips = rng.integers(0, 2 ** 32, size=(H, W, WORDS), dtype=np.uint64).astype(np.uint32)
    flips &= rng.integers(0, 2 ** 32, size=(H, W, WORDS), dtype=np.uint64).astype(np.uint32)
    flips &= rng.integers(0, 2 ** 32, size=(H, W, WORDS), dtype=np.uint64).astype(np.uint32)
    flips &= rng.integers(0, 2 ** 32, size=(H, W, WORDS), dtype=np.uint64).astype(np.uint32)
    b = a[:, np.roll(np.arange(W), 3)] ^ flips  # a shifted copy, 1 bit in 16 flipped
    return a, b


def _ties_pair(H, W, seed):
    # few distinct descriptors (10 bits spread over the 4 words, both sides drawn alike): most
    # minima are repeated -- exactly or at the same distance -- and some are not
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(2):
        v = rng.integers(0, 1024, size=(H, W), dtype=np.uint32)
        d = np.zeros((H, W, WORDS), np.uint32)
        d[..., 0] = v & 7
        d[..., 1] = ((v >> 3) & 3) << 15
        d[..., 2] = ((v >> 5) & 3) << 30
        d[..., 3] = ((v >> 7) & 7) << 16
        out.append(d)
    return out[0], out[1]


def planted_sites(W):
    """(row, col0, first col1, second col1): the two col1 hold the col0's descriptor with one
    bit flipped each -- the same minimum cost 1 twice. The first lies in the lower (rows 0, 2)
    or upper (row 1) half of chunk 0, the second at the end of the row: another chunk where
    W > 1024 (i = 0 always, the others from 1105 columns), another stage in every case."""
    sites = []
    for r in range(ROWS):
        for i, c in enumerate((7, W // 2, W - 3)):
            sites.append((r, c, (517 if r == 1 else 5) + 40 * i, W - 1 - 40 * i))
    return sites


def _planted_pair(W, seed, removed):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 2 ** 32, size=(ROWS, W, WORDS), dtype=np.uint64).astype(np.uint32)
    b = rng.integers(0, 2 ** 32, size=(ROWS, W, WORDS), dtype=np.uint64).astype(np.uint32)
    for i, (r, c, p1, p2) in enumerate(planted_sites(W)):
        b[r, p1] = a[r, c]
        b[r, p1, 0] ^= np.uint32(1 << (i % 3))
        b[r, p2] = a[r, c]
        b[r, p2, 3] ^= np.uint32(1 << (7 + i % 3))
        if removed:
            b[r, p2] = ~a[r, c]
    return a, b


def search_case(kind, W, H=ROWS):
    seed = 7000 + W
    if kind == "random":
        return _random_pair(H, W, seed)
    if kind == "ties":
        return _ties_pair(H, W, seed + 1)
    return _planted_pair(W, seed + 2, kind == "planted_removed")


def search_cases():
    cases = [(k, W, ROWS) for W in WIDTHS for k in KINDS]
    cases += [(k, IDLE_W, ROWS) for k in ("random", "ties")]
    cases.append(("random", WIDE[1], WIDE[0]))
    return cases


def match_case(W):
    from libbicos_amd.synthetic import stereo_stack
    L, R = stereo_stack(MATCH_N, MATCH_ROWS, W, np.uint8, dmin=3, drange=40, seed=W)
    L[:, 1, 200:260] = 9  # flat patch: NaN / low-variance correlations
    return L, R


def _pack(desc):
    from libbicos_amd import _lib
    H, W, words = desc.shape
    pitch = _lib.lib().bicos_desc_pitch(W, words)
    out = np.zeros((H, pitch), np.uint32)
    out[:, : W * words] = desc.reshape(H, W * words)
    return out.view(np.int32)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def gpu_search(eng, a, b):
    W = a.shape[1]
    return eng.search(_dev(_pack(a)), _dev(_pack(b)), W, WORDS, NODUPES).cpu().numpy()


def _dev_stack(s):
    """The stack on the device with its rows padded to a multiple of 4 bytes (the fused agree
    reads the stacks with dword loads: 2049-byte rows would take the separate agree launch)."""
    import torch
    n, H, W = s.shape
    buf = torch.zeros((n, H, (W + 3) // 4 * 4), dtype=torch.uint8, device="cuda")
    buf[:, :, :W] = _dev(s)
    return buf[:, :, :W]


def gpu_match(eng, L, R, want_plan=0):
    from libbicos_amd.device import MatchConfig
    cfg = MatchConfig(nxcorr_threshold=MATCH_THRESHOLD)
    s0, s1 = _dev_stack(L), _dev_stack(R)
    assert eng.plan(s0, s1, cfg) & want_plan == want_plan
    d, c = eng.match(s0, s1, cfg)
    return d.cpu().numpy(), c.cpu().numpy()


def same(a, b):
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    if not np.array_equal(a.view(np.uint8), b.view(np.uint8)):
        diff = np.argwhere((a.view(np.uint8) != b.view(np.uint8)).reshape(a.shape + (-1,)).any(-1))
        raise AssertionError("%d mismatches, first %s: %r vs %r" % (
            len(diff), diff[0], a[tuple(diff[0])], b[tuple(diff[0])]))


def run_all(eng):
    """Every case's maps, keyed by name: what the child process computes with the chunk loop."""
    out = {}
    for kind, W, H in search_cases():
        a, b = search_case(kind, W, H)
        out["search_%s_%d_%d" % (kind, W, H)] = gpu_search(eng, a, b)
    for W in MATCH_WIDTHS:
        d, c = gpu_match(eng, *match_case(W))
        out["match_d_%d" % W] = d
        out["match_c_%d" % W] = c
    return out


@pytest.fixture(scope="module")
def unstreamed(gpu, tmp_path_factory):
    """The same inputs through BICOS_MX_STREAM=0 (the chunk loop), in one child process."""
    path = str(tmp_path_factory.mktemp("mx_stream") / "chunk_loop.npz")
    env = dict(os.environ, BICOS_MX_STREAM="0")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--chunk-loop", path], env=env,
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("W", WIDTHS)
def test_streamed_search_equals_oracle_and_chunk_loop(gpu, oracle, unstreamed, W, kind):
    a, b = search_case(kind, W)
    ref = oracle.search(a, b, NODUPES)
    if kind.startswith("planted"):
        for r, c, p1, p2 in planted_sites(W):
            # the same minimum twice: invalid; once the second is gone: the first wins
            want = c - p1 if kind == "planted_removed" else INVALID
            assert ref[r, c] == want, (r, c, p1, p2, ref[r, c])
    got = gpu_search(gpu, a, b)
    same(got, ref)
    same(got, unstreamed["search_%s_%d_%d" % (kind, W, ROWS)])


@pytest.mark.parametrize("kind", ["random", "ties"])
def test_streamed_search_idle_waves(gpu, oracle, unstreamed, kind):
    """Waves without col0 (the row's last workgroup) still reach every stage's barrier."""
    a, b = search_case(kind, IDLE_W)
    got = gpu_search(gpu, a, b)
    same(got, oracle.search(a, b, NODUPES))
    same(got, unstreamed["search_%s_%d_%d" % (kind, IDLE_W, ROWS)])


def test_streamed_search_four_tiles_per_wave(gpu, oracle, unstreamed):
    """Enough rows for the full frames' shape (4 tiles per wave, 1024 col0 per workgroup),
    the last 33 columns in the tail launch."""
    H, W = WIDE
    a, b = search_case("random", W, H)
    got = gpu_search(gpu, a, b)
    same(got, oracle.search(a, b, NODUPES))
    same(got, unstreamed["search_random_%d_%d" % (W, H)])


@pytest.mark.parametrize("W", MATCH_WIDTHS)
def test_streamed_fused_match_equals_oracle(gpu, oracle, unstreamed, W):
    from libbicos_amd import _lib
    L, R = match_case(W)
    d, c = gpu_match(gpu, L, R, _lib.PLAN_AGREE_IN_SEARCH)  # (asserts the fused plan)
    rd, rc = oracle.match(L, R, oracle.OracleConfig(nxcorr_threshold=MATCH_THRESHOLD))
    same(d, rd)
    same(c, rc)
    same(d, unstreamed["match_d_%d" % W])
    same(c, unstreamed["match_c_%d" % W])


if __name__ == "__main__":
    # child of the `unstreamed` fixture: every case through this process's library switch
    assert sys.argv[1] == "--chunk-loop" and os.environ.get("BICOS_MX_STREAM") == "0"
    from libbicos_amd import device
    np.savez(sys.argv[2], **run_all(device.Engine(0)))
