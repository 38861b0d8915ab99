"""The packed LIMITED transform (kernels.hip transform_limited_pk_kernel: two pixels per 32-bit
register, four adjacent columns per lane from one dword load per plane) against the oracle, bit
for bit, beside the one-pixel kernel it replaces where it applies.

Which kernel runs is asserted, never assumed (bicos_transform_kernel, no HIP call): the packed
one takes u8 LIMITED stacks of n in 9 12 17 24 33 40 48 65 whose base(s), row pitch and plane
pitch are multiples of 4 bytes and which fit the 256 MiB last-level cache together (the size
rule: tests/test_transform_pk.py); every other n and every other view keeps the one-pixel kernel.
So the same stack at base residue 0 and at base residue 1 runs one kernel each, and both must
give the oracle's words.

  sizes      rows 1 and 3 x cols 1 2 3 4 5 7 255 256 257 1023 1025 1027 (the row's last dword
             partly or wholly past `cols`, one and two workgroups per row) x every built n and
             the n on either side of it (66 is no LIMITED stack size: 65 has one neighbour) x
             random, constant, 0/255 alternating and neighbour-extremes inputs
  views      base x row-pitch x plane-pitch residues 0..3, random guard bytes: only the
             all-aligned view reports packed; guards and inputs untouched
  sentinel   the descriptor rows' words past cols * words keep a sentinel, the bytes around the
             descriptor buffer their pattern
  match      both stacks in one launch through match(), aligned and with stack1 off by one
  frame      640 x 480, n = 33: BICOS_TRANSFORM_PK=0 and =1, each in a fresh child process,
             give identical disparity and corrmap
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from libbicos_amd.synthetic import random_stack, stereo_stack
from tests import view_cases as V
from tests.test_gpu_parity import same

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILT = (9, 12, 17, 24, 33, 40, 48, 65)
NEAR = tuple(sorted({m for n in BUILT for m in (n - 1, n, n + 1) if m <= 65}))
ROWS = (1, 3)
COLS = (1, 2, 3, 4, 5, 7, 255, 256, 257, 1023, 1025, 1027)
PATTERNS = ("random", "constant", "alternating", "extremes")
SENTINEL = 0x5A3CA5C3


def pattern(kind, n, H, W, seed):
    """[n, H, W] u8. The four columns of a dword share two registers as (0, 2) and (1, 3):
    `extremes` puts columns c % 4 in (0, 3) on a rising ramp with a 255 at the end and columns
    c % 4 in (1, 2) on the falling mirror image, so both pixels of either register (and every
    two neighbours) sit at opposite extremes, and alternates 0-flat / 255-flat rows below."""
    t = np.arange(n)[:, None, None]
    y = np.arange(H)[None, :, None]
    c = np.arange(W)[None, None, :]
    if kind == "random":
        return random_stack(n, H, W, np.uint8, seed=seed)
    if kind == "constant":
        return np.broadcast_to((c * 37 + y * 11) % 256, (n, H, W)).astype(np.uint8)
    if kind == "alternating":
        return (((t + c + y) % 2) * 255).astype(np.uint8)
    assert kind == "extremes"
    up = np.where(t == n - 1, 255, t * 3)
    rising = (c % 4 == 0) | (c % 4 == 3)
    ramp = np.where(rising, up, 255 - up)
    flat = np.where(rising, 0, 255) + 0 * t
    return np.where(y % 2 == 0, ramp, flat).astype(np.uint8)


def aligned_pitches(H, W):
    rp = (W + 3) // 4 * 4 + 4
    return rp, H * rp


def run_transform(gpu, view, H, W, words):
    """the view's descriptors [H, W, words]; the row tails and the buffer's surroundings intact"""
    import torch
    pitch = gpu._L.bicos_desc_pitch(W, words)
    out, intact = V.out_view((H, pitch), torch.int32, 0)
    out.fill_(np.int32(SENTINEL))
    gpu.transform(view, 0, words, out=out)
    r = out.cpu().numpy().view(np.uint32)
    assert intact(), "transform wrote outside its descriptor buffer"
    assert (r[:, W * words:] == SENTINEL).all(), "transform wrote past a row's descriptors"
    return r[:, :W * words].reshape(H, W, words).copy()


@pytest.mark.parametrize("H", ROWS)
@pytest.mark.parametrize("n", NEAR)
def test_sizes_patterns_and_neighbouring_stack_sizes(gpu, oracle, n, H):
    words = oracle.desc_words(n, 0)
    for W in COLS:
        rp, pp = aligned_pitches(H, W)
        for kind in PATTERNS:
            s = pattern(kind, n, H, W, seed=1000 * n + W)
            ref = oracle.transform(s, 0, words)
            for base in (0, 1):
                buf, view = V.stack_view(s, base, rp, pp, "random", seed=W + base)
                snap = buf.clone()
                want = 1 if n in BUILT and base == 0 else 0
                assert gpu.transform_kernel(view) == want, (n, W, base)
                same(run_transform(gpu, view, H, W, words), ref)
                assert V.unchanged(buf, snap)


@pytest.mark.parametrize("n", [9, 17, 33, 48])
def test_views_only_the_all_aligned_one_is_packed(gpu, oracle, n):
    H, W = 3, 301
    words = oracle.desc_words(n, 0)
    s = random_stack(n, H, W, np.uint8, seed=77 + n)
    s[:, -1, -3:] = 255          # the stack's last pixels: the end of the buffer resource
    s[-1, -1, -1] = 254
    ref = oracle.transform(s, 0, words)
    packed = 0
    for base in range(4):
        for row_mod in range(4):
            for plane_mod in range(4):
                rp = W + 3
                while rp % 4 != row_mod:
                    rp += 1
                pp = H * rp
                while pp % 4 != plane_mod:
                    pp += 1
                res = []
                for guard in ("random", "ones"):
                    buf, view = V.stack_view(s, base, rp, pp, guard, seed=base + 4 * row_mod)
                    snap = buf.clone()
                    aligned = base == 0 and row_mod == 0 and plane_mod == 0
                    assert gpu.transform_kernel(view) == int(aligned), (base, row_mod, plane_mod)
                    packed += int(aligned)
                    res.append(run_transform(gpu, view, H, W, words))
                    assert V.unchanged(buf, snap)
                same(res[0], ref)
                same(res[1], ref)
    assert packed == 2


def test_wider_descriptor_keeps_the_one_pixel_kernel(gpu, oracle):
    """The packed kernel is built at each size's narrowest descriptor only."""
    n, H, W = 9, 3, 261
    s = random_stack(n, H, W, np.uint8, seed=5)
    rp, pp = aligned_pitches(H, W)
    _, view = V.stack_view(s, 0, rp, pp, "random")
    assert gpu.transform_kernel(view, words=1) == 1
    for words in (2, 4, 8):
        assert gpu.transform_kernel(view, words=words) == 0
        same(run_transform(gpu, view, H, W, words), oracle.transform(s, 0, words))
    assert gpu.transform_kernel(view, mode=1, words=2) == 0        # FULL
    u16 = V.stack_view(random_stack(n, H, W, np.uint16, seed=6), 0, rp, pp, "random")[1]
    assert gpu.transform_kernel(u16) == 0


@pytest.mark.parametrize("n", [9, 33, 40])
def test_both_stacks_in_one_launch_through_match(gpu, oracle, n):
    from libbicos_amd.device import MatchConfig
    H, W = 6, 333
    L, R = stereo_stack(n, H, W, np.uint8, dmin=3, drange=30, seed=n + W)
    L[:, -1, -1] = 255 - np.arange(n) % 4
    R[:, -1, -1] = np.arange(n) % 6
    cfg = dict(nxcorr_threshold=0.9)
    rd, rc = oracle.match(L, R, oracle.OracleConfig(**cfg))
    rp, pp = aligned_pitches(H, W)
    for bases, want in (((0, 0), 1), ((0, 1), 0), ((1, 0), 0)):
        (_, v0), (_, v1) = [V.stack_view(s, b, rp, pp, "random", seed=i)
                            for i, (s, b) in enumerate(zip((L, R), bases))]
        assert gpu.transform_kernel(v0, v1) == want, bases
        d, c = gpu.match(v0, v1, MatchConfig(**cfg))
        same(d.cpu().numpy(), rd)
        same(c.cpu().numpy(), rc)


CHILD = r"""
import sys
import numpy as np
import torch
from libbicos_amd import device
from libbicos_amd.synthetic import stereo_stack
L, R = stereo_stack(33, 480, 640)
eng = device.Engine(0)
l, r = torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()
print("kernel", eng.transform_kernel(l, r))
d, c = eng.match(l, r, device.MatchConfig(nxcorr_threshold=0.9))
torch.cuda.synchronize()
np.savez(sys.argv[1], d=d.cpu().numpy(), c=c.cpu().numpy())
"""


def test_whole_frame_with_and_without_the_packed_kernel(tmp_path):
    got = {}
    for pk in ("0", "1"):
        env = dict(os.environ, BICOS_TRANSFORM_PK=pk, PYTHONPATH=ROOT)
        path = str(tmp_path / ("frame%s.npz" % pk))
        r = subprocess.run([sys.executable, "-c", CHILD, path], env=env, cwd=ROOT,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        assert r.stdout.split() == ["kernel", pk], r.stdout
        got[pk] = np.load(path)
    for key in ("d", "c"):
        a, b = got["0"][key], got["1"][key]
        assert a.shape == (480, 640) and a.dtype == b.dtype
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), key
    assert np.isfinite(got["1"]["d"]).mean() > 0.5      # (a frame that matched, not a blank one)
