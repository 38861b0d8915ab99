"""The descriptor entries on descriptors kept at a WORD offset inside a larger buffer.

bicos_search_device, bicos_search_device_range and bicos_search_agree_device take any uint32_t*;
bicos_desc_pitch rounds rows to 16 bytes and the engine's own buffers are 256-byte aligned, so
the branches for a row that is not 16-byte aligned (search_pk.hip pk_copy_row's scalar copy, the
pruned packed search's end of row without its early dwordx4 loads) and the matrix-core kernels'
four-words-per-column loads at a 4-byte address only run for a caller who keeps descriptors in
a pool. Here desc0 and desc1 lie, independently, 0..3 words past a 16-byte boundary
(tests/view_cases.py desc_view: random guard words around them), the int16 map goes into an
out_view 2 bytes past a boundary, and every result must equal the oracle's on the unpadded
descriptors AND the same search on 16-byte aligned copies, byte for byte, with the inputs and
all guards unchanged.

Kernels are forced with Engine.tune as tests/test_gpu_parity.py test_pk_search /
test_search_tail_workgroups do (0: the default plan -- packed keys for 32 / 64-bit descriptors,
one-product keys above; 64 with 4 tiles per wave: main + tail launches, and for 128-bit
descriptors with a used-bits hint <= 127 the pruned packed search, asserted through
bicos_search_packed as tests/test_search_packed_prune.py does; 65: one-product keys; 68: the
packed search for 128-bit descriptors). Descriptor bases that are not 4-byte aligned are no
legal uint32_t* and out of scope.
"""
import functools

import numpy as np
import pytest

from libbicos_amd.synthetic import stereo_stack
from tests import view_cases as V
from tests.test_gpu_parity import same
from tests.test_range_api import search_range

pytestmark = pytest.mark.gpu

ROWS = 3
PAIRS = [(0, 0), (1, 1), (0, 3), (2, 0), (3, 2)]       # word offsets of (desc0, desc1)
WIDTHS = [33, 700, 1281, 2049]  # one LDS chunk; several, ragged; a tail workgroup; chunks + 1
FLAGS = [(0, -1), (1, -1), (2, 1), (3, 1)]


def _mask(words, bits):
    m = np.zeros(words, np.uint32)
    for w in range(words):
        lo = 32 * w
        m[w] = 0 if lo >= bits else (0xFFFFFFFF if bits - lo >= 32 else (1 << (bits - lo)) - 1)
    return m


@functools.lru_cache(maxsize=None)
def descriptors(words, W, bits):
    """tests/test_gpu_parity.py test_search_tail_workgroups' rows: planted matches 9 columns
    away with a few flipped bits (col0 W-10 matches the row's LAST col1: the last words of the
    right row decide a pixel), a row where every col1 ties, a low-entropy row"""
    rng = np.random.default_rng(W * 7 + words + bits)
    a = rng.integers(0, 2 ** 32, size=(ROWS, W, words), dtype=np.uint64).astype(np.uint32)
    b = a[:, np.roll(np.arange(W), 9)] ^ (rng.random((ROWS, W, words)) < 0.03).astype(np.uint32)
    b[1, :, :] = b[1, :1, :]
    a[2] &= 0x0F0F0F0F
    b[2] &= 0x0F0F0F0F
    m = _mask(words, bits if bits else 32 * words)
    if words == 8:
        m[7] &= 0x7FFFFFFF        # bit 255 stays clear (include/bicos_c.h)
    return a & m, b & m


def pack(desc, pitch):
    H, W, words = desc.shape
    out = np.zeros((H, pitch), np.uint32)
    out[:, :W * words] = desc.reshape(H, W * words)
    return out.view(np.int32)


def host(t):
    return t.cpu().numpy()


def on_desc_views(gpu, a, b, W, words, call):
    """call(desc0 view, desc1 view, out) at every pair of word offsets -> the int16 maps;
    inputs and guards unchanged, the output's guards intact, every map byte-identical to the
    one of the 16-byte aligned pair (the first)"""
    import torch
    pitch = gpu._L.bicos_desc_pitch(W, words)
    maps = []
    for o0, o1 in PAIRS:
        buf0, v0 = V.desc_view(pack(a, pitch), o0, seed=3)
        buf1, v1 = V.desc_view(pack(b, pitch), o1, seed=4)
        assert v0.data_ptr() % 16 == 4 * o0 and v1.data_ptr() % 16 == 4 * o1
        snap0, snap1 = buf0.clone(), buf1.clone()
        out, out_ok = V.out_view((ROWS, W), torch.int16, 1)
        assert out.data_ptr() % 16 == 2
        call(v0, v1, out)
        maps.append(host(out))
        assert out_ok(), "the search wrote outside its map (offsets %d, %d)" % (o0, o1)
        assert V.unchanged(buf0, snap0) and V.unchanged(buf1, snap1), "descriptors were written"
    for (o0, o1), m in zip(PAIRS[1:], maps[1:]):
        assert np.array_equal(m, maps[0]), "word offsets (%d, %d) change the result" % (o0, o1)
    return maps[0]


# (words, used-bits hint, tune settings). bits: those of test_pk_search / test_search_tail_workgroups
SEARCH_CASES = [
    (1, 27, [(0, 0, 0, 0), (64, 4, 8, 0), (65, 4, 8, 0)]),
    (1, 32, [(0, 0, 0, 0), (64, 4, 8, 0)]),
    (2, 61, [(0, 0, 0, 0), (64, 4, 8, 0)]),
    (2, 64, [(0, 0, 0, 0), (65, 4, 8, 0)]),
    (4, 99, [(64, 4, 8, 0), (68, 4, 8, 0)]),
    (4, 126, [(0, 0, 0, 0), (64, 4, 8, 0), (68, 8, 8, 0), (65, 2, 8, 0), (65, 4, 8, 0)]),
    (4, 0, [(0, 0, 0, 0), (64, 4, 8, 0)]),
    (8, 0, [(0, 0, 0, 0), (64, 4, 8, 0)]),
    (8, 150, [(0, 0, 0, 0), (64, 4, 8, 0)]),       # 3 K-steps; flags 2: Consistency in one launch
]


@pytest.mark.parametrize("W", WIDTHS)
@pytest.mark.parametrize("words,bits,tunes", SEARCH_CASES)
def test_search_desc_views(gpu, oracle, monkeypatch, words, bits, tunes, W):
    monkeypatch.delenv("BICOS_LR_ONE_PASS", raising=False)
    a, b = descriptors(words, W, bits)
    try:
        for flags, lr in FLAGS:
            ref = oracle.search(a, b, flags, lr)
            if flags == 1:      # the planted match in the row's last column is kept
                assert ref[0, W - 10] == -9
            for s in tunes:
                gpu.tune(*s)
                # the pruned packed search: 128-bit, a hint <= 127, 4 tiles per wave
                # (variant 64 or 65: both plan the any-order one-product keys it replaces)
                pruned = words == 4 and 0 < bits <= 127 and s[0] in (64, 65) and s[1] == 4
                assert gpu.search_packed(ROWS, W, words, bits) == pruned, (s, bits)
                got = on_desc_views(gpu, a, b, W, words, lambda v0, v1, out: gpu.search(
                    v0, v1, W, words, flags, lr, out=out, bits=bits))
                same(got, ref)
    finally:
        gpu.tune(0, 0, 0, 0)


# the windowed search (search_range.hip): every flag combination, a window that cuts the
# planted disparity -9 out and one that holds it, tile and wave counts through the tuning
@pytest.mark.parametrize("W", [33, 700])
@pytest.mark.parametrize("words,bits", [(1, 32), (2, 61), (4, 126), (8, 0), (8, 150)])
def test_search_range_desc_views(gpu, words, bits, W):
    a, b = descriptors(words, W, bits)
    try:
        for flags, lr in FLAGS:
            for lo, hi in ((-30, 25), (0, 40)):
                ref = search_range(a, b, flags, lo, hi, lr)
                for s in [(0, 0, 0, 0), (64, 4, 4, 0)]:
                    gpu.tune(*s)
                    got = on_desc_views(gpu, a, b, W, words, lambda v0, v1, out: gpu.search(
                        v0, v1, W, words, flags, lr, out=out, bits=bits, disparity_range=(lo, hi)))
                    same(got, ref)
    finally:
        gpu.tune(0, 0, 0, 0)


# bicos_search_agree_device: the match from its search on, over descriptor views (the stacks
# contiguous: tests/test_stack_views_gpu.py moves those). n = 8: packed keys + fused agree;
# n = 33: one-product keys + fused agree; n = 40: Consistency in one launch; n = 17 u16.
@pytest.mark.parametrize("n,dt,W,H", [(8, np.uint8, 304, 6), (33, np.uint8, 336, 6), (40, np.uint8, 301, 5),
                                      (17, np.uint16, 150, 5)])
def test_match_from_desc_views(gpu, oracle, monkeypatch, n, dt, W, H):
    import torch
    from libbicos_amd.device import MatchConfig, descriptor_words
    monkeypatch.delenv("BICOS_LR_ONE_PASS", raising=False)
    L, R = stereo_stack(n, H, W, dt, dmin=3, drange=30, seed=n + W)
    L[:, 1, 40:70] = 5
    s0 = torch.from_numpy(L.view(np.int16) if L.itemsize == 2 else L).cuda()
    s1 = torch.from_numpy(R.view(np.int16) if R.itemsize == 2 else R).cuda()
    words = descriptor_words(n, 0)
    pitch = gpu._L.bicos_desc_pitch(W, words)
    d0, d1 = oracle.transform(L, 0, words), oracle.transform(R, 0, words)
    for cfg in (dict(nxcorr_threshold=0.9), dict(nxcorr_threshold=None),
                dict(nxcorr_threshold=0.6, variant=1, max_lr_diff=1),
                dict(nxcorr_threshold=0.7, min_variance=1.0, subpixel_step=0.25),
                dict(nxcorr_threshold=None, variant=1, max_lr_diff=2, no_dupes=True)):
        rd, rc = oracle.match(L, R, oracle.OracleConfig(**cfg))
        nxc = cfg["nxcorr_threshold"] is not None
        first = None
        for o0, o1 in PAIRS:
            buf0, v0 = V.desc_view(pack(d0, pitch), o0, seed=5)
            buf1, v1 = V.desc_view(pack(d1, pitch), o1, seed=6)
            snap0, snap1 = buf0.clone(), buf1.clone()
            out, out_ok = V.out_view((H, W), torch.float32 if nxc else torch.int16, 1)
            corr, corr_ok = V.out_view((H, W), torch.float32, 2) if nxc else (None, None)
            gpu.search_agree(v0, v1, s0, s1, MatchConfig(**cfg), out=out, corrmap=corr)
            got = (host(out), host(corr) if nxc else None)
            assert out_ok() and (corr_ok is None or corr_ok())
            assert V.unchanged(buf0, snap0) and V.unchanged(buf1, snap1)
            same(got[0], rd)
            if nxc:
                same(got[1], rc)
            if first is None:
                first = got
            else:
                assert np.array_equal(got[0].view(np.uint8), first[0].view(np.uint8)), (o0, o1)
                assert not nxc or np.array_equal(got[1].view(np.uint8), first[1].view(np.uint8))
