"""tests/view_cases.py itself, on CPU tensors of the same construction: the view equals its
source, the requested residue past a 16-byte boundary is met, guards of at least GUARD_MIN
elements lie on both sides, and the gaps between rows and between planes hold the guard
pattern -- so that the GPU tests built on it (tests/test_stack_views_gpu.py,
tests/test_desc_views_gpu.py) really hand the kernels what they claim to."""
import numpy as np
import pytest
import torch

from tests import view_cases as V


def _flat(buf):
    a = buf.numpy()
    return a.view({2: np.uint16, 4: np.uint32}.get(a.itemsize, np.uint8)) if a.dtype.kind == "i" else a


def _stack(dt, n=3, H=5, W=13, seed=1):
    rng = np.random.default_rng(seed)
    return rng.integers(0, np.iinfo(dt).max + 1, size=(n, H, W), dtype=np.uint64).astype(dt)


@pytest.mark.parametrize("guard", V.GUARDS)
@pytest.mark.parametrize("dt,base", [(np.uint8, b) for b in range(5)] + [(np.uint16, b) for b in range(4)])
@pytest.mark.parametrize("row_mod,plane_odd", [(0, False), (1, True), (2, False), (3, True), (0, True)])
def test_stack_view(dt, base, row_mod, plane_odd, guard):
    isz = np.dtype(dt).itemsize
    if (row_mod * 1) % isz:
        row_mod -= 1                      # u16: byte residues 0 and 2
    arr = _stack(dt)
    n, H, W = arr.shape
    rp, pp = V.pitches(H, W, row_mod, plane_odd, isz)
    assert (rp * isz) % 4 == row_mod
    if plane_odd:
        assert pp % rp != 0 and (pp - H * rp) % 2 == 1
        assert isz != 1 or pp % 4 != 0
    buf, view = V.stack_view(arr, base, rp, pp, guard, device="cpu", seed=7)
    assert buf.dim() == 1 and tuple(view.shape) == arr.shape
    assert view.stride() == (pp, rp, 1)
    assert view.data_ptr() % 16 == base * isz
    got = view.numpy()
    assert np.array_equal(got.view(arr.dtype), arr)
    flat = _flat(buf)
    off = view.storage_offset()
    span = (n - 1) * pp + (H - 1) * rp + W
    assert off >= V.GUARD_MIN and flat.size - (off + span) >= V.GUARD_MIN
    pix = V.pixel_mask(flat.size, off, arr.shape, (pp, rp, 1))
    assert not pix[:off].any() and not pix[off + span:].any()
    # row gaps and plane gaps exist and hold guard elements
    for t in range(n):
        for y in range(H - 1):
            gap = slice(off + t * pp + y * rp + W, off + t * pp + (y + 1) * rp)
            assert gap.stop - gap.start == rp - W >= 3 and not pix[gap].any()
        if t + 1 < n:
            gap = slice(off + t * pp + (H - 1) * rp + W, off + (t + 1) * pp)
            assert gap.stop > gap.start and not pix[gap].any()
    g = flat[~pix]
    top = np.iinfo(arr.dtype).max
    if guard == "zeros":
        assert (g == 0).all()
    elif guard == "ones":
        assert (g == top).all()
        assert (buf.numpy().view(np.uint8).reshape(-1, isz)[~pix] == 0xFF).all()
    else:
        assert len(np.unique(g)) > min(50, top // 2)           # not a constant
        i = np.nonzero(~pix)[0]
        left = i[(i > 0) & pix[np.maximum(i - 1, 0)]]          # guard elements behind a pixel
        right = i[(i + 1 < flat.size) & pix[np.minimum(i + 1, flat.size - 1)]]
        assert left.size >= n * H and right.size >= n * H
        assert (flat[left] != flat[left - 1]).all()
        assert (flat[right] != flat[right + 1]).all()
        # seeded: the same call gives the same buffer contents
        buf2, view2 = V.stack_view(arr, base, rp, pp, guard, device="cpu", seed=7)
        assert np.array_equal(_flat(buf2)[view2.storage_offset() - 8:][:span + 16],
                              flat[off - 8:][:span + 16])


def test_stack_view_rejects_overlapping_pitches():
    arr = _stack(np.uint8)
    with pytest.raises(AssertionError):
        V.stack_view(arr, 0, 12, 200, "zeros", device="cpu")      # row pitch < W
    with pytest.raises(AssertionError):
        V.stack_view(arr, 0, 16, 4 * 16, "zeros", device="cpu")   # planes overlap


@pytest.mark.parametrize("word_offset", [0, 1, 2, 3])
def test_desc_view(word_offset):
    rng = np.random.default_rng(3)
    desc = rng.integers(0, 2 ** 32, size=(3, 44), dtype=np.uint64).astype(np.uint32)
    buf, view = V.desc_view(desc.view(np.int32), word_offset, device="cpu", seed=5)
    assert view.is_contiguous() and tuple(view.shape) == desc.shape and view.dtype == torch.int32
    assert view.data_ptr() % 16 == 4 * word_offset
    assert np.array_equal(view.numpy().view(np.uint32), desc)
    flat = buf.numpy().view(np.uint32)
    off = view.storage_offset()
    assert off >= V.GUARD_MIN and flat.size - (off + desc.size) >= V.GUARD_MIN
    lead, tail = flat[:off], flat[off + desc.size:]
    assert len(np.unique(lead)) > 32 and len(np.unique(tail)) > 32  # random words, both sides
    assert lead[-1] != desc[0, 0] and tail[0] != desc[-1, -1]


@pytest.mark.parametrize("dtype,elem_offset", [(torch.int16, 1), (torch.float32, 1), (torch.float32, 2),
                                               (torch.float64, 1), (torch.int32, 1), (torch.int16, 0)])
def test_out_view(dtype, elem_offset):
    out, intact = V.out_view((4, 9), dtype, elem_offset, device="cpu", seed=2)
    assert out.is_contiguous() and tuple(out.shape) == (4, 9) and out.dtype == dtype
    assert out.data_ptr() % 16 == elem_offset * out.element_size()
    assert intact()
    before = out.clone()
    out.fill_(3)                       # writing the tensor itself leaves the guards alone
    assert intact() and not torch.equal(out, before)
    base = out.untyped_storage()
    raw = torch.empty(0, dtype=torch.uint8).set_(base)
    first = out.data_ptr() - raw.data_ptr()
    assert first >= V.GUARD_MIN * out.element_size()
    assert raw.numel() - (first + out.numel() * out.element_size()) >= V.GUARD_MIN * out.element_size()
    for i in (first - 1, first + out.numel() * out.element_size()):   # one byte either side
        keep = int(raw[i])
        raw[i] = keep ^ 0x5A
        assert not intact()
        raw[i] = keep
        assert intact()


def test_unchanged():
    arr = _stack(np.uint8)
    buf, view = V.stack_view(arr, 1, 16, 5 * 16 + 7, "random", device="cpu")
    snap = buf.clone()
    assert V.unchanged(buf, snap)
    buf[3] += 1                         # a guard element
    assert not V.unchanged(buf, snap)
