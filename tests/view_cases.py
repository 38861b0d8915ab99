"""Views of larger buffers for the stage tests: an image stack cut out of a pitched frame at any
base, packed descriptors at a word offset, dense outputs inside a guarded allocation.

include/bicos_c.h addresses a stack as base[t*plane_pitch + y*row_pitch + x] with a free base and
free pitches, takes any uint32_t* for descriptors and any dense map for its outputs. These
helpers build exactly such arguments, with a GUARD PATTERN in every byte that is not a pixel (in
front of the view, behind it, between rows, between planes), so that a kernel which takes a pad
byte for a pixel computes something the oracle -- which only ever sees the contiguous source --
does not.

Plain module, no fixtures. The same construction runs on CPU tensors (tests/test_view_cases.py).
Offsets ("base", "word_offset", "elem_offset") count ELEMENTS from a 16-byte boundary.
"""
import numpy as np
import torch

GUARD_MIN = 64          # guard elements on either side of a view, at least
GUARDS = ("zeros", "ones", "random")


def _torch_dtype(dt):
    dt = np.dtype(dt)
    return {np.dtype(np.uint8): torch.uint8, np.dtype(np.uint16): torch.int16,
            np.dtype(np.int16): torch.int16, np.dtype(np.int32): torch.int32,
            np.dtype(np.uint32): torch.int32, np.dtype(np.float32): torch.float32,
            np.dtype(np.float64): torch.float64}[dt]


def _host_bits(a):
    """numpy array as torch sees it (uint16 / uint32 bits in int16 / int32)."""
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:
        return a.view(np.int16)
    if a.dtype == np.uint32:
        return a.view(np.int32)
    return a


def _offset(ptr, itemsize, residue_bytes):
    """smallest element offset >= GUARD_MIN whose address is residue_bytes past a 16-byte
    boundary"""
    assert 0 <= residue_bytes < 16 and residue_bytes % itemsize == 0, (residue_bytes, itemsize)
    assert ptr % itemsize == 0
    off = GUARD_MIN
    while (ptr + off * itemsize) % 16 != residue_bytes:
        off += 1
    return off


def pixel_mask(total, offset, shape, strides):
    """bool [total]: which elements of the flat buffer the strided view covers"""
    idx = np.asarray(offset, np.int64)
    for size, stride in zip(shape, strides):
        idx = idx[..., None] + np.arange(size, dtype=np.int64) * stride
    mask = np.zeros(total, bool)
    mask[idx.reshape(-1)] = True
    assert mask.sum() == int(np.prod(shape)), "the view overlaps itself"
    return mask


def _fill_guard(host, pix, guard, seed):
    """the guard pattern into every element of `host` (unsigned) that is not a pixel. random:
    seeded, and no guard element equals a pixel directly beside it in memory"""
    assert guard in GUARDS, guard
    g = ~pix
    top = np.iinfo(host.dtype).max
    if guard == "zeros":
        host[g] = 0
    elif guard == "ones":
        host[g] = top
    else:
        rng = np.random.default_rng(seed)
        host[g] = rng.integers(0, int(top) + 1, size=int(g.sum()), dtype=np.uint64).astype(host.dtype)
        left = np.zeros_like(pix)
        left[1:] = pix[:-1]           # the element before is a pixel
        right = np.zeros_like(pix)
        right[:-1] = pix[1:]
        prev = np.roll(host, 1)
        nxt = np.roll(host, -1)
        for _ in range(3):            # three candidate values against two neighbours
            bad = g & ((left & (host == prev)) | (right & (host == nxt)))
            if not bad.any():
                break
            host[bad] += 1            # (wraps)
        bad = g & ((left & (host == prev)) | (right & (host == nxt)))
        assert not bad.any()


def stack_view(arr, base, row_pitch, plane_pitch, guard, device="cuda", seed=0):
    """(buffer, view): the contiguous numpy [n, H, W] u8 / u16 stack `arr` as a strided view
    (strides plane_pitch, row_pitch, 1 elements) of one flat buffer filled with the guard
    pattern, view.data_ptr() % 16 == base * itemsize."""
    arr = np.ascontiguousarray(arr)
    assert arr.ndim == 3 and arr.dtype in (np.uint8, np.uint16), (arr.shape, arr.dtype)
    n, H, W = arr.shape
    isz = arr.itemsize
    assert row_pitch >= W and plane_pitch >= (H - 1) * row_pitch + W, (row_pitch, plane_pitch)
    span = (n - 1) * plane_pitch + (H - 1) * row_pitch + W
    total = span + 2 * GUARD_MIN + 16
    buf = torch.empty(total, dtype=_torch_dtype(arr.dtype), device=device)
    off = _offset(buf.data_ptr(), isz, base * isz)
    assert off >= GUARD_MIN and total - (off + span) >= GUARD_MIN
    shape, strides = (n, H, W), (plane_pitch, row_pitch, 1)
    pix = pixel_mask(total, off, shape, strides)
    host = np.zeros(total, arr.dtype)
    host[pix] = arr.reshape(-1)       # (mask order == view order: strides descend)
    _fill_guard(host, pix, guard, seed)
    buf.copy_(torch.from_numpy(_host_bits(host)))
    view = torch.as_strided(buf, shape, strides, off)
    assert view.data_ptr() % 16 == base * isz
    assert view.data_ptr() == buf.data_ptr() + off * isz
    return buf, view


def desc_view(desc, word_offset, device="cuda", seed=0):
    """(buffer, view): the packed [rows, bicos_desc_pitch] int32 / uint32 numpy array `desc` as
    a contiguous 2-D slice of one flat int32 buffer, starting word_offset words past a 16-byte
    boundary, random guard words around it."""
    desc = np.ascontiguousarray(desc)
    assert desc.ndim == 2 and desc.dtype in (np.int32, np.uint32), (desc.shape, desc.dtype)
    rows, pitch = desc.shape
    total = rows * pitch + 2 * GUARD_MIN + 4
    buf = torch.empty(total, dtype=torch.int32, device=device)
    off = _offset(buf.data_ptr(), 4, 4 * word_offset)
    pix = np.zeros(total, bool)
    pix[off:off + rows * pitch] = True
    host = np.zeros(total, np.uint32)
    host[pix] = desc.reshape(-1).view(np.uint32)
    _fill_guard(host, pix, "random", seed)
    buf.copy_(torch.from_numpy(host.view(np.int32)))
    view = buf[off:off + rows * pitch].view(rows, pitch)
    assert view.is_contiguous() and view.data_ptr() % 16 == 4 * word_offset
    return buf, view


def out_view(shape, dtype, elem_offset, device="cuda", seed=0):
    """(out, guards_intact): a dense tensor of `shape` / torch `dtype` inside a byte buffer of a
    random pattern, out.data_ptr() % 16 == elem_offset * itemsize. The tensor itself starts out
    as pattern too (float maps: NaNs or odd numbers, never a result). guards_intact() is True
    while every byte outside the tensor still holds the pattern."""
    isz = torch.empty((), dtype=dtype).element_size()
    nbytes = int(np.prod(shape)) * isz
    lead = GUARD_MIN * isz
    total = nbytes + 2 * lead + 32
    buf = torch.empty(total, dtype=torch.uint8, device=device)
    off = lead
    while (buf.data_ptr() + off) % 16 != elem_offset * isz:
        off += isz
    assert (elem_offset * isz) < 16 and total - (off + nbytes) >= lead
    rng = np.random.default_rng(seed)
    host = rng.integers(1, 256, size=total, dtype=np.uint64).astype(np.uint8)
    buf.copy_(torch.from_numpy(host))
    out = buf[off:off + nbytes].view(dtype).view(*shape)
    assert out.is_contiguous() and out.data_ptr() % 16 == elem_offset * isz

    def guards_intact():
        now = buf.cpu().numpy()
        return bool(np.array_equal(now[:off], host[:off]) and
                    np.array_equal(now[off + nbytes:], host[off + nbytes:]))
    return out, guards_intact


def unchanged(buf, snapshot):
    """whether the flat input buffer still holds the bytes of its snapshot (buf.clone())"""
    return bool(torch.equal(buf, snapshot))


def pitches(H, W, row_mod, plane_odd, itemsize=1):
    """(row_pitch, plane_pitch) in elements for an H x W plane: the row pitch in BYTES is the
    smallest >= W + 3 elements with residue row_mod (mod 4); the plane pitch is H rows, plus an
    odd number k of elements with plane_odd -- then no multiple of the row pitch and, for u8,
    not of 4 either."""
    rp = W + 3
    while (rp * itemsize) % 4 != row_mod:
        rp += 1
    if not plane_odd:
        return rp, H * rp
    k = next(k for k in (7, 5, 3, 1) if k < rp and (itemsize != 1 or (H * rp + k) % 4))
    pp = H * rp + k
    assert k < rp and pp % rp != 0 and (itemsize != 1 or pp % 4 != 0)
    return rp, pp
