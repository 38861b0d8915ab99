"""Device-resident BICOS on MI355X: torch tensors in HBM -> libbicos_amd C-ABI.

This is the reference CUDA build's entry point (BICOS::match on cv::cuda::GpuMat
with a cv::cuda::Stream, reference include/match.hpp:31-41) for Python callers
that keep their stacks on the GPU. torch supplies device memory and the stream;
every kernel is hand-written HIP in libbicos_amd.so. There is no CPU fallback.

Stacks are planar tensors [n, rows, cols] (uint8, or uint16 held in an int16 /
uint16 tensor with depth=2), possibly a row band of a larger frame.
"""
from __future__ import annotations

import ctypes
import dataclasses
from typing import Optional, Sequence, Tuple

import torch

from . import _lib

INVALID_I16 = -32768


@dataclasses.dataclass
class MatchConfig:
    """Python mirror of BICOS::Config (reference include/common.hpp:73-82)."""
    nxcorr_threshold: Optional[float] = 0.5
    subpixel_step: Optional[float] = None
    min_variance: Optional[float] = None
    mode: int = 0              # 0 LIMITED, 1 FULL
    precision: int = 0         # 0 SINGLE, 1 DOUBLE
    variant: int = 0           # 0 NoDuplicates, 1 Consistency
    max_lr_diff: int = 1
    no_dupes: bool = False
    # (lo, hi): search only right columns with lo <= col0 - col1 <= hi (inclusive; bicos_c.h
    # "disparity range"). Not part of BicosConfig: match() passes it to bicos_match_device_range.
    disparity_range: Optional[Tuple[int, int]] = None

    def to_c(self) -> Tuple[_lib.BicosConfig, int]:
        _lib.check_disparity_range(self.disparity_range)
        thr = self.nxcorr_threshold
        if thr is not None and not thr >= 0:
            raise ValueError("device API: nxcorr_threshold must be >= 0 or None "
                             "(BicosConfig maps negatives to the 0.5 default)")
        c = _lib.BicosConfig(
            float(thr if thr is not None else 0.5),
            float(self.subpixel_step if self.subpixel_step is not None else -1.0),
            float(self.min_variance if self.min_variance is not None else -1.0),
            int(self.mode), int(self.precision), int(self.variant), int(self.max_lr_diff),
            int(bool(self.no_dupes)))
        return c, int(thr is not None)


def _depth(t: torch.Tensor) -> int:
    if t.dtype == torch.uint8:
        return 1
    if t.dtype in (torch.int16, getattr(torch, "uint16", torch.int16)):
        return 2
    raise TypeError("stack dtype must be uint8 or (u)int16, got %s" % t.dtype)


def _check_stack(t: torch.Tensor):
    if not t.is_cuda:
        raise ValueError("device API needs CUDA/HIP tensors")
    if t.dim() != 3:
        raise ValueError("stack must be [n, rows, cols]")
    if t.stride(2) != 1:
        raise ValueError("stack rows must be contiguous")
    return t.shape[0], t.shape[1], t.shape[2], t.stride(1), t.stride(0)


def _check_out(t: torch.Tensor, name: str, shape, dtypes, device: torch.device) -> None:
    """The kernels write rows*cols elements of the dtype the config implies straight through
    the tensor's pointer: anything else would be an out-of-bounds HBM write."""
    if t.device != device:
        raise ValueError("%s must be on %s, got %s" % (name, device, t.device))
    if tuple(t.shape) != tuple(shape):
        raise ValueError("%s must have shape %s, got %s" % (name, tuple(shape), tuple(t.shape)))
    if t.dtype not in dtypes:
        raise ValueError("%s must be %s for this config, got %s"
                         % (name, " or ".join(str(d) for d in dtypes), t.dtype))
    if not t.is_contiguous():
        raise ValueError("%s must be contiguous (dense rows)" % name)


def _guide_args(guide: torch.Tensor, rows: int, cols: int, device: torch.device):
    """(pointer, pitch in pixels) of a guide tensor: int16 [rows, cols, 2] on `device`, the
    pairs contiguous, rows a whole number of pairs apart (a view with a row stride is fine)."""
    if not isinstance(guide, torch.Tensor) or guide.dtype != torch.int16:
        raise ValueError("guide must be an int16 tensor")
    if guide.device != device:
        raise ValueError("guide must be on %s, got %s" % (device, guide.device))
    _lib.check_guide_shape(guide.shape, rows, cols)
    if rows * cols == 0:
        return None, cols
    if guide.stride(2) != 1 or (cols > 1 and guide.stride(1) != 2):
        raise ValueError("guide pairs must be contiguous along a row")
    pitch = cols
    if rows > 1:
        if guide.stride(0) % 2 or guide.stride(0) < 2 * cols:
            raise ValueError("guide row stride must be an even number of int16 >= 2 * cols")
        pitch = guide.stride(0) // 2
    if guide.data_ptr() % 4:
        raise ValueError("guide must start at a 4-byte aligned address")
    return guide.data_ptr(), pitch


def _stream(device: torch.device, stream=None) -> int:
    s = stream if stream is not None else torch.cuda.current_stream(device)
    return s.cuda_stream


class Engine:
    """One bicos_engine (workspace + stream-agnostic launcher) per device."""

    def __init__(self, device=None, shared: bool = False):
        """shared=True wraps the library's process-wide engine for the device (the one
        BICOS_Match / pybicos.match use) instead of creating a private one."""
        if not torch.cuda.is_available():
            raise RuntimeError("libbicos_amd device engine needs a ROCm GPU")
        self.device = torch.device("cuda", torch.cuda.current_device() if device is None
                                   else torch.device(device).index or 0)
        self._L = _lib.lib()
        self._owned = not shared
        if shared:
            h = ctypes.c_void_p(self._L.bicos_engine_default(self.device.index))
            if not h.value:
                _lib.check(-5, "bicos_engine_default")
        else:
            h = ctypes.c_void_p()
            _lib.check(self._L.bicos_engine_create(self.device.index, ctypes.byref(h)),
                       "bicos_engine_create")
        self._h = h

    def close(self):
        if getattr(self, "_h", None) and self._owned:
            torch.cuda.synchronize(self.device)
            self._L.bicos_engine_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def tune(self, variant: int = 0, col0_per_lane: int = 0, waves: int = 0,
             split: int = 0) -> None:
        """Search-kernel variant / register blocking / waves / col1 split (0 = automatic)."""
        _lib.check(self._L.bicos_engine_tune(self._h, variant, col0_per_lane, waves, split),
                   "bicos_engine_tune")

    # ------------------------------------------------------------------ match
    def match(self, stack0: torch.Tensor, stack1: torch.Tensor,
              cfg: Optional[MatchConfig] = None, want_corrmap: bool = True,
              out: Optional[torch.Tensor] = None, corrmap: Optional[torch.Tensor] = None,
              stream=None, guide: Optional[torch.Tensor] = None
              ) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
        """Full BICOS::match on device stacks. Returns (disparity, corrmap) on the
        device; asynchronous on `stream` (default: torch's current stream).

        guide: an int16 tensor [rows, cols, 2], one disparity window (lo, hi) per left pixel
        (guide_from_disparity builds one from a prior map; bicos_match_device_guided,
        include/bicos_c.h "disparity guide"); cfg.disparity_range is the global window beside
        it, which Consistency's reverse search runs over -- keep it tight.

        With the NXC stage and no subpixel step, `out` may also be an int16 tensor: the
        integer disparity map (bicos_match_device_i16), whose float32 conversion is exactly
        the float map -- half the bytes, e.g. for a row band that is gathered elsewhere."""
        cfg = cfg or MatchConfig()
        n, rows, cols, rp, pp = _check_stack(stack0)
        if tuple(stack1.shape) != (n, rows, cols) or stack1.stride() != stack0.stride() or \
                stack1.dtype != stack0.dtype:
            raise ValueError("stack1 must match stack0 in shape, strides and dtype")
        c, has_nxcorr = cfg.to_c()
        dev = stack0.device
        disp_dtype = torch.float32 if has_nxcorr else torch.int16
        corr_dtype = torch.float64 if cfg.precision else torch.float32
        i16 = (out is not None and has_nxcorr and out.dtype == torch.int16 and
               cfg.subpixel_step is None)
        if i16:
            disp_dtype = torch.int16
        if out is None:
            out = torch.empty((rows, cols), dtype=disp_dtype, device=dev)
        _check_out(out, "out", (rows, cols), (disp_dtype,), dev)
        if has_nxcorr and want_corrmap and corrmap is None:
            corrmap = torch.empty((rows, cols), device=dev, dtype=corr_dtype)
        if not (has_nxcorr and want_corrmap):
            corrmap = None
        if corrmap is not None:
            _check_out(corrmap, "corrmap", (rows, cols), (corr_dtype,), dev)
        rng = _lib.check_disparity_range(cfg.disparity_range)
        if rng is not None and i16:
            raise ValueError("disparity_range is not supported with an int16 `out` map")
        if guide is not None:
            if i16:
                raise ValueError("guide is not supported with an int16 `out` map")
            gptr, gpitch = _guide_args(guide, rows, cols, dev)
            lo, hi = _lib.guide_window(rng)
            if gptr is None:  # (an empty tensor has no pointer to hand over)
                return out, corrmap
            rc = self._L.bicos_match_device_guided(
                self._h, stack0.data_ptr(), stack1.data_ptr(), n, rows, cols, rp, pp,
                _depth(stack0), ctypes.byref(c), has_nxcorr, lo, hi, gptr, gpitch, out.data_ptr(),
                corrmap.data_ptr() if corrmap is not None else None, _stream(dev, stream))
            _lib.check(rc, "bicos_match_device_guided")
            return out, corrmap
        if rng is not None:
            rc = self._L.bicos_match_device_range(
                self._h, stack0.data_ptr(), stack1.data_ptr(), n, rows, cols, rp, pp,
                _depth(stack0), ctypes.byref(c), has_nxcorr, rng[0], rng[1], out.data_ptr(),
                corrmap.data_ptr() if corrmap is not None else None, _stream(dev, stream))
            _lib.check(rc, "bicos_match_device_range")
            return out, corrmap
        entry = self._L.bicos_match_device_i16 if i16 else self._L.bicos_match_device
        rc = entry(
            self._h, stack0.data_ptr(), stack1.data_ptr(), n, rows, cols, rp, pp, _depth(stack0),
            ctypes.byref(c), has_nxcorr, out.data_ptr(),
            corrmap.data_ptr() if corrmap is not None else None, _stream(dev, stream))
        _lib.check(rc, "bicos_match_device")
        return out, corrmap

    def plan(self, stack0: torch.Tensor, stack1: torch.Tensor,
             cfg: Optional[MatchConfig] = None) -> int:
        """bicos_match_plan: the _lib.PLAN_* bits of what match() runs past the transform for
        these stacks and this config (fused launches, packed keys, compacted reverse search)."""
        cfg = cfg or MatchConfig()
        n, rows, cols, rp, pp = _check_stack(stack0)
        c, has_nxcorr = cfg.to_c()
        rc = self._L.bicos_match_plan(self._h, stack0.data_ptr(), stack1.data_ptr(), n, rows, cols,
                                      rp, pp, _depth(stack0), ctypes.byref(c), has_nxcorr)
        if rc < 0:
            _lib.check(rc, "bicos_match_plan")
        return rc

    def search_packed(self, rows: int, cols: int, words: int = 4, bits: int = 0, n: int = 0,
                      fused: bool = False) -> bool:
        """bicos_search_packed: whether the NoDuplicates search of this shape (fused: inside the
        fused search + agree launch of n-image stacks) runs the pruned packed-key kernel."""
        return bool(self._L.bicos_search_packed(self._h, rows, cols, words, bits, n, int(fused)))

    def agree_kernel(self, stack0: torch.Tensor, stack1: torch.Tensor) -> int:
        """bicos_agree_kernel: which kernel agree() (without a step) runs for these views --
        2 the LDS-staged one, 1 the register one, 0 the generic one (n > 65)."""
        n, rows, cols, rp, pp = _check_stack(stack0)
        rc = self._L.bicos_agree_kernel(stack0.data_ptr(), stack1.data_ptr(), n, rp, pp,
                                        _depth(stack0))
        if rc < 0:
            _lib.check(rc, "bicos_agree_kernel")
        return rc

    def transform_kernel(self, stack0: torch.Tensor, stack1: Optional[torch.Tensor] = None,
                         mode: int = 0, words: Optional[int] = None) -> int:
        """bicos_transform_kernel: which kernel transform() (stack1 None) or match()'s
        transform launch over both stacks runs for these views -- 1 two pixels per register
        from dword loads (aligned u8 LIMITED stacks of a built size within 256 MiB together),
        0 one pixel per lane."""
        n, rows, cols, rp, pp = _check_stack(stack0)
        words = words or descriptor_words(n, mode)
        rc = self._L.bicos_transform_kernel(
            stack0.data_ptr(), stack1.data_ptr() if stack1 is not None else None, n, rows, cols,
            rp, pp, _depth(stack0), mode, words)
        if rc < 0:
            _lib.check(rc, "bicos_transform_kernel")
        return rc

    def search_agree(self, desc0: torch.Tensor, desc1: torch.Tensor, stack0: torch.Tensor,
                     stack1: torch.Tensor, cfg: Optional[MatchConfig] = None,
                     out: Optional[torch.Tensor] = None, corrmap: Optional[torch.Tensor] = None,
                     stream=None) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
        """bicos_search_agree_device: match() from its search on, over descriptors from
        transform() of the two stacks -- the very launches match() issues after its
        transform (bench.py times them in the frame)."""
        cfg = cfg or MatchConfig()
        n, rows, cols, rp, pp = _check_stack(stack0)
        if tuple(stack1.shape) != (n, rows, cols) or stack1.stride() != stack0.stride() or \
                stack1.dtype != stack0.dtype:
            raise ValueError("stack1 must match stack0 in shape, strides and dtype")
        words = descriptor_words(n, cfg.mode)
        pitch = self._L.bicos_desc_pitch(cols, words)
        for name, d in (("desc0", desc0), ("desc1", desc1)):
            if d.device != stack0.device or d.dtype != torch.int32 or not d.is_contiguous() or \
                    tuple(d.shape) != (rows, pitch):
                raise ValueError("%s must be a contiguous int32 [%d, %d] tensor on %s"
                                 % (name, rows, pitch, stack0.device))
        c, has_nxcorr = cfg.to_c()
        dev = stack0.device
        disp_dtype = torch.float32 if has_nxcorr else torch.int16
        corr_dtype = torch.float64 if cfg.precision else torch.float32
        if out is None:
            out = torch.empty((rows, cols), dtype=disp_dtype, device=dev)
        _check_out(out, "out", (rows, cols), (disp_dtype,), dev)
        if has_nxcorr and corrmap is None:
            corrmap = torch.empty((rows, cols), device=dev, dtype=corr_dtype)
        if not has_nxcorr:
            corrmap = None
        if corrmap is not None:
            _check_out(corrmap, "corrmap", (rows, cols), (corr_dtype,), dev)
        rc = self._L.bicos_search_agree_device(
            self._h, desc0.data_ptr(), desc1.data_ptr(), stack0.data_ptr(), stack1.data_ptr(),
            n, rows, cols, rp, pp, _depth(stack0), ctypes.byref(c), has_nxcorr, out.data_ptr(),
            corrmap.data_ptr() if corrmap is not None else None, _stream(dev, stream))
        _lib.check(rc, "bicos_search_agree_device")
        return out, corrmap

    # ------------------------------------------------------------ reprojection
    def _reproject_args(self, disp: torch.Tensor, Q):
        if not disp.is_cuda:
            raise ValueError("device API needs CUDA/HIP tensors")
        if disp.dim() != 2:
            raise ValueError("disparity map must be [rows, cols]")
        if disp.dtype not in (torch.int16, torch.float32):
            raise ValueError("disparity map must be int16 or float32, got %s" % disp.dtype)
        if not disp.is_contiguous():
            raise ValueError("disparity map must be contiguous (dense rows)")
        rows, cols = disp.shape
        if rows * cols >= 2 ** 31:
            raise ValueError("disparity map has more than 2^31 - 1 pixels")
        typ = _lib.CV_32F if disp.dtype == torch.float32 else _lib.CV_16S
        return rows, cols, typ, _lib.reproject_q(Q)

    def reproject_map(self, disp: torch.Tensor, Q, *, allow_negative_z: bool = False,
                      sentinel: bool = True, out: Optional[torch.Tensor] = None,
                      stream=None) -> torch.Tensor:
        """bicos_reproject_device, the dense map: an int16 or float32 disparity map [rows, cols]
        through the 4x4 matrix Q to a float32 [rows, cols, 3] tensor -- the pixel's point
        (X, Y, Z) where it is kept, three NaNs where it is invalid, not finite or (unless
        allow_negative_z) behind the camera. sentinel: a float -32768.0 is invalid too, as
        match() writes it for rejected pixels without a subpixel step. Asynchronous on `stream`
        (default: torch's current stream)."""
        rows, cols, typ, q = self._reproject_args(disp, Q)
        if out is None:
            out = torch.empty((rows, cols, 3), dtype=torch.float32, device=disp.device)
        _check_out(out, "out", (rows, cols, 3), (torch.float32,), disp.device)
        if rows * cols == 0:  # (an empty tensor has no pointer to hand over)
            return out
        rc = self._L.bicos_reproject_device(
            self._h, disp.data_ptr(), typ, rows, cols, q,
            _lib.reproject_flags(allow_negative_z, sentinel), out.data_ptr(), None, None, 0, None,
            _stream(disp.device, stream))
        _lib.check(rc, "bicos_reproject_device")
        return out

    def reproject_points(self, disp: torch.Tensor, Q, *, allow_negative_z: bool = False,
                         sentinel: bool = True, with_index: bool = False,
                         out: Optional[torch.Tensor] = None, stream=None):
        """bicos_reproject_device, the point list: returns (points[:kept], index[:kept] or None,
        stats) -- the kept points as float32 [kept, 3] in row-major pixel order, with
        with_index each point's pixel row * cols + col (int32), and stats = dict(kept, invalid,
        nonfinite, negative_z), which sum to rows * cols. The flags are reproject_map's.

        `out`, a float32 [capacity, 3] tensor, receives the points; without it rows * cols
        points are allocated. The launches are asynchronous on `stream`, but the call then
        synchronises that stream ONCE to read the counts (the size of what it returns). A
        RuntimeError says so if `out` was too small for the kept points (its first `capacity`
        rows are then valid)."""
        rows, cols, typ, q = self._reproject_args(disp, Q)
        dev = disp.device
        if out is None:
            out = torch.empty((rows * cols, 3), dtype=torch.float32, device=dev)
        if out.dim() != 2:
            raise ValueError("out must be [capacity, 3]")
        capacity = out.shape[0]
        _check_out(out, "out", (capacity, 3), (torch.float32,), dev)
        index = torch.empty((capacity,), dtype=torch.int32, device=dev) if with_index else None
        if rows * cols == 0:  # (an empty tensor has no pointer to hand over)
            return out[:0], (index[:0] if with_index else None), \
                dict(kept=0, invalid=0, nonfinite=0, negative_z=0)
        if capacity == 0:
            raise ValueError("out must hold at least one point")
        counts = torch.empty((4,), dtype=torch.int32, device=dev)
        s = stream if stream is not None else torch.cuda.current_stream(dev)
        rc = self._L.bicos_reproject_device(
            self._h, disp.data_ptr(), typ, rows, cols, q,
            _lib.reproject_flags(allow_negative_z, sentinel), None, out.data_ptr(),
            index.data_ptr() if index is not None else None, capacity, counts.data_ptr(),
            s.cuda_stream)
        _lib.check(rc, "bicos_reproject_device")
        with torch.cuda.stream(s):
            host = counts.cpu()  # the one synchronisation
        kept, invalid, nonfinite, negative_z = (int(v) & 0xFFFFFFFF for v in host.tolist())
        stats = dict(kept=kept, invalid=invalid, nonfinite=nonfinite, negative_z=negative_z)
        if kept > capacity:
            raise RuntimeError("reproject_points: out holds %d points, %d were kept"
                               % (capacity, kept))
        return out[:kept], (index[:kept] if index is not None else None), stats

    # ---------------------------------------------------------- speckle filter
    def filter_speckles(self, disp: torch.Tensor, max_size: int, max_diff: float = 1.0, *,
                        sentinel: bool = True, out: Optional[torch.Tensor] = None,
                        labels=False, counts: Optional[torch.Tensor] = None, stream=None):
        """bicos_speckle_device: removes every 4-connected component of similar disparity
        (neighbours differing by at most max_diff) that has at most max_size pixels from an
        int16 or float32 map [rows, cols]; include/bicos_c.h, "speckle filter". Removed pixels
        become invalid (int16 -32768; float NaN, or -32768.0 with `sentinel`, which also makes
        that value invalid on input, as match() writes it without a subpixel step); every
        other pixel keeps its bits. max_size = 0 removes nothing.

        Returns the filtered map -- `out` if given (it may be `disp` itself: in place), else a
        new tensor -- or, with `labels`, the pair (map, labels): int32 [rows, cols], every
        pixel's component label (the smallest row * cols + col in its component; -1 where the
        pixel was invalid on input). `labels` may be True or an int32 tensor to fill.
        `counts`, an int32 [4] tensor on the map's device, receives {kept, removed, invalid,
        removed_components} (uint32 bits).

        The call NEVER synchronises: everything is enqueued on `stream` (default: torch's
        current stream). Reading `counts` (`counts.tolist()`) is where the caller does."""
        if not disp.is_cuda:
            raise ValueError("device API needs CUDA/HIP tensors")
        if disp.dim() != 2:
            raise ValueError("disparity map must be [rows, cols]")
        if disp.dtype not in (torch.int16, torch.float32):
            raise ValueError("disparity map must be int16 or float32, got %s" % disp.dtype)
        if not disp.is_contiguous():
            raise ValueError("disparity map must be contiguous (dense rows)")
        rows, cols = disp.shape
        if rows * cols >= 2 ** 31:
            raise ValueError("disparity map has more than 2^31 - 1 pixels")
        size, diff = _lib.speckle_params(max_size, max_diff)
        dev = disp.device
        if out is None:
            out = torch.empty_like(disp)
        _check_out(out, "out", (rows, cols), (disp.dtype,), dev)
        lab = None
        if labels is True:
            lab = torch.empty((rows, cols), dtype=torch.int32, device=dev)
        elif labels is not False and labels is not None:
            lab = labels
            _check_out(lab, "labels", (rows, cols), (torch.int32,), dev)
        if counts is not None:
            _check_out(counts, "counts", (4,), (torch.int32,), dev)
        if rows * cols == 0:  # (an empty tensor has no pointer to hand over)
            if counts is not None:
                s = stream if stream is not None else torch.cuda.current_stream(dev)
                with torch.cuda.stream(s):
                    counts.zero_()
            return out if lab is None else (out, lab)
        typ = _lib.CV_32F if disp.dtype == torch.float32 else _lib.CV_16S
        rc = self._L.bicos_speckle_device(
            self._h, disp.data_ptr(), typ, rows, cols, size, diff,
            _lib.SPECKLE_F32_SENTINEL if sentinel else 0, out.data_ptr(),
            lab.data_ptr() if lab is not None else None,
            counts.data_ptr() if counts is not None else None, _stream(dev, stream))
        _lib.check(rc, "bicos_speckle_device")
        return out if lab is None else (out, lab)

    # ----------------------------------------------------------- median filter
    def median_filter(self, disp: torch.Tensor, ksize: int = 3, fill_min: int = 0, *,
                      sentinel: bool = True, out: Optional[torch.Tensor] = None,
                      counts: Optional[torch.Tensor] = None, stream=None):
        """bicos_median_device: the ksize x ksize (3 or 5) median filter of an int16 or float32
        map [rows, cols] that knows its invalid values; include/bicos_c.h, "median filter".
        A valid pixel becomes the lower median of the valid values of its window, which is
        clipped at the border; an invalid pixel (int16 -32768; float NaN, and -32768.0 with
        `sentinel`) becomes it too where fill_min > 0 and the window holds at least fill_min
        valid values, and keeps its bits otherwise. Exact: every output is the bits of one
        input pixel.

        Returns the filtered map: `out` if given, else a new tensor. `out` must not share
        storage with `disp` (the filter reads neighbours). `counts`, an int32 [4] tensor on
        the map's device, receives {unchanged, changed, filled, invalid} (uint32 bits).

        The call NEVER synchronises: everything is enqueued on `stream` (default: torch's
        current stream). Reading `counts` (`counts.tolist()`) is where the caller does."""
        if not disp.is_cuda:
            raise ValueError("device API needs CUDA/HIP tensors")
        if disp.dim() != 2:
            raise ValueError("disparity map must be [rows, cols]")
        if disp.dtype not in (torch.int16, torch.float32):
            raise ValueError("disparity map must be int16 or float32, got %s" % disp.dtype)
        if not disp.is_contiguous():
            raise ValueError("disparity map must be contiguous (dense rows)")
        rows, cols = disp.shape
        if rows * cols >= 2 ** 31:
            raise ValueError("disparity map has more than 2^31 - 1 pixels")
        k, fill = _lib.median_params(ksize, fill_min)
        dev = disp.device
        if out is None:
            out = torch.empty_like(disp)
        _check_out(out, "out", (rows, cols), (disp.dtype,), dev)
        if counts is not None:
            _check_out(counts, "counts", (4,), (torch.int32,), dev)
        if rows * cols == 0:  # (an empty tensor has no pointer to hand over)
            if counts is not None:
                s = stream if stream is not None else torch.cuda.current_stream(dev)
                with torch.cuda.stream(s):
                    counts.zero_()
            return out
        if out.untyped_storage().data_ptr() == disp.untyped_storage().data_ptr():
            raise ValueError("out must not share storage with the disparity map: the filter "
                             "reads neighbours")
        typ = _lib.CV_32F if disp.dtype == torch.float32 else _lib.CV_16S
        rc = self._L.bicos_median_device(
            self._h, disp.data_ptr(), typ, rows, cols, k, fill,
            _lib.MEDIAN_F32_SENTINEL if sentinel else 0, out.data_ptr(),
            counts.data_ptr() if counts is not None else None, _stream(dev, stream))
        _lib.check(rc, "bicos_median_device")
        return out

    # --------------------------------------------------------- surface normals
    def normals_map(self, disp: torch.Tensor, Q, *, radius: int = 2, max_diff: float = 1.0,
                    min_points: int = 3, allow_negative_z: bool = False,
                    sentinel: bool = False, out: Optional[torch.Tensor] = None,
                    counts: Optional[torch.Tensor] = None, stream=None) -> torch.Tensor:
        """bicos_normals_device, the dense map: one unit surface normal per pixel of an int16
        or float32 disparity map [rows, cols], oriented towards the camera, as a float32
        [rows, cols, 3] tensor; include/bicos_c.h, "surface normals". The normal is that of the
        least-squares plane of the disparities over the (2 * radius + 1)^2 window (radius 1 ..
        4) in (column, row, disparity), carried through the 4x4 matrix Q; a window pixel takes
        part if it is valid and its disparity lies within max_diff of the centre's. Three NaNs
        where reproject_map with the same flags keeps no point, where fewer than min_points
        pixels take part, or where they are collinear. Meant for SUBPIXEL maps: integer
        disparities stair-step.

        `counts`, an int32 [4] tensor on the map's device, receives {normal, no_point, sparse,
        degenerate} (uint32 bits). The call NEVER synchronises: everything is enqueued on
        `stream` (default: torch's current stream)."""
        rows, cols, typ, q = self._reproject_args(disp, Q)
        r, diff, m = _lib.normals_params(radius, max_diff, min_points)
        dev = disp.device
        if out is None:
            out = torch.empty((rows, cols, 3), dtype=torch.float32, device=dev)
        _check_out(out, "out", (rows, cols, 3), (torch.float32,), dev)
        if counts is not None:
            _check_out(counts, "counts", (4,), (torch.int32,), dev)
        if rows * cols == 0:  # (an empty tensor has no pointer to hand over)
            if counts is not None:
                s = stream if stream is not None else torch.cuda.current_stream(dev)
                with torch.cuda.stream(s):
                    counts.zero_()
            return out
        rc = self._L.bicos_normals_device(
            self._h, disp.data_ptr(), typ, rows, cols, q,
            _lib.normals_flags(allow_negative_z, sentinel), r, diff, m, out.data_ptr(), None, 0,
            None, counts.data_ptr() if counts is not None else None, _stream(dev, stream))
        _lib.check(rc, "bicos_normals_device")
        return out

    def normals_points(self, disp: torch.Tensor, Q, index: torch.Tensor, *, radius: int = 2,
                       max_diff: float = 1.0, min_points: int = 3,
                       allow_negative_z: bool = False, sentinel: bool = False,
                       out: Optional[torch.Tensor] = None,
                       normal_map: Optional[torch.Tensor] = None,
                       counts: Optional[torch.Tensor] = None, stream=None) -> torch.Tensor:
        """bicos_normals_device, the list: the normal of every pixel of `index` (int32 [count],
        row * cols + col, as reproject_points writes it with with_index) as a float32 [count, 3]
        tensor, bit for bit the rows of normals_map; three NaNs for an entry outside the map.
        With `normal_map`, a float32 [rows, cols, 3] tensor, the dense map is written by the
        same call, and `counts` (normals_map's) may be given with it. The parameters are
        normals_map's. The call NEVER synchronises."""
        rows, cols, typ, q = self._reproject_args(disp, Q)
        r, diff, m = _lib.normals_params(radius, max_diff, min_points)
        dev = disp.device
        if index.dim() != 1:
            raise ValueError("index must be [count]")
        count = index.shape[0]
        _check_out(index, "index", (count,), (torch.int32,), dev)
        if out is None:
            out = torch.empty((count, 3), dtype=torch.float32, device=dev)
        _check_out(out, "out", (count, 3), (torch.float32,), dev)
        if normal_map is not None:
            _check_out(normal_map, "normal_map", (rows, cols, 3), (torch.float32,), dev)
        if counts is not None:
            if normal_map is None:
                raise ValueError("counts need normal_map: they count over the map")
            _check_out(counts, "counts", (4,), (torch.int32,), dev)
        s = stream if stream is not None else torch.cuda.current_stream(dev)
        if rows * cols == 0:  # (an empty tensor has no pointer to hand over)
            with torch.cuda.stream(s):
                out.fill_(float("nan"))
                if counts is not None:
                    counts.zero_()
            return out
        if count == 0 and normal_map is None:
            return out
        rc = self._L.bicos_normals_device(
            self._h, disp.data_ptr(), typ, rows, cols, q,
            _lib.normals_flags(allow_negative_z, sentinel), r, diff, m,
            normal_map.data_ptr() if normal_map is not None else None,
            index.data_ptr() if count else None, count, out.data_ptr() if count else None,
            counts.data_ptr() if counts is not None else None, s.cuda_stream)
        _lib.check(rc, "bicos_normals_device")
        return out

    # -------------------------------------------------------------------- mesh
    def mesh(self, disp: torch.Tensor, Q, *, max_diff: float = 1.0,
             allow_negative_z: bool = False, sentinel: bool = True, with_index: bool = False,
             with_vertex_map: bool = False, out_points: Optional[torch.Tensor] = None,
             out_triangles: Optional[torch.Tensor] = None, stream=None):
        """bicos_mesh_device: an int16 or float32 disparity map [rows, cols] triangulated;
        include/bicos_c.h, "mesh". Returns (points[:kept], triangles[:T], index or None,
        vertex_map or None, stats). The vertices are exactly reproject_points' list for the same
        map, Q and flags (float32 [kept, 3], with with_index each vertex's pixel row * cols + col,
        which is what normals_points takes). Every 2x2 block of pixels gives at most two
        triangles (int32 [T, 3], vertex numbers), split along the diagonal with the smaller
        disparity step; a triangle is emitted where its corners are kept and every edge joins
        disparities within max_diff. with_vertex_map: the int32 [rows, cols] map of each pixel's
        vertex number, -1 where the pixel is not kept. stats = dict(kept, invalid, nonfinite,
        negative_z, triangles, quads_full, quads_half, quads_empty).

        `out_points`, a float32 [capacity, 3] tensor, and `out_triangles`, an int32
        [capacity, 3] tensor, receive the results; without them rows * cols points and
        2 * (rows - 1) * (cols - 1) triangles are allocated. The launches are asynchronous on
        `stream`, but the call then synchronises that stream ONCE to read the counts. A
        RuntimeError says so if an out tensor was too small (its rows are then valid up to its
        capacity)."""
        rows, cols, typ, q = self._reproject_args(disp, Q)
        diff = _lib.mesh_max_diff(max_diff)
        dev = disp.device
        quads = _lib.mesh_quads(rows, cols)
        if out_points is None:
            out_points = torch.empty((rows * cols, 3), dtype=torch.float32, device=dev)
        if out_points.dim() != 2:
            raise ValueError("out_points must be [capacity, 3]")
        vcap = out_points.shape[0]
        _check_out(out_points, "out_points", (vcap, 3), (torch.float32,), dev)
        if out_triangles is None:
            out_triangles = torch.empty((max(2 * quads, 1), 3), dtype=torch.int32, device=dev)
        if out_triangles.dim() != 2:
            raise ValueError("out_triangles must be [capacity, 3]")
        tcap = out_triangles.shape[0]
        _check_out(out_triangles, "out_triangles", (tcap, 3), (torch.int32,), dev)
        index = torch.empty((vcap,), dtype=torch.int32, device=dev) if with_index else None
        vmap = torch.empty((rows, cols), dtype=torch.int32, device=dev) if with_vertex_map else None
        keys = ("kept", "invalid", "nonfinite", "negative_z", "triangles", "quads_full",
                "quads_half", "quads_empty")
        if rows * cols == 0:  # (an empty tensor has no pointer to hand over)
            return out_points[:0], out_triangles[:0], (index[:0] if with_index else None), vmap, \
                dict.fromkeys(keys, 0)
        if vcap == 0 or tcap == 0:
            raise ValueError("out_points and out_triangles must hold at least one entry")
        counts = torch.empty((8,), dtype=torch.int32, device=dev)
        s = stream if stream is not None else torch.cuda.current_stream(dev)
        rc = self._L.bicos_mesh_device(
            self._h, disp.data_ptr(), typ, rows, cols, q,
            _lib.mesh_flags(allow_negative_z, sentinel), diff, out_points.data_ptr(),
            index.data_ptr() if index is not None else None, vcap, counts.data_ptr(),
            out_triangles.data_ptr(), tcap, counts.data_ptr() + 16,
            vmap.data_ptr() if vmap is not None else None, s.cuda_stream)
        _lib.check(rc, "bicos_mesh_device")
        with torch.cuda.stream(s):
            host = counts.cpu()  # the one synchronisation
        stats = dict(zip(keys, (int(v) & 0xFFFFFFFF for v in host.tolist())))
        kept, tris = stats["kept"], stats["triangles"]
        if kept > vcap:
            raise RuntimeError("mesh: out_points holds %d points, %d were kept" % (vcap, kept))
        if tris > tcap:
            raise RuntimeError("mesh: out_triangles holds %d triangles, %d were emitted"
                               % (tcap, tris))
        return out_points[:kept], out_triangles[:tris], \
            (index[:kept] if index is not None else None), vmap, stats

    # -------------------------------------------------------------- projection
    PROJECT_OUTPUTS = ("uv", "depth", "cls", "tex", "depth_map", "index_map", "counts")

    def project(self, points: torch.Tensor, K, size=None, *, D=None, R=None, t=None,
                splat: int = 0, tol: float = float("inf"),
                image: Optional[torch.Tensor] = None, fill: int = 0,
                outputs: Optional[Sequence[str]] = None, out: Optional[dict] = None,
                stream=None) -> dict:
        """bicos_project_device: float32 points [count, 3] in the frame of Q (reproject_points',
        mesh's, or a dense xyz map reshaped to a list) projected into the camera Pc = R*P + t,
        K, D with an image of size = (rows, cols); include/bicos_c.h, "projection". Returns a
        dict of tensors, the `outputs` asked for among
            uv [count, 2] float32, depth [count] float32, cls [count] uint8 (0 visible,
            1 occluded, 2 outside, 3 behind, 4 invalid), tex [count, channels] of the image's
            dtype, depth_map / index_map [rows, cols] float32 / int32 (the scan as that camera
            sees it: the nearest depth and its point's position per pixel, NaN / -1 where none),
            counts int32 [5] = visible, occluded, outside, behind, invalid.
        The default is uv, depth, cls and, with an image, tex. `image`: uint8 or uint16
        [rows, cols] or [rows, cols, 3] on the device, the pixels contiguous, any row stride;
        `size` defaults to its shape. A point covers (2*splat+1)^2 pixels of the z-buffer; it is
        occluded where !(depth <= nearest depth at its pixel + tol); tol = inf (the default) with
        no map asked for runs no z-buffer at all. `out`: a dict of caller-provided tensors by the
        same names, written in place and returned. Asynchronous on `stream`; nothing is
        synchronised."""
        if not isinstance(points, torch.Tensor) or points.dtype != torch.float32 or \
                points.dim() != 2 or points.shape[1] != 3:
            raise ValueError("points must be a float32 tensor [count, 3]")
        if not points.is_contiguous():
            raise ValueError("points must be contiguous")
        dev = points.device
        count = points.shape[0]
        ptr, depth, channels, pitch = None, 1, 1, 0
        if image is not None:
            if not isinstance(image, torch.Tensor) or image.dtype not in (torch.uint8, torch.uint16):
                raise ValueError("image must be a uint8 or uint16 tensor")
            if image.device != dev:
                raise ValueError("image must be on %s, got %s" % (dev, image.device))
            if image.dim() not in (2, 3) or (image.dim() == 3 and image.shape[2] not in (1, 3)):
                raise ValueError("image must be [rows, cols] or [rows, cols, 3]")
            channels = image.shape[2] if image.dim() == 3 else 1
            if size is None:
                size = tuple(image.shape[:2])
            if tuple(image.shape[:2]) != tuple(size):
                raise ValueError("image must have the camera's size %s" % (tuple(size),))
            rows_i, cols_i = image.shape[:2]
            if image.dim() == 3 and cols_i > 0 and channels > 1 and image.stride(2) != 1:
                raise ValueError("image channels must be interleaved")
            if cols_i > 1 and image.stride(1) != channels:
                raise ValueError("image pixels must be contiguous along a row")
            pitch = cols_i * channels
            if rows_i > 1:
                if image.stride(0) < pitch:
                    raise ValueError("image row stride must be >= a row")
                pitch = image.stride(0)
            depth = image.element_size()
            ptr = image.data_ptr() if rows_i * cols_i else None
        if size is None:
            raise ValueError("size = (rows, cols) is required without an image")
        rows, cols, splat, tol, fill = _lib.project_params(size, splat, tol, fill)
        r, tt, k, d, nd = _lib.project_camera(K, D, R, t)
        out = dict(out) if out else {}
        if outputs is None:
            outputs = () if out else ("uv", "depth", "cls") + (("tex",) if image is not None else ())
        names = [n for n in self.PROJECT_OUTPUTS if n in outputs or n in out]
        unknown = [n for n in list(outputs) + list(out) if n not in self.PROJECT_OUTPUTS]
        if unknown:
            raise ValueError("unknown outputs %r (of %r)" % (unknown, self.PROJECT_OUTPUTS))
        if not names:
            raise ValueError("at least one output is required")
        if "tex" in names and image is None:
            raise ValueError("tex requires an image")
        spec = {"uv": ((count, 2), torch.float32), "depth": ((count,), torch.float32),
                "cls": ((count,), torch.uint8),
                "tex": ((count, channels), image.dtype if image is not None else torch.uint8),
                "depth_map": ((rows, cols), torch.float32),
                "index_map": ((rows, cols), torch.int32), "counts": ((5,), torch.int32)}
        res = {}
        for n in names:
            shape, dtype = spec[n]
            if n in out:
                _check_out(out[n], n, shape, (dtype,), dev)
                res[n] = out[n]
            else:
                res[n] = torch.empty(shape, dtype=dtype, device=dev)

        def p(n):  # (an empty tensor has no pointer to hand over; it is not written either)
            return res[n].data_ptr() if n in res and res[n].numel() else None
        args = [p(n) for n in self.PROJECT_OUTPUTS]
        if all(a is None for a in args):  # nothing but empty outputs: nothing to do
            return res
        rc = self._L.bicos_project_device(
            self._h, points.data_ptr() if count else None, count, r, tt, k, d, nd, rows, cols,
            splat, tol, ptr, depth, channels, pitch, fill, *args, _stream(dev, stream))
        _lib.check(rc, "bicos_project_device")
        return res

    # --------------------------------------------------------- disparity guide
    def guide_from_disparity(self, prior: torch.Tensor, radius: int, spread: int = 0,
                             scale: int = 1, fallback: Optional[Tuple[int, int]] = None,
                             shape: Optional[Tuple[int, int]] = None, sentinel: bool = True,
                             out: Optional[torch.Tensor] = None,
                             counts: Optional[torch.Tensor] = None, stream=None) -> torch.Tensor:
        """bicos_guide_device: the guide of match(guide=) / search(guide=) -- an int16 tensor
        [rows, cols, 2] of windows (lo, hi) -- from a prior disparity map, int16 or float32
        [prows, pcols] (invalid: int16 -32768, float NaN, and -32768.0 with `sentinel`);
        include/bicos_c.h, "disparity guide". The output pixel (r, c) looks at the valid prior
        values of the (2 spread + 1)^2 window around (r // scale, c // scale), clipped to the
        prior: lo = scale * floor(min) - radius, hi = scale * ceil(max) + scale - 1 + radius,
        clamped to +-32767; where there is none, `fallback` (None: every disparity; a pair
        with lo > hi: do not search there). shape: (rows, cols) of the guide, default the
        prior's size times scale. `counts`, an int32 [2] tensor on the map's device, receives
        {from_prior, fallback} (uint32 bits).

        The call NEVER synchronises: one launch on `stream` (default: torch's current stream)."""
        if not prior.is_cuda:
            raise ValueError("device API needs CUDA/HIP tensors")
        if prior.dim() != 2:
            raise ValueError("prior map must be [rows, cols]")
        if prior.dtype not in (torch.int16, torch.float32):
            raise ValueError("prior map must be int16 or float32, got %s" % prior.dtype)
        if not prior.is_contiguous():
            raise ValueError("prior map must be contiguous (dense rows)")
        prows, pcols = prior.shape
        if prows * pcols >= 2 ** 31:
            raise ValueError("prior map has more than 2^31 - 1 pixels")
        r, sp, sc, flo, fhi = _lib.guide_params(radius, spread, scale, fallback)
        rows, cols = _lib.guide_shape(shape, (prows, pcols), sc)
        dev = prior.device
        if out is None:
            out = torch.empty((rows, cols, 2), dtype=torch.int16, device=dev)
        gptr, gpitch = _guide_args(out, rows, cols, dev)
        if counts is not None:
            _check_out(counts, "counts", (2,), (torch.int32,), dev)
        if gptr is None:  # (an empty tensor has no pointer to hand over)
            if counts is not None:
                s = stream if stream is not None else torch.cuda.current_stream(dev)
                with torch.cuda.stream(s):
                    counts.zero_()
            return out
        if prows * pcols == 0:
            raise ValueError("prior map is empty")
        typ = _lib.CV_32F if prior.dtype == torch.float32 else _lib.CV_16S
        rc = self._L.bicos_guide_device(
            self._h, prior.data_ptr(), typ, prows, pcols, rows, cols, sc, r, sp, flo, fhi,
            _lib.GUIDE_F32_SENTINEL if sentinel else 0, gptr, gpitch,
            counts.data_ptr() if counts is not None else None, _stream(dev, stream))
        _lib.check(rc, "bicos_guide_device")
        return out

    # ----------------------------------------------------------- rectification
    def rectify_maps(self, K, D, R, P, size, stream=None):
        """bicos_rectify_maps_device: the float32 lookup maps (map_x, map_y), each [rows, cols]
        on this engine's device, of one camera for `size` = (rows, cols) output pixels -- the
        model of cv::initUndistortRectifyMap (include/bicos_c.h "rectification"). K: 3x3
        intrinsics, D: None or 4, 5 or 8 distortion coefficients, R: None (identity) or the 3x3
        rectifying rotation, P: the 3x3 or 3x4 new projection matrix. Asynchronous on `stream`
        (default: torch's current stream)."""
        k, d, nd, r, p, p_cols, rows, cols = _lib.rectify_camera(K, D, R, P, size)
        map_x = torch.empty((rows, cols), dtype=torch.float32, device=self.device)
        map_y = torch.empty((rows, cols), dtype=torch.float32, device=self.device)
        rc = self._L.bicos_rectify_maps_device(k, d, nd, r, p, p_cols, rows, cols,
                                               map_x.data_ptr(), map_y.data_ptr(),
                                               _stream(self.device, stream))
        _lib.check(rc, "bicos_rectify_maps_device")
        return map_x, map_y

    def rectify(self, stack: torch.Tensor, map_x: torch.Tensor, map_y: torch.Tensor, *,
                border: int = 0, out: Optional[torch.Tensor] = None, valid=False, stream=None):
        """bicos_rectify_device: the planar stack [n, src_rows, src_cols] (uint8, or 16 bits in
        an int16 / uint16 tensor) remapped bilinearly through the float32 maps [rows, cols] of
        absolute source coordinates to a stack [n, rows, cols] of the same dtype
        (include/bicos_c.h "rectification"); pixels whose coordinates lie outside the source get
        `border`. Plane and row strides of `stack`, `out` and the maps may be anything (the
        last dimension contiguous), as for match(); the result can go straight into match().

        Returns the stack -- `out` if given -- or, with `valid`, the pair (stack, valid): uint8
        [rows, cols], 1 where every tap that contributed lies in the source. `valid` may be
        True or a contiguous uint8 tensor to fill.

        The call NEVER synchronises: one launch on `stream` (default: torch's current stream)."""
        n, src_rows, src_cols, rp, pp = _check_stack(stack)
        dev = stack.device
        for name, m in (("map_x", map_x), ("map_y", map_y)):
            if m.device != dev or m.dtype != torch.float32 or m.dim() != 2 or \
                    (m.shape[1] > 1 and m.stride(1) != 1):
                raise ValueError("%s must be a float32 [rows, cols] tensor on %s with contiguous "
                                 "rows" % (name, dev))
        if tuple(map_y.shape) != tuple(map_x.shape) or \
                (map_x.shape[0] > 1 and map_y.stride(0) != map_x.stride(0)):
            raise ValueError("map_y must match map_x in shape and row stride")
        rows, cols = map_x.shape
        if n < 1 or rows < 1 or cols < 1 or src_rows < 1 or src_cols < 1:
            raise ValueError("rectify needs a non-empty stack and non-empty maps")
        if out is None:
            out = torch.empty((n, rows, cols), dtype=stack.dtype, device=dev)
        if out.device != dev or out.dtype != stack.dtype or tuple(out.shape) != (n, rows, cols) \
                or out.stride(2) != 1:
            raise ValueError("out must be a %s [%d, %d, %d] tensor on %s with contiguous rows"
                             % (stack.dtype, n, rows, cols, dev))
        val = None
        if valid is True:
            val = torch.empty((rows, cols), dtype=torch.uint8, device=dev)
        elif valid is not False and valid is not None:
            val = valid
            _check_out(val, "valid", (rows, cols), (torch.uint8,), dev)
        map_pitch = 4 * (map_x.stride(0) if rows > 1 else cols)
        rc = self._L.bicos_rectify_device(
            self._h, stack.data_ptr(), n, src_rows, src_cols,
            # (the stride of a dimension of size one means nothing)
            rp if src_rows > 1 else src_cols, pp if n > 1 else src_cols, _depth(stack),
            map_x.data_ptr(), map_y.data_ptr(), map_pitch, rows, cols, out.data_ptr(),
            out.stride(1) if rows > 1 else cols, out.stride(0) if n > 1 else cols,
            int(border), val.data_ptr() if val is not None else None, _stream(dev, stream))
        _lib.check(rc, "bicos_rectify_device")
        return out if val is None else (out, val)

    # ----------------------------------------------------------- stack pooling
    def pool(self, stack: torch.Tensor, scale: int, *, out: Optional[torch.Tensor] = None,
             stream=None) -> torch.Tensor:
        """bicos_pool_device: the planar stack [n, rows, cols] (uint8, or 16 bits in an int16 /
        uint16 tensor) pooled by `scale` in 2..8 to [n, rows // scale, cols // scale] of the same
        dtype: each output pixel is (sum of its scale x scale block + scale*scale // 2) //
        (scale*scale), the mean rounded half up in integers (include/bicos_c.h "stack pooling").
        The rows % scale last rows and cols % scale last columns are not read. Plane and row
        strides of `stack` and `out` may be anything (the last dimension contiguous), as for
        match(); the result can go straight into match(). Returns the stack -- `out` if given.

        The call NEVER synchronises: one launch on `stream` (default: torch's current stream)."""
        sc = _lib.pool_scale(scale)
        n, rows, cols, rp, pp = _check_stack(stack)
        dev = stack.device
        if n < 1:
            raise ValueError("pool needs a non-empty stack")
        prows, pcols = _lib.pool_shape(rows, cols, sc)
        if out is None:
            out = torch.empty((n, prows, pcols), dtype=stack.dtype, device=dev)
        if out.device != dev or out.dtype != stack.dtype or tuple(out.shape) != (n, prows, pcols) \
                or out.stride(2) != 1:
            raise ValueError("out must be a %s [%d, %d, %d] tensor on %s with contiguous rows"
                             % (stack.dtype, n, prows, pcols, dev))
        rc = self._L.bicos_pool_device(
            self._h, stack.data_ptr(), n, rows, cols,
            # (the stride of a dimension of size one means nothing)
            rp if rows > 1 else cols, pp if n > 1 else cols, _depth(stack), sc, out.data_ptr(),
            out.stride(1) if prows > 1 else pcols, out.stride(0) if n > 1 else pcols,
            _stream(dev, stream))
        _lib.check(rc, "bicos_pool_device")
        return out

    def pool_kernel(self, stack: torch.Tensor, out: torch.Tensor) -> int:
        """bicos_pool_kernel: bit 0 set if pool(stack, out=out) runs the dword-load kernel, clear
        if the per-element kernel (the source's alignment decides); bit 1 set if `out` is aligned
        for the dword-load kernel's vector stores. The results are the same."""
        n, rows, cols, rp, pp = _check_stack(stack)
        return self._L.bicos_pool_kernel(
            stack.data_ptr(), rp if rows > 1 else cols, pp if n > 1 else cols, _depth(stack),
            out.data_ptr(), out.stride(1) if out.shape[1] > 1 else out.shape[2],
            out.stride(0) if n > 1 else out.shape[2])

    # ------------------------------------------------------------ pyramid match
    def match_pyramid(self, stack0: torch.Tensor, stack1: torch.Tensor,
                      cfg: Optional[MatchConfig] = None, *, scale: int = 2, radius: int = 2,
                      spread: int = 1, fallback: Optional[Tuple[int, int]] = None,
                      return_guide=False, return_coarse=False,
                      counts: Optional[torch.Tensor] = None, want_corrmap: bool = True,
                      out: Optional[torch.Tensor] = None, corrmap: Optional[torch.Tensor] = None,
                      stream=None):
        """bicos_match_device_pyramid: the coarse-to-fine match in one call, for windows too
        wide for one search. Byte for byte pool(stack, scale) of both stacks, match() of the
        pooled stacks without a subpixel step over cfg.disparity_range divided by `scale`
        (floor, ceil), guide_from_disparity(coarse, radius, spread, scale, fallback,
        shape=(rows, cols)) and match(guide=) of the full stacks (include/bicos_c.h "pyramid
        match"). cfg.disparity_range is required. fallback None: the global window, clamped to
        +-32767; a pair with lo > hi: do not search where the coarse map knows nothing.

        Returns (disparity, corrmap), followed by the guide (int16 [rows, cols, 2]) with
        return_guide and by the coarse map ([rows // scale, cols // scale], float32 with the
        NXC stage, else int16) with return_coarse; either may be True or a tensor to fill.
        `counts`, an int32 [2] tensor, receives the guide's {from_prior, fallback}.

        The call NEVER synchronises: everything is enqueued on `stream`."""
        cfg = cfg or MatchConfig()
        rng, sc, r, sp, flo, fhi = _lib.pyramid_params(cfg.disparity_range, scale, radius,
                                                       spread, fallback)
        n, rows, cols, rp, pp = _check_stack(stack0)
        if tuple(stack1.shape) != (n, rows, cols) or stack1.stride() != stack0.stride() or \
                stack1.dtype != stack0.dtype:
            raise ValueError("stack1 must match stack0 in shape, strides and dtype")
        prows, pcols = _lib.pool_shape(rows, cols, sc)
        c, has_nxcorr = cfg.to_c()
        dev = stack0.device
        disp_dtype = torch.float32 if has_nxcorr else torch.int16
        corr_dtype = torch.float64 if cfg.precision else torch.float32
        if out is None:
            out = torch.empty((rows, cols), dtype=disp_dtype, device=dev)
        _check_out(out, "out", (rows, cols), (disp_dtype,), dev)
        if has_nxcorr and want_corrmap and corrmap is None:
            corrmap = torch.empty((rows, cols), device=dev, dtype=corr_dtype)
        if not (has_nxcorr and want_corrmap):
            corrmap = None
        if corrmap is not None:
            _check_out(corrmap, "corrmap", (rows, cols), (corr_dtype,), dev)
        guide = coarse = None
        if return_guide is True:
            guide = torch.empty((rows, cols, 2), dtype=torch.int16, device=dev)
        elif return_guide is not False and return_guide is not None:
            guide = return_guide
            _check_out(guide, "guide", (rows, cols, 2), (torch.int16,), dev)
        if return_coarse is True:
            coarse = torch.empty((prows, pcols), dtype=disp_dtype, device=dev)
        elif return_coarse is not False and return_coarse is not None:
            coarse = return_coarse
            _check_out(coarse, "coarse", (prows, pcols), (disp_dtype,), dev)
        if counts is not None:
            _check_out(counts, "counts", (2,), (torch.int32,), dev)
        rc = self._L.bicos_match_device_pyramid(
            self._h, stack0.data_ptr(), stack1.data_ptr(), n, rows, cols, rp, pp, _depth(stack0),
            ctypes.byref(c), has_nxcorr, rng[0], rng[1], sc, r, sp, flo, fhi, out.data_ptr(),
            corrmap.data_ptr() if corrmap is not None else None,
            coarse.data_ptr() if coarse is not None else None,
            guide.data_ptr() if guide is not None else None,
            counts.data_ptr() if counts is not None else None, _stream(dev, stream))
        _lib.check(rc, "bicos_match_device_pyramid")
        res = (out, corrmap)
        if guide is not None:
            res += (guide,)
        if coarse is not None:
            res += (coarse,)
        return res

    # ----------------------------------------------------------------- stages
    def transform(self, stack: torch.Tensor, mode: int = 0, words: Optional[int] = None,
                  out: Optional[torch.Tensor] = None, stream=None) -> torch.Tensor:
        """Descriptors as int32 [rows, desc_pitch] (uint32 bit patterns)."""
        n, rows, cols, rp, pp = _check_stack(stack)
        words = words or descriptor_words(n, mode)
        pitch = self._L.bicos_desc_pitch(cols, words)
        if out is None:
            out = torch.empty((rows, pitch), dtype=torch.int32, device=stack.device)
        _check_out(out, "out", (rows, pitch), (torch.int32,), stack.device)
        rc = self._L.bicos_transform_device(stack.data_ptr(), n, rows, cols, rp, pp,
                                            _depth(stack), mode, words, out.data_ptr(),
                                            _stream(stack.device, stream))
        _lib.check(rc, "bicos_transform_device")
        return out

    def search(self, desc0: torch.Tensor, desc1: torch.Tensor, cols: int, words: int,
               flags: int = 1, max_lr_diff: int = -1, out: Optional[torch.Tensor] = None,
               stream=None, bits: int = 0,
               disparity_range: Optional[Tuple[int, int]] = None,
               guide: Optional[torch.Tensor] = None) -> torch.Tensor:
        """bits: how many low descriptor bits may be set (0 = all; see used_bits) -- the
        matrix-core search skips the K-steps above them (bicos_c.h flags bits 16-24).
        disparity_range: (lo, hi), search only col1 with lo <= col0 - col1 <= hi
        (bicos_search_device_range).
        guide: an int16 tensor [rows, cols, 2], one window (lo, hi) per left pixel, joined with
        disparity_range (None: no global bound) -- bicos_search_device_guided."""
        rng = _lib.check_disparity_range(disparity_range)
        if not 0 <= bits <= 256:
            raise ValueError("bits must be in [0, 256]")
        flags = (flags & 0xFFFF) | (bits << 16)
        rows = desc0.shape[0]
        pitch = self._L.bicos_desc_pitch(cols, words)
        for name, d in (("desc0", desc0), ("desc1", desc1)):
            if d.device != desc0.device or d.dtype != torch.int32 or not d.is_contiguous() or \
                    d.dim() != 2 or tuple(d.shape) != (rows, pitch):
                raise ValueError("%s must be a contiguous int32 [%d, %d] tensor on %s "
                                 "(bicos_desc_pitch)" % (name, rows, pitch, desc0.device))
        if out is None:
            out = torch.empty((rows, cols), dtype=torch.int16, device=desc0.device)
        _check_out(out, "out", (rows, cols), (torch.int16,), desc0.device)
        if guide is not None:
            gptr, gpitch = _guide_args(guide, rows, cols, desc0.device)
            lo, hi = _lib.guide_window(rng)
            if gptr is None:  # (an empty tensor has no pointer to hand over)
                return out
            rc = self._L.bicos_search_device_guided(
                self._h, desc0.data_ptr(), desc1.data_ptr(), rows, cols, words, flags, max_lr_diff,
                lo, hi, gptr, gpitch, out.data_ptr(), _stream(desc0.device, stream))
            _lib.check(rc, "bicos_search_device_guided")
            return out
        if rng is not None:
            rc = self._L.bicos_search_device_range(
                self._h, desc0.data_ptr(), desc1.data_ptr(), rows, cols, words, flags, max_lr_diff,
                rng[0], rng[1], out.data_ptr(), _stream(desc0.device, stream))
            _lib.check(rc, "bicos_search_device_range")
            return out
        rc = self._L.bicos_search_device(self._h, desc0.data_ptr(), desc1.data_ptr(), rows, cols,
                                         words, flags, max_lr_diff, out.data_ptr(),
                                         _stream(desc0.device, stream))
        _lib.check(rc, "bicos_search_device")
        return out

    def agree(self, raw: torch.Tensor, stack0: torch.Tensor, stack1: torch.Tensor,
              threshold: float, minvar_scaled: Optional[float] = None,
              step: Optional[float] = None, stream=None, precision: int = 0,
              out: Optional[torch.Tensor] = None, corrmap: Optional[torch.Tensor] = None
              ) -> Tuple[torch.Tensor, torch.Tensor]:
        """NXC agree (step None) or subpixel refine of an int16 search result -> (float32
        disparity, corrmap float32 / float64 with precision=1), into `out` / `corrmap` where
        given (dense)."""
        if step is not None and not step > 0:
            raise ValueError("subpixel step must be positive")
        n, rows, cols, rp, pp = _check_stack(stack0)
        corr_dtype = torch.float64 if precision else torch.float32
        if out is None:
            out = torch.empty((rows, cols), dtype=torch.float32, device=stack0.device)
        _check_out(out, "out", (rows, cols), (torch.float32,), stack0.device)
        corr = corrmap
        if corr is None:
            corr = torch.empty((rows, cols), dtype=corr_dtype, device=stack0.device)
        _check_out(corr, "corrmap", (rows, cols), (corr_dtype,), stack0.device)
        hm = int(minvar_scaled is not None)
        mv = float(minvar_scaled or 0.0)
        st = _stream(stack0.device, stream)
        rc = self._L.bicos_agree_stage_device(raw.data_ptr(), stack0.data_ptr(),
                                              stack1.data_ptr(), n, rows, cols, rp, pp,
                                              _depth(stack0), threshold,
                                              -1.0 if step is None else step, hm, mv,
                                              int(bool(precision)), out.data_ptr(),
                                              corr.data_ptr(), st)
        _lib.check(rc, "bicos_agree_stage_device")
        return out, corr


def used_bits(n: int, mode: int = 0) -> int:
    """Upper bound of the descriptor bits the transform sets (LIMITED 4n-6 for n >= 4, 7 for
    n = 3, 4 for n = 2 (descriptor_transform.hpp:62-68 alone); FULL n^2-2n+3; reference
    descriptor_transform.hpp:31-123)."""
    return n * n - 2 * n + 3 if mode else max(4 * n - 5, 4)


def descriptor_words(n: int, mode: int = 0) -> int:
    w = _lib.lib().bicos_descriptor_words(n, mode)
    if w < 0:
        _lib.check(w, "bicos_descriptor_words")
    return w


_ENGINES = {}


def default_engine(device=None) -> Engine:
    idx = torch.cuda.current_device() if device is None else torch.device(device).index or 0
    if idx not in _ENGINES:
        _ENGINES[idx] = Engine(idx, shared=True)
    return _ENGINES[idx]


def match_bands(bands0: Sequence[torch.Tensor], bands1: Sequence[torch.Tensor],
                cfg: Optional[MatchConfig] = None, want_corrmap: bool = True, guide=None
                ) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """Single-process multi-GPU match (bicos_match_bands_device):
    bands0[b] / bands1[b] are the planar stacks [n, rows_b, cols] of row band b (bands in
    frame order), each on the GPU that matches it. Returns the whole frame's (disparity,
    corrmap) on bands0[0]'s device, gathered there by peer copies. Synchronous: the work
    queued on every band device's current stream is finished first."""
    cfg = cfg or MatchConfig()
    if cfg.disparity_range is not None:
        raise ValueError("disparity_range is not supported with several GPUs yet")
    if guide is not None:
        raise ValueError("a disparity guide is not supported with several GPUs yet")
    if len(bands0) == 0 or len(bands0) != len(bands1):
        raise ValueError("need the same number (>= 1) of left and right bands")
    k = len(bands0)
    shapes = [_check_stack(t) for t in bands0]
    n, _, cols, _, _ = shapes[0]
    for b in range(k):
        t0, t1 = bands0[b], bands1[b]
        if t0.shape[0] != n or t0.shape[2] != cols or t0.dtype != bands0[0].dtype:
            raise ValueError("every band needs the same n, cols and dtype")
        if tuple(t1.shape) != tuple(t0.shape) or t1.stride() != t0.stride() or \
                t1.dtype != t0.dtype or t1.device != t0.device:
            raise ValueError("bands1[%d] must match bands0[%d] in shape, strides, dtype, device"
                             % (b, b))
    c, has_nxcorr = cfg.to_c()
    root = bands0[0].device
    rows = sum(int(t.shape[1]) for t in bands0)
    disp_dtype = torch.float32 if has_nxcorr else torch.int16
    corr_dtype = torch.float64 if cfg.precision else torch.float32
    out = torch.empty((rows, cols), dtype=disp_dtype, device=root)
    corrmap = torch.empty((rows, cols), dtype=corr_dtype, device=root) \
        if has_nxcorr and want_corrmap else None
    for dev in {t.device for t in bands0} | {root}:
        torch.cuda.synchronize(dev)
    devs = (ctypes.c_int * k)(*[t.device.index or 0 for t in bands0])
    p0 = (ctypes.c_void_p * k)(*[t.data_ptr() for t in bands0])
    p1 = (ctypes.c_void_p * k)(*[t.data_ptr() for t in bands1])
    br = (ctypes.c_int * k)(*[int(t.shape[1]) for t in bands0])
    rp = (ctypes.c_size_t * k)(*[s[3] for s in shapes])
    pp = (ctypes.c_size_t * k)(*[s[4] for s in shapes])
    rc = _lib.lib().bicos_match_bands_device(
        devs, k, p0, p1, br, rp, pp, n, cols, _depth(bands0[0]), ctypes.byref(c), has_nxcorr,
        out.data_ptr(), corrmap.data_ptr() if corrmap is not None else None)
    _lib.check(rc, "bicos_match_bands_device")
    return out, corrmap


def match(stack0: torch.Tensor, stack1: torch.Tensor, cfg: Optional[MatchConfig] = None,
          **kw) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """Module-level convenience: BICOS::match on device tensors."""
    return default_engine(stack0.device).match(stack0, stack1, cfg, **kw)
