"""TEST INFRASTRUCTURE ONLY -- ctypes front end for the reference's own CPU code.

oracle/_ref/libbicos_ref.so is the reference's src/impl/cpu.cpp and include/impl/cpu/*.hpp,
compiled unchanged from the reference tree behind oracle/ref_driver.cpp, with the cv::
stand-in of oracle/ref_shim for storage and threading (`make -C oracle ref`). The call
signatures are those of oracle/oracle.py, so a test can put the two side by side.

Only tests/test_reference_parity.py and tests/golden/make_ref_frames.py import this module.
The product path (libbicos_amd), bench.py and smoke() never do, and nothing under
oracle/_ref/ is committed.

The reference tree is taken from $BICOS_REFERENCE (default /root/reference). Where it is
absent, a library built earlier is used as it is; where both are absent, available() is
False.
"""
from __future__ import annotations

import ctypes
import dataclasses
import os
import subprocess
from typing import Optional, Tuple

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIBS = {}

NODUPES = 1
CONSISTENCY = 2


def reference_tree() -> str:
    return os.environ.get("BICOS_REFERENCE", "/root/reference")


def lib_path(variant: str = "") -> str:
    """variant "" = the reference's Release flags (-O3), "O0" = the same sources at -O0."""
    return os.path.join(_HERE, "_ref", "libbicos_ref%s.so" % ("_" + variant if variant else ""))


def have_tree() -> bool:
    return os.path.exists(os.path.join(reference_tree(), "src", "impl", "cpu.cpp"))


def available() -> bool:
    return have_tree() or (os.path.exists(lib_path()) and os.path.exists(lib_path("O0")))


def build(quiet: bool = True) -> None:
    """Compile both reference libraries from the reference tree (g++; about 15 s)."""
    if not have_tree():
        raise FileNotFoundError("no reference tree at %s" % reference_tree())
    out = subprocess.run(["make", "-C", _HERE, "ref", "REFERENCE=" + reference_tree()],
                         capture_output=True, text=True)
    if out.returncode != 0:
        raise RuntimeError("reference build failed:\n" + out.stdout + out.stderr)
    if not quiet:
        print(out.stdout)


class _Cfg(ctypes.Structure):
    _fields_ = [
        ("has_nxcorr", ctypes.c_int), ("nxcorr_threshold", ctypes.c_float),
        ("has_step", ctypes.c_int), ("subpixel_step", ctypes.c_float),
        ("has_minvar", ctypes.c_int), ("min_variance", ctypes.c_float),
        ("mode", ctypes.c_int), ("variant", ctypes.c_int),
        ("max_lr_diff", ctypes.c_int), ("no_dupes", ctypes.c_int),
    ]


@dataclasses.dataclass
class ReferenceConfig:
    """BICOS::Config of the reference (include/common.hpp), field for field as
    oracle.OracleConfig; match() takes either."""
    nxcorr_threshold: Optional[float] = 0.5
    subpixel_step: Optional[float] = None
    min_variance: Optional[float] = None
    mode: int = 0            # 0 LIMITED, 1 FULL
    variant: int = 0         # 0 NoDuplicates, 1 Consistency
    max_lr_diff: int = 1
    no_dupes: bool = False


def _cfg(c) -> _Cfg:
    return _Cfg(
        int(c.nxcorr_threshold is not None), float(c.nxcorr_threshold or 0.0),
        int(c.subpixel_step is not None), float(c.subpixel_step or 0.0),
        int(c.min_variance is not None), float(c.min_variance or 0.0),
        int(c.mode), int(c.variant), int(c.max_lr_diff), int(bool(c.no_dupes)))


def lib(variant: str = "") -> ctypes.CDLL:
    if variant in _LIBS:
        return _LIBS[variant]
    if have_tree():
        build()       # make: nothing to do when the libraries are current
    L = ctypes.CDLL(lib_path(variant))
    P = ctypes.c_void_p
    I = ctypes.c_int
    F = ctypes.c_float
    E = [ctypes.c_char_p, I]
    L.bicos_ref_match.argtypes = [P, P, I, I, I, I, ctypes.POINTER(_Cfg), P, P, I] + E
    L.bicos_ref_transform.argtypes = [P, I, I, I, I, I, I, P, I] + E
    L.bicos_ref_search.argtypes = [P, P, I, I, I, I, I, P, I] + E
    L.bicos_ref_agree.argtypes = [P, P, P, I, I, I, I, F, I, F, P, I] + E
    L.bicos_ref_agree_subpixel.argtypes = [P, P, P, I, I, I, I, F, F, I, F, P, P, I] + E
    L.bicos_ref_shim_selfcheck.argtypes = []
    for f in (L.bicos_ref_match, L.bicos_ref_transform, L.bicos_ref_search, L.bicos_ref_agree,
              L.bicos_ref_agree_subpixel, L.bicos_ref_shim_selfcheck):
        f.restype = I
    _LIBS[variant] = L
    return L


class RefError(RuntimeError):
    """The reference threw. `kind` names the exception type: "BICOS::Exception",
    "std::invalid_argument" or "other"."""

    def __init__(self, kind: str, message: str):
        super().__init__("%s: %s" % (kind, message))
        self.kind = kind
        self.message = message


_KINDS = {-1: "BICOS::Exception", -3: "std::invalid_argument"}


def _call(fn, *args):
    err = ctypes.create_string_buffer(256)
    rc = fn(*args, err, len(err))
    if rc < 0:
        raise RefError(_KINDS.get(rc, "other"), err.value.decode(errors="replace"))
    return rc


def _ptr(a: np.ndarray):
    return ctypes.c_void_p(a.ctypes.data)


def _threads(nthreads: Optional[int]) -> int:
    return nthreads if nthreads else 0     # 0: the stand-in's own bound (16)


def _stack(stack) -> np.ndarray:
    s = np.ascontiguousarray(np.asarray(stack))
    assert s.ndim == 3 and s.dtype in (np.uint8, np.uint16), (s.shape, s.dtype)
    return s


def shim_selfcheck(variant: str = "") -> int:
    """0, or the number of the first failed check of the cv:: stand-in (ref_driver.cpp)."""
    return lib(variant).bicos_ref_shim_selfcheck()


def required_bits(n: int, mode: int) -> int:
    return n * n - 2 * n + 3 if mode == 1 else 4 * n - 7      # src/impl/cpu.cpp, match()


def desc_words(n: int, mode: int) -> int:
    bits = required_bits(n, mode)
    return 1 if bits <= 32 else 2 if bits <= 64 else 4 if bits <= 128 else 8 if bits <= 256 else -1


def transform(stack, mode: int = 0, words: Optional[int] = None, nthreads=None,
              variant: str = "") -> np.ndarray:
    """Planar [n,H,W] stack -> descriptors [H,W,words] uint32 (descriptor_transform)."""
    s = _stack(stack)
    n, h, w = s.shape
    words = words or desc_words(n, mode)
    out = np.zeros((h, w, words), np.uint32)
    _call(lib(variant).bicos_ref_transform, _ptr(s), n, h, w, s.itemsize, mode, words, _ptr(out),
          _threads(nthreads))
    return out


def search(d0: np.ndarray, d1: np.ndarray, flags: int = NODUPES, max_lr_diff: int = -1,
           nthreads=None, variant: str = "") -> np.ndarray:
    d0 = np.ascontiguousarray(d0, np.uint32)
    d1 = np.ascontiguousarray(d1, np.uint32)
    h, w, words = d0.shape
    out = np.empty((h, w), np.int16)
    _call(lib(variant).bicos_ref_search, _ptr(d0), _ptr(d1), h, w, words, flags, max_lr_diff,
          _ptr(out), _threads(nthreads))
    return out


def agree(disp: np.ndarray, stack0, stack1, threshold: float, minvar_scaled: Optional[float],
          nthreads=None, variant: str = "") -> Tuple[np.ndarray, np.ndarray]:
    s0, s1 = _stack(stack0), _stack(stack1)
    n, h, w = s0.shape
    d = np.array(disp, np.int16, copy=True, order="C")
    corr = np.full((h, w), np.nan, np.float32)
    _call(lib(variant).bicos_ref_agree, _ptr(d), _ptr(s0), _ptr(s1), n, h, w, s0.itemsize,
          threshold, int(minvar_scaled is not None), float(minvar_scaled or 0.0), _ptr(corr),
          _threads(nthreads))
    return d, corr


def agree_subpixel(disp: np.ndarray, stack0, stack1, threshold: float, step: float,
                   minvar_scaled: Optional[float], nthreads=None,
                   variant: str = "") -> Tuple[np.ndarray, np.ndarray]:
    s0, s1 = _stack(stack0), _stack(stack1)
    n, h, w = s0.shape
    d = np.ascontiguousarray(disp, np.int16)
    out = np.empty((h, w), np.float32)
    corr = np.full((h, w), np.nan, np.float32)
    _call(lib(variant).bicos_ref_agree_subpixel, _ptr(d), _ptr(s0), _ptr(s1), n, h, w,
          s0.itemsize, threshold, step, int(minvar_scaled is not None),
          float(minvar_scaled or 0.0), _ptr(out), _ptr(corr), _threads(nthreads))
    return out, corr


def match(stack0, stack1, cfg=None, nthreads=None,
          variant: str = "") -> Tuple[np.ndarray, Optional[np.ndarray]]:
    """BICOS::impl::cpu::match. Returns (disparity, corrmap): int16 and None when the
    reference returned an int16 map, float32 and the float32 corrmap otherwise."""
    cfg = cfg or ReferenceConfig()
    s0, s1 = _stack(stack0), _stack(stack1)
    assert s0.shape == s1.shape and s0.dtype == s1.dtype
    n, h, w = s0.shape
    buf = np.empty((h, w), np.float32)
    corr = np.empty((h, w), np.float32)
    c = _cfg(cfg)
    kind = _call(lib(variant).bicos_ref_match, _ptr(s0), _ptr(s1), n, h, w, s0.itemsize,
                 ctypes.byref(c), _ptr(buf), _ptr(corr), _threads(nthreads))
    if kind == 0:
        return buf.view(np.int16).reshape(-1)[: h * w].reshape(h, w).copy(), None
    return buf, corr
