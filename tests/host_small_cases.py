"""Frames shared by the host-buffer pipeline's tests: tests/test_host_plan.py (the CPU check
of the pipeline's arithmetic must cover every one of them) and tests/test_host_small_gpu.py
(the GPU runs, in this process and in its child processes). No torch, no GPU here."""
import ctypes

import numpy as np

from libbicos_amd.synthetic import SEED, stereo_stack

# (n, H, W, dtype): bytes of a band = 2 n band_rows W itemsize, around the 4096-byte page the
# upload split rounds to, and bands of under a page in frames of 2, 4 and 8 bands
SMALL = [
    (4, 8, 8, np.uint8),       # 512: one band
    (8, 5, 51, np.uint8),      # 4080: one band, just under 4096
    (8, 4, 64, np.uint8),      # exactly 4096
    (10, 5, 41, np.uint8),     # 4100: second part of 4 bytes
    (12, 9, 19, np.uint8),     # 4104: second part of 8 bytes
    (17, 1, 241, np.uint8),    # 8194: first part 8192, second part 2
    (6, 64, 10, np.uint8),     # 3840: 2 bands
    (6, 64, 5, np.uint16),     # 3840: 2 bands
    (6, 256, 5, np.uint8),     # 3840: 4 bands
    (6, 257, 5, np.uint8),     # 3900: 4 bands, ragged last band of 62 rows
    (5, 1030, 3, np.uint8),    # 3870: 8 bands, last band of 127 rows
    (6, 1030, 2, np.uint8),    # 3096: 8 bands
]
MULTI_BAND = [s for s in SMALL if s[1] >= 64]
# full-size bands: 4 and 8 of them, the 3 slots reused
LARGE = [(12, 301, 256, np.uint8), (12, 1100, 256, np.uint8)]
# a band's bytes of a map = 8 * 64 k + r, 0 < r < 8: the delivery's last chunk (1 band of
# 129 float pixels, 2 such bands, 257 int16 or float pixels, 4 bands of 75 * 99 = 128 * 58 + 1
# float pixels)
DELIVERY_TAIL = [(4, 43, 3, np.uint8), (4, 86, 3, np.uint8), (12, 1, 257, np.uint8),
                 (12, 300, 99, np.uint8)]
# Precision.DOUBLE through the band offsets
DOUBLE = [(12, 63, 256, np.uint8), (12, 301, 256, np.uint8), (12, 1100, 256, np.uint8),
          (6, 257, 5, np.uint8), (5, 1030, 3, np.uint8)]
# one engine, changing frames: (n, H, W, dtype, config)
SEQUENCE = [
    (12, 1100, 256, np.uint8, dict(nxcorr_threshold=0.5)),
    (4, 8, 8, np.uint8, dict(nxcorr_threshold=0.5)),
    (12, 301, 256, np.uint16, dict(nxcorr_threshold=0.5, precision=1)),
    (6, 64, 10, np.uint8, dict(nxcorr_threshold=None)),
    (12, 1100, 256, np.uint8, dict(nxcorr_threshold=0.5)),
]

CONFIGS = {
    "raw": dict(nxcorr_threshold=None),
    "thr": dict(nxcorr_threshold=0.5),
    "subpixel": dict(nxcorr_threshold=0.5, subpixel_step=0.25),
    "consistency": dict(nxcorr_threshold=0.5, variant=1, max_lr_diff=1, no_dupes=True),
}


def every_frame():
    """(n, H, W, itemsize) of every frame a GPU test of the host path's small bands runs"""
    frames = SMALL + LARGE + DELIVERY_TAIL + DOUBLE + [s[:4] for s in SEQUENCE]
    return sorted({(n, H, W, np.dtype(dt).itemsize) for n, H, W, dt in frames})


def case_id(shape):
    n, H, W, dt = shape[:4]
    return "n%d_%dx%d_%s" % (n, H, W, np.dtype(dt).name)


def stacks(n, H, W, dt, seed=SEED):
    return stereo_stack(n, H, W, dt, dmin=1, drange=2, seed=seed)


def c_config(**kw):
    """(BicosConfig, has_nxcorr) of a config given as MatchConfig's fields; torch-free
    (libbicos_amd.device.MatchConfig.to_c is the same mapping, behind `import torch`)."""
    from libbicos_amd import _lib
    thr = kw.get("nxcorr_threshold", 0.5)
    step, mv = kw.get("subpixel_step"), kw.get("min_variance")
    c = _lib.BicosConfig(float(0.5 if thr is None else thr), float(-1.0 if step is None else step),
                         float(-1.0 if mv is None else mv), int(kw.get("mode", 0)),
                         int(kw.get("precision", 0)), int(kw.get("variant", 0)),
                         int(kw.get("max_lr_diff", 1)), int(bool(kw.get("no_dupes", False))))
    return c, int(thr is not None)


GUARD = 0xA5
PAD = 96  # guard bytes either side of a map (not a multiple of 64: the maps start unaligned)


def match_host_guarded(L, R, engine=None, **kw):
    """bicos_match_host on the stacks' planes, the maps written into the middle of larger
    buffers filled with GUARD. Returns (disparity, corrmap or None) as copies; asserts that
    every guard byte and both input stacks are as they were."""
    from libbicos_amd import _lib
    n, H, W = L.shape
    cfgc, has = c_config(**kw)
    L0, R0 = L.copy(), R.copy()
    p0 = (ctypes.c_void_p * n)(*[L[t].ctypes.data for t in range(n)])
    p1 = (ctypes.c_void_p * n)(*[R[t].ctypes.data for t in range(n)])
    ddt = np.float32 if has else np.int16
    cdt = np.float64 if kw.get("precision") else np.float32
    bufs = []
    for dt in (ddt, cdt):
        buf = np.full(PAD + H * W * np.dtype(dt).itemsize + PAD, GUARD, np.uint8)
        bufs.append(buf)
    dptr = bufs[0].ctypes.data + PAD
    cptr = bufs[1].ctypes.data + PAD if has else None
    rc = _lib.lib().bicos_match_host(engine, p0, p1, n, H, W, 0, L.dtype.itemsize,
                                     ctypes.byref(cfgc), has, dptr, cptr)
    _lib.check(rc, "bicos_match_host")
    for buf in bufs:
        assert (buf[:PAD] == GUARD).all() and (buf[-PAD:] == GUARD).all(), "guard bytes written"
    if not has:
        assert (bufs[1] == GUARD).all(), "a corrmap was written without the NXC stage"
    assert np.array_equal(L, L0) and np.array_equal(R, R0), "the input images changed"
    disp = bufs[0][PAD:-PAD].copy().view(ddt).reshape(H, W)
    corr = bufs[1][PAD:-PAD].copy().view(cdt).reshape(H, W) if has else None
    return disp, corr
