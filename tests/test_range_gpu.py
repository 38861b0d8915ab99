"""The disparity range on the GPU (include/bicos_c.h, "disparity range"): the windowed
matrix-core search (search_range.hip) against the numpy restatement of tests/test_range_api.py,
the whole match through the device, host and C++ entry points against oracle.transform ->
the restatement -> oracle.agree / agree_subpixel. Every comparison is exact.
"""
import functools
import os
import subprocess

import numpy as np
import pytest

from libbicos_amd.synthetic import stereo_stack
from tests.test_range_api import rolled_descriptors, search_range

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -32768


def dev(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:
        a = a.view(np.int16)
    return torch.from_numpy(a).cuda()


def host(t):
    return t.cpu().numpy()


def same(a, b, what=""):
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    if not np.array_equal(a.view(np.uint8), b.view(np.uint8)):
        ne = np.argwhere(~((a == b) | ((a != a) & (b != b))))
        raise AssertionError("%s: %d of %d differ, first at %s: got %s want %s" % (
            what, len(ne), a.size, ne[:4].tolist(), [a[tuple(i)] for i in ne[:4]],
            [b[tuple(i)] for i in ne[:4]]))


def _pack(desc):
    from libbicos_amd import _lib
    H, W, words = desc.shape
    pitch = _lib.lib().bicos_desc_pitch(W, words)
    out = np.zeros((H, pitch), np.uint32)
    out[:, : W * words] = desc.reshape(H, W * words)
    return out.view(np.int32)


# words, period, low bits kept (ties): 32-bit with ties, periodic 128-bit, 256-bit
DESCS = {"w1_ties": (1, None, 10), "w4_period97": (4, 97, None), "w8": (8, None, None)}
SHAPES = [(3, 301), (2, 1100), (2, 20)]
FLAGS = [(1, -1), (2, 1), (3, 2)]


def ranges(W):
    return [(0, 63), (-17, 5), (20, 20), (3, 40), (250, 400), (-400, -290), (-(W - 1), W - 1)]


@functools.lru_cache(maxsize=None)
def descs(kind, H, W):
    words, period, low = DESCS[kind]
    d0, d1 = rolled_descriptors(H, W, words, period, low)
    return words, d0, d1


@functools.lru_cache(maxsize=None)
def expected(kind, H, W, flags, lr, lo, hi):
    _, d0, d1 = descs(kind, H, W)
    return search_range(d0, d1, flags, lo, hi, lr)


def check_search(gpu, kind, H, W, flags, lr, bits=0):
    words, d0, d1 = descs(kind, H, W)
    g0, g1 = dev(_pack(d0)), dev(_pack(d1))
    for lo, hi in ranges(W):
        got = host(gpu.search(g0, g1, W, words, flags, lr, bits=bits, disparity_range=(lo, hi)))
        same(got, expected(kind, H, W, flags, lr, lo, hi), "range (%d, %d)" % (lo, hi))
    # the covering range is the unrestricted search, byte for byte
    cover = host(gpu.search(g0, g1, W, words, flags, lr, bits=bits,
                            disparity_range=(-(W - 1), W - 1)))
    same(cover, host(gpu.search(g0, g1, W, words, flags, lr, bits=bits)), "covering range")
    # ... and so is any wider one (the window is clamped to the row's disparities)
    wide = host(gpu.search(g0, g1, W, words, flags, lr, bits=bits,
                           disparity_range=(-2 ** 31, 2 ** 31 - 1)))
    same(wide, cover, "widest range")


@pytest.mark.parametrize("flags,lr", FLAGS, ids=["nodupes", "cons", "nodupes_cons"])
@pytest.mark.parametrize("H,W", SHAPES, ids=lambda v: str(v))
@pytest.mark.parametrize("kind", list(DESCS))
def test_search_range_matches_the_restatement(gpu, kind, H, W, flags, lr):
    check_search(gpu, kind, H, W, flags, lr)


@pytest.mark.parametrize("tiles,waves", [(4, 8), (2, 8), (4, 3), (2, 1)])
@pytest.mark.parametrize("kind", list(DESCS))
def test_search_range_tile_and_wave_counts(gpu, kind, tiles, waves):
    """4 tiles per wave are otherwise chosen only for frames of hundreds of rows: 2 x 1100 is
    more than one workgroup per row at 8 waves x 4 tiles x 32 col0 = 1024 and three LDS fills
    at 256 bits"""
    try:
        gpu.tune(64, tiles, waves, 0)
        for flags, lr in ((1, -1), (2, 1)):
            check_search(gpu, kind, 2, 1100, flags, lr)
    finally:
        gpu.tune(0, 0, 0, 0)


@pytest.mark.parametrize("bits", [154, 0], ids=["3_ksteps", "4_ksteps_bit255"])
@pytest.mark.parametrize("flags,lr", FLAGS, ids=["nodupes", "cons", "nodupes_cons"])
def test_search_range_256_bit_kstep_counts(gpu, bits, flags, lr):
    """words 8 with a used-bits hint of 154 (3 K-steps; the bits above are zero) and with
    none (4 K-steps; bit 255 set on the left side only must be ignored, as in the full-row
    search)"""
    H, W = 3, 301
    _, d0, d1 = descs("w8", H, W)
    d0, d1 = d0.copy(), d1.copy()
    if bits:
        for d in (d0, d1):
            d[..., 4] &= np.uint32((1 << (bits - 128)) - 1)
            d[..., 5:] = 0
    ref0, ref1 = d0, d1
    if not bits:
        d0 = d0.copy()
        d0[..., 7] |= np.uint32(0x80000000)
    g0, g1 = dev(_pack(d0)), dev(_pack(d1))
    for lo, hi in ranges(W):
        got = host(gpu.search(g0, g1, W, 8, flags, lr, bits=bits, disparity_range=(lo, hi)))
        same(got, search_range(ref0, ref1, flags, lo, hi, lr), "range (%d, %d)" % (lo, hi))


def test_search_range_is_not_a_no_op(gpu):
    """the windows change the result: against the unrestricted search, at least 7 % of the
    pixels differ for each of the four near ranges wherever it keeps any pixel"""
    H, W = 3, 301
    for kind in DESCS:
        words, d0, d1 = descs(kind, H, W)
        g0, g1 = dev(_pack(d0)), dev(_pack(d1))
        full = host(gpu.search(g0, g1, W, words, 1))
        for lo, hi in ranges(W)[:4]:
            got = host(gpu.search(g0, g1, W, words, 1, disparity_range=(lo, hi)))
            if (full != INVALID).any():
                assert (got != full).mean() >= 0.07, (kind, lo, hi)
            ok = got != INVALID
            assert ((got[ok] >= lo) & (got[ok] <= hi)).all()


def test_search_range_argument_errors(gpu):
    _, d0, d1 = descs("w4_period97", 3, 301)
    with pytest.raises(ValueError):
        gpu.search(dev(_pack(d0)), dev(_pack(d1)), 301, 4, 1, disparity_range=(5, 4))


# ------------------------------------------------------------------ whole match
RANGE = (8, 71)
MATCH_CASES = {
    "n8_u8": dict(n=8, dt=np.uint8, cfg=dict(nxcorr_threshold=0.9)),
    "n33_u8_raw": dict(n=33, dt=np.uint8, cfg=dict(nxcorr_threshold=None)),
    "n33_u16_subpixel_minvar": dict(n=33, dt=np.uint16, cfg=dict(
        nxcorr_threshold=0.9, subpixel_step=0.25, min_variance=2.0)),
    "n40_consistency": dict(n=40, dt=np.uint8, cfg=dict(nxcorr_threshold=0.9, variant=1,
                                                        max_lr_diff=1)),
    "n40_consistency_raw": dict(n=40, dt=np.uint8, cfg=dict(nxcorr_threshold=None, variant=1,
                                                            max_lr_diff=1, no_dupes=True)),
}


@functools.lru_cache(maxsize=None)
def stacks(n, dt):
    return stereo_stack(n, 4, 301, dt)


@functools.lru_cache(maxsize=None)
def expected_raw(n, dt, mode, variant, max_lr_diff, no_dupes):
    from oracle import oracle as O
    O.build()
    L, R = stacks(n, dt)
    d0, d1 = O.transform(L, mode), O.transform(R, mode)
    flags = (2 | (1 if no_dupes else 0)) if variant else 1
    return search_range(d0, d1, flags, RANGE[0], RANGE[1], max_lr_diff if variant else -1)


def expected_match(case):
    """oracle.transform -> the restatement -> oracle.agree / agree_subpixel (the route of
    oracle/ref_numpy.py match)"""
    from oracle import oracle as O
    n, dt, cfg = case["n"], case["dt"], case["cfg"]
    L, R = stacks(n, dt)
    raw = expected_raw(n, dt, cfg.get("mode", 0), cfg.get("variant", 0), cfg.get("max_lr_diff", 1),
                       cfg.get("no_dupes", False))
    thr = cfg.get("nxcorr_threshold")
    if thr is None:
        return raw, None
    mv = cfg.get("min_variance")
    mv = None if mv is None else float(np.float32(mv) * np.float32(n))
    if cfg.get("subpixel_step") is not None:
        return O.agree_subpixel(raw, L, R, thr, cfg["subpixel_step"], mv)
    d, corr = O.agree(raw, L, R, thr, mv)
    return d.astype(np.float32), corr


@pytest.mark.parametrize("name", list(MATCH_CASES))
def test_match_with_a_range_bit_exact(gpu, name):
    from libbicos_amd.device import MatchConfig
    case = MATCH_CASES[name]
    L, R = stacks(case["n"], case["dt"])
    d, c = gpu.match(dev(L), dev(R), MatchConfig(disparity_range=RANGE, **case["cfg"]))
    rd, rc = expected_match(case)
    same(host(d), rd, "disparity")
    if rc is None:
        assert c is None
    else:
        same(host(c), rc, "corrmap")


def test_match_range_changes_the_map(gpu):
    """n = 8: the ranged map differs from the unrestricted one (a no-op would not)"""
    from libbicos_amd.device import MatchConfig
    L, R = stacks(8, np.uint8)
    a, _ = gpu.match(dev(L), dev(R), MatchConfig(nxcorr_threshold=None))
    b, _ = gpu.match(dev(L), dev(R), MatchConfig(nxcorr_threshold=None, disparity_range=RANGE))
    a, b = host(a), host(b)
    assert (a != b).mean() > 0.05
    assert (b != INVALID).mean() > 0.9
    ok = b != INVALID
    assert ((b[ok] >= RANGE[0]) & (b[ok] <= RANGE[1])).all()


def test_match_plan_is_unchanged_by_the_feature(gpu):
    """no range set: the plan (fused agree for n = 33 u8) is what it was"""
    from libbicos_amd import _lib
    from libbicos_amd.device import MatchConfig
    L, R = stereo_stack(33, 32, 512)
    plan = gpu.plan(dev(L), dev(R), MatchConfig(nxcorr_threshold=0.9))
    assert plan & _lib.PLAN_MATRIX_CORES and plan & _lib.PLAN_AGREE_IN_SEARCH


def test_match_double_precision_with_a_range(gpu):
    """Precision::DOUBLE: byte equality with the float64 oracle (agree_subpixel_f64 on the
    restated ranged search), and, as a differently rounded witness, the numpy float64
    restatement of tests/test_gpu_parity.py test_double_subpixel_exact_depths within 1e-12"""
    from libbicos_amd.device import MatchConfig
    from oracle import oracle as O
    from tests.test_gpu_parity import _subpixel_f64
    n, step = 12, 0.25
    L, R = stereo_stack(n, 4, 301, dmin=3, drange=30, seed=n + 17)
    d0, d1 = O.transform(L, 1), O.transform(R, 1)
    raw = search_range(d0, d1, 1, 2, 40)
    out, corr = gpu.match(dev(L), dev(R), MatchConfig(
        nxcorr_threshold=0.5, subpixel_step=step, mode=1, precision=1, disparity_range=(2, 40)))
    ref_d, ref_c = _subpixel_f64(L, R, raw, 0.5, step, None)
    got_c = host(corr)
    assert got_c.dtype == np.float64
    fin = np.isfinite(ref_c)
    assert (np.isfinite(got_c) == fin).all()
    assert np.abs(got_c[fin] - ref_c[fin]).max() < 1e-12
    same(host(out), ref_d, "disparity")
    ora_d, ora_c = O.agree_subpixel_f64(raw, L, R, 0.5, step, None)
    from tests.double_cases import same as same_bits
    same_bits(host(out), ora_d)
    same_bits(got_c, ora_c)


# -------------------------------------------------------------------- host path
@pytest.mark.parametrize("name", ["n8_u8", "n33_u16_subpixel_minvar", "n40_consistency"])
def test_pybicos_match_with_a_range_equals_the_device_path(gpu, name):
    import pybicos
    from libbicos_amd.device import MatchConfig
    case = MATCH_CASES[name]
    kw = case["cfg"]
    L, R = stacks(case["n"], case["dt"])
    cfg = pybicos.Config()
    cfg.nxcorr_threshold = kw["nxcorr_threshold"]
    cfg.subpixel_step = kw.get("subpixel_step")
    cfg.min_variance = kw.get("min_variance")
    if kw.get("variant"):
        cfg.set_consistency(kw["max_lr_diff"], kw.get("no_dupes", False))
    cfg.disparity_range = RANGE
    hd, hc = pybicos.match(list(L), list(R), cfg)
    d, c = gpu.match(dev(L), dev(R), MatchConfig(disparity_range=RANGE, **kw))
    same(hd, host(d), "disparity")
    same(hc, host(c), "corrmap")
    rd, rc = expected_match(case)
    same(hd, rd, "disparity vs oracle route")


# -------------------------------------------------------------------------- C++
RANGE_EXE = os.path.join(ROOT, "build", "range_consumer", "range_style")


def _range_exe():
    """build() builds it against the installed tree; built here if it has not been"""
    if not os.access(RANGE_EXE, os.X_OK):
        from tools.cpp_install import build_range_consumer, install_and_build_consumer
        prefix = os.path.join(ROOT, "build", "bicos_install")
        install_and_build_consumer(prefix, os.path.join(ROOT, "build", "consumer"))
        build_range_consumer(prefix, os.path.dirname(RANGE_EXE))
    return RANGE_EXE


def _run_cpp(tmp_path, case, lo, hi):
    n, dt, cfg = case["n"], case["dt"], case["cfg"]
    L, R = stacks(n, dt)
    inp = tmp_path / "in.bin"
    with open(inp, "wb") as f:
        f.write(np.array([n, L.shape[1], L.shape[2], np.dtype(dt).itemsize], np.int32).tobytes())
        f.write(np.ascontiguousarray(L).tobytes())
        f.write(np.ascontiguousarray(R).tobytes())
    g = cfg.get
    nxc = g("nxcorr_threshold")
    args = [_range_exe(), str(inp), str(tmp_path / "out"), str(-1 if nxc is None else nxc),
            str(g("subpixel_step") or -1), str(-1 if g("min_variance") is None else g("min_variance")),
            str(g("variant", 0)), str(g("max_lr_diff", 1)), str(int(g("no_dupes", False))),
            str(lo), str(hi)]
    return subprocess.run(args, capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("name", ["n8_u8", "n33_u8_raw", "n40_consistency"])
def test_cpp_config_disparity_range(gpu, tmp_path, name):
    """BICOS::Config::disparity_range through the cv::Mat and the native overload equals the
    Python device result (and so the oracle route)"""
    from libbicos_amd.device import MatchConfig
    case = MATCH_CASES[name]
    L, R = stacks(case["n"], case["dt"])
    r = _run_cpp(tmp_path, case, *RANGE)
    assert r.returncode == 0, r.stdout + r.stderr
    d, c = gpu.match(dev(L), dev(R), MatchConfig(disparity_range=RANGE, **case["cfg"]))
    d, c = host(d), (host(c) if c is not None else None)
    for branch in ("mat", "native"):
        got = np.fromfile(tmp_path / ("out.%s.disp" % branch), dtype=d.dtype).reshape(d.shape)
        same(got, d, branch + " disparity")
        cpath = tmp_path / ("out.%s.corr" % branch)
        if c is None:
            assert not cpath.exists()
        else:
            same(np.fromfile(cpath, dtype=c.dtype).reshape(c.shape), c, branch + " corrmap")


def test_cpp_range_min_above_max_throws(gpu, tmp_path):
    r = _run_cpp(tmp_path, MATCH_CASES["n8_u8"], 5, 4)
    assert r.returncode == 5, r.stdout + r.stderr
    assert r.stdout.startswith("exception:") and "disparity" in r.stdout
