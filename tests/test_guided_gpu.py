"""The disparity guide on the GPU (include/bicos_c.h, "disparity guide"): the guided
matrix-core search (search_guided.hip) and the guide builder against the numpy restatements of
tests/test_guided_api.py, the whole guided match through the device and host entry points
against oracle.transform -> the restatement -> oracle.agree / agree_subpixel. Every comparison
is exact.
"""
import functools

import numpy as np
import pytest

from libbicos_amd.synthetic import stereo_stack
from tests.test_guided_api import (INT_MAX, INT_MIN, constant_guide, guide_ref, row_costs,
                                   search_guided)
from tests.test_range_gpu import (DESCS, FLAGS, MATCH_CASES, RANGE, SHAPES, _pack, descs, dev,
                                  expected as expected_range, host, ranges, same, stacks)

pytestmark = pytest.mark.gpu

INV = -32768
NO_WINDOW = (INT_MIN, INT_MAX)


@functools.lru_cache(maxsize=None)
def costs(kind, H, W):
    _, d0, d1 = descs(kind, H, W)
    return row_costs(d0, d1)


@functools.lru_cache(maxsize=None)
def guides(H, W):
    """name -> (guide, global window): where the per-lane windows, the wave-uniform spans and
    the mask-skipping test can go wrong"""
    rng = np.random.default_rng(1000 * H + W)
    out = {}
    # a random centre and width per pixel
    centre = rng.integers(-W, W, (H, W))
    width = rng.integers(0, 40, (H, W))
    g = np.stack([centre - width, centre + width], -1).astype(np.int16)
    out["random"] = (g, NO_WINDOW)
    # a step inside one tile: columns < 150 around the planted -20, the rest far to the left
    g = constant_guide(H, W, 250, 400)
    g[:, :150] = (-22, -18)
    out["step_in_a_tile"] = (g, NO_WINDOW)
    # one covering pixel in a row of +-1 windows: its tile's union is the whole row, its
    # intersection is empty
    g = constant_guide(H, W, -21, -19)
    g[:, min(W - 1, 77)] = (-(W - 1), W - 1)
    out["one_covering_pixel"] = (g, NO_WINDOW)
    # 30 % empty windows (lo > hi), and an all-empty row
    g = constant_guide(H, W, -25, -15)
    g[rng.random((H, W)) < 0.3] = (3, 2)
    g[H - 1] = (32767, -32768)
    out["empty_30_percent_and_a_row"] = (g, NO_WINDOW)
    # the int16 extremes
    out["int16_extremes"] = (constant_guide(H, W, -32768, 32767), NO_WINDOW)
    g = constant_guide(H, W, -32768, -20)
    g[:, 1::2] = (-20, 32767)
    out["int16_half_lines"] = (g, NO_WINDOW)
    # windows wholly outside the image, on either side, among a few that reach into it
    g = constant_guide(H, W, W + 5, W + 50)
    g[:, 1::2] = (-W - 50, -W - 5)
    g[:, 5::16] = (-W - 50, -W + 30)
    out["outside_the_image"] = (g, NO_WINDOW)
    # a global window that cuts every pixel's window
    lo = rng.integers(-60, -25, (H, W))
    g = np.stack([lo, lo + rng.integers(20, 60, (H, W))], -1).astype(np.int16)
    out["global_window_cuts_all"] = (g, (-24, -8))
    return out


def check_guides(gpu, kind, H, W, flags, lr, bits=0, d01=None, constants=True):
    words, d0, d1 = descs(kind, H, W)
    ref0, ref1, cst = d0, d1, costs(kind, H, W)
    if d01 is not None:
        d0, d1, ref0, ref1 = d01
        cst = row_costs(ref0, ref1)
    g0, g1 = dev(_pack(d0)), dev(_pack(d1))
    for name, (g, (lo, hi)) in guides(H, W).items():
        got = host(gpu.search(g0, g1, W, words, flags, lr, bits=bits, guide=dev(g),
                              disparity_range=None if (lo, hi) == NO_WINDOW else (lo, hi)))
        same(got, search_guided(ref0, ref1, flags, g, lo, hi, lr, costs=cst), name)
    if not constants:
        return
    # a constant guide is the ranged search: the restatement's and the range kernel's
    for lo, hi in ranges(W):
        g = dev(constant_guide(H, W, max(lo, -32768), min(hi, 32767)))
        got = host(gpu.search(g0, g1, W, words, flags, lr, bits=bits, guide=g,
                              disparity_range=(lo, hi)))
        what = "constant guide (%d, %d)" % (lo, hi)
        if d01 is None:
            same(got, expected_range(kind, H, W, flags, lr, lo, hi), what)
        same(got, host(gpu.search(g0, g1, W, words, flags, lr, bits=bits,
                                  disparity_range=(lo, hi))), what + " vs the range kernel")
        # ... with no global window too, but for Consistency's reverse search, which then
        # runs over the whole row
        if not flags & 2:
            same(host(gpu.search(g0, g1, W, words, flags, lr, bits=bits, guide=g)), got,
                 what + " without a global window")
    # a covering guide under a covering window is the unrestricted search
    cover = dev(constant_guide(H, W, -(W - 1), W - 1))
    full = host(gpu.search(g0, g1, W, words, flags, lr, bits=bits))
    same(host(gpu.search(g0, g1, W, words, flags, lr, bits=bits, guide=cover,
                         disparity_range=(-(W - 1), W - 1))), full, "covering guide and window")
    same(host(gpu.search(g0, g1, W, words, flags, lr, bits=bits, guide=cover)), full,
         "covering guide, no window")


@pytest.mark.parametrize("flags,lr", FLAGS, ids=["nodupes", "cons", "nodupes_cons"])
@pytest.mark.parametrize("H,W", SHAPES, ids=lambda v: str(v))
@pytest.mark.parametrize("kind", list(DESCS))
def test_search_guided_matches_the_restatement(gpu, kind, H, W, flags, lr):
    check_guides(gpu, kind, H, W, flags, lr)


@pytest.mark.parametrize("tiles,waves", [(4, 8), (2, 8), (4, 3), (2, 1)])
@pytest.mark.parametrize("kind", list(DESCS))
def test_search_guided_tile_and_wave_counts(gpu, kind, tiles, waves):
    """the (tiles, waves) of test_search_range_tile_and_wave_counts: 2 x 1100 is more than one
    workgroup per row at 8 waves x 4 tiles and several LDS fills at 256 bits"""
    try:
        gpu.tune(64, tiles, waves, 0)
        for flags, lr in ((1, -1), (2, 1)):
            check_guides(gpu, kind, 2, 1100, flags, lr)
    finally:
        gpu.tune(0, 0, 0, 0)


@pytest.mark.parametrize("bits", [154, 0], ids=["3_ksteps", "4_ksteps_bit255"])
@pytest.mark.parametrize("flags,lr", FLAGS, ids=["nodupes", "cons", "nodupes_cons"])
def test_search_guided_256_bit_kstep_counts(gpu, bits, flags, lr):
    """words 8 with a used-bits hint of 154 (3 K-steps) and with none (4 K-steps; bit 255 set
    on the left side only must be ignored), as test_search_range_256_bit_kstep_counts"""
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
    check_guides(gpu, "w8", H, W, flags, lr, bits=bits, d01=(d0, d1, ref0, ref1))


def test_search_guided_is_not_a_no_op(gpu):
    """the guide changes the result: against the ranged search over the same global window,
    taking the planted disparity -20 out of the even columns' windows changes those columns"""
    H, W = 3, 301
    words, d0, d1 = descs("w8", H, W)
    g0, g1 = dev(_pack(d0)), dev(_pack(d1))
    ranged = host(gpu.search(g0, g1, W, words, 1, disparity_range=(-40, 0)))
    assert (ranged[:, : W - 20] == -20).all()
    g = constant_guide(H, W, -40, 0)
    g[:, 0::2, 1] = -21
    got = host(gpu.search(g0, g1, W, words, 1, disparity_range=(-40, 0), guide=dev(g)))
    assert (got[:, 1: W - 20: 2] == -20).all()
    assert (got[:, 0: W - 20: 2] != -20).all()


def test_search_guided_views_and_guards(gpu):
    """the guide as a view of a larger buffer (pitch > cols, a base 4 pixels in) and the output
    inside guard elements that stay as they were"""
    import torch
    H, W = 3, 301
    words, d0, d1 = descs("w4_period97", H, W)
    g0, g1 = dev(_pack(d0)), dev(_pack(d1))
    g, (lo, hi) = guides(H, W)["random"]
    big = torch.full((H + 2, W + 13, 2), 12345, dtype=torch.int16, device="cuda")
    view = big[1: 1 + H, 4: 4 + W]
    view.copy_(dev(g))
    assert view.stride(0) == 2 * (W + 13) and not view.is_contiguous()
    pad = 64
    buf = torch.full((pad + H * W + pad,), -12345, dtype=torch.int16, device="cuda")
    out = buf[pad: pad + H * W].view(H, W)
    for flags, lr in FLAGS:
        buf.fill_(-12345)
        gpu.search(g0, g1, W, words, flags, lr, guide=view, out=out)
        same(host(out), search_guided(d0, d1, flags, g, lo, hi, lr,
                                      costs=costs("w4_period97", H, W)), "view")
        b = host(buf)
        assert (b[:pad] == -12345).all() and (b[pad + H * W:] == -12345).all()
    assert (host(big)[0] == 12345).all() and (host(big)[:, :4] == 12345).all()
    # an odd offset in int16 units is a misaligned base
    with pytest.raises(ValueError, match="aligned"):
        odd = torch.zeros((H * W * 2 + 2,), dtype=torch.int16, device="cuda")[1: 1 + H * W * 2]
        gpu.search(g0, g1, W, words, 1, guide=odd.view(H, W, 2))


def test_search_guided_argument_errors(gpu):
    import torch
    H, W = 3, 301
    words, d0, d1 = descs("w4_period97", H, W)
    g0, g1 = dev(_pack(d0)), dev(_pack(d1))
    good = dev(constant_guide(H, W, -5, 5))
    with pytest.raises(ValueError):
        gpu.search(g0, g1, W, words, 1, guide=good, disparity_range=(5, 4))
    with pytest.raises(ValueError, match="shape"):
        gpu.search(g0, g1, W, words, 1, guide=good[:, :-1])
    with pytest.raises(ValueError, match="int16"):
        gpu.search(g0, g1, W, words, 1, guide=good.to(torch.int32))
    with pytest.raises(ValueError, match="must be on"):
        gpu.search(g0, g1, W, words, 1, guide=good.cpu())


# ------------------------------------------------------------------ the builder
def prior_map(dtype, sentinel):
    """5 x 70: smooth disparities with fractions (float), 20 % invalid -- NaN, and the float
    sentinel where it counts --, one fully invalid 3 x 9 patch, one isolated valid pixel"""
    rng = np.random.default_rng(5)
    r, c = np.mgrid[0:5, 0:70]
    v = 20 + 3 * r + 0.37 * c + rng.normal(0, 2, (5, 70))
    if dtype == np.int16:
        p = np.round(v).astype(np.int16)
        p[rng.random((5, 70)) < 0.2] = INV
        p[1:4, 30:39] = INV
        p[2, 34] = -7
        p[0, 0], p[4, 69] = 32767, -32767
        return p
    p = v.astype(np.float32)
    bad = rng.random((5, 70)) < 0.2
    p[bad] = np.nan
    p[bad & (rng.random((5, 70)) < 0.5)] = -32768.0  # invalid only with the sentinel flag
    p[1:4, 30:39] = np.nan
    p[2, 34] = -7.5
    p[0, 0], p[4, 69], p[0, 69] = np.inf, -np.inf, 1e9
    return p


@pytest.mark.parametrize("shape", [(14, 209), (16, 215)], ids=str)
@pytest.mark.parametrize("spread", [0, 1, 3])
@pytest.mark.parametrize("scale", [1, 2, 3])
@pytest.mark.parametrize("kind", ["int16", "float32_sentinel", "float32_nan_only"])
def test_guide_builder_matches_the_restatement(gpu, kind, scale, spread, shape):
    import torch
    dtype = np.int16 if kind == "int16" else np.float32
    sentinel = kind != "float32_nan_only"
    prior = prior_map(dtype, sentinel)
    p = torch.from_numpy(prior).cuda()
    for radius, fallback in ((0, (3, 2)), (5, None), (32767, (-32768, 32767))):
        want, wc = guide_ref(prior, shape, radius, spread, scale,
                             fallback or (-32767, 32767), sentinel)
        counts = torch.full((2,), -1, dtype=torch.int32, device="cuda")
        got = gpu.guide_from_disparity(p, radius, spread, scale, fallback, shape, sentinel,
                                       counts=counts)
        same(host(got), want, "guide r%d" % radius)
        assert counts.tolist() == wc and sum(wc) == shape[0] * shape[1]
        assert wc[0] and (wc[1] or spread == 3)


def test_guide_builder_default_shape_view_output_and_host_entry(gpu):
    import torch
    from libbicos_amd import pybicos
    prior = prior_map(np.float32, True)
    want, wc = guide_ref(prior, (10, 140), 2, 1, 2)
    p = torch.from_numpy(prior).cuda()
    same(host(gpu.guide_from_disparity(p, 2, spread=1, scale=2)), want, "default shape")
    big = torch.full((12, 150, 2), 777, dtype=torch.int16, device="cuda")
    view = big[1:11, 6:146]
    assert gpu.guide_from_disparity(p, 2, spread=1, scale=2, out=view) is view
    same(host(view.contiguous()), want, "view")
    b = host(big)
    assert (b[0] == 777).all() and (b[11] == 777).all() and (b[:, :6] == 777).all() and \
        (b[:, 146:] == 777).all()
    g, stats = pybicos.guide_from_disparity(prior, 2, spread=1, scale=2)
    same(g, want, "host entry")
    assert [stats["from_prior"], stats["fallback"]] == wc


# ------------------------------------------------------------------ whole match
def _cfg(case, **extra):
    from libbicos_amd.device import MatchConfig
    return MatchConfig(disparity_range=RANGE, **case["cfg"], **extra)


def _flags(cfg):
    if cfg.get("variant", 0):
        return 2 | (1 if cfg.get("no_dupes", False) else 0), cfg.get("max_lr_diff", 1)
    return 1, -1


@functools.lru_cache(maxsize=None)
def match_costs(n, dt, mode):
    from oracle import oracle as O
    O.build()
    L, R = stacks(n, dt)
    d0, d1 = O.transform(L, mode), O.transform(R, mode)
    return d0, d1, row_costs(d0, d1)


def expected_guided_match(case, guide):
    """oracle.transform -> the guided restatement -> oracle.agree / agree_subpixel, the route
    of tests/test_range_gpu.py expected_match"""
    from oracle import oracle as O
    n, dt, cfg = case["n"], case["dt"], case["cfg"]
    L, R = stacks(n, dt)
    d0, d1, cst = match_costs(n, dt, cfg.get("mode", 0))
    flags, lr = _flags(cfg)
    raw = search_guided(d0, d1, flags, guide, RANGE[0], RANGE[1], lr, costs=cst)
    thr = cfg.get("nxcorr_threshold")
    if thr is None:
        return raw, None
    mv = cfg.get("min_variance")
    mv = None if mv is None else float(np.float32(mv) * np.float32(n))
    if cfg.get("subpixel_step") is not None:
        return O.agree_subpixel(raw, L, R, thr, cfg["subpixel_step"], mv)
    d, corr = O.agree(raw, L, R, thr, mv)
    return d.astype(np.float32), corr


def guided_inputs(gpu, case):
    """the unguided match under the global window, and the guide the GPU builds from its map
    (radius 2, spread 1, fallback = the global window), checked against the restatement"""
    L, R = stacks(case["n"], case["dt"])
    d, c = gpu.match(dev(L), dev(R), _cfg(case))
    guide = gpu.guide_from_disparity(d, 2, spread=1, fallback=RANGE)
    want, _ = guide_ref(host(d), d.shape, 2, 1, 1, RANGE)
    same(host(guide), want, "guide")
    return host(d), guide


@pytest.mark.parametrize("name", list(MATCH_CASES))
def test_match_with_a_guide_bit_exact(gpu, name):
    case = MATCH_CASES[name]
    L, R = stacks(case["n"], case["dt"])
    unguided, guide = guided_inputs(gpu, case)
    d, c = gpu.match(dev(L), dev(R), _cfg(case), guide=guide)
    rd, rc = expected_guided_match(case, host(guide))
    same(host(d), rd, "disparity")
    if rc is None:
        assert c is None
    else:
        same(host(c), rc, "corrmap")
    # Where the prior is valid, the pixel's window holds its own match, and the minimum of a
    # subset that holds the set's first minimum is that minimum: such a pixel's raw result
    # cannot change (a unique minimum stays unique). The guided map can differ from the
    # unguided one only at pixels the prior lost -- to a repeated minimum, the left-right
    # check or the NXC threshold -- where the neighbours' narrower window finds another
    # answer; a prior without invalid pixels admits no difference at all.
    # On these stacks the lost pixels are mostly the columns whose match lies outside the
    # image, which no window brings back: the oracle route gives one changed pixel for n8_u8
    # and none for the other cases, so "differs somewhere" cannot be asked of them;
    # test_match_guide_changes_the_map shows a guide that does change the map.
    prior_invalid = ~np.isfinite(unguided.astype(np.float64)) | (unguided == INV)
    got = host(d)
    differs = got.view(np.uint8).reshape(got.shape + (-1,)) != \
        unguided.view(np.uint8).reshape(got.shape + (-1,))
    differs = differs.any(axis=-1)
    print("%s: prior invalid %d, guided differs at %d" % (name, prior_invalid.sum(), differs.sum()))
    assert not (differs & ~prior_invalid).any()
    if name == "n8_u8":
        assert differs.any()


def test_match_guide_changes_the_map(gpu):
    """a guide that shuts out every other column gives a map that differs there (a no-op
    would not), and the rest of the map is the ranged one"""
    L, R = stacks(8, np.uint8)
    case = dict(n=8, dt=np.uint8, cfg=dict(nxcorr_threshold=None))
    ranged, _ = gpu.match(dev(L), dev(R), _cfg(case))
    ranged = host(ranged)
    g = constant_guide(4, 301, -32768, 32767)
    g[:, 0::2] = (1, 0)
    d, _ = gpu.match(dev(L), dev(R), _cfg(case), guide=dev(g))
    d = host(d)
    assert (d[:, 0::2] == INV).all() and (ranged[:, 0::2] != INV).mean() > 0.9
    same(d[:, 1::2].copy(), ranged[:, 1::2].copy(), "odd columns")


def test_match_double_precision_with_a_guide(gpu):
    """Precision::DOUBLE once: byte equality with the float64 oracle (agree_subpixel_f64 on
    the restated guided search)"""
    from libbicos_amd.device import MatchConfig
    from oracle import oracle as O
    from tests.double_cases import same as same_bits
    n, step = 12, 0.25
    L, R = stereo_stack(n, 4, 301, dmin=3, drange=30, seed=n + 17)
    d0, d1 = O.transform(L, 1), O.transform(R, 1)
    cfg = MatchConfig(nxcorr_threshold=0.5, subpixel_step=step, mode=1, precision=1,
                      disparity_range=(2, 40))
    prior, _ = gpu.match(dev(L), dev(R), cfg)
    guide = gpu.guide_from_disparity(prior, 2, spread=1, fallback=(2, 40), sentinel=False)
    same(host(guide), guide_ref(host(prior), prior.shape, 2, 1, 1, (2, 40), False)[0], "guide")
    raw = search_guided(d0, d1, 1, host(guide), 2, 40)
    out, corr = gpu.match(dev(L), dev(R), cfg, guide=guide)
    assert host(corr).dtype == np.float64
    ora_d, ora_c = O.agree_subpixel_f64(raw, L, R, 0.5, step, None)
    same_bits(host(out), ora_d)
    same_bits(host(corr), ora_c)


def test_match_guided_argument_errors(gpu):
    import torch
    case = MATCH_CASES["n8_u8"]
    L, R = stacks(case["n"], case["dt"])
    good = dev(constant_guide(4, 301, 8, 71))
    with pytest.raises(ValueError, match="int16 `out`"):
        gpu.match(dev(L), dev(R), _cfg(case), guide=good,
                  out=torch.empty((4, 301), dtype=torch.int16, device="cuda"))
    with pytest.raises(ValueError, match="shape"):
        gpu.match(dev(L), dev(R), _cfg(case), guide=good[:3])


def test_match_plan_is_unchanged_by_the_guide(gpu):
    """no guide and no range set: the plan (fused agree for n = 33 u8) is what it was, before
    and after a guided match on the same engine"""
    from libbicos_amd import _lib
    from libbicos_amd.device import MatchConfig
    L, R = stereo_stack(33, 32, 512)
    cfg = MatchConfig(nxcorr_threshold=0.9)
    before = gpu.plan(dev(L), dev(R), cfg)
    assert before & _lib.PLAN_MATRIX_CORES and before & _lib.PLAN_AGREE_IN_SEARCH
    gpu.match(dev(L), dev(R), cfg, guide=dev(constant_guide(32, 512, 0, 40)))
    assert gpu.plan(dev(L), dev(R), cfg) == before


def test_several_gpus_and_bands_refuse_a_guide(gpu):
    import pybicos
    from libbicos_amd import device
    L, R = stacks(8, np.uint8)
    g = constant_guide(4, 301, 8, 71)
    with pytest.raises(ValueError, match="several GPUs"):
        pybicos.match(list(L), list(R), pybicos.Config(), devices=[0, 0], guide=g)
    with pytest.raises(ValueError, match="several GPUs"):
        device.match_bands([dev(L)], [dev(R)], device.MatchConfig(), guide=dev(g))


# -------------------------------------------------------------------- host path
@pytest.mark.parametrize("name", ["n8_u8", "n33_u16_subpixel_minvar", "n40_consistency"])
def test_pybicos_match_with_a_guide_equals_the_device_path(gpu, name):
    import pybicos
    case = MATCH_CASES[name]
    kw = case["cfg"]
    L, R = stacks(case["n"], case["dt"])
    _, guide = guided_inputs(gpu, case)
    cfg = pybicos.Config()
    cfg.nxcorr_threshold = kw["nxcorr_threshold"]
    cfg.subpixel_step = kw.get("subpixel_step")
    cfg.min_variance = kw.get("min_variance")
    if kw.get("variant"):
        cfg.set_consistency(kw["max_lr_diff"], kw.get("no_dupes", False))
    cfg.disparity_range = RANGE
    hd, hc = pybicos.match(list(L), list(R), cfg, guide=host(guide))
    d, c = gpu.match(dev(L), dev(R), _cfg(case), guide=guide)
    same(hd, host(d), "disparity")
    same(hc, host(c), "corrmap")
    rd, _ = expected_guided_match(case, host(guide))
    same(hd, rd, "disparity vs oracle route")
