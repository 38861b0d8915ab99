"""Every stage on VIEWS of larger buffers: stack bases that are not 4-byte (or 16-byte) aligned,
row and plane pitches of every residue mod 4, guard bytes that are not zero, outputs at odd
bases inside guarded allocations.

include/bicos_c.h addresses a stack as base[t*plane_pitch + y*row_pitch + x] with free base and
pitches; alignment only selects kernels (engine.cpp match_plan `aligned4`, kernels.hip
launch_agree_m). Every case here

  * is compared bit for bit with the oracle run on the contiguous source -- the view and its
    guards do not exist for the oracle;
  * runs with guard "random", then "ones" (tests/view_cases.py): the two GPU results must be
    byte-identical to each other and to the oracle, so a pad byte taken for a pixel (a neighbour
    from the next row's padding, a plane index off by one, a dword tail, a StackReader range
    that is too tight or too wide) shows wherever it happens;
  * leaves the whole input buffer, view and guards, unchanged;
  * writes into out_views (int16 maps 2 bytes, float maps 4 or 8, double maps 8 bytes past a
    16-byte boundary) whose guards must be intact afterwards;
  * asserts which kernel the alignment selects (bicos_agree_kernel, bicos_match_plan), so no
    case passes through the other kernel unnoticed.

Geometries (view_cases.pitches): every base residue x {aligned pitches, unaligned pitches} plus
every row-pitch residue x {plane = rows * row_pitch, + an odd k} at base 0; H = 5..8 rows, W
about one and a half agree tiles (u8 301 / 333, u16 150 / 301), 3..5 columns for the subpixel.
"""
import functools

import numpy as np
import pytest

from libbicos_amd import _lib
from libbicos_amd.synthetic import random_stack, stereo_stack
from tests import view_cases as V
from tests.double_cases import same as same_bits
from tests.test_gpu_parity import CFGS, same
from tests.test_range_api import search_range

pytestmark = pytest.mark.gpu

GUARD_RUNS = ("random", "ones")


def geometries(dt):
    """(base elements, row pitch bytes mod 4, odd plane pitch) -- see the module docstring"""
    u8 = np.dtype(dt) == np.uint8
    bases = range(5) if u8 else range(4)        # bytes 0 1 2 3 4 / 0 2 4 6
    rowmods = (0, 1, 2, 3) if u8 else (0, 2)
    odd = 3 if u8 else 2
    geos = [(b, 0, False) for b in bases] + [(b, odd, True) for b in bases]
    geos += [(0, m, po) for m in rowmods for po in (False, True)]
    return sorted(set(geos))


def dword_aligned(view):
    """what the kernels' dispatch looks at: base and both pitches, in bytes, multiples of 4"""
    isz = view.element_size()
    return view.data_ptr() % 4 == 0 and (view.stride(1) * isz) % 4 == 0 and \
        (view.stride(0) * isz) % 4 == 0


def views_of(stacks, geo, guard, bases=None):
    """[(buffer, view, snapshot)] of the stacks at one geometry, each in a buffer of its own;
    bases: per-stack base residues where they differ from geo's"""
    base, row_mod, plane_odd = geo
    out = []
    for i, s in enumerate(stacks):
        n, H, W = s.shape
        rp, pp = V.pitches(H, W, row_mod, plane_odd, s.itemsize)
        b = base if bases is None else bases[i]
        buf, view = V.stack_view(s, b, rp, pp, guard, seed=17 + i)
        out.append((buf, view, buf.clone()))
    return out


def host(t):
    return t.cpu().numpy()


def check_inputs(vs):
    for buf, _, snap in vs:
        assert V.unchanged(buf, snap), "an input buffer (view or guards) was written"


def both_guards(stacks, geo, run, bases=None):
    """run(views) -> tuple of numpy results, for guard "random" then "ones": inputs unchanged,
    the two runs byte-identical; returns the results"""
    res = []
    for guard in GUARD_RUNS:
        vs = views_of(stacks, geo, guard, bases)
        res.append(run([v for _, v, _ in vs]))
        check_inputs(vs)
    for a, b in zip(*res):
        if a is None:
            assert b is None
            continue
        assert a.dtype == b.dtype and a.shape == b.shape
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), \
            "guard bytes changed the result (geometry %r)" % (geo,)
    return res[0]


# ----------------------------------------------------------------- transform
def _transform_case(gpu, oracle, s, mode, words, geo):
    n, H, W = s.shape
    pitch = gpu._L.bicos_desc_pitch(W, words)
    import torch

    def run(views):
        # (16-byte aligned: the transform stores whole vectors, include/bicos_c.h)
        out, intact = V.out_view((H, pitch), torch.int32, 0)
        got = gpu.transform(views[0], mode, words, out=out)
        assert got.data_ptr() == out.data_ptr() and out.data_ptr() % 16 == 0
        r = host(out).view(np.uint32)
        assert intact(), "transform wrote outside its descriptors"
        return (r[:, :W * words].reshape(H, W, words).copy(),)
    return both_guards([s], geo, run)[0]


def _extremes(s):
    top = np.iinfo(s.dtype).max
    s[:, 0, :5] = 0
    s[:, 1, :5] = top
    s[:, -1, -3:] = top       # the stack's last pixels: the end of a StackReader range
    s[-1, -1, -1] = top - 1
    return s


# one n in each kernel bucket (kernels.hip launch_transform_w: MAXN 9 | 12, 17 | 24, 33 | 40,
# 48, 65), exact (n == MAXN) and padded
@pytest.mark.parametrize("dt,widths", [(np.uint8, (301, 333)), (np.uint16, (150, 301))])
@pytest.mark.parametrize("n", [2, 4, 9, 12, 17, 24, 33, 40, 41, 65])
def test_transform_limited_views(gpu, oracle, n, dt, widths):
    H = 5
    words = oracle.desc_words(n, 0)
    for W in widths:
        s = _extremes(random_stack(n, H, W, dt, seed=300 + n + W))
        ref = oracle.transform(s, 0, words)
        for geo in geometries(dt):
            same(_transform_case(gpu, oracle, s, 0, words, geo), ref)


# FULL: the static kernels (n = 2, 7, 12, 16) and the generic one through a wider descriptor
@pytest.mark.parametrize("dt,widths", [(np.uint8, (301, 333)), (np.uint16, (150, 301))])
@pytest.mark.parametrize("n", [2, 7, 12, 16])
def test_transform_full_views(gpu, oracle, n, dt, widths):
    H = 5
    words = oracle.desc_words(n, 1)
    for W in widths:
        s = _extremes(random_stack(n, H, W, dt, seed=400 + n + W))
        for w in (words,) if words == 8 else (words, 2 * words):
            ref = oracle.transform(s, 1, w)
            for geo in geometries(dt):
                same(_transform_case(gpu, oracle, s, 1, w, geo), ref)


# --------------------------------------------------------------------- agree
def _agree_raw(H, W, seed):
    """tests/test_gpu_parity.py test_agree_disparity_patterns cut down to W columns: flat runs,
    jitter, jumps, anything incl. matches off either end of the row, invalid pixels, negative
    disparities, the one column whose match is column 0"""
    assert H == 8
    rng = np.random.default_rng(seed)
    raw = np.empty((H, W), np.int16)
    raw[0] = 3                                              # the planted disparity: pixels pass
    raw[1] = 8 + rng.integers(-1, 2, size=W)                # (planted 8) jitter
    raw[2] = 30 + rng.integers(-2, 3, size=W)
    raw[3] = np.where(np.arange(W) % 64 < 32, 5, W - 50)
    raw[4] = rng.integers(-40, W + 70, size=W)              # off-row matches on both sides
    raw[5] = 28                                             # planted, with invalid pixels
    raw[5, ::7] = -32768
    raw[6] = np.arange(W) % 9 - 4                           # col1 > col0
    raw[7] = W - 1                                          # only the last column in the row
    return raw


@functools.lru_cache(maxsize=None)
def _agree_inputs(n, dt, W):
    H = 8
    L, R = stereo_stack(n, H, W, dt, dmin=3, drange=40, seed=n + 1000 + W)
    R[:, 0, 40:48] = 9                                      # constant right samples: NaN
    top = np.iinfo(dt).max
    L[:, -1, -2:] = top                                     # the stack's very last pixels
    L[-1, -1, -1] = 1
    R[:, -1, -1] = np.arange(n) % 7
    return L, R, _agree_raw(H, W, n)


@functools.lru_cache(maxsize=None)
def _agree_refs(n, dt, W):
    from oracle import oracle as O
    L, R, raw = _agree_inputs(n, dt, W)
    refs = {}
    for minvar in (None, 2.0):
        mv = None if minvar is None else float(np.float32(minvar) * np.float32(n))
        d, c = O.agree(raw, L, R, 0.5, mv)
        refs[minvar, 0] = (d.astype(np.float32), c)
        d, c = O.agree_f64(raw, L, R, 0.5, mv)
        refs[minvar, 1] = (d.astype(np.float32), c)
    return refs


def _agree_geos(dt):
    """(geo, bases): the stage geometries with both stacks at the same base, then stacks cut
    from different buffers at different bases -- stack0 aligned with stack1 at residue 1
    element (the LDS kernel must run), stack0 at residue 1 with stack1 aligned (the register
    kernel), on aligned and on unaligned pitches"""
    odd = 3 if np.dtype(dt) == np.uint8 else 2
    both = [(g, None) for g in geometries(dt)]
    apart = [((0, 0, False), (0, 1)), ((0, 0, False), (1, 0)), ((0, 0, False), (4 // np.dtype(dt).itemsize, 3)),
             ((0, odd, True), (0, 1)), ((0, odd, True), (1, 0))]
    return both + apart


# one n per launch_agree_t bucket (8 16 24 33 40 48 65) and one beyond for the generic kernel
@pytest.mark.parametrize("dt,widths", [(np.uint8, (301, 333)), (np.uint16, (150, 301))])
@pytest.mark.parametrize("n", [8, 16, 24, 33, 40, 48, 65, 70])
def test_agree_views(gpu, oracle, n, dt, widths):
    import torch
    isz = np.dtype(dt).itemsize
    settings = [(minvar, prec) for minvar in (None, 2.0) for prec in (0, 1)]
    for W in widths:
        L, R, raw = _agree_inputs(n, dt, W)
        refs = _agree_refs(n, dt, W)
        H = raw.shape[0]
        raw_t = torch.from_numpy(raw).cuda()
        for geo, bases in _agree_geos(dt):
            def run(views):
                v0, v1 = views
                assert v0.stride() == v1.stride()
                assert v0.untyped_storage().data_ptr() != v1.untyped_storage().data_ptr()
                # the kernel the launcher picks: stack0's base and the pitches alone decide
                want = 0 if n > 65 else (2 if dword_aligned(v0) else 1)
                if bases is not None and n <= 65 and geo == (0, 0, False):
                    assert v1.data_ptr() % 16 == bases[1] * isz and v0.data_ptr() % 16 == bases[0] * isz
                    assert want == (1 if (bases[0] * isz) % 4 else 2)
                assert gpu.agree_kernel(v0, v1) == want, (geo, bases)
                res = []
                for minvar, prec in settings:
                    mv = None if minvar is None else float(np.float32(minvar) * np.float32(n))
                    out, out_ok = V.out_view((H, W), torch.float32, 1 + prec)      # 4 / 8 bytes
                    corr, corr_ok = V.out_view((H, W), torch.float64 if prec else torch.float32, 1)
                    gpu.agree(raw_t, v0, v1, 0.5, mv, precision=prec, out=out, corrmap=corr)
                    res += [host(out), host(corr)]
                    assert out_ok() and corr_ok(), "agree wrote outside its maps"
                return tuple(res)
            got = both_guards([L, R], geo, run, bases)
            for i, key in enumerate(settings):
                rd, rc = refs[key]
                same(got[2 * i], rd)
                (same_bits if key[1] else same)(got[2 * i + 1], rc)
        assert np.array_equal(host(raw_t), raw)


# ------------------------------------------------------------------ subpixel
def _subpixel_raw(H, W, seed):
    """col1 on 0, 1, W-2 and W-1 (the edge columns take the plain NXC, their neighbours read
    the row's first / last pixel as a neighbour), interior matches, invalid pixels, matches off
    the row; below 6 columns every (col0, col1) pair"""
    raw = np.empty((H, W), np.int16)
    if W < 6:
        for y in range(H):
            for x in range(W):
                raw[y, x] = x - ((x + y) % W)
        return raw
    rng = np.random.default_rng(seed)
    raw[:] = rng.integers(-3, 12, size=(H, W))
    raw[rng.random((H, W)) < 0.1] = -32768
    raw[:, 3] = 3                  # col1 = 0
    raw[:, 4] = 3                  # col1 = 1
    raw[:, 0] = -(W - 1)           # col1 = W - 1 from column 0
    raw[:, 1] = -(W - 3)           # col1 = W - 2
    raw[:, W - 1] = 0              # col1 = W - 1
    raw[:, W - 2] = 0              # col1 = W - 2
    raw[:, W - 3] = -2             # col1 = W - 1
    raw[:, W - 4] = W - 5          # col1 = 1
    raw[0, 7] = 9                  # col1 = -2: off the row
    raw[0, W - 5] = -9             # col1 = W + 4: off the row
    return raw


SUBPIXEL_SETTINGS = [(0.25, None, 0), (0.1, 1.0, 0), (0.25, 1.0, 1), (0.1, None, 1)]


# one n per instantiation of subpixel.hip / subpixel_wide.hip: exact 6 10 12, buckets <= 8, 16,
# 24, 33 (25: padded; 33: exact, its own LDS-staged form), 40, 48, 56, 65
@pytest.mark.parametrize("dt,wide", [(np.uint8, 301), (np.uint16, 150)])
@pytest.mark.parametrize("n", [6, 8, 10, 12, 16, 24, 25, 33, 40, 41, 56, 65])
def test_subpixel_views(gpu, oracle, n, dt, wide):
    import torch
    H = 6
    for W in (wide, 5, 4, 3):
        L = random_stack(n, H, W, dt, seed=n + W + 1)
        R = random_stack(n, H, W, dt, seed=n + W + 2)
        top = np.iinfo(dt).max
        R[:, -1, -1] = top - np.arange(n) % 5               # the stack's last pixel, as a neighbour
        R[:, 0, 0] = np.arange(n) % 3
        raw = _subpixel_raw(H, W, n)
        raw_t = torch.from_numpy(raw).cuda()
        refs = []
        for step, minvar, prec in SUBPIXEL_SETTINGS:
            mv = None if minvar is None else float(np.float32(minvar) * np.float32(n))
            refs.append((oracle.agree_subpixel_f64 if prec else oracle.agree_subpixel)(
                raw, L, R, 0.2, step, mv))
        for geo in geometries(dt):
            def run(views):
                v0, v1 = views
                res = []
                for step, minvar, prec in SUBPIXEL_SETTINGS:
                    mv = None if minvar is None else float(np.float32(minvar) * np.float32(n))
                    out, out_ok = V.out_view((H, W), torch.float32, 2 - prec)      # 8 / 4 bytes
                    corr, corr_ok = V.out_view((H, W), torch.float64 if prec else torch.float32, 1)
                    gpu.agree(raw_t, v0, v1, 0.2, mv, step=step, precision=prec, out=out, corrmap=corr)
                    res += [host(out), host(corr)]
                    assert out_ok() and corr_ok(), "subpixel wrote outside its maps"
                return tuple(res)
            got = both_guards([L, R], geo, run)
            for i, (step, minvar, prec) in enumerate(SUBPIXEL_SETTINGS):
                (same_bits if prec else same)(got[2 * i], refs[i][0])
                (same_bits if prec else same)(got[2 * i + 1], refs[i][1])


# --------------------------------------------------------------- whole match
FUSIONS = _lib.PLAN_AGREE_IN_SEARCH | _lib.PLAN_CONSISTENCY_IN_AGREE
RANGE = (-5, 40)
MATCH_CASES = [dict(cfg=c) for c in CFGS] + [
    dict(cfg=dict(nxcorr_threshold=0.9, precision=1)),
    dict(cfg=dict(nxcorr_threshold=0.8, min_variance=1.0, subpixel_step=0.25, precision=1)),
    dict(cfg=dict(nxcorr_threshold=0.5, variant=1, max_lr_diff=2, no_dupes=True, precision=1)),
    dict(cfg=dict(nxcorr_threshold=0.9), ranged=True),
    dict(cfg=dict(nxcorr_threshold=0.9, min_variance=1.0), i16=True),       # bicos_match_device_i16
    dict(cfg=dict(nxcorr_threshold=0.9), from_desc=True),                   # bicos_search_agree_device
    dict(cfg=dict(nxcorr_threshold=0.6, variant=1, max_lr_diff=1), from_desc=True),
]


def _match_ref(O, L, R, mode, case):
    cfg = case["cfg"]
    if case.get("ranged"):
        d0, d1 = O.transform(L, mode), O.transform(R, mode)
        raw = search_range(d0, d1, 1, RANGE[0], RANGE[1])
        d, c = O.agree(raw, L, R, cfg["nxcorr_threshold"], None)
        return d.astype(np.float32), c
    ocfg = {k: v for k, v in cfg.items() if k != "precision"}
    d, c = (O.match_f64 if cfg.get("precision") else O.match)(L, R, O.OracleConfig(mode=mode, **ocfg))
    if case.get("i16"):
        assert (d == d.astype(np.int16)).all()
        d = d.astype(np.int16)
    return d, c


def _match_run(gpu, n, mode, case, v0, v1, H, W):
    """one match on two views into out_views; (disparity, corrmap) as numpy"""
    import torch
    from libbicos_amd.device import MatchConfig, descriptor_words
    cfg = case["cfg"]
    mc = MatchConfig(mode=mode, disparity_range=RANGE if case.get("ranged") else None, **cfg)
    nxc = cfg.get("nxcorr_threshold") is not None
    i16 = case.get("i16") or not nxc
    out, out_ok = V.out_view((H, W), torch.int16 if i16 else torch.float32, 1)   # 2 / 4 bytes
    corr = corr_ok = None
    if nxc:
        prec = cfg.get("precision", 0)
        corr, corr_ok = V.out_view((H, W), torch.float64 if prec else torch.float32, 1 if prec else 2)
    if case.get("from_desc"):
        words = descriptor_words(n, mode)
        d0, d1 = gpu.transform(v0, mode, words), gpu.transform(v1, mode, words)
        gpu.search_agree(d0, d1, v0, v1, mc, out=out, corrmap=corr)
    else:
        gpu.match(v0, v1, mc, out=out, corrmap=corr)
    res = (host(out), host(corr) if corr is not None else None)
    assert out_ok() and (corr_ok is None or corr_ok()), "match wrote outside its maps"
    return res


def _check_plan(gpu, n, dt, mode, case, v0, v1, flat_plan):
    """the plan the view's pointers must produce: the contiguous stacks' plan where both bases
    and the pitches are dword aligned, that plan without either fusion elsewhere"""
    from libbicos_amd.device import MatchConfig
    cfg = case["cfg"]
    plan = gpu.plan(v0, v1, MatchConfig(mode=mode, **cfg))
    if dword_aligned(v0) and dword_aligned(v1):
        assert plan == flat_plan, (plan, flat_plan)
    else:
        assert plan & FUSIONS == 0 and plan == flat_plan & ~FUSIONS, (plan, flat_plan)


@pytest.mark.parametrize("n,dt,mode,W", [
    (8, np.uint8, 0, 301),      # 32-bit descriptors: the packed search, its fused agree
    (33, np.uint8, 0, 333),     # 128-bit: the one-product search with its fused agree
    (17, np.uint16, 0, 150),    # u16, 64-bit
    (10, np.uint8, 1, 301),     # FULL, 128-bit
    (40, np.uint8, 0, 301),     # 256-bit: Consistency in one launch
    (16, np.uint16, 1, 150),    # FULL u16, 256-bit with 4 K-steps
])
def test_match_views(gpu, oracle, monkeypatch, n, dt, mode, W):
    from libbicos_amd.device import MatchConfig
    monkeypatch.delenv("BICOS_LR_ONE_PASS", raising=False)
    H = 6
    L, R = stereo_stack(n, H, W, dt, dmin=3, drange=30, seed=n + W)
    L[:, 1, 40:70] = 5                                      # flat patch: ties, NaN correlations
    top = np.iinfo(dt).max
    L[:, -1, -1] = top - np.arange(n) % 4                   # the stacks' last pixels
    R[:, -1, -1] = np.arange(n) % 6
    isz = np.dtype(dt).itemsize
    # the plan of a padded view with aligned bases and pitches: what every aligned view must plan
    (_, c0, _), (_, c1, _) = views_of([L, R], (0, 0, False), "zeros")
    assert dword_aligned(c0) and dword_aligned(c1) and c0.stride(1) > W
    apart = [((0, 0, False), (0, 1)), ((0, 0, False), (1, 0))]
    for case in MATCH_CASES:
        cfg = case["cfg"]
        ref_d, ref_c = _match_ref(oracle, L, R, mode, case)
        flat_plan = gpu.plan(c0, c1, MatchConfig(mode=mode, **cfg))
        # what the aligned plan must hold, so that the views below cannot all run unfused
        plain_nxc = cfg.get("nxcorr_threshold") is not None and cfg.get("subpixel_step") is None
        if plain_nxc and not cfg.get("variant") and not cfg.get("precision") and isz == 1 and n in (8, 33):
            assert flat_plan & _lib.PLAN_AGREE_IN_SEARCH
        two_pass = cfg.get("variant") and not flat_plan & _lib.PLAN_CONSISTENCY_ONE_PASS
        if plain_nxc and two_pass:
            assert flat_plan & _lib.PLAN_CONSISTENCY_IN_AGREE
        for geo, bases in [(g, None) for g in geometries(dt)] + apart:
            def run(views):
                v0, v1 = views
                if not case.get("ranged"):
                    _check_plan(gpu, n, dt, mode, case, v0, v1, flat_plan)
                return _match_run(gpu, n, mode, case, v0, v1, H, W)
            got_d, got_c = both_guards([L, R], geo, run, bases)
            same(got_d, ref_d)
            if ref_c is None:
                assert got_c is None
            else:
                (same_bits if cfg.get("precision") else same)(got_c, ref_c)


def test_fused_search_agree_on_an_aligned_view(gpu, oracle):
    """The tall geometry of test_fused_search_agree_equals_stages (300 x 1800, n = 33: 4 tiles
    per wave, the row's last workgroup partly filled) on one view whose base is dword but not
    16-byte aligned (residue 4) with a row pitch of 1856 and random guards: the fused search +
    agree launch is planned and exact against the oracle."""
    import torch
    from libbicos_amd.device import MatchConfig
    n, H, W, rp = 33, 300, 1800, 1856
    L, R = stereo_stack(n, H, W, np.uint8, dmin=3, drange=40, seed=W + H)
    L[:, 5, 200:260] = 9
    cfg = dict(nxcorr_threshold=0.5, min_variance=2.0)
    vs = [V.stack_view(s, 4, rp, H * rp, "random", seed=5 + i) for i, s in enumerate((L, R))]
    snaps = [b.clone() for b, _ in vs]
    v0, v1 = vs[0][1], vs[1][1]
    assert v0.data_ptr() % 16 == 4 and v0.stride() == (H * rp, rp, 1)
    assert gpu.plan(v0, v1, MatchConfig(**cfg)) & _lib.PLAN_AGREE_IN_SEARCH
    out, out_ok = V.out_view((H, W), torch.float32, 1)
    corr, corr_ok = V.out_view((H, W), torch.float32, 2)
    gpu.match(v0, v1, MatchConfig(**cfg), out=out, corrmap=corr)
    rd, rc = oracle.match(L, R, oracle.OracleConfig(**cfg))
    same(host(out), rd)
    same(host(corr), rc)
    assert out_ok() and corr_ok()
    for (b, _), s in zip(vs, snaps):
        assert V.unchanged(b, s)
