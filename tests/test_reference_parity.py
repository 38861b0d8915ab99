"""The C oracle and the HIP engine against the reference's own CPU code.

oracle/_ref/libbicos_ref.so is the reference's src/impl/cpu.cpp and include/impl/cpu/*.hpp
compiled unchanged (oracle/Makefile target `ref`, oracle/ref_driver.cpp, oracle/reference.py);
only storage and threading are a stand-in (oracle/ref_shim, checked here too). Every
comparison is byte for byte, dtype and shape included.

CPU tests: the oracle (oracle/bicos_oracle.c) against the reference, whole match and stage by
stage; the reference reproduces the committed oracle-made fixtures (golden.npz, frames.json)
and its own (ref_frames.json). They skip only where neither the reference tree nor a built
reference library exists.

GPU tests: Engine.match against tests/golden/ref_frames.json, results recorded from the
reference alone (tests/golden/make_ref_frames.py). They read nothing else of the reference.
"""
import json
import os

import numpy as np
import pytest

from libbicos_amd.synthetic import _uniform, random_descriptors, random_stack, stereo_stack
from tests.golden import make_ref_frames as MRF
from tests.golden.make_ref_frames import CONFIGS

HERE = os.path.dirname(os.path.abspath(__file__))
INVALID = -32768
SUBPIX = [c for c, v in CONFIGS.items() if v.get("subpixel_step") is not None]

LIMITED_N = [2, 3, 4, 5, 9, 10, 17, 18, 33, 34, 40, 65]
FULL_N = [2, 3, 4, 6, 7, 8, 9, 12, 13, 16]
KINDS = ["random", "lowtex", "periodic", "constant"]
MATCH_H = 3
MATCH_WIDTHS = [1, 2, 41]


@pytest.fixture(scope="module")
def ref():
    """oracle/reference.py with both reference libraries built (or found built)."""
    from oracle import reference as R
    if not R.available():
        pytest.skip("neither the reference tree nor oracle/_ref/libbicos_ref*.so exists")
    R.lib()
    R.lib("O0")
    return R


def identical(a, b):
    if a is None or b is None:
        return a is None and b is None
    return a.dtype == b.dtype and a.shape == b.shape and \
        np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def valid_mask(d):
    """Invalid is -32768 in int16 maps and in their float conversion (NXC without a subpixel
    step: convertTo of the int16 map), NaN in subpixel maps."""
    return np.isfinite(d) & (d != INVALID)


def maxval(dt):
    return 255 if np.dtype(dt) == np.uint8 else 65535


# ------------------------------------------------------------------- inputs
def half_pixel(rows):
    """Mean of each column and its right neighbour (the last column stays): the view moves
    half a column, so a subpixel search finds its best correlation off the integer."""
    wide = rows.astype(np.int64)
    wide[..., :-1] = (wide[..., :-1] + wide[..., 1:] + 1) // 2
    return wide.astype(rows.dtype)


def match_inputs(kind, n, dt, W, H=MATCH_H):
    """Small stacks of the four kinds, full range of the type."""
    mv = maxval(dt)
    if kind == "random":            # right = left moved 2..4 columns + U{-1,0,1}, clamped;
        L, R = stereo_stack(n, H, W, dt, dmin=2, drange=3 * H, maxval=mv)
        R[:, -1] = half_pixel(R[:, -1])                             # last row: 4.5 columns
        return L, R
    if kind == "lowtex":            # 4 grey levels in 2-column runs, moved 3 columns; +U{0..3}
        lv = _uniform(np.arange(n * H * (W + 8), dtype=np.int64), 77, 3).reshape(n, H, W + 8)
        # last row: the same level in every image. A pixel then varies by its noise alone, a
        # variance of about 1.25 n: above min_variance 2.0, below the scaled 2.0 n
        lv[:, -1] = lv[0, -1]
        scene = np.repeat(lv, 2, axis=2) * (mv // 4)
        nz = _uniform(np.arange(2 * n * H * W, dtype=np.int64), 78, 3).reshape(2, n, H, W)
        return ((scene[:, :, :W] + nz[0]).astype(dt), (scene[:, :, 3:W + 3] + nz[1]).astype(dt))
    if kind == "periodic":          # one random 8-column cell repeated; right moved 3 columns
        cell = random_stack(n, H, 8, dt, seed=5, maxval=mv)
        wide = np.tile(cell, (1, 1, W // 8 + 2))
        return np.ascontiguousarray(wide[:, :, :W]), np.ascontiguousarray(wide[:, :, 3:W + 3])
    if kind == "constant":          # zero variance everywhere: NaN correlation
        return np.full((n, H, W), mv // 3, dt), np.full((n, H, W), mv // 3, dt)
    raise KeyError(kind)


# ------------------------------------------------------------ shim self-check
@pytest.mark.parametrize("variant", ["", "O0"])
def test_shim_selfcheck(ref, variant):
    """merge channel order (u8, u16), strided views, row/at/ptr aliasing, convertTo of
    -32768, setTo(NaN), parallel_for_ coverage: 0, or the number of the failed check."""
    assert ref.shim_selfcheck(variant) == 0


# ------------------------------------------------- whole match, oracle vs reference
_SEEN = {}      # (config, kind) -> [valid pixels, invalid pixels, fractional valid disparities]


def _match_case(oracle, ref, mode, n, dt):
    for kind in KINDS:
        for W in MATCH_WIDTHS:
            L, R = match_inputs(kind, n, dt, W)
            for cname, cfg in CONFIGS.items():
                rd, rc = ref.match(L, R, ref.ReferenceConfig(mode=mode, **cfg), nthreads=1)
                od, oc = oracle.match(L, R, oracle.OracleConfig(mode=mode, **cfg), nthreads=1)
                assert identical(od, rd), ("disparity", mode, n, dt, kind, W, cname)
                assert identical(oc, rc), ("corrmap", mode, n, dt, kind, W, cname)
                assert (rc is None) == (cfg["nxcorr_threshold"] is None)
                v = valid_mask(rd)
                seen = _SEEN.setdefault((cname, kind), [0, 0, 0])
                seen[0] += int(v.sum())
                seen[1] += int((~v).sum())
                if rd.dtype.kind == "f":
                    seen[2] += int((rd[v] != np.round(rd[v])).sum())


@pytest.mark.parametrize("dt", [np.uint8, np.uint16], ids=["u8", "u16"])
@pytest.mark.parametrize("n", LIMITED_N)
def test_match_limited_oracle_equals_reference(oracle, ref, n, dt):
    _match_case(oracle, ref, 0, n, dt)


@pytest.mark.parametrize("dt", [np.uint8, np.uint16], ids=["u8", "u16"])
@pytest.mark.parametrize("n", FULL_N)
def test_match_full_oracle_equals_reference(oracle, ref, n, dt):
    _match_case(oracle, ref, 1, n, dt)


def test_match_comparison_is_not_trivial(oracle, ref):
    """Conditions on the reference's own results over the matrix above (run here again at
    two stack sizes, so the test stands alone): per config, valid and invalid pixels over
    the random and low-texture inputs; fractional disparities for the subpixel configs;
    NaN correlations that pass the threshold for constant input."""
    _SEEN.clear()
    for n, dt in ((9, np.uint8), (17, np.uint16)):
        _match_case(oracle, ref, 0, n, dt)
    for cname in CONFIGS:
        valid = sum(_SEEN[(cname, k)][0] for k in ("random", "lowtex"))
        invalid = sum(_SEEN[(cname, k)][1] for k in ("random", "lowtex"))
        assert valid > 0 and invalid > 0, (cname, valid, invalid)
    for cname in SUBPIX:
        assert sum(_SEEN[(cname, k)][2] for k in ("random", "lowtex")) > 0, cname
    # min-variance decides pixels, and its scaling by n does: on the low-texture input the
    # reference marks pixels -1 that an n times smaller threshold lets through
    for cname in ("nxc_minvar", "subpix_minvar"):
        L, R = match_inputs("lowtex", 9, np.uint8, 41)
        c = ref.match(L, R, ref.ReferenceConfig(**CONFIGS[cname]))[1]
        small = dict(CONFIGS[cname], min_variance=CONFIGS[cname]["min_variance"] / 9)
        c9 = ref.match(L, R, ref.ReferenceConfig(**small))[1]
        assert ((c == -1) & (c9 != -1)).any() and (c[np.isfinite(c)] != -1).any(), cname
    L, R = match_inputs("constant", 9, np.uint8, 41)
    d, c = ref.match(L, R, ref.ReferenceConfig(nxcorr_threshold=0.9, variant=1, max_lr_diff=1))
    # every cost ties: the first minimum is column 0 both ways, so columns 0 and 1 pass
    # max_lr_diff 1 with disparity 0; their NaN correlation passes (NaN < 0.9 is false)
    assert np.isnan(c).all() and (d[:, :2] == 0).all() and (d[:, 2:] == INVALID).all()


@pytest.mark.parametrize("dt", [np.uint8, np.uint16], ids=["u8", "u16"])
def test_subpixel_samples_leave_the_input_range(ref, dt):
    """The subpixel configs evaluate interpolated samples outside [0, max] of the input type,
    so the narrowing cast of agree_subpixel is exercised: counted in float64 on the pixels the
    reference refines (raw disparity valid, right column interior), 0.5 beyond the range."""
    n, W = 9, 41
    L, R = match_inputs("random", n, dt, W)
    outside = 0
    for cname in SUBPIX:
        cfg = CONFIGS[cname]
        raw, _ = ref.match(L, R, ref.ReferenceConfig(**dict(
            cfg, nxcorr_threshold=None, subpixel_step=None, min_variance=None)))
        step = np.float32(cfg["subpixel_step"])
        xs, x = [], np.float32(-1)
        while x <= 1:
            xs.append(float(x))
            x = np.float32(x + step)
        for y, col in zip(*np.nonzero(raw != INVALID)):
            col1 = col - int(raw[y, col])
            if not 0 < col1 < W - 1:
                continue
            y0, y1, y2 = (R[:, y, col1 + k].astype(np.float64) for k in (-1, 0, 1))
            a, b = 0.5 * (y0 - 2 * y1 + y2), 0.5 * (y2 - y0)
            v = np.array([a * x * x + b * x + y1 for x in xs])
            outside += int(((v < -0.5) | (v > maxval(dt) + 0.5)).sum())
    assert outside > 0


# ------------------------------------------------------ stages, oracle vs reference
def transform_stack(n, dt, W=24):
    """Rows: full-range random; every image equal (the average is the value itself, so no
    comparison holds); 0 / max alternating over the images, phase by column;
    values near the top of the range (u16 pair sums above 65535); values 0..3 (the average
    falls between neighbouring integers)."""
    mv = maxval(dt)
    s = np.empty((n, 5, W), dt)
    s[:, 0] = random_stack(n, 1, W, dt, seed=31, maxval=mv)[:, 0]
    s[:, 1] = random_stack(1, 1, W, dt, seed=32, maxval=mv)[0, 0][None, :]
    s[:, 1, :3] = (0, mv, mv // 2)
    t = np.arange(n)[:, None] + np.arange(W)[None, :]
    s[:, 2] = np.where(t % 2 == 0, 0, mv)
    s[:, 3] = mv - random_stack(n, 1, W, dt, seed=33, maxval=mv // 3)[:, 0]
    s[:, 4] = random_stack(n, 1, W, dt, seed=34, maxval=3)[:, 0]
    return s


@pytest.mark.parametrize("dt", [np.uint8, np.uint16], ids=["u8", "u16"])
@pytest.mark.parametrize("mode,ns", [(0, range(2, 66)), (1, range(2, 17))], ids=["limited", "full"])
def test_transform_oracle_equals_reference(oracle, ref, mode, ns, dt):
    for n in ns:
        s = transform_stack(n, dt)
        if dt == np.uint16:
            assert (s[:-1, 3].astype(np.int64) + s[1:, 3] > 65535).any()
        want = ref.transform(s, mode, nthreads=1)
        assert want.shape[2] == oracle.desc_words(n, mode) == ref.desc_words(n, mode)
        assert identical(oracle.transform(s, mode, nthreads=1), want), (mode, n)
        # all-equal pixels: no comparison holds, but LIMITED's last bit at n < 4, where the
        # pair sum is compared with the initial -1
        only = np.zeros(want.shape[2], np.uint32)
        if mode == 0 and n < 4:
            only[0] = 1 << (3 if n == 2 else 6)
        assert want.any() and (want[1] == only).all(), (mode, n)
        # the same bits in the widest descriptor, zeros above them
        wide = ref.transform(s, mode, 8, nthreads=1)
        assert identical(oracle.transform(s, mode, 8, nthreads=1), wide), (mode, n, "wide")
        assert identical(wide[:, :, :want.shape[2]], want) and not wide[:, :, want.shape[2]:].any()


def search_descriptors(kind, H, W, words):
    d0 = random_descriptors(H, W, words, 101)
    d1 = random_descriptors(H, W, words, 202)
    if kind == "ties":              # 5 used bits: every minimum is shared
        d0[:, :, 1:] = 0
        d1[:, :, 1:] = 0
        d0[:, :, 0] &= 0x1F
        d1[:, :, 0] &= 0x1F
    elif kind == "topbit":          # few low bits + the last bit of the descriptor
        top = np.uint32(1 << 31)
        for d, seed in ((d0, 303), (d1, 404)):
            flip = random_descriptors(H, W, 1, seed)[:, :, 0]
            d[:, :, :-1] = 0
            d[:, :, 0] = flip & np.uint32(0x7)
            d[:, :, -1] = np.where((flip >> np.uint32(8)) & np.uint32(1), top, np.uint32(0))
    return d0, d1


@pytest.mark.parametrize("W", [1, 2, 41, 333])
@pytest.mark.parametrize("kind", ["random", "ties", "topbit"])
@pytest.mark.parametrize("words", [1, 2, 4, 8])
def test_search_oracle_equals_reference(oracle, ref, words, kind, W):
    H = 3
    d0, d1 = search_descriptors(kind, H, W, words)
    if kind == "topbit":
        assert (d0[:, :, -1] >> np.uint32(31)).any() or W < 3
    seen = set()
    for flags, lrs in ((1, (-1,)), (2, (0, 1, 5)), (3, (0, 1, 5))):
        for lr in lrs:
            want = ref.search(d0, d1, flags, lr, nthreads=1)
            assert identical(oracle.search(d0, d1, flags, lr, nthreads=1), want), (flags, lr)
            seen.update(np.unique(want != INVALID).tolist())
    if W >= 41:
        assert seen == {True, False}


AGREE_N = [2, 8, 33, 45, 65]
AGREE_W = 29


def agree_inputs(n, dt):
    """Stacks [n, 4, W] and an arbitrary raw map. Rows: right = left moved 2 columns +
    U{-1,0,1} (2.5 columns in the right half); independent random; values 0..3 (min-variance decides); constant (NaN)."""
    mv, W = maxval(dt), AGREE_W
    L, R = stereo_stack(n, 4, W, dt, dmin=2, drange=0, maxval=mv)
    R[:, 0, W // 2:] = half_pixel(R[:, 0, W // 2:])     # right half of row 0: 2.5 columns
    R[:, 1] = random_stack(n, 1, W, dt, seed=41, maxval=mv)[:, 0]
    L[:, 2] = random_stack(n, 1, W, dt, seed=42, maxval=3)[:, 0]
    R[:, 2] = random_stack(n, 1, W, dt, seed=43, maxval=3)[:, 0]
    L[:, 3] = R[:, 3] = mv // 2
    pick = _uniform(np.arange(4 * W, dtype=np.int64), 44, 9).reshape(4, W)
    anyd = _uniform(np.arange(4 * W, dtype=np.int64), 45, 2 * W + 6).reshape(4, W) - (W + 3)
    col = np.arange(W)[None, :].repeat(4, 0)
    raw = np.select(
        [pick == 0, pick == 1, pick == 2, pick <= 4, pick <= 7],
        [INVALID,           # invalid on entry
         col,               # col1 = 0
         col - (W - 1),     # col1 = W - 1 (negative disparities)
         anyd,              # anything in [-W-3, W+3]: also outside the row
         2],                # the planted disparity
        -1).astype(np.int16)
    return L, R, raw


@pytest.mark.parametrize("dt", [np.uint8, np.uint16], ids=["u8", "u16"])
@pytest.mark.parametrize("n", AGREE_N)
def test_agree_oracle_equals_reference(oracle, ref, n, dt):
    L, R, raw = agree_inputs(n, dt)
    assert (raw == INVALID).any() and (raw < 0).any()
    col1 = np.arange(AGREE_W)[None, :] - raw.astype(np.int64)
    assert (col1 < 0).any() and (col1 >= AGREE_W).any()
    assert ((col1 == 0) & (raw != INVALID)).any() and (col1 == AGREE_W - 1).any()
    for thr in (0.5, -0.2):
        for mv in (None, 2.0 * n, 0.5 * n):
            wd, wc = ref.agree(raw, L, R, thr, mv, nthreads=1)
            od, oc = oracle.agree(raw, L, R, thr, mv, nthreads=1)
            assert identical(od, wd) and identical(oc, wc), (thr, mv)
            assert (wd != INVALID).any() and ((wd == INVALID) & (raw != INVALID)).any()
            assert np.isnan(wc[3][wd[3] != INVALID]).all()      # constant row: NaN passes
            if mv is not None:
                assert (wc == -1).any()


@pytest.mark.parametrize("dt", [np.uint8, np.uint16], ids=["u8", "u16"])
@pytest.mark.parametrize("n", AGREE_N)
def test_agree_subpixel_oracle_equals_reference(oracle, ref, n, dt):
    """Also optimisation independence: the -O0 build of the reference gives the same bytes,
    although (TInput)roundevenf(v) of an out-of-range v is undefined in C++."""
    L, R, raw = agree_inputs(n, dt)
    for step in (0.1, 0.25, 0.05, 0.7, 1.0 / 3.0, 2.5):
        for mv in (None, 1.5 * n):
            wd, wc = ref.agree_subpixel(raw, L, R, 0.3, step, mv, nthreads=1)
            od, oc = oracle.agree_subpixel(raw, L, R, 0.3, step, mv, nthreads=1)
            assert identical(od, wd) and identical(oc, wc), (step, mv)
            zd, zc = ref.agree_subpixel(raw, L, R, 0.3, step, mv, nthreads=1, variant="O0")
            assert identical(zd, wd) and identical(zc, wc), ("-O0 differs from -O3", step, mv)
            v = np.isfinite(wd)
            assert v.any() and (~v & (raw != INVALID)).any()
            if step < 2:
                assert (wd[v] != np.round(wd[v])).any()


# --------------------------------------------------------------------- errors
@pytest.mark.parametrize("n,mode,kind,message", [
    (1, 0, "BICOS::Exception", "need at least two images"),
    (1, 1, "BICOS::Exception", "need at least two images"),
    (66, 0, "std::invalid_argument", "input stacks too large"),
    (17, 1, "std::invalid_argument", "input stacks too large"),
])
def test_errors_match(oracle, ref, n, mode, kind, message):
    s = random_stack(n, 2, 5)
    with pytest.raises(ref.RefError) as r:
        ref.match(s, s, ref.ReferenceConfig(mode=mode))
    assert r.value.kind == kind and r.value.message.startswith(message)
    with pytest.raises(oracle.OracleError) as o:
        oracle.match(s, s, oracle.OracleConfig(mode=mode))
    assert str(o.value) == message
    # the largest stacks that do fit
    for nn, m in ((65, 0), (16, 1)):
        s = random_stack(nn, 1, 3)
        assert identical(ref.match(s, s, ref.ReferenceConfig(mode=m))[0],
                         oracle.match(s, s, oracle.OracleConfig(mode=m))[0])


# ----------------------------------------------------- optimisation independence
@pytest.mark.parametrize("dt", [np.uint8, np.uint16], ids=["u8", "u16"])
@pytest.mark.parametrize("cname", SUBPIX)
def test_match_subpixel_O0_equals_O3(ref, cname, dt):
    for mode, n in ((0, 9), (0, 40), (1, 8)):
        for kind in ("random", "lowtex"):
            L, R = match_inputs(kind, n, dt, 41)
            cfg = ref.ReferenceConfig(mode=mode, **CONFIGS[cname])
            d3, c3 = ref.match(L, R, cfg)
            d0, c0 = ref.match(L, R, cfg, variant="O0")
            assert identical(d0, d3) and identical(c0, c3), (mode, n, kind)


# ----------------------------------------------------------- existing fixtures
def test_reference_reproduces_golden_npz(ref):
    from tests.golden.make_golden import CASES, inputs
    from tests.golden.make_golden import CONFIGS as GOLDEN_CONFIGS
    golden = np.load(os.path.join(HERE, "golden", "golden.npz"), allow_pickle=False)
    checked = set()
    for name, n, H, W, dt, mode, gen in CASES:
        L, R = inputs(n, H, W, dt, gen)
        for cname, cfg in GOLDEN_CONFIGS:
            d, c = ref.match(L, R, ref.ReferenceConfig(mode=mode, **cfg))
            key = "%s/%s/disparity" % (name, cname)
            assert identical(d, golden[key]), key
            checked.add(key)
            key = "%s/%s/corrmap" % (name, cname)
            assert (c is None) == (key not in golden.files), key
            if c is not None:
                assert identical(c, golden[key]), key
                checked.add(key)
    assert checked == {k for k in golden.files if not k.endswith("inputs_sha256")}


def _frames():
    return json.load(open(os.path.join(HERE, "golden", "frames.json")))


def test_reference_reproduces_frame_cfg1(ref):
    from tests.golden.make_frames import frame_record
    rec = _frames()["cfg1"]
    L, R = stereo_stack(rec["n"], rec["H"], rec["W"])
    d, c = ref.match(L, R, ref.ReferenceConfig(**rec["config"]))
    assert frame_record(rec["n"], rec["H"], rec["W"], rec["config"], L, R, d, c) == rec


def _frame_names():
    from tests.golden.make_frames import FRAMES
    return [f for f in FRAMES if f != "cfg1"]


@pytest.mark.parametrize("name", _frame_names())
def test_reference_reproduces_frame_band0(ref, name):
    from tests.golden.make_frames import FRAMES, band_hashes, frame_stacks
    rec = _frames()[name]
    rows = rec["band_rows"]
    L, R = frame_stacks(FRAMES[name], 0, rows)
    d, c = ref.match(L, R, ref.ReferenceConfig(**rec["config"]))
    assert str(d.dtype) == rec["disparity_dtype"]
    assert band_hashes(d, rows)[0] == rec["disparity_bands"][0]
    assert (c is None) == (rec["corrmap_bands"] is None)
    if c is not None:
        assert band_hashes(c, rows)[0] == rec["corrmap_bands"][0]


@pytest.mark.parametrize("kind", ["random", "periodic64", "lowtex", "random_u32", "random_u64"])
def test_reference_reproduces_search_band0(ref, kind):
    from tests.golden.make_frames import SEARCH_FLAGS, band_hashes, search_inputs
    db = _frames()
    rows = db["search_%s_nodupes" % kind]["band_rows"]
    d0, d1, bits = search_inputs(kind, ref, 0, rows)    # lowtex: the reference's transform
    for fl, (flags, lr) in SEARCH_FLAGS.items():
        d = ref.search(d0, d1, flags, lr)
        assert band_hashes(d, rows)[0] == db["search_%s_%s" % (kind, fl)]["disparity_bands"][0], fl


# ------------------------------------------------ reference-made fixtures (ref_frames.json)
@pytest.fixture(scope="module")
def ref_frames():
    return json.load(open(MRF.PATH))


def test_ref_frames_is_current(ref, ref_frames):
    """make_ref_frames.py reproduces the committed file exactly, from the reference alone."""
    assert MRF.generate(ref.match, ref.ReferenceConfig) == ref_frames


def test_oracle_reproduces_ref_frames(oracle, ref_frames):
    assert MRF.generate(oracle.match, oracle.OracleConfig) == ref_frames


def test_ref_frames_cover_the_plans(ref_frames):
    """No reference needed: the committed file has every case and config, its inputs
    regenerate to the stored hashes, and the stored results are not trivial."""
    assert ref_frames["configs"] == CONFIGS
    assert sorted(ref_frames["cases"]) == sorted(MRF.CASES)
    for name, case in MRF.CASES.items():
        rec = ref_frames["cases"][name]
        assert {k: rec[k] for k in case} == case
        L, R = MRF.case_stacks(case)
        assert [MRF.sha(L), MRF.sha(R)] == rec["inputs_sha256"], name
        assert sorted(rec["results"]) == sorted(CONFIGS)
        for cname, cfg in CONFIGS.items():
            r = rec["results"][cname]
            nxc = cfg["nxcorr_threshold"] is not None
            assert r["disparity_dtype"] == ("float32" if nxc else "int16")
            assert (r["corrmap_sha256"] is not None) == nxc
            assert len(r["disparity_rows"]) == case["H"]
            assert len(set(r["disparity_rows"])) == case["H"]       # rows differ: not all invalid


def _gpu_match(eng, L, R, **kw):
    import torch
    from libbicos_amd.device import MatchConfig

    def dev(a):
        a = np.ascontiguousarray(a)
        return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda()

    d, c = eng.match(dev(L), dev(R), MatchConfig(**kw))
    return d.cpu().numpy(), (None if c is None else c.cpu().numpy())


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(MRF.CASES))
def test_gpu_reproduces_reference(gpu, ref_frames, name):
    """Engine.match against results the reference itself produced, every config."""
    rec = ref_frames["cases"][name]
    L, R = MRF.case_stacks(rec)
    assert [MRF.sha(L), MRF.sha(R)] == rec["inputs_sha256"], "synthetic generator changed"
    failures = []
    for cname, cfg in ref_frames["configs"].items():
        want = rec["results"][cname]
        d, c = _gpu_match(gpu, L, R, mode=rec["mode"], **cfg)
        assert str(d.dtype) == want["disparity_dtype"], cname
        assert (c is None) == (want["corrmap_sha256"] is None) and d.shape == (rec["H"], rec["W"])
        for what, m in (("disparity", d), ("corrmap", c)):
            if m is None or MRF.sha(m) == want[what + "_sha256"]:
                continue
            rows = [y for y, (a, b) in enumerate(zip(MRF.row_hashes(m), want[what + "_rows"]))
                    if a != b]
            failures.append("%s %s: rows %s differ from the reference" % (cname, what, rows))
    assert not failures, "%s: %s" % (name, "; ".join(failures))
