"""The host-buffer match (host.cpp match_host: bicos_match_host, pybicos.match) at small bands
and through its other pipelines.

match_host uploads each row band in one copy, or in two over two copy streams cut at a
multiple of 4096 bytes. A band of under 4096 bytes once got a first copy of 4096: past its
pinned slot and, on the device, over the following bands and the finished disparity rows of
band 0 (tests/test_host_plan.py has the arithmetic, on the CPU). Here the frames whose bands
lie around that page (tests/host_small_cases.py SMALL) run on the GPU, byte for byte against
the device-resident match and the CPU oracle: every config that changes the maps' types,
back to back on one engine, under the three environment switches that select the library's
other pipelines (read once per process: one child process each), with Precision.DOUBLE, in a
sequence that changes the band plan on one engine, and at the band sizes whose last bytes the
delivery into the caller's buffers once left out (DELIVERY_TAIL).
"""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests.host_small_cases import (CONFIGS, DELIVERY_TAIL, DOUBLE, LARGE, MULTI_BAND,  # noqa: E402
                                    SEQUENCE, SMALL, case_id, match_host_guarded, stacks)

pytestmark = pytest.mark.gpu

THR = CONFIGS["thr"]
MIN_VALID = 0.40  # of the oracle's map: a comparison of two empty maps would prove nothing
PIPELINES = {
    "dl_once": dict(BICOS_HOST_DL="once"),
    "one_stream_one_thread": dict(BICOS_HOST_UPLOAD_STREAMS="1", BICOS_HOST_THREADS="1"),
    "dl_once_one_stream": dict(BICOS_HOST_DL="once", BICOS_HOST_UPLOAD_STREAMS="1"),
}
SWITCHES = ("BICOS_HOST_DL", "BICOS_HOST_UPLOAD_STREAMS", "BICOS_HOST_THREADS")


def same(a, b):
    from tests.test_gpu_parity import same as same_bytes
    same_bytes(a, b)


def valid_fraction(d):
    v = d.astype(np.float64)
    return float((np.isfinite(v) & (v != -32768)).mean())


_DEVICE = {}


def device_match(gpu, shape, cfg_name, kw):
    """the device-resident match of the frame's stacks (default seed), computed once"""
    key = (case_id(shape), cfg_name)
    if key not in _DEVICE:
        from tests.test_gpu_parity import gpu_match
        L, R = stacks(*shape[:4])
        _DEVICE[key] = gpu_match(gpu, L, R, **kw)
    return _DEVICE[key]


def oracle_match(oracle, L, R, kw):
    return oracle.match(L, R, oracle.OracleConfig(**kw))


# ------------------------------------------------------------------ a. small-band matrix
@pytest.mark.parametrize("cfg_name", list(CONFIGS))
@pytest.mark.parametrize("shape", SMALL, ids=case_id)
def test_small_bands_equal_device_and_oracle(gpu, oracle, shape, cfg_name):
    kw = CONFIGS[cfg_name]
    L, R = stacks(*shape)
    d, c = match_host_guarded(L, R, **kw)  # (asserts guards and inputs untouched)
    od, oc = oracle_match(oracle, L, R, kw)
    frac = valid_fraction(od)
    print("%s %s: %.3f of the oracle's pixels valid" % (case_id(shape), cfg_name, frac))
    assert frac >= MIN_VALID, frac
    gd, gc = device_match(gpu, shape, cfg_name, kw)
    same(d, gd)
    same(d, od)
    assert (c is None) == (oc is None) == (gc is None)
    if c is not None:
        same(c, gc)
        same(c, oc)


# ----------------------------------------------------- the delivery's last chunk (DELIVERY_TAIL)
@pytest.mark.parametrize("cfg_name", ["raw", "thr"])
@pytest.mark.parametrize("shape", DELIVERY_TAIL, ids=case_id)
def test_last_bytes_of_every_band_are_delivered(gpu, oracle, shape, cfg_name):
    """Bands whose bytes of a map are 512 k + r, 0 < r < 8: the 8 chunks the pool copies into
    the caller's buffers once ended r bytes short. The caller's buffers start as guard bytes,
    which no map holds."""
    kw = CONFIGS[cfg_name]
    L, R = stacks(*shape)
    d, c = match_host_guarded(L, R, **kw)
    gd, gc = device_match(gpu, shape, cfg_name, kw)
    same(d, gd)
    od, oc = oracle_match(oracle, L, R, kw)
    assert valid_fraction(od) >= MIN_VALID
    same(d, od)
    if c is not None:
        same(c, gc)
        same(c, oc)


# -------------------------------------------------------------------- b. back to back
@pytest.mark.parametrize("shape", MULTI_BAND, ids=case_id)
def test_back_to_back_calls_on_one_engine(gpu, oracle, shape):
    """Eight calls, eight different frames: data left in the stage, the slots or the pinned
    maps by the call before would show."""
    from libbicos_amd.synthetic import SEED
    for i in range(8):
        L, R = stacks(*shape, seed=SEED + 1 + i)
        d, c = match_host_guarded(L, R, **THR)
        od, oc = oracle_match(oracle, L, R, THR)
        same(d, od)
        same(c, oc)


# ---------------------------------------------------------------- c. the other pipelines
def run_pipeline_cases():
    """Every SMALL and LARGE frame at threshold 0.5 through this process's pipeline
    (pybicos.match on numpy arrays: no torch), keyed by frame."""
    import pybicos
    out = {}
    cfg = pybicos.Config()
    cfg.nxcorr_threshold = THR["nxcorr_threshold"]
    for shape in SMALL + LARGE:
        L, R = stacks(*shape)
        d, c = pybicos.match(list(L), list(R), cfg)
        out["d_" + case_id(shape)] = d
        out["c_" + case_id(shape)] = c
    return out


@pytest.fixture(scope="module")
def default_pipeline(gpu):
    assert not any(k in os.environ for k in SWITCHES), "the suite runs the default pipeline"
    return run_pipeline_cases()


@pytest.mark.parametrize("name", list(PIPELINES))
def test_other_pipelines_give_the_same_bytes(gpu, default_pipeline, tmp_path, name):
    path = str(tmp_path / (name + ".npz"))
    env = dict(os.environ, **PIPELINES[name])
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--pipeline", name, path],
                       env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    with np.load(path) as z:
        got = {k: z[k] for k in z.files}
    assert set(got) == set(default_pipeline)
    for shape in SMALL + LARGE:
        gd, gc = device_match(gpu, shape, "thr", THR)
        for k, ref in (("d_", gd), ("c_", gc)):
            same(got[k + case_id(shape)], default_pipeline[k + case_id(shape)])
            same(got[k + case_id(shape)], ref)


# ------------------------------------------------------------------- d. Precision.DOUBLE
@pytest.mark.parametrize("shape", DOUBLE, ids=case_id)
def test_double_corrmap_through_the_bands(gpu, shape):
    import pybicos
    from tests.test_gpu_parity import gpu_match
    L, R = stacks(*shape)
    cfg = pybicos.Config()
    cfg.nxcorr_threshold = 0.5
    cfg.precision = pybicos.Precision.DOUBLE
    d, c = pybicos.match(list(L), list(R), cfg)
    assert c.dtype == np.float64
    gd, gc = gpu_match(gpu, L, R, nxcorr_threshold=0.5, precision=1)
    same(d, gd)
    same(c, gc)
    assert valid_fraction(d) >= MIN_VALID


# ------------------------------------------------------- e. one engine, changing frames
def test_one_engine_changing_frames(gpu):
    """K goes 3 -> 1 -> 3 along the sequence, events and pinned buffers are reused, and the
    maps' types change: uint8 / uint16 stacks, float / int16 disparity, float / double
    corrmap."""
    from tests.test_gpu_parity import gpu_match
    for n, H, W, dt, kw in SEQUENCE:
        L, R = stacks(n, H, W, dt)
        d, c = match_host_guarded(L, R, **kw)
        gd, gc = gpu_match(gpu, L, R, **kw)
        same(d, gd)
        assert (c is None) == (gc is None)
        if c is not None:
            same(c, gc)


if __name__ == "__main__":
    # child of test_other_pipelines_give_the_same_bytes: this process's library switches
    assert sys.argv[1] == "--pipeline"
    want = PIPELINES[sys.argv[2]]
    assert {k: os.environ.get(k) for k in SWITCHES} == {k: want.get(k) for k in SWITCHES}
    np.savez(sys.argv[3], **run_pipeline_cases())
    assert "torch" not in sys.modules
