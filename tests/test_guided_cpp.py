"""BICOS::guide_from_disparity and the guided BICOS::match overload (include/bicos/guide.hpp,
include/bicos/match.hpp) through tests/cpp/guided_cpp.cpp, in host and in device memory,
against the restatements of tests/test_guided_api.py and the Python device path.
"""
import os
import subprocess

import numpy as np
import pytest

from libbicos_amd import _lib
from tests.test_guided_api import guide_ref
from tests.test_range_gpu import RANGE, dev, host, same, stacks

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUIDED_CPP = os.path.join(ROOT, "tests", "cpp", "guided_cpp")
N, DT = 8, np.uint8
RADIUS, SPREAD, SCALE, FALLBACK = 3, 1, 2, (8, 71)


def _exe():
    """build() builds it; built here if it has not been"""
    if not os.access(GUIDED_CPP, os.X_OK):
        subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "cpp"), "-f", "guided.mk"],
                       check=True, capture_output=True)
    return GUIDED_CPP


def _prior(dtype):
    """a half-size prior of the 4 x 301 stacks: 2 x 151 disparities around half the planted
    range, with holes"""
    rng = np.random.default_rng(11)
    p = rng.uniform(4, 35, (2, 151)).astype(np.float32)
    if dtype == np.int16:
        p = np.round(p).astype(np.int16)
        p[rng.random(p.shape) < 0.2] = -32768
    else:
        p[rng.random(p.shape) < 0.2] = np.nan
        p[0, 5] = -32768.0
    p[:, 40:44] = -32768 if dtype == np.int16 else np.nan
    return p


def _run(tmp_path, prior, lo, hi):
    L, R = stacks(N, DT)
    inp = tmp_path / "in.bin"
    with open(inp, "wb") as f:
        f.write(np.array([N, L.shape[1], L.shape[2], np.dtype(DT).itemsize], np.int32).tobytes())
        f.write(np.ascontiguousarray(L).tobytes())
        f.write(np.ascontiguousarray(R).tobytes())
    raw = tmp_path / "prior.raw"
    raw.write_bytes(prior.tobytes())
    typ = _lib.CV_32F if prior.dtype == np.float32 else _lib.CV_16S
    args = [_exe(), str(inp), str(raw), str(prior.shape[0]), str(prior.shape[1]), str(typ),
            str(RADIUS), str(SPREAD), str(SCALE), str(FALLBACK[0]), str(FALLBACK[1]), str(lo),
            str(hi), str(tmp_path / "o")]
    return subprocess.run(args, capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("dtype", [np.int16, np.float32], ids=["int16", "float32"])
def test_cpp_guide_and_guided_match(gpu, tmp_path, dtype):
    from libbicos_amd.device import MatchConfig
    L, R = stacks(N, DT)
    rows, cols = L.shape[1:]
    prior = _prior(dtype)
    want, wc = guide_ref(prior, (rows, cols), RADIUS, SPREAD, SCALE, FALLBACK, True)
    assert wc[0] and wc[1]
    r = _run(tmp_path, prior, *RANGE)
    assert r.returncode == 0, r.stdout + r.stderr
    line = "%d %d" % tuple(wc)
    assert r.stdout.split("\n")[:3] == ["host " + line, "dev " + line, "buf " + line]
    for form in ("host", "dev", "buf"):
        g = np.fromfile(tmp_path / ("o.%s.guide" % form), np.int16).reshape(rows, cols, 2)
        same(g, want, form + " guide")
    d, c = gpu.match(dev(L), dev(R), MatchConfig(nxcorr_threshold=0.9, disparity_range=RANGE),
                     guide=dev(want))
    d, c = host(d), host(c)
    unguided, _ = gpu.match(dev(L), dev(R), MatchConfig(nxcorr_threshold=0.9,
                                                         disparity_range=RANGE))
    assert (host(unguided) != d).any()  # random windows: not the ranged map
    for form in ("host", "dev"):
        same(np.fromfile(tmp_path / ("o.%s.disp" % form), np.float32).reshape(d.shape), d,
             form + " disparity")
        same(np.fromfile(tmp_path / ("o.%s.corr" % form), np.float32).reshape(c.shape), c,
             form + " corrmap")


def test_cpp_guided_min_above_max_throws(gpu, tmp_path):
    r = _run(tmp_path, _prior(np.int16), 5, 4)
    assert r.returncode == 5, r.stdout + r.stderr
    assert "exception:" in r.stdout and "disparity" in r.stdout
