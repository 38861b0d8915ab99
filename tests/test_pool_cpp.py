"""BICOS::pool_stack and BICOS::match_pyramid (include/bicos/pool.hpp) through
tests/cpp/pool_cpp.cpp, in host and in device memory, against the restatement of
tests/test_pool_api.py and the Python device path.
"""
import os
import subprocess

import numpy as np
import pytest

from tests.test_pool_api import pool_ref
from tests.test_pool_gpu import COLS, ROWS, WINDOW, stacks
from tests.test_range_gpu import dev, host, same

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POOL_CPP = os.path.join(ROOT, "tests", "cpp", "pool_cpp")
N, DT = 8, np.uint8
RADIUS, SPREAD = 2, 1


def _exe():
    """build() builds it; built here if it has not been"""
    if not os.access(POOL_CPP, os.X_OK):
        subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "cpp"), "-f", "pool.mk"],
                       check=True, capture_output=True)
    return POOL_CPP


def _run(tmp_path, scale, lo, hi):
    L, R = stacks(N, DT)
    inp = tmp_path / "in.bin"
    with open(inp, "wb") as f:
        f.write(np.array([N, ROWS, COLS, np.dtype(DT).itemsize], np.int32).tobytes())
        f.write(np.ascontiguousarray(L).tobytes())
        f.write(np.ascontiguousarray(R).tobytes())
    args = [_exe(), str(inp), str(scale), str(RADIUS), str(SPREAD), str(lo), str(hi),
            str(tmp_path / "o")]
    return subprocess.run(args, capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("scale", [2, 3])
def test_cpp_pool_stack_and_match_pyramid(gpu, tmp_path, scale):
    import torch
    from libbicos_amd.device import MatchConfig
    L, R = stacks(N, DT)
    counts = torch.zeros((2,), dtype=torch.int32, device="cuda")
    d, c, guide, coarse = gpu.match_pyramid(
        dev(L), dev(R), MatchConfig(nxcorr_threshold=0.9, disparity_range=WINDOW), scale=scale,
        radius=RADIUS, spread=SPREAD, return_guide=True, return_coarse=True, counts=counts)
    wc = host(counts).view(np.uint32)
    r = _run(tmp_path, scale, *WINDOW)
    assert r.returncode == 0, r.stdout + r.stderr
    line = "%d %d" % (wc[0], wc[1])
    assert r.stdout.split("\n")[:2] == ["host " + line, "dev " + line]
    pooled = pool_ref(L, scale)
    for form in ("host", "dev"):
        def load(what, like):
            return np.fromfile(tmp_path / ("o.%s.%s" % (form, what)), like.dtype).reshape(like.shape)
        same(load("pool", pooled), pooled, form + " pooled stack")
        same(load("disp", host(d)), host(d), form + " disparity")
        same(load("corr", host(c)), host(c), form + " corrmap")
        same(load("coarse", host(coarse)), host(coarse), form + " coarse map")
        same(load("guide", host(guide)), host(guide), form + " guide")


def test_cpp_pyramid_min_above_max_throws(gpu, tmp_path):
    r = _run(tmp_path, 2, 5, 4)
    assert r.returncode == 5, r.stdout + r.stderr
    assert "exception:" in r.stdout and "disparity" in r.stdout
