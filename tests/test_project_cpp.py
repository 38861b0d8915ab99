"""BICOS::project (include/bicos/project.hpp) in its two forms, host vectors and device buffers,
through the driver tests/cpp/project_cpp on arrays this test writes: every dumped file byte for
byte against the restatement of tests/project_ref.py, the counts as integers. The driver itself
checks that the error cases throw BICOS::Exception.
"""
import os
import subprocess

import numpy as np
import pytest

from tests import project_ref as ref
from tests.test_cli import _built

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROJECT_CPP = os.path.join(ROOT, "tests", "cpp", "project_cpp")
FILES = dict(uv="uv", depth="depth", cls="cls", tex="tex", dmap="depth_map", imap="index_map")


@pytest.mark.parametrize("nd,channels,dtype,pad,splat,tol",
                         [(0, 1, np.uint8, 0, 0, 0.0), (5, 3, np.uint8, 6, 1, 0.5),
                          (8, 3, np.uint16, 3, 3, float("inf"))],
                         ids=["grey_u8", "rgb_u8_pitched", "rgb_u16_no_test"])
def test_cpp_api(gpu, nd, channels, dtype, pad, splat, tol, tmp_path):
    _built()
    if not os.path.exists(PROJECT_CPP):
        subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "cpp"), "-f", "project.mk"],
                       check=True, capture_output=True)
    rows, cols, n = 48, 64, 1025
    K, D, R, t = ref.rig(rows, cols, nd)
    pts = ref.cloud(n, rows, cols, K)
    img = ref.picture(rows, cols, channels, dtype)
    want = ref.restate(pts, ref.camera(K, D, R, t), (rows, cols), splat, tol, img, 5)
    assert (want["counts"][[0, 2, 3, 4]] > 0).all()
    himg = np.zeros((rows, cols * channels + pad), dtype)
    himg[:, :cols * channels] = img.reshape(rows, -1)
    (tmp_path / "p.raw").write_bytes(pts.tobytes())
    cam = np.concatenate([K.ravel(), R.ravel(), t.ravel(), np.zeros(0) if D is None else D])
    (tmp_path / "c.raw").write_bytes(cam.astype(np.float64).tobytes())
    (tmp_path / "i.raw").write_bytes(himg.tobytes())
    prefix = str(tmp_path / "o")
    r = subprocess.run([PROJECT_CPP, str(tmp_path / "p.raw"), str(n), str(tmp_path / "c.raw"),
                        str(nd), str(rows), str(cols), str(tmp_path / "i.raw"), str(channels),
                        str(himg.itemsize), str(pad), str(splat), repr(tol), "5", prefix],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr + r.stdout
    line = " ".join(str(int(v)) for v in want["counts"])
    assert r.stdout.split("\n")[:2] == ["host " + line, "dev " + line]
    for form in ("host", "dev"):
        for ext, name in FILES.items():
            got = open("%s.%s.%s" % (prefix, form, ext), "rb").read()
            assert got == want[name].tobytes(), (form, name)
