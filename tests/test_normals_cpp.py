"""BICOS::normals (include/bicos/normals.hpp) in its three forms, on a host and on a device
map, through the driver tests/cpp/normals_cpp: every dumped map and list bit for bit against
restatement (a) of tests/normals_ref.py, the counts as integers. The driver itself checks that
the error cases throw BICOS::Exception.
"""
import os
import subprocess

import numpy as np
import pytest

from libbicos_amd import _lib
from tests import normals_ref as ref
from tests.test_cli import _built

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NORMALS_CPP = os.path.join(ROOT, "tests", "cpp", "normals_cpp")


@pytest.mark.parametrize("dtype,flags,radius,max_diff,min_points",
                         [("int16", 0, 1, 1.0, 3), ("float32", 2, 2, 1.0, 5),
                          ("float32", 1, 4, 0.5, 3)])
def test_cpp_api(gpu, dtype, flags, radius, max_diff, min_points, tmp_path):
    _built()
    if not os.path.exists(NORMALS_CPP):
        subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "cpp"), "-f", "normals.mk"],
                       check=True, capture_output=True)
    tr, tc = _lib.normals_tile()
    rows, cols = tr + 3, tc + 5
    name = "odd-q" if flags & 1 else "random-holes"
    d, q = [p for p in ref.patterns(rows, cols, np.dtype(dtype).type) if p[0] == name][0][1:]
    want = ref.restate(d, q, flags, radius, max_diff, min_points)
    assert want["counts"][0] and want["counts"][1]
    rng = np.random.default_rng(5)
    index = np.concatenate([rng.permutation(rows * cols)[:500], [0, 0, -1, rows * cols]]).astype(np.int32)
    listed = ref.gather(want["map"], index)
    (tmp_path / "d.raw").write_bytes(d.tobytes())
    (tmp_path / "q.raw").write_bytes(np.ascontiguousarray(q, np.float64).tobytes())
    (tmp_path / "i.raw").write_bytes(index.tobytes())
    prefix = str(tmp_path / "o")
    r = subprocess.run([NORMALS_CPP, str(tmp_path / "d.raw"), str(rows), str(cols),
                        str(_lib.CV_32F if dtype == "float32" else _lib.CV_16S),
                        str(tmp_path / "q.raw"), str(tmp_path / "i.raw"), str(index.size),
                        str(flags), str(radius), repr(max_diff), str(min_points), prefix],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr + r.stdout
    line = " ".join(str(int(v)) for v in want["counts"])
    assert r.stdout.split("\n")[:3] == ["hostboth " + line, "devboth " + line, "buf " + line]
    for form in ("host", "dev", "hostboth", "devboth", "buf"):
        assert open(prefix + "." + form + ".map", "rb").read() == want["map"].tobytes(), form
    for form in ("host", "dev", "hostboth", "devboth", "buf"):
        assert open(prefix + "." + form + ".list", "rb").read() == listed.tobytes(), form
