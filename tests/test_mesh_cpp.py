"""BICOS::mesh (include/bicos/mesh.hpp) in its forms, on a host and on a device map, through the
driver tests/cpp/mesh_cpp: every dumped file byte for byte against the restatement of
tests/mesh_ref.py, the counts as integers. The driver itself checks that the error cases throw
BICOS::Exception.
"""
import os
import subprocess

import numpy as np
import pytest

from libbicos_amd import _lib
from tests import mesh_ref as ref
from tests.test_cli import Q, _built

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MESH_CPP = os.path.join(ROOT, "tests", "cpp", "mesh_cpp")


@pytest.mark.parametrize("dtype,flags,max_diff", [("int16", 0, 1.0), ("float32", 2, 1.0),
                                                  ("float32", 1, 0.5)])
def test_cpp_api(gpu, dtype, flags, max_diff, tmp_path):
    _built()
    if not os.path.exists(MESH_CPP):
        subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "cpp"), "-f", "mesh.mk"],
                       check=True, capture_output=True)
    rows, cols = 3, _lib.lib().bicos_reproject_segment() + 1
    d, want = ref.case(rows, cols, dtype, flags, max_diff)
    if max_diff == 1.0:
        ref.conditions(want, rows, cols)
    assert want["mesh_counts"][0] > 0 and want["mesh_counts"][3] > 0
    (tmp_path / "d.raw").write_bytes(d.tobytes())
    (tmp_path / "q.raw").write_bytes(np.ascontiguousarray(Q, np.float64).tobytes())
    prefix = str(tmp_path / "o")
    r = subprocess.run([MESH_CPP, str(tmp_path / "d.raw"), str(rows), str(cols),
                        str(_lib.CV_32F if dtype == "float32" else _lib.CV_16S),
                        str(tmp_path / "q.raw"), str(flags), repr(max_diff), prefix],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr + r.stdout
    line = " ".join(str(int(v)) for v in list(want["counts"]) + list(want["mesh_counts"]))
    assert r.stdout.split("\n")[:3] == ["host " + line, "dev " + line, "buf " + line]
    for form in ("host", "dev", "buf"):
        assert open(prefix + "." + form + ".pts", "rb").read() == want["points"].tobytes(), form
        assert open(prefix + "." + form + ".tri", "rb").read() == want["triangles"].tobytes(), form
        assert open(prefix + "." + form + ".idx", "rb").read() == want["index"].tobytes(), form
    assert open(prefix + ".buf.vmap", "rb").read() == want["vertex_map"].tobytes()
