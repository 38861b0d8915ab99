"""bicos-cli -q Q.yml --mesh [--mesh-diff F]: the .ply beside the .xyz. Its vertices and faces
must be the restatement (tests/mesh_ref.py) of the TIFF map that the CLI wrote, with the CLI's
flags (no sentinel flag), and its vertices the points of the .xyz.
"""
import os
import subprocess

import numpy as np
import pytest

from tests import mesh_ref as ref
from tests.test_cli import CLI, Q, YAML, _built, _write_folder, read_tiff
from tests.test_mesh_api import read_ply
from tests.test_reproject_api import xyz_text

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no ROCm GPU")
    _built()
    from libbicos_amd.synthetic import stereo_stack
    L, R = stereo_stack(12, 40, 200)
    base = tmp_path_factory.mktemp("mesh_cli")
    src = str(base / "in")
    _write_folder(src, L, R, False)
    qf = base / "q.yml"
    qf.write_text(YAML.format(", ".join(repr(float(v)) for v in Q.ravel())))
    return src, str(qf)


def cli(folder, tmp_path, extra, with_q=True):
    src, qf = folder
    out = str(tmp_path / "out" / "disp.png")
    os.makedirs(os.path.dirname(out))
    r = subprocess.run([CLI, src] + extra + ["-o", out] + (["-q", qf] if with_q else []),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr + r.stdout
    return r, str(tmp_path / "out")


@pytest.mark.parametrize("extra,flags,max_diff",
                         [(["--mesh"], 0, 1.0),
                          (["--mesh", "--mesh-diff", "2"], 0, 2.0),
                          (["--mesh", "--allow-negative-z", "-t", "0"], ref.ALLOW_NEGATIVE_Z, 1.0),
                          (["--mesh", "-s", "0.2", "--mesh-diff", "1.5"], 0, 1.5)],
                         ids=["default", "diff_2", "int16_allow_negative_z", "subpixel_diff_1.5"])
def test_cli_mesh(folder, tmp_path, extra, flags, max_diff):
    r, out = cli(folder, tmp_path, extra)
    d = read_tiff(os.path.join(out, "disp.tiff"))
    want = ref.restate(d, Q, flags, max_diff)
    # (the floor of the end-to-end test: more triangles than quads)
    assert want["mesh_counts"][0] > 39 * 199 and want["counts"][0] > 0.3 * d.size
    pts, tri = read_ply(os.path.join(out, "disp.ply"))
    assert np.array_equal(pts.view(np.uint32), want["points"].view(np.uint32))
    assert np.array_equal(tri, want["triangles"])
    assert open(os.path.join(out, "disp.xyz"), "rb").read() == xyz_text(pts)
    assert "Saved mesh (%d vertices, %d triangles)" % (len(pts), len(tri)) in r.stdout
    assert "no effect" not in r.stderr


def test_cli_mesh_with_normals_keeps_the_points(folder, tmp_path):
    """--normals changes the .xyz lines, not the mesh: the same call feeds both"""
    r, out = cli(folder, tmp_path, ["--mesh", "-s", "0.2", "--normals", "2"])
    d = read_tiff(os.path.join(out, "disp.tiff"))
    want = ref.restate(d, Q, 0, 1.0)
    pts, tri = read_ply(os.path.join(out, "disp.ply"))
    assert np.array_equal(pts.view(np.uint32), want["points"].view(np.uint32))
    assert np.array_equal(tri, want["triangles"])
    lines = open(os.path.join(out, "disp.xyz")).read().split("\n")[:-1]
    assert len(lines) == len(pts) and all(len(ln.split()) == 6 for ln in lines)


def test_cli_mesh_warnings(folder, tmp_path):
    r, out = cli(folder, tmp_path / "a", ["--mesh", "--mesh-diff", "2"], with_q=False)
    assert "'mesh' has no effect without a Q matrix." in r.stderr
    assert "'mesh-diff' has no effect without a Q matrix." in r.stderr
    assert not os.path.exists(os.path.join(out, "disp.ply"))
    r, out = cli(folder, tmp_path / "b", ["--mesh-diff", "2"])
    assert "'mesh-diff' has no effect without 'mesh'." in r.stderr
    assert not os.path.exists(os.path.join(out, "disp.ply"))
    assert os.path.exists(os.path.join(out, "disp.xyz"))
