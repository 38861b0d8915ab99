"""bicos-cli -q Q.yml --mesh --texture IMAGE --texture-camera FILE [--texture-tol F]
[--texture-splat S]: the coloured .ply of a tiny stack, byte for byte against the Python layers:
the mesh of the TIFF map that the CLI wrote (pybicos.mesh) and its vertices projected into the
texture camera (pybicos.project), packed as the definition of write_ply_colored says.
"""
import os
import subprocess

import numpy as np
import pytest

from tests import project_ref as ref
from tests.test_cli import CLI, Q, YAML, _built, _write_folder, png_bytes, read_tiff
from tests.test_project_api import ply_colored_bytes

pytestmark = pytest.mark.gpu

ROWS, COLS = 40, 200
CAMERA = """%YAML:1.0
---
K: !!opencv-matrix
   rows: 3
   cols: 3
   dt: d
   data: [ {} ]
"""
MATRIX = """{}: !!opencv-matrix
   rows: {}
   cols: {}
   dt: d
   data: [ {} ]
"""


def numbers(a):
    return ", ".join(repr(float(v)) for v in np.asarray(a).ravel())


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no ROCm GPU")
    _built()
    from libbicos_amd.synthetic import stereo_stack
    L, R = stereo_stack(12, ROWS, COLS)
    base = tmp_path_factory.mktemp("project_cli")
    src = str(base / "in")
    _write_folder(src, L, R, False)
    qf = base / "q.yml"
    qf.write_text(YAML.format(numbers(Q)))
    img = ref.picture(ROWS, COLS, 1, np.uint8)
    (base / "tex.png").write_bytes(png_bytes(img, 0, 8))
    return src, str(qf), str(base / "tex.png"), img, base


# the rectified left camera itself (Q's focal length and centre), and a camera beside it
def own_camera():
    return np.array([[Q[2, 3], 0, -Q[0, 3]], [0, Q[2, 3], -Q[1, 3]], [0, 0, 1]]), None, None, None


def other_camera():
    K, D, R, t = ref.rig(ROWS, COLS, 5)
    K[0, 0], K[1, 1], K[0, 2], K[1, 2] = Q[2, 3], Q[2, 3] * 1.01, -Q[0, 3] + 3.3, -Q[1, 3] - 2.1
    return K, D, R, np.array([0.004, -0.002, 0.01])


@pytest.mark.parametrize("camera,extra,splat,tol",
                         [(own_camera, [], 0, float("inf")),
                          (other_camera, [], 0, float("inf")),
                          (other_camera, ["--texture-tol", "0.25"], 1, 0.25),
                          (other_camera, ["--texture-tol", "0", "--texture-splat", "3"], 3, 0.0)],
                         ids=["own", "other", "other_tol", "other_tol_0_splat_3"])
def test_cli_texture(folder, tmp_path, camera, extra, splat, tol):
    import pybicos
    src, qf, png, img, base = folder
    K, D, R, t = camera()
    cam = tmp_path / "cam.yml"
    text = CAMERA.format(numbers(K))
    for name, m, shape in (("D", D, (1, 5)), ("R", R, (3, 3)), ("T", t, (3, 1))):
        if m is not None:
            text += MATRIX.format(name, shape[0], shape[1], numbers(m))
    cam.write_text(text)
    out = str(tmp_path / "out" / "disp.png")
    os.makedirs(os.path.dirname(out))
    r = subprocess.run([CLI, src, "-s", "0.25", "--mesh", "--texture", png, "--texture-camera",
                        str(cam), "-o", out, "-q", qf] + extra,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr + r.stdout
    assert "no effect" not in r.stderr
    d = read_tiff(os.path.join(os.path.dirname(out), "disp.tiff"))
    pts, tri = pybicos.mesh(d, Q, sentinel=False)
    assert len(pts) > 0.3 * d.size and len(tri) > 1000
    res = pybicos.project(pts, K, D=D, R=R, t=t, image=img, splat=splat, tol=tol,
                          outputs=("tex", "counts"))
    # (tol = 0 under a 7 x 7 splat leaves only the points nearest in their neighbourhood)
    assert res["counts"][0] > (1000 if tol > 0 else 0)
    if camera is own_camera:
        assert res["counts"].tolist() == [len(pts), 0, 0, 0, 0]
    elif tol == 0.0:
        assert res["counts"][1] > 0
    rgb = np.repeat(res["tex"], 3, axis=1)
    got = open(os.path.join(os.path.dirname(out), "disp.ply"), "rb").read()
    assert got == ply_colored_bytes(pts, rgb, tri)
    assert "Texture:\t%d vertices seen, %d occluded" % (res["counts"][0], res["counts"][1]) \
        in r.stdout


def test_cli_texture_errors_and_warnings(folder, tmp_path):
    src, qf, png, img, base = folder
    cam = tmp_path / "cam.yml"
    cam.write_text(CAMERA.format(numbers(own_camera()[0])))
    out = str(tmp_path / "disp.png")
    r = subprocess.run([CLI, src, "--mesh", "--texture", png, "-o", out, "-q", qf],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "go together" in r.stderr
    r = subprocess.run([CLI, src, "--texture", png, "--texture-camera", str(cam), "-o", out,
                        "-q", qf], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "'texture' has no effect without 'mesh'." in r.stderr
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=120)
    for word in ("--texture IMAGE", "--texture-camera FILE", "--texture-tol F",
                 "--texture-splat S"):
        assert word in r.stdout
