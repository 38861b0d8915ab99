"""bicos-cli --normals: the point cloud gains three columns that equal restatement (a) of
tests/normals_ref.py applied to the disparity the same run saves; without the option the .xyz
is byte for byte what it was; and without a Q matrix the option is reported as ineffective.
"""
import os
import subprocess

import numpy as np
import pytest

from tests import normals_ref as ref
from tests.test_cli import CLI, Q, YAML, _built, _write_folder, read_tiff
from tests.test_reproject_api import restate as reproject_restate
from tests.test_reproject_api import xyz_text

pytestmark = pytest.mark.gpu

FILES = ("disp.png", "disp.tiff", "disp.xyz")


def _run(src, outdir, qf, extra):
    os.makedirs(outdir)
    q = ["-q", str(qf)] if qf is not None else []
    r = subprocess.run([CLI, src] + extra + ["-o", os.path.join(outdir, "disp.png")] + q,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr + r.stdout
    return {f: open(os.path.join(outdir, f), "rb").read() for f in FILES
            if os.path.exists(os.path.join(outdir, f))}, r


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no ROCm GPU")
    _built()
    from libbicos_amd.synthetic import stereo_stack
    L, R = stereo_stack(12, 40, 200)
    base = tmp_path_factory.mktemp("normals_cli")
    src = str(base / "in")
    _write_folder(src, L, R, False)
    qf = base / "q.yml"
    qf.write_text(YAML.format(", ".join(repr(float(v)) for v in Q.ravel())))
    return base, src, qf


def six_columns(points, normals):
    """the writer's lines: an ostream's default float format is printf's %g; 0 0 0 for no normal"""
    out = []
    for p, n in zip(points, normals):
        tail = "0 0 0" if np.isnan(n[0]) else "%g %g %g" % tuple(float(v) for v in n)
        out.append("%g %g %g %s\n" % (float(p[0]), float(p[1]), float(p[2]), tail))
    return "".join(out).encode()


@pytest.mark.parametrize("extra,opts,radius,max_diff,min_points,flags",
                         [(["-s", "0.2"], ["--normals", "2"], 2, 1.0, 3, 0),
                          (["-s", "0.2", "--allow-negative-z"],
                           ["--normals=4", "--normals-diff", "2", "--normals-min", "9"], 4, 2.0, 9, 1),
                          (["-t", "0"], ["--normals", "1", "--normals-min=9"], 1, 1.0, 9, 0)],
                         ids=["subpixel_2", "subpixel_4_diff_min_negz", "int16_1_full_window"])
def test_cli_normals(folder, extra, opts, radius, max_diff, min_points, flags):
    base, src, qf = folder
    tag = "-".join(extra + opts).replace("--", "").replace("=", "")
    plain, _ = _run(src, str(base / ("plain" + tag)), qf, extra)
    with_n, r = _run(src, str(base / ("normals" + tag)), qf, extra + opts)
    assert with_n["disp.tiff"] == plain["disp.tiff"] and with_n["disp.png"] == plain["disp.png"]
    d = read_tiff(str(base / ("normals" + tag) / "disp.tiff"))
    points = reproject_restate(d, Q, flags)
    # without the option the file is what the reprojection alone writes
    assert plain["disp.xyz"] == xyz_text(points["points"])
    want = ref.restate(d, Q, flags, radius, max_diff, min_points)
    listed = ref.gather(want["map"], points["index"])
    have = int((~np.isnan(listed[:, 0])).sum())
    assert have > 100
    if min_points == (2 * radius + 1) ** 2:  # a point on the image border has no full window
        assert have < len(listed) and b" 0 0 0\n" in with_n["disp.xyz"]
    assert with_n["disp.xyz"] == six_columns(points["points"], listed)
    assert "Normals:\t%d of %d points" % (have, len(listed)) in r.stdout


def test_cli_normals_without_q_is_a_notice(folder):
    base, src, qf = folder
    plain, _ = _run(src, str(base / "noq_plain"), None, ["-s", "0.2"])
    alone, r = _run(src, str(base / "noq"), None, ["-s", "0.2", "--normals", "2", "--normals-diff", "2"])
    assert set(alone) == {"disp.png", "disp.tiff"}
    for f in alone:
        assert alone[f] == plain[f], f
    assert "'normals' has no effect without a Q matrix" in r.stderr
    assert "'normals-diff' has no effect without a Q matrix" in r.stderr
    # the lesser options without --normals: a notice too, and the same cloud
    cloud, _ = _run(src, str(base / "q_plain"), qf, ["-s", "0.2"])
    lesser, r = _run(src, str(base / "q_lesser"), qf, ["-s", "0.2", "--normals-min", "5"])
    assert lesser["disp.xyz"] == cloud["disp.xyz"]
    assert "'normals-min' has no effect without 'normals'" in r.stderr


def test_cli_refuses_other_radii_and_documents_the_options(folder):
    base, src, qf = folder
    for bad in (["--normals", "0"], ["--normals", "5"], ["--normals", "1", "--normals-min", "10"],
                ["--normals", "2", "--normals-min", "2"], ["--normals", "2", "--normals-diff", "-1"]):
        r = subprocess.run([CLI, src] + bad + ["-o", str(base / "bad.png"), "-q", str(qf)],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode != 0, bad
    h = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60)
    for word in ("--normals R", "--normals-diff F", "--normals-min M", "stair-step"):
        assert word in h.stdout + h.stderr
