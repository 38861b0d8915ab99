"""bicos-cli --median / --median-fill: the saved disparity and the point cloud are the
restatements (tests/median_ref.py, then tests/test_reproject_api.py) applied to what the same
run without the options saves; with --speckle-size the speckle filter comes first; and
--median-fill alone changes nothing but prints a notice.
"""
import os
import subprocess

import pytest

from tests import median_ref as ref
from tests import speckle_ref
from tests.test_cli import CLI, Q, YAML, _built, _write_folder, read_tiff
from tests.test_reproject_api import restate as reproject_restate
from tests.test_reproject_api import xyz_text

pytestmark = pytest.mark.gpu

FILES = ("disp.png", "disp.tiff", "disp.xyz")


def _run(src, outdir, qf, extra):
    os.makedirs(outdir)
    r = subprocess.run([CLI, src] + extra + ["-o", os.path.join(outdir, "disp.png"), "-q", str(qf)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr + r.stdout
    return {f: open(os.path.join(outdir, f), "rb").read() for f in FILES}, r


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no ROCm GPU")
    _built()
    from libbicos_amd.synthetic import stereo_stack
    L, R = stereo_stack(12, 40, 200)
    base = tmp_path_factory.mktemp("median_cli")
    src = str(base / "in")
    _write_folder(src, L, R, False)
    qf = base / "q.yml"
    qf.write_text(YAML.format(", ".join(repr(float(v)) for v in Q.ravel())))
    return base, src, qf


@pytest.mark.parametrize("extra,median,ksize,fill_min",
                         [([], ["--median", "3"], 3, 0),
                          (["-t", "0"], ["--median", "5", "--median-fill", "13"], 5, 13),
                          (["-s", "0.2"], ["--median=5", "--median-fill", "13"], 5, 13)],
                         ids=["default_3", "int16_5_fill", "subpixel_5_fill"])
def test_cli_median_filter(folder, extra, median, ksize, fill_min):
    base, src, qf = folder
    tag = "-".join(extra + median).replace("--", "").replace("=", "")
    plain, _ = _run(src, str(base / ("plain" + tag)), qf, extra)
    filtered, r = _run(src, str(base / ("filtered" + tag)), qf, extra + median)
    d = read_tiff(str(base / ("plain" + tag) / "disp.tiff"))
    # the flags of the tool's speckle and reprojection calls: no sentinel
    want = ref.restate(d, ksize, fill_min, False)
    assert want["counts"][1] > 0 and (fill_min == 0 or want["counts"][2] > 0)
    got = read_tiff(str(base / ("filtered" + tag) / "disp.tiff"))
    assert got.dtype == d.dtype and got.tobytes() == want["out"].tobytes()
    points = reproject_restate(want["out"], Q, 0)
    assert filtered["disp.xyz"] == xyz_text(points["points"])
    assert filtered["disp.xyz"] != plain["disp.xyz"]
    assert "changed %d pixels, filled %d" % (want["counts"][1], want["counts"][2]) in r.stdout


def test_cli_speckle_filter_runs_before_the_median(folder):
    base, src, qf = folder
    _run(src, str(base / "order_plain"), qf, ["-t", "0"])
    _run(src, str(base / "order_both"), qf, ["-t", "0", "--median", "5", "--median-fill", "13",
                                             "--speckle-size", "20"])
    d = read_tiff(str(base / "order_plain" / "disp.tiff"))
    first = speckle_ref.restate(d, 20, 1.0, False)["out"]
    want = ref.restate(first, 5, 13, False)["out"]
    other = speckle_ref.restate(ref.restate(d, 5, 13, False)["out"], 20, 1.0, False)["out"]
    assert want.tobytes() != other.tobytes()  # the order matters on this frame
    got = read_tiff(str(base / "order_both" / "disp.tiff"))
    assert got.tobytes() == want.tobytes()


def test_cli_median_fill_alone_is_a_notice(folder):
    base, src, qf = folder
    plain, _ = _run(src, str(base / "alone_plain"), qf, [])
    alone, r = _run(src, str(base / "alone"), qf, ["--median-fill", "5"])
    for f in FILES:
        assert alone[f] == plain[f], f
    assert "'median-fill' has no effect without 'median'" in r.stderr


def test_cli_refuses_other_apertures_and_documents_the_options(folder):
    base, src, qf = folder
    for bad in (["--median", "4"], ["--median", "3", "--median-fill", "10"]):
        r = subprocess.run([CLI, src] + bad + ["-o", str(base / "bad.png")], capture_output=True,
                           text=True, timeout=120)
        assert r.returncode != 0
    h = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60)
    assert "--median K" in h.stdout + h.stderr and "--median-fill M" in h.stdout + h.stderr
