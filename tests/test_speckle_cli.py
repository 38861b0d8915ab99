"""bicos-cli --speckle-size / --speckle-diff: the saved disparity and the point cloud are the
restatements (tests/speckle_ref.py, then tests/test_reproject_api.py) applied to what the same
run without the options saves; without the options nothing changes (tests/test_cli.py and
tests/test_reproject_gpu.py pin those files; here a filter that removes nothing must reproduce
them byte for byte).
"""
import os
import subprocess

import numpy as np
import pytest

from tests import speckle_ref as ref
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


@pytest.mark.parametrize("extra,speckle", [([], ["--speckle-size", "20"]),
                                           (["-t", "0"], ["--speckle-size", "30", "--speckle-diff", "2"]),
                                           (["-s", "0.2"], ["--speckle-size=12", "--speckle-diff", "0.5"])],
                         ids=["default", "int16", "subpixel"])
def test_cli_speckle_filter(extra, speckle, tmp_path):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no ROCm GPU")
    _built()
    from libbicos_amd.synthetic import stereo_stack
    L, R = stereo_stack(12, 40, 200)
    src = str(tmp_path / "in")
    _write_folder(src, L, R, False)
    qf = tmp_path / "q.yml"
    qf.write_text(YAML.format(", ".join(repr(float(v)) for v in Q.ravel())))
    corr = [] if extra == ["-t", "0"] else ["--corrmap"]  # (it would turn the int16 map float)
    plain, _ = _run(src, str(tmp_path / "plain"), qf, extra + corr)
    filtered, r = _run(src, str(tmp_path / "filtered"), qf, extra + corr + speckle)
    max_size = int(speckle[0].split("=")[1] if "=" in speckle[0] else speckle[1])
    max_diff = float(speckle[-1]) if "--speckle-diff" in speckle else 1.0

    d = read_tiff(str(tmp_path / "plain" / "disp.tiff"))
    # the flags of the tool's reprojection call: no sentinel
    want = ref.restate(d, max_size, max_diff, False)
    assert want["counts"][1] > 0 and want["counts"][0] > 0
    got = read_tiff(str(tmp_path / "filtered" / "disp.tiff"))
    assert got.dtype == d.dtype and got.tobytes() == want["out"].tobytes()
    points = reproject_restate(want["out"], Q, 0)
    assert filtered["disp.xyz"] == xyz_text(points["points"])
    assert filtered["disp.xyz"] != plain["disp.xyz"]
    assert "removed %d pixels in %d regions" % (want["counts"][1], want["counts"][3]) in r.stdout
    # the corrmap is left alone
    for f in ("disp-corrmap.png", "disp-corrmap.tiff") if corr else ():
        assert open(str(tmp_path / "filtered" / f), "rb").read() == \
            open(str(tmp_path / "plain" / f), "rb").read()

    if not extra:
        # a filter that removes nothing, and --speckle-diff alone, reproduce the plain files
        same, _ = _run(src, str(tmp_path / "zero"), qf, ["--speckle-size", "0"])
        alone, r2 = _run(src, str(tmp_path / "alone"), qf, ["--speckle-diff", "3"])
        for f in FILES:
            assert same[f] == alone[f] == plain[f], f
        assert "no effect" in r2.stderr
