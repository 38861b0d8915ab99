"""The C++ API (include/bicos/match.hpp, hip.hpp, opencv.hpp) as a reference C++ caller
uses it (reference include/match.hpp:31-41, src/lib.cpp:31-49): tests/cpp/match_cpp runs
BICOS::match through every input branch -- host images with padded rows, host images with
dense and padded rows mixed in one stack (one step per image), device images
that form one planar buffer (zero-copy), device images in separate pitched allocations
(2-D staging), an OpenCV-shaped matrix type through bicos/opencv.hpp, and the
impl::hip::match backend seam -- and each branch's maps must equal the CPU oracle's bit
for bit.
"""
import os
import subprocess

import numpy as np
import pytest

from libbicos_amd.synthetic import stereo_stack

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "match_cpp")
BRANCHES = ("host", "host_mixed", "dev_planar", "dev_staged", "mats", "seam")


def test_cpp_driver_is_built():
    """build() compiles the driver (hipcc, no GPU needed) against the in-tree library."""
    if not os.path.exists(EXE):
        subprocess.run(["make", "-C", os.path.dirname(EXE)], check=True, capture_output=True)
    assert os.access(EXE, os.X_OK)


CASES = [
    dict(n=8, H=37, W=300, dt=np.uint8, cfg=dict(nxcorr_threshold=0.9)),
    dict(n=33, H=24, W=515, dt=np.uint8, cfg=dict(nxcorr_threshold=0.96, min_variance=2.0,
                                                  subpixel_step=0.1)),
    dict(n=12, H=19, W=257, dt=np.uint16, cfg=dict(nxcorr_threshold=None)),
    dict(n=40, H=16, W=300, dt=np.uint8, cfg=dict(nxcorr_threshold=0.96, variant=1,
                                                  max_lr_diff=1)),
    dict(n=10, H=21, W=190, dt=np.uint8, cfg=dict(nxcorr_threshold=0.5, mode=1, variant=1,
                                                  max_lr_diff=2, no_dupes=True)),
]


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: "n%d_%dx%d_%s" % (
    c["n"], c["H"], c["W"], np.dtype(c["dt"]).name))
def test_cpp_match_branches_bit_exact(case, oracle, tmp_path):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no ROCm GPU")
    test_cpp_driver_is_built()
    n, H, W, dt, cfg = case["n"], case["H"], case["W"], case["dt"], case["cfg"]
    L, R = stereo_stack(n, H, W, dt)
    inp = tmp_path / "in.bin"
    with open(inp, "wb") as f:
        f.write(np.array([n, H, W, np.dtype(dt).itemsize], np.int32).tobytes())
        f.write(np.ascontiguousarray(L).tobytes())
        f.write(np.ascontiguousarray(R).tobytes())
    g = lambda k, d: cfg.get(k, d)  # noqa: E731
    nxc = g("nxcorr_threshold", None)
    args = [EXE, str(inp), str(tmp_path / "out"), str(-1 if nxc is None else nxc),
            str(g("subpixel_step", None) or -1), str(-1 if g("min_variance", None) is None
                                                     else cfg["min_variance"]),
            str(g("mode", 0)), str(g("variant", 0)), str(g("max_lr_diff", 1)),
            str(int(g("no_dupes", False))), "0"]
    r = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = dict(l.split(" ", 1) for l in r.stdout.strip().splitlines())
    assert lines["error_case"] == "need at least two images"
    rd, rc = oracle.match(L, R, oracle.OracleConfig(**cfg))
    for b in BRANCHES:
        assert b in lines, r.stdout
        mem = "host" if b in ("host", "host_mixed", "mats", "seam") else "device"
        assert lines[b].endswith("mem=" + mem), lines[b]
        d = np.fromfile(tmp_path / ("out.%s.disp" % b), dtype=rd.dtype).reshape(H, W)
        assert np.array_equal(d.view(np.uint8), rd.view(np.uint8)), b
        cpath = tmp_path / ("out.%s.corr" % b)
        if rc is None:
            assert not cpath.exists(), b
        else:
            c = np.fromfile(cpath, dtype=rc.dtype).reshape(H, W)
            assert np.array_equal(c.view(np.uint8), rc.view(np.uint8)), b


# ----------------------------------------- the reference's installed layout (include/BICOS)
REF_EXE = os.path.join(ROOT, "build", "consumer", "ref_style")


from tools.cpp_install import install_and_build_consumer  # noqa: E402,F401


def test_installed_tree_has_the_reference_layout_and_builds_a_reference_caller(tmp_path):
    """include/BICOS/{common,match,config}.hpp + libBICOS.so / pybicos_c.so next to
    libbicos_amd.so (reference CMakeLists.txt:82-104), and a translation unit written against
    the reference's names only (#include <BICOS/match.hpp>, BICOS::Image = cv::Mat,
    BICOS::match / Config / Variant / is_invalid) builds unchanged against the installed tree
    through find_package(BICOS). CPU only: nothing is run."""
    prefix = str(tmp_path / "prefix")
    exe = install_and_build_consumer(prefix, str(tmp_path / "consumer"))
    for h in ("common.hpp", "match.hpp", "config.hpp"):
        assert os.path.exists(os.path.join(prefix, "include", "BICOS", h)), h
    lib = os.path.join(prefix, "lib")
    assert os.path.realpath(os.path.join(lib, "libBICOS.so")) == \
        os.path.realpath(os.path.join(lib, "libbicos_amd.so"))
    assert os.path.realpath(os.path.join(lib, "pybicos_c.so")) == \
        os.path.realpath(os.path.join(lib, "libbicos_amd.so"))
    assert os.access(exe, os.X_OK)
    cfg = open(os.path.join(prefix, "include", "BICOS", "config.hpp")).read()
    assert "#define BICOS_HIP" in cfg and "BICOS_VERSION" in cfg


REF_CASES = [
    dict(n=33, H=20, W=400, cfg=dict(nxcorr_threshold=0.96, min_variance=2.0, subpixel_step=0.1)),
    dict(n=8, H=30, W=256, cfg=dict(nxcorr_threshold=None)),
    dict(n=40, H=12, W=300, cfg=dict(nxcorr_threshold=0.9, variant=1, max_lr_diff=1)),
    dict(n=12, H=16, W=200, cfg=dict(nxcorr_threshold=0.5, mode=1, variant=1, max_lr_diff=2,
                                     no_dupes=True)),
]


@pytest.mark.gpu
@pytest.mark.parametrize("case", REF_CASES, ids=lambda c: "n%d_%dx%d" % (c["n"], c["H"], c["W"]))
def test_reference_style_caller_bit_exact(case, oracle, tmp_path):
    """The reference-style TU (built by build() against the installed tree) matches the oracle
    bit for bit through BICOS::match on cv::Mat stacks."""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no ROCm GPU")
    assert os.access(REF_EXE, os.X_OK), "build() builds build/consumer/ref_style"
    n, H, W, cfg = case["n"], case["H"], case["W"], case["cfg"]
    L, R = stereo_stack(n, H, W, np.uint8)
    inp = tmp_path / "in.bin"
    with open(inp, "wb") as f:
        f.write(np.array([n, H, W, 1], np.int32).tobytes())
        f.write(np.ascontiguousarray(L).tobytes())
        f.write(np.ascontiguousarray(R).tobytes())
    g = cfg.get
    nxc = g("nxcorr_threshold")
    args = [REF_EXE, str(inp), str(tmp_path / "out"), str(-1 if nxc is None else nxc),
            str(g("subpixel_step") or -1), str(-1 if g("min_variance") is None else g("min_variance")),
            str(0 if g("mode", 0) else 1), str(g("variant", 0)), str(g("max_lr_diff", 1)),
            str(int(g("no_dupes", False)))]
    r = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    rd, rc = oracle.match(L, R, oracle.OracleConfig(**cfg))
    d = np.fromfile(tmp_path / "out.ref.disp", dtype=rd.dtype).reshape(H, W)
    assert np.array_equal(d.view(np.uint8), rd.view(np.uint8))
    cpath = tmp_path / "out.ref.corr"
    if rc is None:
        assert not cpath.exists()
    else:
        c = np.fromfile(cpath, dtype=rc.dtype).reshape(H, W)
        assert np.array_equal(c.view(np.uint8), rc.view(np.uint8))
    assert ("type=%d" % (3 if rc is None else 5)) in r.stdout
