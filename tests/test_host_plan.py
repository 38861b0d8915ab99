"""The arithmetic of the banded host-buffer pipeline (libbicos_amd/csrc/host_plan.hpp: the
band plan, the upload split over two copy streams, the delivery's chunks), which host.cpp's
match_host calls for every copy it issues. tests/cpp/host_plan_check links nothing but that
header and checks, with no GPU:

  bands     rows 1 .. 20000: the bands tile [0, rows) once and in order, 1 <= height <=
            band_rows, B <= 8, K <= 3, K = 1 iff B = 1
  split     up 0 .. 70000 and sizes up to 2^33, 1 and 2 streams: first <= up, [0, first) and
            [first, up) tile [0, up), first == up with one stream, a multiple of 4096 or up
            with two, first > 0 where up > 0
  delivery  bytes 0 .. 20000 and sizes up to 2^36: the 8 parts tile [0, bytes)
  layout    a table of frames (every frame of tests/test_host_small_gpu.py among them) x
            int16 / float disparity x float / double corrmap x 1 / 2 streams: every upload
            copy of band b inside the band's own bytes on the device and in its pinned slot,
            every download and delivered chunk inside its map

The split is what was wrong: match_host took the middle of a band rounded up to 4096 bytes
as its first copy, which for a band of under 4096 bytes is 4096 -- more than the band, read
past its pinned slot and written over what follows the band in the stage (the next bands, the
finished disparity rows of band 0). `host_plan_check parent` runs the same split properties on
that one expression: they must fail for exactly 0 < up < 4096 with two streams (up = 1 by
`first > 0`: the expression gives 0 there, and all of the band to the second stream), and
nowhere with one. The delivery was wrong too: a band whose bytes of a map were 512 k + r,
0 < r < 8, had its last r bytes in no chunk (the share was rounded down before it was rounded
up to 64); found by this check, fixed in deliver_part.
"""
import os
import re
import subprocess

import pytest

from tests.host_small_cases import every_frame

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "host_plan_check")
ENGINE_HPP = os.path.join(ROOT, "libbicos_amd", "csrc", "engine.hpp")


@pytest.fixture(scope="module")
def check():
    subprocess.run(["make", "-C", os.path.dirname(EXE), "host_plan_check"], check=True,
                   capture_output=True)
    return EXE


def stage_alignment():
    m = re.search(r"constexpr size_t ALIGN = (\d+);", open(ENGINE_HPP).read())
    assert m, "engine.hpp no longer states the stage's alignment as ALIGN"
    return int(m.group(1))


def test_pipeline_arithmetic_holds_everywhere(check):
    r = subprocess.run([check, str(stage_alignment())], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    lines = dict(l.split(" ok ") for l in r.stdout.splitlines())
    assert set(lines) == {"bands", "split", "delivery", "layout"}, r.stdout
    assert int(lines["bands"]) == 20000
    assert int(lines["split"]) >= 2 * 70001 + 2 * 8
    assert int(lines["delivery"]) >= 20001 + 4
    assert int(lines["layout"]) >= 6 * len(every_frame())


def test_layout_table_covers_the_gpu_tests_frames(check):
    r = subprocess.run([check, "frames"], capture_output=True, text=True, check=True)
    table = {tuple(int(v) for v in l.split()) for l in r.stdout.splitlines()}
    missing = [f for f in every_frame() if f not in table]
    assert not missing, "frames run on the GPU but not checked on the CPU: %s" % missing


def test_split_properties_reject_the_unclamped_middle(check):
    """Sensitivity: on the expression match_host used to compute, the split properties fail
    for exactly the bands of under 4096 bytes with two streams."""
    r = subprocess.run([check, "parent"], capture_output=True, text=True, check=True)
    assert r.stdout.splitlines()[:2] == ["split streams=1 violations none",
                                         "split streams=2 violations 1..4095"]


def test_delivery_tiling_rejects_the_share_rounded_down(check):
    """... and on the chunk deliver_band used to compute, the tiling fails for exactly the
    bytes = 512 k + r, 0 < r < 8, of 0 .. 20000: 40 values of k, 7 of r."""
    r = subprocess.run([check, "parent"], capture_output=True, text=True, check=True)
    assert r.stdout.splitlines()[2:] == ["delivery violations 280, 0 not of the form 512 k + 1..7"]
