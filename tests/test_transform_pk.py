"""The integer arithmetic of the packed LIMITED transform (libbicos_amd/csrc/transform_pk.hpp:
two pixels per 32-bit register as 16-bit fields), which transform_limited_pk_kernel runs on the
GPU. tests/cpp/transform_pk_check links nothing but that header and checks, with no GPU:

  compare     (0x7FFF7FFF - X) + Y has bit 15 / bit 31 set exactly where x < y in that field,
              for every x, y in 0..510 in one field and independent pairs in the other
  threshold   ceil_div is ceil(sum / n) for every n in 2..65 and every sum of n u8 samples, and
              a < ceil(sum / n) is the reference's float comparison a < sum / n
  split       a dword's bytes to packed samples
  descriptor  the two-pixel descriptor against a plain restatement of the reference's, for
              n = 2 3 4 5 9 12 17 24 33 40 48 65: random, constant, 0/255 alternating and
              neighbour pixels at opposite extremes (fields must not leak into each other)

The same program is built and run once more under the address and undefined-behaviour
sanitizers.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
SIZES = (2, 3, 4, 5, 9, 12, 17, 24, 33, 40, 48, 65)


def run_check(name):
    subprocess.run(["make", "-C", CPP, "-f", "transform_pk.mk", name], check=True,
                   capture_output=True)
    r = subprocess.run([os.path.join(CPP, name)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    return {what: int(count) for what, count in (l.split(" ok ") for l in r.stdout.splitlines())}


@pytest.mark.parametrize("name", ["transform_pk_check", "transform_pk_check_san"])
def test_packed_transform_arithmetic(name):
    lines = run_check(name)
    assert set(lines) == {"compare", "threshold", "split", "descriptor"}, lines
    assert lines["compare"] >= 2 * 511 * 511 * 8
    assert lines["threshold"] == sum(n * 255 + 1 for n in range(2, 66))
    assert lines["split"] == 4 * 256
    # per size: 4000 random + 512 constant + 2 alternating + 4 extremes, two pixels each
    assert lines["descriptor"] == len(SIZES) * 2 * (4000 + 512 + 2 + 4)


def test_check_program_covers_the_sizes_the_kernel_is_built_for():
    """The sizes transform_pk.hpp's built() names are among those the program instantiates."""
    import re
    hpp = open(os.path.join(ROOT, "libbicos_amd", "csrc", "transform_pk.hpp")).read()
    m = re.search(r"constexpr bool built\(int n\) \{\s*return ([^;]*);", hpp)
    assert m, "transform_pk.hpp no longer states its sizes in built()"
    built = {int(v) for v in re.findall(r"n == (\d+)", m.group(1))}
    assert built == {9, 12, 17, 24, 33, 40, 48, 65}
    src = open(os.path.join(CPP, "transform_pk_check.cpp")).read()
    checked = {int(v) for v in re.findall(r"check_descriptor<(\d+)>\(\);", src)}
    assert checked == set(SIZES) and built <= checked


def test_dispatch_query_sizes_alignment_and_cache_fit(blib):
    """bicos_transform_kernel (no HIP call, the pointers only inspected): the packed kernel
    takes aligned u8 LIMITED stacks of a built size at its narrowest descriptor that fit the
    256 MiB last-level cache together -- the benchmark's 2048 x 1536 frames of 33 and of 40
    images, not its 3840 x 2160 and 3208 x 2200 ones, which measured slower with it."""
    q = blib.bicos_transform_kernel
    a, b = 0x10000000, 0x30000000

    def kind(n=33, rows=1536, cols=2048, s0=a, s1=b, rp=None, pp=None, depth=1, mode=0, words=None):
        rp = cols if rp is None else rp
        pp = rows * rp if pp is None else pp
        words = words or blib.bicos_descriptor_words(n, mode)
        return q(s0, s1, n, rows, cols, rp, pp, depth, mode, words)

    assert kind() == 1 and kind(s1=None) == 1
    assert kind(n=40) == 1                               # 2 x 120 MiB
    assert kind(rows=2160, cols=3840) == 0               # 2 x 261 MiB
    assert kind(rows=2160, cols=3840, s1=None) == 0
    assert kind(rows=2200, cols=3208) == 0               # 2 x 222 MiB
    assert kind(rows=2200, cols=3208, s1=None) == 1
    assert [n for n in range(2, 66) if kind(n=n, rows=48, cols=64)] == [9, 12, 17, 24, 33, 40, 48, 65]
    for off in (1, 2, 3):
        assert kind(s0=a + off) == 0 and kind(s1=b + off) == 0
        assert kind(rp=2048 + off) == 0 and kind(pp=1536 * 2048 + off) == 0
    assert kind(s0=a + 4, s1=b + 8, rp=2052, pp=1536 * 2052 + 4) == 1
    assert kind(n=9, words=2) == 0 and kind(n=9, words=1) == 1
    assert kind(n=9, mode=1, words=2) == 0 and kind(depth=2) == 0
