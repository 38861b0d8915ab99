"""bicos_match_plan against tests/golden/plan_table.json (tests/golden/make_plan_table.py):
the host orchestration plans every row of the table as the commit that wrote the file did.
"""
import json

import pytest

from tests.golden import make_plan_table as T


@pytest.fixture(scope="module")
def golden():
    with open(T.PATH) as f:
        db = json.load(f)
    axes = {k: [list(v) if isinstance(v, tuple) else v for v in vs] for k, vs in T.AXES.items()}
    assert db["axes"] == axes and db["extra"] == [list(e) for e in T.EXTRA], \
        "plan_table.json was written for another table: run tests/golden/make_plan_table.py"
    return db["plans"]


def compare(got, want):
    assert len(got) == len(want)
    bad = [(i, case) for i, case in enumerate(T.cases()) if got[i] != want[i]]
    assert not bad, "%d of %d rows differ, first: %r planned 0x%x, the table has 0x%x" % (
        len(bad), len(want), bad[0][1], got[bad[0][0]] & 0xFFFFFFFF, want[bad[0][0]] & 0xFFFFFFFF)


def test_plan_table_null_engine(blib, golden, monkeypatch):
    for name in ("BICOS_SEARCH", "BICOS_FUSE_AGREE", "BICOS_FUSE_CONS", "BICOS_REV_FULL",
                 "BICOS_DENSE_ROWS", "BICOS_LR_ONE_PASS"):
        monkeypatch.delenv(name, raising=False)
    compare(T.table(blib), golden)


def test_plan_table_spot_values(blib, golden):
    """the table holds what the header documents: packed keys and the fused agree at cfg1's
    shape, one-pass Consistency at n = 40, BICOS_E_BITS past 256 bits, BICOS_E_ARG for n = 1"""
    rows = dict(zip(((c[0], c[1], c[2], c[3], c[4], c[5], c[6], c[7]) for c in T.cases()), golden))
    nodup, cons = (0.9, -1.0, -1.0, 0, 0, 0, 1, 0), (0.9, -1.0, -1.0, 0, 0, 1, 1, 0)
    assert rows[(8, 480, 640, 640, 1, 0, nodup, 1)] == 0x7
    assert rows[(33, 480, 2048, 2048, 1, 0, nodup, 1)] == 0x5
    assert rows[(40, 480, 2048, 2048, 1, 0, cons, 1)] == 0x41
    assert rows[(33, 480, 2048, 2048, 1, 0, cons, 1)] == 0x39
    assert rows[(17, 480, 640, 640, 1, 0, (0.9, -1.0, -1.0, 1, 0, 0, 1, 0), 1)] == -2
    assert golden[-4] == -1 and golden[-3] == -1


@pytest.mark.gpu
def test_plan_table_real_engine(gpu, golden):
    """a real, untuned engine plans as the NULL engine does (256 compute units)"""
    compare(T.table(gpu._L, gpu._h), golden)
