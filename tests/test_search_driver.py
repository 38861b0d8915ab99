"""The search stage has one driver (engine.cpp search_plan / run_search): the stage entries
bicos_search_device[_range] and the match run the same launches, and an entry needs an engine
only where the search needs workspace (two-pass Consistency).
"""
import numpy as np
import pytest

from libbicos_amd import _lib
from libbicos_amd.synthetic import stereo_stack


# ------------------------------------------------------------------ without a GPU
def test_consistency_search_needs_an_engine(blib):
    """NoDuplicates + Consistency is never the one-launch form: two maps of workspace"""
    rc = blib.bicos_search_device(None, None, None, 4, 64, 4, 3, 1, None, None)
    assert rc == _lib.BICOS_E_ARG
    assert "engine" in blib.bicos_last_error().decode()


def test_nodupes_search_accepts_a_null_engine(blib):
    """one search, no workspace: a NULL engine is no argument error. Without a GPU the launch
    itself fails (BICOS_E_HIP, not a word about the engine); with one the search runs, over
    real buffers."""
    import torch
    if not torch.cuda.is_available():
        rc = blib.bicos_search_device(None, None, None, 4, 64, 4, 1, 1, None, None)
        assert rc == _lib.BICOS_E_HIP, blib.bicos_last_error().decode()
        assert "engine" not in blib.bicos_last_error().decode()
        return
    desc = torch.zeros((4, blib.bicos_desc_pitch(64, 4)), dtype=torch.int32, device="cuda")
    desc[:, ::4] = torch.arange(64, device="cuda", dtype=torch.int32)[None, :]
    out = torch.empty((4, 64), dtype=torch.int16, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    rc = blib.bicos_search_device(None, desc.data_ptr(), desc.data_ptr(), 4, 64, 4, 1, 1,
                                  out.data_ptr(), st)
    torch.cuda.synchronize()
    assert rc == _lib.BICOS_OK, blib.bicos_last_error().decode()
    assert (out == 0).all()  # every descriptor is unique in its row and matches itself


# ------------------------------------------------------------------------ on the GPU
def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def same(a, b, what):
    a, b = a.cpu().numpy(), b.cpu().numpy()
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    ne = np.argwhere(a != b)
    assert not len(ne), "%s: %d of %d differ, first at %s" % (what, len(ne), a.size, ne[:4].tolist())


# flags, max_lr_diff -> the match configuration that runs that search
FLAGS = {(1, -1): dict(variant=0), (2, 1): dict(variant=1, max_lr_diff=1),
         (3, 2): dict(variant=1, max_lr_diff=2, no_dupes=True)}
RANGE = (-8, 40)


_FRAMES = {}


def frame(gpu, n):
    """40 x 300 stacks on the device and their descriptors (Engine.transform), made once"""
    if n not in _FRAMES:
        L, R = stereo_stack(n, 40, 300, seed=100 + n)
        s0, s1 = dev(L), dev(R)
        _FRAMES[n] = (s0, s1, gpu.transform(s0), gpu.transform(s1))
    return _FRAMES[n]


# n = 12: 64-bit descriptors, packed keys; 33: 128-bit; 36: 256-bit with 138 written bits,
# Consistency without NoDuplicates in one launch
@pytest.mark.gpu
@pytest.mark.parametrize("rng", [None, RANGE], ids=["full_row", "range"])
@pytest.mark.parametrize("flags,lr", list(FLAGS), ids=["nodupes", "cons", "nodupes_cons"])
@pytest.mark.parametrize("n", [12, 33, 36])
def test_search_entry_is_the_match(gpu, monkeypatch, n, flags, lr, rng):
    from libbicos_amd import device
    monkeypatch.delenv("BICOS_LR_ONE_PASS", raising=False)
    s0, s1, d0, d1 = frame(gpu, n)
    words = device.descriptor_words(n)
    assert words == {12: 2, 33: 4, 36: 8}[n]
    cfg = device.MatchConfig(nxcorr_threshold=None, disparity_range=rng, **FLAGS[(flags, lr)])
    plan = gpu.plan(s0, s1, cfg)  # (of the full-row match)
    if n == 12 and flags == 1:
        assert plan & _lib.PLAN_PACKED_KEYS
    assert bool(plan & _lib.PLAN_CONSISTENCY_ONE_PASS) == (n == 36 and flags == 2)
    want, _ = gpu.match(s0, s1, cfg)
    got = gpu.search(d0, d1, 300, words, flags, lr, bits=device.used_bits(n), disparity_range=rng)
    same(got, want, "search entry against match")
    if n == 36 and flags == 2 and rng is None:
        monkeypatch.setenv("BICOS_LR_ONE_PASS", "0")
        assert not gpu.plan(s0, s1, cfg) & _lib.PLAN_CONSISTENCY_ONE_PASS
        two = gpu.search(d0, d1, 300, words, flags, lr, bits=device.used_bits(n))
        same(two, want, "two-pass search entry against the one-launch match")
        same(gpu.match(s0, s1, cfg)[0], want, "two-pass match against the one-launch match")
