"""Generate tests/golden/ref_frames.json -- results recorded from the reference's own CPU code.

Every hash in the file comes from oracle/_ref/libbicos_ref.so alone: the reference's
src/impl/cpu.cpp and include/impl/cpu/*.hpp compiled unchanged (oracle/Makefile, target `ref`;
oracle/reference.py). The C oracle is not involved. The GPU machine has no reference tree, so
tests/test_reference_parity.py::test_gpu_reproduces_reference reads only this file: it
regenerates the inputs, runs Engine.match and compares hashes, with no restatement in between.

Cases: the smallest shapes at which the engine's plans differ, ROWS rows each.
  descriptor widths / K-steps   LIMITED n = 8 (1 word), 17 (2), 33 (4), 40 (8 words, 153 bits,
                                3 K-steps, eligible for the one-launch Consistency search),
                                65 (253 bits, 4 K-steps); FULL n = 6, 8, 12, 16
  input types                   u8 for all; u16 for LIMITED n = 17 (full range) and 33 (12 bit)
  widths                        333 (several 32-column tiles and a ragged end), 1100 (tail
                                workgroups), 2049 (just past the float-key / one-pass limit 2048)
  configs                       CONFIGS below

For each case the file holds the generator parameters and the sha256 of both input stacks; for
each case and config the sha256 of the disparity map and the corrmap exactly as match() returns
them (int16 without NXC, float32 otherwise; raw bytes, NaN payloads included) and the first 16
hex digits of the sha256 of each row of both, so a mismatch names its rows.

  python tests/golden/make_ref_frames.py          (needs the reference tree; about 20 s)
"""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from libbicos_amd.synthetic import SEED, _uniform, stereo_stack  # noqa: E402

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "ref_frames.json")
ROWS = 4
WIDTHS = (333, 1100, 2049)

# the eight match configurations of the reference parity tests (fields of BICOS::Config)
CONFIGS = {
    "plain": dict(nxcorr_threshold=None),
    "nxc": dict(nxcorr_threshold=0.9),
    "nxc_minvar": dict(nxcorr_threshold=0.8, min_variance=2.0),
    "subpix": dict(nxcorr_threshold=0.5, subpixel_step=0.1),
    "subpix_minvar": dict(nxcorr_threshold=0.5, subpixel_step=0.3, min_variance=2.0),
    "cons_lr1": dict(nxcorr_threshold=None, variant=1, max_lr_diff=1),
    "cons_lr0_nd": dict(nxcorr_threshold=0.9, variant=1, max_lr_diff=0, no_dupes=True),
    "cons_lr3_subpix": dict(nxcorr_threshold=0.5, variant=1, max_lr_diff=3, subpixel_step=0.25),
}

# (n, mode, dtype, maxval)
STACKS = [(n, 0, "u8", 255) for n in (8, 17, 33, 40, 65)] \
    + [(n, 1, "u8", 255) for n in (6, 8, 12, 16)] \
    + [(17, 0, "u16", 65535), (33, 0, "u16", 4095)]

CASES = {
    "%s_n%d_%s_w%d" % ("full" if mode else "lim", n, dt, W):
        dict(n=n, mode=mode, dtype=dt, maxval=maxval, H=ROWS, W=W)
    for (n, mode, dt, maxval) in STACKS for W in WIDTHS
}


def case_stacks(case):
    """The synthetic stacks of a case: planted disparities 16 .. 52 over the rows. The last
    row is a still scene moved 16 columns: every image shows the same grey values + U{0..3}
    of noise, so a pixel's variance is about 1.25 n -- above min_variance 2.0, mostly below
    2.0 n, which is what the min-variance configs must compare it with."""
    dt = np.uint16 if case["dtype"] == "u16" else np.uint8
    n, W = case["n"], case["W"]
    L, R = stereo_stack(n, case["H"], W, dt, maxval=case["maxval"])
    scene = _uniform(np.arange(W + 16, dtype=np.int64), SEED ^ 0x57111, case["maxval"] - 3)
    noise = _uniform(np.arange(2 * n * W, dtype=np.int64), SEED ^ 0x2015E, 3).reshape(2, n, W)
    L[:, -1] = scene[None, :W] + noise[0]
    R[:, -1] = scene[None, 16:] + noise[1]
    return L, R


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def row_hashes(a):
    return [sha(a[y])[:16] for y in range(a.shape[0])]


def result_record(d, c):
    """What is stored of one match() result (disparity d, corrmap c or None)."""
    return {
        "disparity_dtype": str(d.dtype),
        "disparity_sha256": sha(d),
        "disparity_rows": row_hashes(d),
        "corrmap_sha256": None if c is None else sha(c),
        "corrmap_rows": None if c is None else row_hashes(c),
    }


def generate(match, make_config):
    """The whole fixture from a match(stack0, stack1, config) -> (disparity, corrmap)."""
    db = {"configs": CONFIGS, "cases": {}}
    for name, case in CASES.items():
        L, R = case_stacks(case)
        rec = dict(case, inputs_sha256=[sha(L), sha(R)], results={})
        for cname, cfg in CONFIGS.items():
            d, c = match(L, R, make_config(mode=case["mode"], **cfg))
            rec["results"][cname] = result_record(d, c)
        db["cases"][name] = rec
    return db


def main():
    from oracle import reference as ref
    ref.build()
    db = generate(ref.match, ref.ReferenceConfig)
    with open(PATH, "w") as f:
        json.dump(db, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", PATH, len(db["cases"]), "cases x", len(CONFIGS), "configs")


if __name__ == "__main__":
    main()
