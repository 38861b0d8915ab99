"""The windowed search (search_range.hip, Engine.search(..., disparity_range=)) against the
unrestricted matrix-core search on the cfg2 shape: 2048 x 1536, n = 33 LIMITED descriptors
of the planted-disparity synthetic stack (disparities 16..63), NoDuplicates. The two are
warmed and then alternated in one process; each figure is the median over `--windows`
windows of `--reps` back-to-back launches between two device events. Also the whole match()
with and without the range (a ranged match cannot fuse the agree into the search, so its
frame gains less than its search) and the covering range (-2047, 2047), where the
absolute-key window kernel is expected to lose to the tuned full-row kernel.

  python tools/range_search_bench.py [--reps 10] [--windows 5] [--out profiles/range_search.jsonl]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from libbicos_amd import device  # noqa: E402
from libbicos_amd.synthetic import stereo_stack  # noqa: E402

H, W, N = 1536, 2048, 33
WORDS = 4
RANGE = (0, 127)
WIDE = (-(W - 1), W - 1)


def window(fn, reps):
    st = torch.cuda.current_stream()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(st)
    for _ in range(reps):
        fn()
    b.record(st)
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def alternate(fns, reps, windows):
    """{name: [ms per launch of each window]} with the candidates interleaved window by window"""
    for fn in fns.values():  # warm
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(windows):
        for k, fn in fns.items():
            ts[k].append(window(fn, reps))
    return ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    assert args.reps >= 10 and args.windows >= 3
    eng = device.Engine(0)
    L, R = stereo_stack(N, H, W, np.uint8)
    s0, s1 = torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()
    d0, d1 = eng.transform(s0, 0, WORDS), eng.transform(s1, 0, WORDS)
    bits = device.used_bits(N, 0)
    out = torch.empty((H, W), dtype=torch.int16, device="cuda")

    def search(rng):
        return lambda: eng.search(d0, d1, W, WORDS, 1, -1, out=out, bits=bits, disparity_range=rng)

    lines = []

    def report(what, ts, base, extra):
        med = {k: statistics.median(v) for k, v in ts.items()}
        for k in ts:
            line = {"bench": what, "rows": H, "cols": W, "n": N, "descriptor_bits": 32 * WORDS,
                    "case": k, "ms_median": round(med[k], 4), "ms_min": round(min(ts[k]), 4),
                    "ms_windows": [round(t, 4) for t in ts[k]], "reps_per_window": args.reps,
                    "speedup_vs_" + base: round(med[base] / med[k], 3)}
            line.update(extra.get(k, {}))
            print(json.dumps(line), flush=True)
            lines.append(line)

    full = eng.search(d0, d1, W, WORDS, 1, -1, bits=bits).cpu().numpy()
    extra = {"unrestricted": {"disparity_range": None,
                              "valid_fraction": round(float((full != -32768).mean()), 4)}}
    for name, rng in (("range_0_127", RANGE), ("range_covering", WIDE)):
        got = eng.search(d0, d1, W, WORDS, 1, -1, bits=bits, disparity_range=rng).cpu().numpy()
        extra[name] = {"disparity_range": list(rng),
                       "valid_fraction": round(float((got != -32768).mean()), 4),
                       "differs_from_unrestricted": round(float((got != full).mean()), 4)}
    ts = alternate({"unrestricted": search(None), "range_0_127": search(RANGE),
                    "range_covering": search(WIDE)}, args.reps, args.windows)
    report("search launch, NODUPES", ts, "unrestricted", extra)

    def match(rng):
        cfg = device.MatchConfig(nxcorr_threshold=0.9, disparity_range=rng)
        disp = torch.empty((H, W), dtype=torch.float32, device="cuda")
        corr = torch.empty((H, W), dtype=torch.float32, device="cuda")
        return lambda: eng.match(s0, s1, cfg, out=disp, corrmap=corr)

    ts = alternate({"unrestricted": match(None), "range_0_127": match(RANGE)}, args.reps,
                   args.windows)
    plan = eng.plan(s0, s1, device.MatchConfig(nxcorr_threshold=0.9))
    report("match(), NoDuplicates, threshold 0.9", ts, "unrestricted",
           {"unrestricted": {"plan": plan}})
    if args.out:
        with open(args.out, "a") as f:
            for l in lines:
                f.write(json.dumps(l) + "\n")


if __name__ == "__main__":
    main()
