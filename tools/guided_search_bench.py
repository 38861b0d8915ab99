"""The guided search (search_guided.hip, Engine.search(..., guide=)) on the cfg2 shape: 2048 x
1536, n = 33 LIMITED descriptors of the planted-disparity synthetic stack, NoDuplicates. The
method is tools/range_search_bench.py's: the candidates are warmed and then alternated in one
process; each figure is the median over `--windows` windows of `--reps` back-to-back launches
between two device events.

  (a) the unrestricted search
  (b) disparity_range = the bounding window of the guide: the windowed kernel
      (search_range.hip), which this feature does not touch
  (c) the guided search with the constant guide of (b): the price of per-lane windows
  (d) the guided search with the guide built from the unguided match's map, at radius 8 /
      spread 2 and at radius 2 / spread 1, under the global window of (b)
  (e) the builder launch, beside a device copy of the bytes it reads and writes
  (f) the whole match(): unrestricted, ranged (b), guided (d)

  python tools/guided_search_bench.py [--reps 20] [--windows 5] [--out profiles/guided_search.jsonl]
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
from tools.range_search_bench import alternate  # noqa: E402

H, W, N = 1536, 2048, 33
WORDS = 4
GUIDES = {"r8_s2": (8, 2), "r2_s1": (2, 1)}  # name -> (radius, spread)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--rows", type=int, default=H, help="(a smaller frame for a dry run)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    assert args.reps >= 10 and args.windows >= 3
    rows = args.rows
    eng = device.Engine(0)
    L, R = stereo_stack(N, rows, W, np.uint8)
    s0, s1 = torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()
    d0, d1 = eng.transform(s0, 0, WORDS), eng.transform(s1, 0, WORDS)
    bits = device.used_bits(N, 0)
    out = torch.empty((rows, W), dtype=torch.int16, device="cuda")
    lines = []

    def report(what, ts, base, extra):
        med = {k: statistics.median(v) for k, v in ts.items()}
        for k in ts:
            line = {"bench": what, "rows": rows, "cols": W, "n": N, "descriptor_bits": 32 * WORDS,
                    "case": k, "ms_median": round(med[k], 4), "ms_min": round(min(ts[k]), 4),
                    "ms_max": round(max(ts[k]), 4),
                    "ms_windows": [round(t, 4) for t in ts[k]], "reps_per_window": args.reps,
                    "speedup_vs_" + base: round(med[base] / med[k], 3)}
            line.update(extra.get(k, {}))
            print(json.dumps(line), flush=True)
            lines.append(line)

    # the prior: the unguided match's own map; the guides; their bounding window
    cfg0 = device.MatchConfig(nxcorr_threshold=0.9)
    prior, _ = eng.match(s0, s1, cfg0)
    guides, extra = {}, {}
    lo, hi = 32767, -32768
    for name, (radius, spread) in GUIDES.items():
        counts = torch.zeros((2,), dtype=torch.int32, device="cuda")
        g = eng.guide_from_disparity(prior, radius, spread=spread, fallback=(1, 0), counts=counts)
        guides[name] = g
        has = g[..., 0] <= g[..., 1]
        lo = min(lo, int(g[..., 0][has].min()))
        hi = max(hi, int(g[..., 1][has].max()))
        width = (g[..., 1] - g[..., 0] + 1)[has].float()
        extra["guided_" + name] = {"radius": radius, "spread": spread,
                                   "from_prior": int(counts[0]), "fallback_empty": int(counts[1]),
                                   "window_mean": round(float(width.mean()), 2),
                                   "window_max": int(width.max())}
    bound = (lo, hi)
    const = torch.empty((rows, W, 2), dtype=torch.int16, device="cuda")
    const[..., 0], const[..., 1] = lo, hi

    def search(rng=None, guide=None):
        return lambda: eng.search(d0, d1, W, WORDS, 1, -1, out=out, bits=bits,
                                  disparity_range=rng, guide=guide)

    fns = {"unrestricted": search(), "range_bounding": search(bound),
           "guided_constant": search(bound, const)}
    for name, g in guides.items():
        fns["guided_" + name] = search(bound, g)
    full = eng.search(d0, d1, W, WORDS, 1, -1, bits=bits).cpu().numpy()
    for k, fn in fns.items():
        got = fn().cpu().numpy()
        e = extra.setdefault(k, {})
        e["disparity_range"] = None if k == "unrestricted" else list(bound)
        e["valid_fraction"] = round(float((got != -32768).mean()), 4)
        e["differs_from_unrestricted"] = round(float((got != full).mean()), 4)
    ranged = fns["range_bounding"]().cpu().numpy()
    assert np.array_equal(fns["guided_constant"]().cpu().numpy(), ranged)
    ts = alternate(fns, args.reps, args.windows)
    report("search launch, NODUPES", ts, "range_bounding", extra)

    # (e) the builder, beside a copy of as many bytes as it reads and writes
    radius, spread = GUIDES["r8_s2"]
    gout = torch.empty((rows, W, 2), dtype=torch.int16, device="cuda")
    nbytes = prior.numel() * prior.element_size() + gout.numel() * 2
    src = torch.empty((nbytes // 2,), dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    ts = alternate({"copy_same_bytes": lambda: dst.copy_(src),
                    "guide_builder_r8_s2": lambda: eng.guide_from_disparity(
                        prior, radius, spread=spread, fallback=(1, 0), out=gout),
                    "guide_builder_r2_s1": lambda: eng.guide_from_disparity(
                        prior, 2, spread=1, fallback=(1, 0), out=gout)},
                   args.reps, args.windows)
    report("guide builder launch", ts, "copy_same_bytes",
           {k: {"bytes_read_and_written": nbytes} for k in ts})

    # (f) the whole match
    def match(rng=None, guide=None):
        cfg = device.MatchConfig(nxcorr_threshold=0.9, disparity_range=rng)
        disp = torch.empty((rows, W), dtype=torch.float32, device="cuda")
        corr = torch.empty((rows, W), dtype=torch.float32, device="cuda")
        return lambda: eng.match(s0, s1, cfg, out=disp, corrmap=corr, guide=guide)

    fns = {"unrestricted": match(), "range_bounding": match(bound)}
    for name, g in guides.items():
        fns["guided_" + name] = match(bound, g)
    ts = alternate(fns, args.reps, args.windows)
    report("match(), NoDuplicates, threshold 0.9", ts, "range_bounding",
           {"unrestricted": {"plan": eng.plan(s0, s1, cfg0)},
            "range_bounding": {"disparity_range": list(bound)}})
    if args.out:
        with open(args.out, "a") as f:
            for l in lines:
                f.write(json.dumps(l) + "\n")


if __name__ == "__main__":
    main()
