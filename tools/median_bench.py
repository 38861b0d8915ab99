"""The median filter (libbicos_amd/csrc/median.hip) at the shapes users run: cfg2's 2048 x 1536
and the README frame's 3208 x 2200, int16 maps (a match without the NXC stage) and float32 maps
(with it: rejected pixels -32768.0, or NaN with the subpixel step) -- the map of a real
Engine.match() of the synthetic planted-disparity stacks -- for ksize 3 and 5, without filling
and with fill_min = ksize^2 / 2 + 1.

Timed with device events, each window `--reps` back-to-back calls after a warm-up, the
candidates alternated window by window in one process, `--repeats` (>= 3) windows each;
reported: the median and the spread of the windows. Next to each case:

  copy       a device-to-device copy (torch's Tensor.copy_ of a contiguous tensor) of the map:
             the algorithmic bytes of the filter, map read + map written. These maps fit the
             Infinity Cache, so it is a warm figure, not an HBM rate.
  speckle    Engine.filter_speckles at that shape
  match      that configuration's Engine.match() in the same session, for proportion

Before anything is timed one call per aperture is compared bit for bit with the restatement
of tests/median_ref.py at a small shape. Without a GPU the tool fails.

  python tools/median_bench.py [--reps 100] [--repeats 3] [--out profiles/median.jsonl]
  rocprofv3 --kernel-trace --stats ... -- python tools/median_bench.py --trace   (kernel time:
      the filter alone, 50 calls per case at the README shape, no copies and no timing)
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from libbicos_amd import _lib, device  # noqa: E402
from libbicos_amd.synthetic import stereo_stack  # noqa: E402
from tests import median_ref  # noqa: E402
from tools.speckle_bench import SHAPES, alternate  # noqa: E402


def self_check(eng):
    tr, tc = _lib.median_tile()
    for dtype in (np.int16, np.float32):
        name, d, sentinel = [p for p in median_ref.patterns(tr + 5, tc + 7, dtype)
                             if p[0].startswith("holes")][0]
        for ksize in (3, 5):
            fill_min = ksize * ksize // 2 + 1
            want = median_ref.restate(d, ksize, fill_min, sentinel)
            cnt = torch.zeros((4,), dtype=torch.int32, device="cuda")
            out = eng.median_filter(torch.from_numpy(d).cuda(), ksize, fill_min, sentinel=sentinel,
                                    counts=cnt)
            got = out.cpu().numpy()
            assert np.array_equal(median_ref.bits(got), median_ref.bits(want["out"])), (name, ksize)
            assert cnt.cpu().numpy().view(np.uint32).tolist() == want["counts"].tolist()
            assert want["counts"][1] and want["counts"][2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--match-reps", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--shapes", default="cfg2,readme")
    ap.add_argument("--dtypes", default="int16,float32")
    ap.add_argument("--trace", action="store_true",
                    help="for a profiler: the README shape, 50 filter calls per case, nothing else")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    assert args.reps >= 50 and args.repeats >= 3
    if not torch.cuda.is_available():
        sys.exit("median_bench: no GPU")
    if args.trace:
        args.shapes = "readme"
    eng = device.Engine(0)
    self_check(eng)
    tile = _lib.median_tile()
    lines = []
    for name in args.shapes.split(","):
        sh = SHAPES[name]
        H, W = sh["H"], sh["W"]
        l, r = stereo_stack(sh["n"], H, W, np.uint8)
        tl, tr = torch.from_numpy(l).cuda(), torch.from_numpy(r).cuda()
        del l, r
        for dtype in args.dtypes.split(","):
            cfg = device.MatchConfig(**sh["cfg"][dtype])

            def match():
                return eng.match(tl, tr, cfg, want_corrmap=False)

            disp, _ = match()
            assert str(disp.dtype) == "torch." + dtype
            out = torch.empty_like(disp)
            speckle_out = torch.empty_like(disp)
            cnt = torch.zeros((4,), dtype=torch.int32, device="cuda")
            copy_dst = torch.empty_like(disp)

            def call(ksize, fill_min):
                return lambda: eng.median_filter(disp, ksize, fill_min, out=out, counts=cnt)

            params = [(k, f) for k in (3, 5) for f in (0, k * k // 2 + 1)]
            counts = {}
            for p in params:
                call(*p)()
                torch.cuda.synchronize()
                counts[p] = [int(v) & 0xFFFFFFFF for v in cnt.cpu().tolist()]
                assert sum(counts[p]) == H * W
            if args.trace:
                for p in params:
                    for _ in range(50):
                        call(*p)()
                torch.cuda.synchronize()
                continue
            fns = {p: call(*p) for p in params}
            fns["copy"] = lambda: copy_dst.copy_(disp, non_blocking=True)
            fns["speckle"] = lambda: eng.filter_speckles(disp, 100, 1.0, out=speckle_out)
            fns["match"] = match
            reps = {k: args.match_reps if k == "match" else args.reps for k in fns}
            ts = alternate(fns, reps, args.repeats)
            med = {k: statistics.median(v) for k, v in ts.items()}
            nbytes = 2 * H * W * disp.element_size()
            for p in params:
                line = {"bench": "median", "shape": name, "rows": H, "cols": W, "map": dtype,
                        "ksize": p[0], "fill_min": p[1], "counts": counts[p],
                        "algorithmic_bytes": nbytes, "ms_median": round(med[p], 5),
                        "ms_windows": [round(t, 5) for t in ts[p]],
                        "spread": round((max(ts[p]) - min(ts[p])) / med[p], 4),
                        "algorithmic_GBps": round(nbytes / med[p] / 1e6, 1),
                        "copy_ms_median": round(med["copy"], 5),
                        "copy_ms_windows": [round(t, 5) for t in ts["copy"]],
                        "time_over_copy": round(med[p] / med["copy"], 2),
                        "speckle_ms_median": round(med["speckle"], 5),
                        "time_over_speckle": round(med[p] / med["speckle"], 3),
                        "match_ms_median": round(med["match"], 4),
                        "match_ms_windows": [round(t, 4) for t in ts["match"]],
                        "time_over_match": round(med[p] / med["match"], 4),
                        "reps_per_window": args.reps, "match_reps_per_window": args.match_reps,
                        "tile": list(tile)}
                print(json.dumps(line), flush=True)
                lines.append(line)
            del disp, out, copy_dst, speckle_out
        del tl, tr
    if args.out:
        with open(args.out, "a") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
