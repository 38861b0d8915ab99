"""The speckle filter (libbicos_amd/csrc/speckle.hip) at the shapes users run: cfg2's
2048 x 1536 and the README frame's 3208 x 2200, int16 maps (a match without the NXC stage) and
float32 maps (with it: rejected pixels -32768.0, or NaN with the subpixel step), on two inputs:

  matched    the map of a real Engine.match() of the synthetic planted-disparity stacks
  one        every pixel valid and equal: one component over the whole frame, every link
             united, every tile adding its size to one address -- the atomic worst case

Timed with device events, each window `--reps` back-to-back calls after a warm-up, the
candidates alternated window by window in one process, `--repeats` (>= 3) windows each;
reported: the median and the spread of the windows. Next to each case:

  copy       a device-to-device copy (torch's Tensor.copy_ of a contiguous tensor) of the map:
             the algorithmic bytes of the filter, map read + map written
  match      that configuration's Engine.match() in the same session, for proportion

The filter itself moves more than its algorithmic bytes: the label and size arrays (8 B per
pixel) are written by the tile launch, the sizes read by the resolve launch and both read by
the apply launch.

  python tools/speckle_bench.py [--reps 100] [--repeats 3] [--out profiles/speckle.jsonl]
  rocprofv3 --kernel-trace --stats ... -- python tools/speckle_bench.py --trace   (per-kernel
      split: the filter alone, 50 calls per case at the README shape, no copies and no timing)
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

SHAPES = {
    "cfg2": dict(n=33, H=1536, W=2048,
                 cfg={"float32": dict(nxcorr_threshold=0.96), "int16": dict(nxcorr_threshold=None)}),
    "readme": dict(n=33, H=2200, W=3208,
                   cfg={"float32": dict(nxcorr_threshold=0.96, min_variance=2.0, subpixel_step=0.1),
                        "int16": dict(nxcorr_threshold=None)}),
}
MAX_SIZE, MAX_DIFF = 100, 1.0


def window(fn, reps):
    st = torch.cuda.current_stream()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(st)
    for _ in range(reps):
        fn()
    b.record(st)
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def alternate(fns, reps, repeats):
    for fn in fns.values():  # warm
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            ts[k].append(window(fn, reps[k]))
    return ts


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
    if args.trace:
        args.shapes = "readme"
    eng = device.Engine(0)
    tile = _lib.speckle_tile()
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
            one = torch.full_like(disp, 7)
            out = torch.empty_like(disp)
            cnt = torch.zeros((4,), dtype=torch.int32, device="cuda")
            copy_dst = torch.empty_like(disp)

            def call(src):
                return lambda: eng.filter_speckles(src, MAX_SIZE, MAX_DIFF, out=out, counts=cnt)

            inputs = {"matched": disp, "one": one}
            counts = {}
            for k, src in inputs.items():
                call(src)()
                torch.cuda.synchronize()
                counts[k] = [int(v) & 0xFFFFFFFF for v in cnt.cpu().tolist()]
                assert sum(counts[k][:3]) == H * W
            assert counts["one"] == [H * W, 0, 0, 0]
            if args.trace:
                for src in inputs.values():
                    for _ in range(50):
                        call(src)()
                torch.cuda.synchronize()
                continue
            fns = {"matched": call(disp), "one": call(one),
                   "copy": lambda: copy_dst.copy_(disp, non_blocking=True), "match": match}
            reps = {k: args.match_reps if k == "match" else args.reps for k in fns}
            ts = alternate(fns, reps, args.repeats)
            med = {k: statistics.median(v) for k, v in ts.items()}
            nbytes = 2 * H * W * disp.element_size()
            for k in inputs:
                line = {"bench": "speckle", "shape": name, "rows": H, "cols": W, "map": dtype,
                        "input": k, "max_size": MAX_SIZE, "max_diff": MAX_DIFF, "counts": counts[k],
                        "algorithmic_bytes": nbytes, "ms_median": round(med[k], 5),
                        "ms_windows": [round(t, 5) for t in ts[k]],
                        "spread": round((max(ts[k]) - min(ts[k])) / med[k], 4),
                        "algorithmic_GBps": round(nbytes / med[k] / 1e6, 1),
                        "copy_ms_median": round(med["copy"], 5),
                        "copy_ms_windows": [round(t, 5) for t in ts["copy"]],
                        "time_over_copy": round(med[k] / med["copy"], 2),
                        "match_ms_median": round(med["match"], 4),
                        "match_ms_windows": [round(t, 4) for t in ts["match"]],
                        "time_over_match": round(med[k] / med["match"], 4),
                        "one_over_matched": round(med["one"] / med["matched"], 3),
                        "reps_per_window": args.reps, "match_reps_per_window": args.match_reps,
                        "tile": list(tile)}
                print(json.dumps(line), flush=True)
                lines.append(line)
            del disp, one, out, copy_dst
        del tl, tr
    if args.out:
        with open(args.out, "a") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
