"""Stack pooling (libbicos_amd/csrc/pool.hip) and the pyramid match at the shapes users run. The
method is tools/range_search_bench.py's: the candidates are warmed and then alternated in one
process; each figure is the median over `--windows` windows of `--reps` back-to-back calls
between two device events, with the windows' minimum and maximum beside it.

Pooling: cfg2's 2048 x 1536 and the README frame's 3208 x 2200, one stack of n = 33 images, u8 and
u16, scale 2 and 4.
  pool       bicos_pool_device of one stack: one launch; reads the stack once, writes 1 / s^2 of it
  pool_per_element  the same stack pooled from a view that starts one element later, which the
             per-element kernel serves: what a source that is not dword-aligned costs, and what
             a dense output that is not (the README frame's 802 u8 columns at scale 4) would
             cost if the output's alignment chose the kernel too
  copy       a device-to-device copy of the source stack (Tensor.copy_): reads it once, writes it
             once -- 2 x the source bytes against pooling's 1 + 1 / s^2
  transform  bicos_transform_device of the same stack, for scale

The pyramid: the planted cfg2 scene (disparities 16 .. 63), n = 33 u8, NoDuplicates, NXC threshold
0.9, under the wide global window disparity_range = (0, 511), and again under (-2047, 2047),
which at 2048 columns bounds nothing.
  ranged        Engine.match over that window
  pyramid_s2    Engine.match_pyramid, scale 2, radius 2, spread 1
  pyramid_s4    ... scale 4
  four_calls_s2 / _s4  the four public calls the pyramid is defined as (pool x 2, ranged coarse
                match, guide, guided match), output buffers allocated once
  pyramid_s2_second_record / _s4_  the one call with BICOS_PYRAMID_SINGLE_RECORD=0: its own
                lease records the workspace event once more at the end (engine.cpp
                match_pyramid_device)
and, per pyramid, the share of pixels whose disparity differs from the ranged match's and the
share invalid in each.

Pooling launches take tens of microseconds, so their windows hold `--pool-reps` (1000) of them.

  python tools/pool_bench.py [--reps 20] [--pool-reps 1000] [--windows 5] [--out profiles/pool.jsonl]
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
from tools.range_search_bench import alternate  # noqa: E402

SHAPES = {"cfg2": (1536, 2048), "readme": (2200, 3208)}
N = 33
WINDOWS = ((0, 511), (-2047, 2047))  # the issue's wide window; no bound at all at this width


def stats(ts):
    return {"ms_median": round(statistics.median(ts), 5), "ms_min": round(min(ts), 5),
            "ms_max": round(max(ts), 5), "ms_windows": [round(t, 5) for t in ts],
            "windows_spread": round((max(ts) - min(ts)) / statistics.median(ts), 4)}


def pool_ref(a, s):
    """include/bicos_c.h "stack pooling" in numpy, for the check of what is timed"""
    n, rows, cols = a.shape
    pr, pc = rows // s, cols // s
    total = a[:, :pr * s, :pc * s].astype(np.uint32).reshape(n, pr, s, pc, s).sum(axis=(2, 4))
    return ((total + s * s // 2) // (s * s)).astype(a.dtype)


def pool_lines(eng, args, emit):
    for name in args.shapes.split(","):
        H, W = SHAPES[name]
        H = min(H, args.rows) if args.rows else H
        for dt, depth in ((torch.uint8, 1), (torch.int16, 2)):
            g = torch.Generator(device="cuda").manual_seed(7)
            src = torch.randint(0, 256, (N, H, W * depth), dtype=torch.uint8, device="cuda",
                                generator=g).view(dt).view(N, H, W)
            dst = torch.empty_like(src)
            flat = torch.empty((src.numel() + 4,), dtype=dt, device="cuda")
            odd = flat[1:1 + src.numel()].view(N, H, W)  # one element past a dword boundary
            odd.copy_(src)
            words = device.descriptor_words(N, 0)
            desc = eng.transform(src, 0, words)
            for scale in (2, 4):
                out = torch.empty((N, H // scale, W // scale), dtype=dt, device="cuda")
                # what is timed is also right: two planes against the numpy restatement
                eng.pool(src[:2], scale, out=out[:2])
                np_dt = np.uint8 if depth == 1 else np.uint16
                assert np.array_equal(out[:2].cpu().numpy().view(np_dt),
                                      pool_ref(src[:2].cpu().numpy().view(np_dt), scale))
                assert eng.pool_kernel(odd, out) & 1 == 0
                eng.pool(odd[:2], scale, out=out[:2])
                assert np.array_equal(out[:2].cpu().numpy().view(np_dt),
                                      pool_ref(src[:2].cpu().numpy().view(np_dt), scale))
                fns = {"pool": lambda: eng.pool(src, scale, out=out),
                       "pool_per_element": lambda: eng.pool(odd, scale, out=out),
                       "copy": lambda: dst.copy_(src, non_blocking=True),
                       "transform": lambda: eng.transform(src, 0, words, out=desc)}
                ts = alternate(fns, args.pool_reps, args.windows)
                src_bytes = src.numel() * depth
                line = {"bench": "pool", "shape": name, "rows": H, "cols": W, "n": N,
                        "depth": depth, "scale": scale, "tile": list(_lib.pool_tile()),
                        "kernel_bits": eng.pool_kernel(src, out), "warm": True,
                        "source_bytes": src_bytes,
                        "pool_bytes": src_bytes + out.numel() * depth, "copy_bytes": 2 * src_bytes,
                        "reps_per_window": args.pool_reps}
                for k in fns:
                    line[k] = stats(ts[k])
                med = {k: line[k]["ms_median"] for k in fns}
                line["pool_GBps"] = round(line["pool_bytes"] / med["pool"] / 1e6, 1)
                line["copy_GBps"] = round(line["copy_bytes"] / med["copy"] / 1e6, 1)
                line["pool_time_over_copy"] = round(med["pool"] / med["copy"], 3)
                line["per_element_time_over_copy"] = round(med["pool_per_element"] / med["copy"], 3)
                line["pool_time_over_transform"] = round(med["pool"] / med["transform"], 3)
                emit(line)
                del out
            del src, dst, desc, flat, odd


def pyramid_lines(eng, args, emit):
    H, W = SHAPES["cfg2"]
    H = min(H, args.rows) if args.rows else H
    L, R = stereo_stack(N, H, W, np.uint8)
    s0, s1 = torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()
    del L, R
    for window in WINDOWS:
        pyramid_window_lines(eng, args, emit, s0, s1, H, W, window)


def pyramid_window_lines(eng, args, emit, s0, s1, H, W, WINDOW):
    kw = dict(nxcorr_threshold=0.9)
    cfg = device.MatchConfig(disparity_range=WINDOW, **kw)
    disp = torch.empty((H, W), dtype=torch.float32, device="cuda")
    corr = torch.empty((H, W), dtype=torch.float32, device="cuda")
    radius, spread = 2, 1

    def four_calls(scale):
        ph, pw = H // scale, W // scale
        p0 = torch.empty((N, ph, pw), dtype=torch.uint8, device="cuda")
        p1 = torch.empty_like(p0)
        coarse = torch.empty((ph, pw), dtype=torch.float32, device="cuda")
        guide = torch.empty((H, W, 2), dtype=torch.int16, device="cuda")
        ccfg = device.MatchConfig(disparity_range=_lib.pyramid_window(WINDOW, scale), **kw)

        def run():
            eng.pool(s0, scale, out=p0)
            eng.pool(s1, scale, out=p1)
            eng.match(p0, p1, ccfg, want_corrmap=False, out=coarse)
            eng.guide_from_disparity(coarse, radius, spread, scale, WINDOW, shape=(H, W), out=guide)
            return eng.match(s0, s1, cfg, out=disp, corrmap=corr, guide=guide)
        return run

    def pyramid(scale):
        return lambda: eng.match_pyramid(s0, s1, cfg, scale=scale, radius=radius, spread=spread,
                                         out=disp, corrmap=corr)

    # (within a window round the one call runs after its four calls at scale 2 and before them
    # at scale 4, so a position effect would show with opposite signs)
    def second_record(fn):
        def run():
            os.environ["BICOS_PYRAMID_SINGLE_RECORD"] = "0"
            try:
                return fn()
            finally:
                del os.environ["BICOS_PYRAMID_SINGLE_RECORD"]
        return run

    fns = {"ranged": lambda: eng.match(s0, s1, cfg, out=disp, corrmap=corr),
           "four_calls_s2": four_calls(2), "pyramid_s2": pyramid(2),
           "pyramid_s2_second_record": second_record(pyramid(2)),
           "pyramid_s4_second_record": second_record(pyramid(4)),
           "pyramid_s4": pyramid(4), "four_calls_s4": four_calls(4)}
    maps = {}
    for k, fn in fns.items():
        maps[k] = fn()[0].cpu().numpy().copy()
    for scale in (2, 4):  # the one call is its four calls
        for k in ("pyramid_s%d", "pyramid_s%d_second_record"):
            assert np.array_equal(maps[k % scale].view(np.uint32),
                                  maps["four_calls_s%d" % scale].view(np.uint32))
    ts = alternate(fns, args.reps, args.windows)
    ranged = maps["ranged"]
    inv = np.float32(-32768.0)
    for k in fns:
        line = {"bench": "pyramid", "case": k, "rows": H, "cols": W, "n": N, "depth": 1,
                "scene": "planted, disparities 16..63", "disparity_range": list(WINDOW),
                "nxcorr_threshold": 0.9, "radius": radius, "spread": spread,
                "reps_per_window": args.reps,
                "invalid_fraction": round(float((maps[k] == inv).mean()), 5),
                "differs_from_ranged": round(float((maps[k] != ranged).mean()), 5)}
        line.update(stats(ts[k]))
        line["speedup_vs_ranged"] = round(statistics.median(ts["ranged"]) /
                                          statistics.median(ts[k]), 3)
        emit(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--pool-reps", type=int, default=1000)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--shapes", default="cfg2,readme")
    ap.add_argument("--rows", type=int, default=0, help="(a smaller frame for a dry run)")
    ap.add_argument("--skip", default="", help="pool or pyramid")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    assert args.reps >= 10 and args.windows >= 3
    eng = device.Engine(0)
    lines = []

    def emit(line):
        print(json.dumps(line), flush=True)
        lines.append(line)
        if args.out:
            with open(args.out, "a") as f:
                f.write(json.dumps(line) + "\n")

    if args.skip != "pool":
        pool_lines(eng, args, emit)
    if args.skip != "pyramid":
        pyramid_lines(eng, args, emit)


if __name__ == "__main__":
    main()
