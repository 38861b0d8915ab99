"""Reprojection (libbicos_amd/csrc/reproject.hip) at the shapes users run: cfg2's 2048 x 1536
(float map of a match with the NXC stage, rejected pixels -32768.0) and the README frame's
3208 x 2200 (subpixel map, rejected pixels NaN), the maps coming from a real match() of the
synthetic planted-disparity frame. Timed with device events, each window `--reps` (>= 200)
back-to-back calls after a warm-up, the candidates alternated window by window in one process,
`--repeats` (>= 3) windows each; reported: the median and the spread of the windows.

  dense        bicos_reproject_device, xyz_map only: one launch
  list         ... points only: count, scan, write
  list_index   ... points and index
  copy_<case>  next to each: a device-to-device hipMemcpyAsync (torch's Tensor.copy_ of a
               contiguous byte tensor) of HALF the case's algorithmic bytes -- a copy of N bytes
               moves 2N, so this is what the machine sustains for that much traffic

Algorithmic bytes: dense = pixels * (elem + 12); list = 2 * pixels * elem + kept * 12 (+ kept * 4
with the index); the segment counts (16 B per 2048 pixels) are left out. The working sets fit
the 256 MB Infinity Cache, so the rates are not HBM rates.

  python tools/reproject_bench.py [--reps 200] [--repeats 3] [--out profiles/reproject.jsonl]
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
    "cfg2": dict(n=33, H=1536, W=2048, cfg=dict(nxcorr_threshold=0.96)),
    "readme": dict(n=33, H=2200, W=3208,
                   cfg=dict(nxcorr_threshold=0.96, min_variance=2.0, subpixel_step=0.1)),
}


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
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            ts[k].append(window(fn, reps))
    return ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--shapes", default="cfg2,readme")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    assert args.reps >= 200 and args.repeats >= 3
    L = _lib.lib()
    eng = device.Engine(0)
    lines = []
    for name in args.shapes.split(","):
        sh = SHAPES[name]
        H, W = sh["H"], sh["W"]
        l, r = stereo_stack(sh["n"], H, W, np.uint8)
        disp, _ = eng.match(torch.from_numpy(l).cuda(), torch.from_numpy(r).cuda(),
                            device.MatchConfig(**sh["cfg"]), want_corrmap=False)
        del l, r
        Q = [[1, 0, 0, -W / 2], [0, 1, 0, -H / 2], [0, 0, 0, 800.0], [0, 0, 1 / 0.12, 0]]
        q = _lib.reproject_q(Q)
        flags = _lib.REPROJECT_F32_SENTINEL
        pixels = H * W
        xyz = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
        pts = torch.empty((pixels, 3), dtype=torch.float32, device="cuda")
        idx = torch.empty((pixels,), dtype=torch.int32, device="cuda")
        cnt = torch.zeros((4,), dtype=torch.int32, device="cuda")
        st = torch.cuda.current_stream().cuda_stream

        def call(m, p, i):
            def fn():
                rc = L.bicos_reproject_device(eng._h, disp.data_ptr(), _lib.CV_32F, H, W, q, flags,
                                              m, p, i, pixels, cnt.data_ptr() if p else None, st)
                if rc:
                    _lib.check(rc, "bicos_reproject_device")
            return fn

        cases = {"dense": call(xyz.data_ptr(), None, None),
                 "list": call(None, pts.data_ptr(), None),
                 "list_index": call(None, pts.data_ptr(), idx.data_ptr())}
        cases["list"]()
        torch.cuda.synchronize()
        counts = [int(v) & 0xFFFFFFFF for v in cnt.cpu().tolist()]
        kept = counts[0]
        # the list is the dense map's non-NaN pixels (what is timed is also right)
        cases["dense"]()
        torch.cuda.synchronize()
        flat = xyz.view(-1, 3)
        assert torch.equal(flat[~torch.isnan(flat).any(dim=1)].view(torch.int32),
                           pts[:kept].view(torch.int32))
        elem = disp.element_size()
        nbytes = {"dense": pixels * (elem + 12), "list": 2 * pixels * elem + kept * 12,
                  "list_index": 2 * pixels * elem + kept * 16}
        src = torch.empty((max(nbytes.values()) // 2,), dtype=torch.uint8, device="cuda")
        dst = torch.empty_like(src)

        def copy(n):
            return lambda: dst[:n].copy_(src[:n], non_blocking=True)

        fns = {}
        for k, fn in cases.items():
            fns[k] = fn
            fns["copy_" + k] = copy(nbytes[k] // 2)
        ts = alternate(fns, args.reps, args.repeats)
        med = {k: statistics.median(v) for k, v in ts.items()}
        for k in cases:
            line = {"bench": "reproject", "shape": name, "rows": H, "cols": W, "case": k,
                    "map": "float32", "kept_fraction": round(kept / pixels, 4), "counts": counts,
                    "algorithmic_bytes": nbytes[k], "ms_median": round(med[k], 5),
                    "ms_windows": [round(t, 5) for t in ts[k]],
                    "spread": round((max(ts[k]) - min(ts[k])) / med[k], 4),
                    "algorithmic_GBps": round(nbytes[k] / med[k] / 1e6, 1),
                    "copy_half_bytes_ms_median": round(med["copy_" + k], 5),
                    "copy_half_bytes_ms_windows": [round(t, 5) for t in ts["copy_" + k]],
                    "time_over_copy": round(med[k] / med["copy_" + k], 3),
                    "time_over_dense": round(med[k] / med["dense"], 3),
                    "reps_per_window": args.reps, "segment": L.bicos_reproject_segment()}
            print(json.dumps(line), flush=True)
            lines.append(line)
        del xyz, pts, idx, src, dst, disp
    if args.out:
        with open(args.out, "a") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
