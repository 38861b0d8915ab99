"""Rectification (libbicos_amd/csrc/rectify.hip) at the shapes users run: cfg2's 2048 x 1536 and
the README frame's 3208 x 2200, one stack of n = 33 u8 images per call, source and output of one
size. The maps are a real rig's kind: a 2 degree rotation about the optical axis plus radial
distortion k1, from Engine.rectify_maps. Timed with device events, each window `--reps` (>= 100)
back-to-back calls after a warm-up, the candidates alternated window by window in one process,
`--repeats` (>= 3) windows each; reported: the median and the spread of the windows.

  rectify   bicos_rectify_device of one stack (with the valid map): one launch
  copy      a device-to-device copy (torch's Tensor.copy_ of a contiguous byte tensor) of HALF the
            call's algorithmic bytes -- a copy of N bytes moves 2N, so this is what the machine
            sustains for that much traffic
  match     that shape's Engine.match on two such stacks (cfg2: NXC threshold; README: threshold,
            minimum variance, subpixel step)
  maps      bicos_rectify_maps_device, once per rig: for the record

Algorithmic bytes of one call: n planes read, n planes written, both maps read, valid written =
pixels * (2 n + 9). A frame needs two stacks: 2 x rectify is set against one match.
The figures are WARM: the same buffers every call. cfg2's 233 MB just fit the 256 MB Infinity
Cache, the README frame's 529 MB exceed it, so its stacks stream from HBM while its maps may stay.

  python tools/rectify_bench.py [--reps 100] [--repeats 3] [--out profiles/rectify.jsonl]
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
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            ts[k].append(window(fn, reps))
    return ts


def rig(H, W):
    f = 0.9 * W
    K = np.array([[f, 0, W / 2], [0, f, H / 2], [0, 0, 1]])
    a = np.deg2rad(2.0)
    R = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    return K, np.array([-0.05, 0, 0, 0]), R, K


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--shapes", default="cfg2,readme")
    ap.add_argument("--tag", default="", help="a label for the kernel variant measured")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    assert args.reps >= 100 and args.repeats >= 3
    L = _lib.lib()
    eng = device.Engine(0)
    lines = []
    for name in args.shapes.split(","):
        sh = SHAPES[name]
        H, W, n = sh["H"], sh["W"], sh["n"]
        l, r = stereo_stack(n, H, W, np.uint8)
        tl, tr = torch.from_numpy(l).cuda(), torch.from_numpy(r).cuda()
        K, D, R, P = rig(H, W)
        mx, my = eng.rectify_maps(K, D, R, P, (H, W))
        out = torch.empty_like(tl)
        valid = torch.empty((H, W), dtype=torch.uint8, device="cuda")
        cfg = device.MatchConfig(**sh["cfg"])
        disp = torch.empty((H, W), dtype=torch.float32, device="cuda")
        # what is timed is also right: two planes against the numpy restatement
        from tests import rectify_ref
        eng.rectify(tl[:2], mx, my, out=out[:2], valid=valid)
        torch.cuda.synchronize()
        want, wv = rectify_ref.remap(l[:2], mx.cpu().numpy(), my.cpu().numpy(), 0)
        assert np.array_equal(out[:2].cpu().numpy(), want) and np.array_equal(valid.cpu().numpy(), wv)
        valid_fraction = float(wv.mean())
        del want, wv, l, r
        pixels = H * W
        nbytes = pixels * (2 * n + 9)
        src = torch.empty((nbytes // 2,), dtype=torch.uint8, device="cuda")
        dst = torch.empty_like(src)
        k, d, nd, rr, p, p_cols, _, _ = _lib.rectify_camera(K, D, R, P, (H, W))
        st = torch.cuda.current_stream().cuda_stream

        def maps():
            rc = L.bicos_rectify_maps_device(k, d, nd, rr, p, p_cols, H, W, mx.data_ptr(),
                                             my.data_ptr(), st)
            if rc:
                _lib.check(rc, "bicos_rectify_maps_device")

        fns = {"rectify": lambda: eng.rectify(tl, mx, my, out=out, valid=valid),
               "copy": lambda: dst.copy_(src, non_blocking=True),
               "match": lambda: eng.match(tl, tr, cfg, want_corrmap=False, out=disp),
               "maps": maps}
        ts = alternate(fns, args.reps, args.repeats)
        med = {k_: statistics.median(v) for k_, v in ts.items()}
        line = {"bench": "rectify", "tag": args.tag, "shape": name, "rows": H, "cols": W, "n": n,
                "depth": 1, "map": "2 degree rotation + k1 = -0.05",
                "valid_fraction": round(valid_fraction, 4), "warm": True,
                "algorithmic_bytes": nbytes, "tile": list(_lib.rectify_tile()),
                "reps_per_window": args.reps}
        for k_ in fns:
            line[k_ + "_ms_median"] = round(med[k_], 5)
            line[k_ + "_ms_windows"] = [round(t, 5) for t in ts[k_]]
            line[k_ + "_spread"] = round((max(ts[k_]) - min(ts[k_])) / med[k_], 4)
        line["algorithmic_GBps"] = round(nbytes / med["rectify"] / 1e6, 1)
        line["copy_GBps"] = round(nbytes / med["copy"] / 1e6, 1)
        line["time_over_copy"] = round(med["rectify"] / med["copy"], 3)
        line["two_stacks_over_match"] = round(2 * med["rectify"] / med["match"], 3)
        print(json.dumps(line), flush=True)
        lines.append(line)
        del tl, tr, out, valid, src, dst, mx, my, disp
    if args.out:
        with open(args.out, "a") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
