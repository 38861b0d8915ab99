"""Surface normals (libbicos_amd/csrc/normals.hip) at the shapes users run: cfg2's 2048 x 1536
and the README frame's 3208 x 2200, on the map of a real Engine.match() of the synthetic
planted-disparity stacks -- float32 from the README configuration (NXC, variance filter,
subpixel step 0.1: the maps the stage is meant for) and int16 from a match without the NXC
stage -- for radius 1, 2 and 4, the dense map and the list over reproject's index.

Timed with device events, each window `--reps` back-to-back calls after a warm-up, the
candidates alternated window by window in one process, `--repeats` (>= 3) windows each;
reported: the median and the spread of the windows. Next to each case:

  copy       a device-to-device copy (torch's Tensor.copy_ of a contiguous tensor) that moves
             the algorithmic bytes of the dense form, map read + 12 bytes per pixel written,
             half of them read and half written. These buffers fit the Infinity Cache, so it
             is a warm figure, not an HBM rate.
  reproject  Engine.reproject_map of the same map: the dense stage beside this one
  match      that configuration's Engine.match() in the same session: the stage this one follows

Before anything is timed one call per radius and form is compared bit for bit with the
restatement of tests/normals_ref.py at a small shape. Without a GPU the tool fails.

  python tools/normals_bench.py [--reps 100] [--repeats 3] [--out profiles/normals.jsonl]
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
from tests import normals_ref  # noqa: E402
from tools.speckle_bench import alternate  # noqa: E402

SUBPIXEL = dict(nxcorr_threshold=0.96, min_variance=2.0, subpixel_step=0.1)  # the README's
SHAPES = {
    "cfg2": dict(n=33, H=1536, W=2048),
    "readme": dict(n=33, H=2200, W=3208),
}
CFG = {"float32": SUBPIXEL, "int16": dict(nxcorr_threshold=None)}
RADII = (1, 2, 4)
MAX_DIFF, MIN_POINTS = 1.0, 3


def self_check(eng):
    tr, tc = _lib.normals_tile()
    rows, cols = tr + 5, tc + 7
    rng = np.random.default_rng(0)
    index = rng.permutation(rows * cols).astype(np.int32)
    for dtype in (np.int16, np.float32):
        name, d, q = [p for p in normals_ref.patterns(rows, cols, dtype) if p[0] == "random-holes"][0]
        t, it = torch.from_numpy(d).cuda(), torch.from_numpy(index).cuda()
        for radius in RADII:
            want = normals_ref.restate(d, q, 2, radius, MAX_DIFF, MIN_POINTS)
            assert want["counts"][0] and want["counts"][1] and want["counts"][2]
            cnt = torch.zeros((4,), dtype=torch.int32, device="cuda")
            out = eng.normals_map(t, q, radius=radius, sentinel=True, counts=cnt)
            lst = eng.normals_points(t, q, it, radius=radius, sentinel=True)
            assert np.array_equal(normals_ref.bits(out.cpu().numpy()), normals_ref.bits(want["map"]))
            assert cnt.cpu().numpy().view(np.uint32).tolist() == want["counts"].tolist()
            assert np.array_equal(normals_ref.bits(lst.cpu().numpy()),
                                  normals_ref.bits(normals_ref.gather(want["map"], index)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--match-reps", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--shapes", default="cfg2,readme")
    ap.add_argument("--dtypes", default="int16,float32")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    assert args.reps >= 50 and args.repeats >= 3
    if not torch.cuda.is_available():
        sys.exit("normals_bench: no GPU")
    eng = device.Engine(0)
    self_check(eng)
    tile = _lib.normals_tile()
    lines = []
    for name in args.shapes.split(","):
        sh = SHAPES[name]
        H, W = sh["H"], sh["W"]
        Q = normals_ref.rig_q(H, W)
        l, r = stereo_stack(sh["n"], H, W, np.uint8)
        tl, tr = torch.from_numpy(l).cuda(), torch.from_numpy(r).cuda()
        del l, r
        for dtype in args.dtypes.split(","):
            cfg = device.MatchConfig(**CFG[dtype])

            def match():
                return eng.match(tl, tr, cfg, want_corrmap=False)

            disp, _ = match()
            assert str(disp.dtype) == "torch." + dtype
            _, index, stats = eng.reproject_points(disp, Q, sentinel=False, with_index=True)
            index = index.clone()
            out = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
            lst = torch.empty((index.shape[0], 3), dtype=torch.float32, device="cuda")
            xyz = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
            cnt = torch.zeros((4,), dtype=torch.int32, device="cuda")
            nbytes = H * W * (disp.element_size() + 12)
            copy_src = torch.zeros((nbytes // 2,), dtype=torch.uint8, device="cuda")
            copy_dst = torch.empty_like(copy_src)

            def dense(radius):
                return lambda: eng.normals_map(disp, Q, radius=radius, max_diff=MAX_DIFF,
                                               min_points=MIN_POINTS, out=out, counts=cnt)

            def listed(radius):
                return lambda: eng.normals_points(disp, Q, index, radius=radius, max_diff=MAX_DIFF,
                                                  min_points=MIN_POINTS, out=lst)

            counts = {}
            for radius in RADII:
                dense(radius)()
                torch.cuda.synchronize()
                counts[radius] = [int(v) & 0xFFFFFFFF for v in cnt.cpu().tolist()]
                assert sum(counts[radius]) == H * W
                listed(radius)()
                torch.cuda.synchronize()
                assert torch.equal(out.reshape(-1, 3)[index.long()].view(torch.int32),
                                   lst.view(torch.int32))
            fns = {}
            for radius in RADII:
                fns[("dense", radius)] = dense(radius)
                fns[("list", radius)] = listed(radius)
            fns["copy"] = lambda: copy_dst.copy_(copy_src, non_blocking=True)
            fns["reproject"] = lambda: eng.reproject_map(disp, Q, sentinel=False, out=xyz)
            fns["match"] = match
            reps = {k: args.match_reps if k == "match" else args.reps for k in fns}
            ts = alternate(fns, reps, args.repeats)
            med = {k: statistics.median(v) for k, v in ts.items()}
            for key in fns:
                if not isinstance(key, tuple):
                    continue
                form, radius = key
                line = {"bench": "normals", "shape": name, "rows": H, "cols": W, "map": dtype,
                        "form": form, "radius": radius, "max_diff": MAX_DIFF,
                        "min_points": MIN_POINTS, "counts": counts[radius],
                        "list_entries": int(index.shape[0]), "kept_points": stats["kept"],
                        "algorithmic_bytes": nbytes, "ms_median": round(med[key], 5),
                        "ms_windows": [round(t, 5) for t in ts[key]],
                        "spread": round((max(ts[key]) - min(ts[key])) / med[key], 4),
                        "copy_ms_median": round(med["copy"], 5),
                        "copy_ms_windows": [round(t, 5) for t in ts["copy"]],
                        "time_over_copy": round(med[key] / med["copy"], 2),
                        "reproject_ms_median": round(med["reproject"], 5),
                        "reproject_ms_windows": [round(t, 5) for t in ts["reproject"]],
                        "time_over_reproject": round(med[key] / med["reproject"], 2),
                        "match_ms_median": round(med["match"], 4),
                        "match_ms_windows": [round(t, 4) for t in ts["match"]],
                        "time_over_match": round(med[key] / med["match"], 4),
                        "reps_per_window": args.reps, "match_reps_per_window": args.match_reps,
                        "tile": list(tile)}
                print(json.dumps(line), flush=True)
                lines.append(line)
            del disp, out, lst, xyz, copy_src, copy_dst, index
        del tl, tr
    if args.out:
        with open(args.out, "a") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
