"""The mesh (libbicos_amd/csrc/mesh.hip) at the shapes users run: cfg2's 2048 x 1536 (float map
of a match with the NXC stage, rejected pixels -32768.0) and the README frame's 3208 x 2200
(subpixel map, rejected pixels NaN), the maps coming from a real match() of the synthetic
planted-disparity frame. Timed with device events, each window `--reps` (>= 200) back-to-back
calls after a warm-up, the candidates alternated window by window in one process, `--repeats`
(>= 3) windows each; reported: the median and the spread of the windows.

  mesh         bicos_mesh_device: points, index, triangles; the ranks in the workspace
  mesh_vmap    ... with the caller's vertex_map as the rank array
  list_index   bicos_reproject_device, points and index: the mesh's first three launches
  copy         a device-to-device hipMemcpyAsync (torch's Tensor.copy_ of a contiguous byte
               tensor) of the bytes the mesh WRITES: kept * 16 + pixels * 4 + triangles * 12
  match        the match that produced the map (fewer calls per window: it is the long one)

Bytes: written as above; read = 4 passes over the map (two for the vertices, two for the quads,
whose neighbour reads hit the cache) + 2 passes over the ranks; the segment counts (32 B per 2048
pixels) are left out. No threshold: the numbers go into profiles/mesh.jsonl and DESIGN.md 5.11.

  python tools/mesh_bench.py [--reps 200] [--repeats 3] [--out profiles/mesh.jsonl]
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
MATCH_REPS = 20  # calls per window of the match


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
    for fn, _ in fns.values():  # warm
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(repeats):
        for k, (fn, n) in fns.items():
            ts[k].append(window(fn, n or reps))
    return ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--shapes", default="cfg2,readme")
    ap.add_argument("--max-diff", type=float, default=1.0)
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
        tl, tr = torch.from_numpy(l).cuda(), torch.from_numpy(r).cuda()
        del l, r
        mcfg = device.MatchConfig(**sh["cfg"])
        disp, _ = eng.match(tl, tr, mcfg, want_corrmap=False)
        scratch = torch.empty_like(disp)
        Q = [[1, 0, 0, -W / 2], [0, 1, 0, -H / 2], [0, 0, 0, 800.0], [0, 0, 1 / 0.12, 0]]
        q = _lib.reproject_q(Q)
        flags = _lib.MESH_F32_SENTINEL
        pixels, tcap = H * W, 2 * (H - 1) * (W - 1)
        pts = torch.empty((pixels, 3), dtype=torch.float32, device="cuda")
        idx = torch.empty((pixels,), dtype=torch.int32, device="cuda")
        tri = torch.empty((tcap, 3), dtype=torch.int32, device="cuda")
        vmap = torch.empty((H, W), dtype=torch.int32, device="cuda")
        cnt = torch.zeros((8,), dtype=torch.int32, device="cuda")
        st = torch.cuda.current_stream().cuda_stream

        def mesh(vm):
            def fn():
                rc = L.bicos_mesh_device(eng._h, disp.data_ptr(), _lib.CV_32F, H, W, q, flags,
                                         args.max_diff, pts.data_ptr(), idx.data_ptr(), pixels,
                                         cnt.data_ptr(), tri.data_ptr(), tcap, cnt.data_ptr() + 16,
                                         vm, st)
                if rc:
                    _lib.check(rc, "bicos_mesh_device")
            return fn

        def points():
            rc = L.bicos_reproject_device(eng._h, disp.data_ptr(), _lib.CV_32F, H, W, q, flags,
                                          None, pts.data_ptr(), idx.data_ptr(), pixels,
                                          cnt.data_ptr(), st)
            if rc:
                _lib.check(rc, "bicos_reproject_device")

        def match():
            eng.match(tl, tr, mcfg, want_corrmap=False, out=scratch)

        mesh(vmap.data_ptr())()
        torch.cuda.synchronize()
        counts = [int(v) & 0xFFFFFFFF for v in cnt.cpu().tolist()]
        kept, tris = counts[0], counts[4]
        # what is timed is also right: the vertex map is the inverse of the index, every
        # triangle's corners are vertices, and the quads add up
        assert torch.equal(vmap.view(-1)[idx[:kept].long()],
                           torch.arange(kept, dtype=torch.int32, device="cuda"))
        assert int(tri[:tris].min()) >= 0 and int(tri[:tris].max()) < kept
        assert tris == 2 * counts[5] + counts[6] and sum(counts[5:]) == (H - 1) * (W - 1)
        elem = disp.element_size()
        written = kept * 16 + pixels * 4 + tris * 12
        read = 4 * pixels * elem + 2 * pixels * 4
        src = torch.empty((written,), dtype=torch.uint8, device="cuda")
        dst = torch.empty_like(src)
        fns = {"mesh": (mesh(None), 0), "mesh_vmap": (mesh(vmap.data_ptr()), 0),
               "list_index": (points, 0),
               "copy": (lambda: dst.copy_(src, non_blocking=True), 0),
               "match": (match, MATCH_REPS)}
        ts = alternate(fns, args.reps, args.repeats)
        med = {k: statistics.median(v) for k, v in ts.items()}
        for k in fns:
            line = {"bench": "mesh", "shape": name, "rows": H, "cols": W, "case": k,
                    "map": "float32", "max_diff": args.max_diff, "counts": counts[:4],
                    "mesh_counts": counts[4:], "kept_fraction": round(kept / pixels, 4),
                    "triangles_per_pixel": round(tris / pixels, 4),
                    "bytes_written": written, "bytes_read": read,
                    "bytes_per_pixel": round((written + read) / pixels, 2),
                    "ms_median": round(med[k], 5), "ms_windows": [round(t, 5) for t in ts[k]],
                    "spread": round((max(ts[k]) - min(ts[k])) / med[k], 4),
                    "time_over_copy": round(med[k] / med["copy"], 3),
                    "time_over_list_index": round(med[k] / med["list_index"], 3),
                    "time_over_match": round(med[k] / med["match"], 4),
                    "reps_per_window": fns[k][1] or args.reps,
                    "segment": L.bicos_mesh_segment()}
            if k in ("mesh", "mesh_vmap"):
                line["GBps_written_plus_read"] = round((written + read) / med[k] / 1e6, 1)
            if k == "copy":
                line["GBps_copy_read_plus_written"] = round(2 * written / med[k] / 1e6, 1)
            print(json.dumps(line), flush=True)
            lines.append(line)
        del pts, idx, tri, vmap, src, dst, disp, scratch, tl, tr
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
