"""The projection (libbicos_amd/csrc/project.hip) at the shapes users run: the point list of a
real match() of the synthetic planted-disparity frame at cfg2's 2048 x 1536 and the README
frame's 3208 x 2200, projected into a camera of the same size that is rotated a few degrees,
shifted and mildly distorted. Timed with device events, each window `--reps` (>= 200)
back-to-back calls after a warm-up, the candidates alternated window by window in one process,
`--repeats` (>= 3) windows each; reported: the median and the spread of the windows.

  plain[_tex]      tol = inf and no map: no z-buffer, one launch (uv, depth, cls, counts[, tex])
  z_s<S>[_tex]     tol = 0.01 with splat S in 0, 1, 2: memset, splat, resolve
  z_s1_maps        ... and the depth and index images: the fourth launch
  copy_<case>      a device-to-device copy (torch's Tensor.copy_ of a contiguous byte tensor) that
                   moves the bytes the case reads and writes: half of them, read and written
  list_index       bicos_reproject_device, points and index: what made the list
  match            the match that produced the map (fewer calls per window: it is the long one)

Bytes per point: 12 read per launch that projects (the resolve computes a point again instead
of reading what the splat could have stored), 13 written (uv, depth, cls), 3 more with a u8
3-channel texture and its 4 taps of 3 bytes read (counted once: neighbours share them in cache);
per pixel of the camera 8 written by the memset, and 8 read and 8 written by the maps' launch.
The atomics are counted exactly, as OFFERS (the clipped splat of every inside point; the kernel
skips the atomic of an offer that a plain load shows cannot win), and not as bytes.
No threshold: the numbers go into profiles/project.jsonl and DESIGN.md 5.12.

  python tools/project_bench.py [--reps 200] [--repeats 3] [--out profiles/project.jsonl]
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
TOL = 0.01


def rotation(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


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
        f = 800.0
        Q = [[1, 0, 0, -W / 2], [0, 1, 0, -H / 2], [0, 0, 0, f], [0, 0, 1 / 0.12, 0]]
        q = _lib.reproject_q(Q)
        pixels = H * W
        pts = torch.empty((pixels, 3), dtype=torch.float32, device="cuda")
        idx = torch.empty((pixels,), dtype=torch.int32, device="cuda")
        cnt = torch.zeros((8,), dtype=torch.int32, device="cuda")
        st = torch.cuda.current_stream().cuda_stream
        flags = _lib.REPROJECT_F32_SENTINEL

        def points():
            rc = L.bicos_reproject_device(eng._h, disp.data_ptr(), _lib.CV_32F, H, W, q, flags,
                                          None, pts.data_ptr(), idx.data_ptr(), pixels,
                                          cnt.data_ptr(), st)
            if rc:
                _lib.check(rc, "bicos_reproject_device")

        def match():
            eng.match(tl, tr, mcfg, want_corrmap=False, out=scratch)

        points()
        torch.cuda.synchronize()
        n = int(cnt[0]) & 0xFFFFFFFF
        K = np.array([[f, 0, W / 2 + 3.3], [0, f * 1.01, H / 2 - 2.1], [0, 0, 1]])
        D = [-0.05, 0.01, 0.0005, -0.0003, -0.001]
        R, t = rotation(0.02, -0.035, 0.01), [0.004, -0.002, 0.01]
        r_, t_, k_, d_, nd = _lib.project_camera(K, D, R, t)
        image = torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, device="cuda")
        uv = torch.empty((n, 2), dtype=torch.float32, device="cuda")
        z = torch.empty((n,), dtype=torch.float32, device="cuda")
        cls = torch.empty((n,), dtype=torch.uint8, device="cuda")
        tex = torch.empty((n, 3), dtype=torch.uint8, device="cuda")
        dmap = torch.empty((H, W), dtype=torch.float32, device="cuda")
        imap = torch.empty((H, W), dtype=torch.int32, device="cuda")
        pc = torch.zeros((5,), dtype=torch.int32, device="cuda")

        def project(splat, tol, with_tex, with_maps=False):
            def fn():
                rc = L.bicos_project_device(
                    eng._h, pts.data_ptr(), n, r_, t_, k_, d_, nd, H, W, splat, tol,
                    image.data_ptr(), 1, 3, 3 * W, 0, uv.data_ptr(), z.data_ptr(), cls.data_ptr(),
                    tex.data_ptr() if with_tex else None, dmap.data_ptr() if with_maps else None,
                    imap.data_ptr() if with_maps else None, pc.data_ptr(), st)
                if rc:
                    _lib.check(rc, "bicos_project_device")
            return fn

        def nbytes(zbuf, with_tex, with_maps=False):
            read = 12 * n * (2 if zbuf else 1) + (12 * n if with_tex else 0)
            written = 13 * n + (3 * n if with_tex else 0)
            if zbuf:
                written += 8 * pixels
            if with_maps:
                read, written = read + 8 * pixels, written + 8 * pixels
            return read, written

        cases = {"plain": (0, float("inf"), False, False), "plain_tex": (0, float("inf"), True, False)}
        for s in (0, 1, 2):
            cases["z_s%d" % s] = (s, TOL, False, False)
            cases["z_s%d_tex" % s] = (s, TOL, True, False)
        cases["z_s1_maps"] = (1, TOL, False, True)

        # what is timed is also right: the classes add up, and what each case counts
        stats, atomics = {}, {}
        for k, (s, tol, wt, wm) in cases.items():
            project(s, tol, wt, wm)()
            torch.cuda.synchronize()
            c = [int(v) & 0xFFFFFFFF for v in pc.cpu().tolist()]
            assert sum(c) == n and c[0] > 0
            stats[k] = c
            inside = cls <= 1
            px = torch.floor(uv[inside, 0] + 0.5).long()
            py = torch.floor(uv[inside, 1] + 0.5).long()
            wx = torch.clamp(px + s, max=W - 1) - torch.clamp(px - s, min=0) + 1
            wy = torch.clamp(py + s, max=H - 1) - torch.clamp(py - s, min=0) + 1
            atomics[k] = int((wx * wy).sum()) if tol < float("inf") or wm else 0
        assert stats["plain"][1] == 0 and stats["z_s0"][1] > 0

        fns, copies = {}, {}
        for k, (s, tol, wt, wm) in cases.items():
            fns[k] = (project(s, tol, wt, wm), 0)
            rd, wr = nbytes(tol < float("inf") or wm, wt, wm)
            half = (rd + wr) // 2
            if half not in copies:
                src = torch.empty((half,), dtype=torch.uint8, device="cuda")
                copies[half] = (src, torch.empty_like(src))
            a, b = copies[half]
            fns["copy_" + k] = ((lambda a=a, b=b: b.copy_(a, non_blocking=True)), 0)
        fns["list_index"] = (points, 0)
        fns["match"] = (match, MATCH_REPS)
        ts = alternate(fns, args.reps, args.repeats)
        med = {k: statistics.median(v) for k, v in ts.items()}
        for k in fns:
            line = {"bench": "project", "shape": name, "rows": H, "cols": W, "case": k,
                    "points": n, "ms_median": round(med[k], 5),
                    "ms_windows": [round(v, 5) for v in ts[k]],
                    "spread": round((max(ts[k]) - min(ts[k])) / med[k], 4),
                    "time_over_list_index": round(med[k] / med["list_index"], 3),
                    "time_over_match": round(med[k] / med["match"], 4),
                    "reps_per_window": fns[k][1] or args.reps,
                    "group": L.bicos_project_group()}
            if k in cases:
                s, tol, wt, wm = cases[k]
                rd, wr = nbytes(tol < float("inf") or wm, wt, wm)
                line.update(splat=s, tol=tol if tol < float("inf") else "inf", texture=wt, maps=wm,
                            counts=stats[k], bytes_read=rd, bytes_written=wr,
                            bytes_per_point=round((rd + wr) / n, 2),
                            GBps_read_plus_written=round((rd + wr) / med[k] / 1e6, 1),
                            time_over_copy=round(med[k] / med["copy_" + k], 3),
                            atomics=atomics[k])
                if atomics[k]:
                    line["atomics_per_point"] = round(atomics[k] / n, 3)
                    line["Gatomics_per_s_whole_call"] = round(atomics[k] / med[k] / 1e6, 2)
                    # the splat launch alone: the call less the same call's resolve-only twin
                    twin = "plain_tex" if wt else "plain"
                    extra = med[k] - med[twin]
                    line["ms_over_plain"] = round(extra, 5)
                    if extra > 0 and not wm:
                        line["Gatomics_per_s_over_plain"] = round(atomics[k] / extra / 1e6, 2)
            print(json.dumps(line), flush=True)
            lines.append(line)
        del pts, idx, uv, z, cls, tex, dmap, imap, image, disp, scratch, tl, tr, copies, fns
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
