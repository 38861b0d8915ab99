"""How often the pruned 128-bit NoDuplicates search (search_mx.hip search_mx_kernel PRUNE)
needs a block's second K-step -- a CPU simulation in reach_sim's visiting order, on the
synthetic stereo frame, on the same frame with a share of the right descriptor bits flipped,
or on random descriptors.

The kernel's test x_lo - |a_hi| <= running x is, in Hamming terms, ham_lo <= running ham
(ham = x + |a|, |a| = |a_lo| + |a_hi|): a unit "reaches" when some col0 of it has its block
minimum over the FIRST 64 descriptor bits <= its running minimum cost over all bits. Units
are 32-col0 tiles or the kernel's tile pairs (64 col0, one branch). A unit that does not reach
skips the block; the simulation checks that the minima and the last minima then still equal
the full scan's. With --fallback the wave's window rule is simulated too (PRUNE_WINDOW blocks,
>= 7/8 of the pair-blocks reaching sends the wave to the unpruned loop for the rest of the row).

--probe-words D simulates the packed kernel instead (search_pk.hip search_pkp_kernel): units
are its wide tiles (64 col0, two per wave), the probe is the first D 32-bit descriptor words
from --lo-bits on, and a wave starts at depth D and follows the chain 1 -> 2 -> unpruned under
the same window rule (a wave never goes back up). It prints the reach rate per depth, the
waves that left each depth, and the scaled MFMAs and trees per wave-block that follow (probe
2 D, + (4 - D) per reaching tile; trees 2, + 1 per reaching tile; unpruned 8 and 2).

--mix K (with --probe-words) chooses which 32 bits each of the kernel's four products holds.
expand_bits puts the bits p of a word with (p mod 8) div 2 == m into dword m of its expansion;
product k < K takes dword m from word (k - m) mod K, the products from K on their own word. K = 1:
a product is a descriptor word (the kernel before the mix); K = 2: the kernel's map
(search_plan.hpp pkp_dword_word; tests/test_pkp_probe_mix.py holds the two together); K = 3, 4:
the wider rotations. The probe at depth D is then the first D products.

  python tools/prune_sim.py [--rows 0 500 767 1535] [--W 2048] [--flip 0 0.02 0.05 0.1]
                            [--random] [--lo-bits 0] [--fallback] [--probe-words 1] [--window1 8]
                            [--mix 1]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from reach_sim import costs, limited_bits, order_current, pack  # noqa: E402
from libbicos_amd.synthetic import random_stack, stereo_stack  # noqa: E402

PRUNE_WINDOW = 8  # search_mx.hip


def simulate(C, Clo, cols, unit_tiles, fallback, waves=8, T=4, chunk=1024):
    """-> (units, partial reaches, units whose second K-step runs, waves, waves fallen back)"""
    units = reach = second = nwaves = fell = 0
    per_wg = waves * T * 32
    full_min = C.min(axis=1)
    for wg in range((cols + per_wg - 1) // per_wg):
        for w in range(waves):
            c0_wave = wg * per_wg + w * T * 32
            if c0_wave >= cols:
                continue
            nwaves += 1
            blocks = order_current(c0_wave, (wg + 1) * per_wg - 1, cols, chunk)
            spans = []
            for t in range(0, T, unit_tiles):
                lo, hi = c0_wave + 32 * t, min(cols, c0_wave + 32 * (t + unit_tiles))
                if lo < cols:
                    spans.append((lo, hi))
            run = {s: np.full(s[1] - s[0], 1 << 30) for s in spans}
            last = {s: np.full(s[1] - s[0], -1) for s in spans}
            pruning, wb, wr = True, 0, 0
            for B in blocks:
                e = min(cols, B + 32)
                full = e - B == 32  # the partial last block never prunes
                for s in spans:
                    units += 1
                    c = C[s[0]:s[1], B:e]
                    bm = c.min(axis=1)
                    r = bool((Clo[s[0]:s[1], B:e].min(axis=1) <= run[s]).any())
                    if full and pruning:
                        reach += r
                        wr += r
                    if r or not (full and pruning):
                        second += 1
                        # the last column at the running minimum cost, any visiting order
                        arg = B + c.shape[1] - 1 - np.argmin(c[:, ::-1], axis=1)
                        take = (bm < run[s]) | ((bm == run[s]) & (arg > last[s]))
                        last[s] = np.where(take, arg, last[s])
                        run[s] = np.minimum(run[s], bm)
                if full and pruning and fallback:
                    wb += 1
                    if wb == PRUNE_WINDOW:
                        if 8 * wr >= 7 * PRUNE_WINDOW * len(spans):
                            pruning = False
                            fell += 1
                        wb = wr = 0
            for s in spans:  # pruning changed nothing
                assert (run[s] == full_min[s[0]:s[1]]).all()
                c = C[s[0]:s[1]]
                want = cols - 1 - np.argmin(c[:, ::-1], axis=1)
                assert (last[s] == want).all()
    return units, reach, second, nwaves, fell


def mix_product(bit, K):
    """The product (0-3) that holds descriptor bit 0-127 under --mix K"""
    w, m = bit // 32, (bit % 8) // 2
    return (w + m) % K if w < K else w


def mix_order(K):
    """The 128 descriptor bit positions, product by product"""
    return np.array(sorted(range(128), key=lambda b: (mix_product(b, K), b)))


def simulate_chain(C, Cw, cols, depth0, window1=PRUNE_WINDOW, waves=8, chunk=1024):
    """The packed kernel's chain. Cw[d]: costs over the first d words (d = 1, 2). -> int64[11]:
    wave-blocks, wide-tile-blocks, tile-blocks tested and reaching at depth 1, at depth 2,
    MFMAs, trees, waves that left depth 1, waves that left depth 2, pruned wave-blocks with a
    reaching tile"""
    out = np.zeros(11, np.int64)
    per_wg = waves * 128
    full_min = C.min(axis=1)
    for wg in range((cols + per_wg - 1) // per_wg):
        for w in range(waves):
            c0_wave = wg * per_wg + w * 128
            if c0_wave >= cols:
                continue
            blocks = order_current(c0_wave, (wg + 1) * per_wg - 1, cols, chunk)
            spans = [(lo, min(cols, lo + 64)) for lo in (c0_wave, c0_wave + 64) if lo < cols]
            run = {s: np.full(s[1] - s[0], 1 << 30) for s in spans}
            last = {s: np.full(s[1] - s[0], -1) for s in spans}
            depth, wb, wr = depth0, 0, 0
            for B in blocks:
                e = min(cols, B + 32)
                d = depth if e - B == 32 else 0  # the partial last block never prunes
                out[0] += 1
                any_reach = False
                out[6] += 8 if d == 0 else 2 * d   # both tiles' slots run (an idle tile too)
                out[7] += 2
                for s in spans:
                    out[1] += 1
                    c = C[s[0]:s[1], B:e]
                    bm = c.min(axis=1)
                    r = d == 0 or bool((Cw[d][s[0]:s[1], B:e].min(axis=1) <= run[s]).any())
                    if d:
                        out[2 * d] += 1
                        out[2 * d + 1] += r
                        wr += r
                        any_reach |= r
                        out[6] += (4 - d) * r
                        out[7] += r
                    if r:
                        arg = B + c.shape[1] - 1 - np.argmin(c[:, ::-1], axis=1)
                        take = (bm < run[s]) | ((bm == run[s]) & (arg > last[s]))
                        last[s] = np.where(take, arg, last[s])
                        run[s] = np.minimum(run[s], bm)
                if d:
                    out[10] += any_reach
                    wb += 1
                    win = window1 if depth == 1 else PRUNE_WINDOW
                    if wb == win:
                        if 8 * wr >= 7 * win * 2:
                            out[7 + depth] += 1
                            depth = 2 if depth == 1 else 0
                        wb = wr = 0
            for s in spans:  # pruning changed nothing
                assert (run[s] == full_min[s[0]:s[1]]).all()
                want = cols - 1 - np.argmin(C[s[0]:s[1], ::-1], axis=1)
                assert (last[s] == want).all()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[0, 500, 767, 1535])
    ap.add_argument("--W", type=int, default=2048)
    ap.add_argument("--n", type=int, default=33)
    ap.add_argument("--flip", type=float, nargs="+", default=[0.0, 0.02, 0.05, 0.10])
    ap.add_argument("--random", action="store_true")
    ap.add_argument("--lo-bits", type=int, default=0, help="first bit of the 64-bit partial subset")
    ap.add_argument("--fallback", action="store_true")
    ap.add_argument("--probe-words", type=int, default=0, choices=[0, 1, 2],
                    help="the packed kernel's chain from this probe depth (0: the one-product kernel)")
    ap.add_argument("--window1", type=int, default=PRUNE_WINDOW, help="the chain's window at depth 1, in blocks")
    ap.add_argument("--mix", type=int, default=1, choices=[1, 2, 3, 4],
                    help="the packed kernel's products: expansion dwords rotated over the first K words")
    args = ap.parse_args()
    if args.mix > 1 and (not args.probe_words or args.lo_bits):
        ap.error("--mix goes with --probe-words and without --lo-bits")
    H = 1536
    for flip in ([0.0] if args.random else args.flip):
        tot = {1: np.zeros(5, np.int64), 2: np.zeros(5, np.int64)}
        med = []
        chain = np.zeros(11, np.int64)
        for r in args.rows:
            if args.random:
                L = random_stack(args.n, 1, args.W, seed=int(r) + 1)
                R = random_stack(args.n, 1, args.W, seed=int(r) + 7)
            else:
                L, R = stereo_stack(args.n, H, args.W, row_begin=int(r), row_end=int(r) + 1)
            b0, b1 = limited_bits(L)[0], limited_bits(R)[0]
            if flip:
                b1 = b1 ^ (np.random.default_rng(int(r)).random(b1.shape) < flip)
            nb = b0.shape[-1]
            sel = (np.arange(64) + args.lo_bits) % nb
            C = costs(pack(b0), pack(b1))
            if args.mix > 1:    # (the zero bits past the used ones take their places too)
                z = np.zeros(b0.shape[:-1] + (128 - nb,), bool)
                b0, b1 = np.concatenate([b0, z], -1), np.concatenate([b1, z], -1)
                sel = mix_order(args.mix)
            if args.probe_words:
                Cw = {d: costs(pack(b0[:, sel[:32 * d]]), pack(b1[:, sel[:32 * d]])) for d in (1, 2)}
                chain = chain + simulate_chain(C, Cw, args.W, args.probe_words, args.window1)
                continue
            Clo = costs(pack(b0[:, sel]), pack(b1[:, sel]))
            med.append(float(np.median(C.min(axis=1))))
            for ut in (1, 2):
                tot[ut] += np.array(simulate(C, Clo, args.W, ut, args.fallback))
        name = "random" if args.random else "flip %.2f" % flip
        if args.mix > 1:
            name += " mix %d" % args.mix
        if args.probe_words:
            wb, tb, t1, r1, t2, r2, mf, tr, f1, f2, wr = chain
            print("%-10s start depth %d: depth 1 reach %.3f of %d tile-blocks, depth 2 reach %.3f of %d, "
                  "%.3f of pruned wave-blocks hold a reaching tile; per wave-block %.3f scaled MFMAs, "
                  "%.3f trees; waves leaving depth 1: %d, depth 2: %d" % (
                      name, args.probe_words, r1 / max(1, t1), t1, r2 / max(1, t2), t2,
                      wr / max(1, (t1 + t2) // 2), mf / wb, tr / wb, f1, f2))
            continue
        for ut, label in ((1, "tile"), (2, "pair")):
            u, rch, sec, nw, fell = tot[ut]
            # (partial reach counts the blocks tested while pruning: after a wave falls back its
            # blocks are not tested any more and all run their second K-step)
            print("%-10s median match cost %4.1f  per %s: partial reach %.3f, second K-step %.3f of "
                  "unit-blocks, %d of %d waves fell back" % (name, np.median(med), label,
                                                             rch / max(1, u), sec / u, fell, nw))


if __name__ == "__main__":
    main()
