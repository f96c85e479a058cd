#!/usr/bin/env python3
"""Times the full-catalogue rank of held-out clicks under MANNeR's z-scored ensemble two ways, in ONE process on one GPU, the two
sides alternating (A, B, A, B, ...) after a shared warm-up, device-event timed (nothing is read back inside the timed region),
median / min / max of --iters:

* fused: ``ops.catalogue_ensemble_ranks`` (``nrl_catalogue_ensemble_ranks``: a statistics pass and a count pass over the tables,
  no (B, V) matrix is written);
* torch: the same ranks in torch ops -- one GEMM per sub-model to (B, V), the mean and ``std`` (unbiased) over the user's
  population through a mask, the weighted sum of the z-scores, ``-inf`` written at the excluded positions, then per click
  ``(z > z_t) | (z == z_t & row < t)`` summed over the user's row, in pieces of --piece clicks where the (clicks, V) comparison
  does not fit at once.

Shape: --users users, --news table rows, D = --dim, T = --models sub-models with the weights 1.0, 0.2, -0.25, 1..5 clicks per
user, ragged exclusion lists of 0..50 rows per user.  Peak allocated memory of each side is the allocator's high-water mark
above the inputs.  The two results are compared (the torch GEMM and its reductions round differently, so a rank may move where
scores are within rounding of each other; the report counts them).  The fused call makes two passes over the tables where
torch makes one.  Needs a GPU: there is no CPU path to time."""
import argparse
import os
import socket
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.topk_time import timed  # noqa: E402

WEIGHTS = (1.0, 0.2, -0.25)
NEG_INF = float("-inf")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--users", type=int, default=512)
    ap.add_argument("--news", type=int, default=65536)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--models", type=int, default=3)
    ap.add_argument("--piece", type=int, default=4096, help="clicks per piece of the torch side's comparison")
    ap.add_argument("--iters", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("catalogue_rank_ensemble_time: no GPU; a time measured anywhere else says nothing about this path")
    from newsreclib_amd import _lib, ops
    B, V, D, T = args.users, args.news, args.dim, args.models
    weights = list(WEIGHTS[:T])
    g = torch.Generator().manual_seed(args.seed + D)
    users = [torch.randn(B, D, generator=g).cuda() for _ in range(T)]
    tables = [torch.randn(V, D, generator=g).cuda() for _ in range(T)]
    sizes = torch.randint(0, 51, (B,), generator=g)
    excl_idx = torch.randint(0, V, (int(sizes.sum()),), generator=g).cuda()
    excl_user = torch.repeat_interleave(torch.arange(B), sizes).cuda()
    clicks = torch.randint(1, 6, (B,), generator=g)
    n_clicks = int(clicks.sum())
    tgt_idx = torch.randint(0, V, (n_clicks,), generator=g).cuda()
    tgt_user = torch.repeat_interleave(torch.arange(B), clicks).cuda()
    off = lambda n: torch.cat([torch.zeros(1, dtype=torch.int64), n.cumsum(0)]).cuda()  # noqa: E731
    excl_off, tgt_off = off(sizes), off(clicks)
    rows = torch.arange(V, device="cuda")
    lines = [f"catalogue_rank_ensemble_time: B = {B} users, V = {V} news, D = {D}, T = {T} sub-models (weights {weights}), 1..5 clicks "
             f"per user ({n_clicks}), exclusion lists of 0..50 rows; {torch.cuda.get_device_name()} on {socket.gethostname()}; library "
             f"build id {_lib.load().nrl_build_id().decode()}; torch {torch.__version__}; warm-up {args.warmup}, {args.iters} "
             f"alternating repeats, device events, whole calls; the T (B, V) fp32 matrices {T * B * V * 4 / 2 ** 20:.0f} MiB; torch "
             f"compares in pieces of {args.piece} clicks"]

    def fused():
        return ops.catalogue_ensemble_ranks(users, tables, weights, tgt_idx, tgt_off, excl_idx, excl_off)

    def torch_ops():
        keep = torch.ones((B, V), dtype=torch.bool, device="cuda")
        keep[excl_user, excl_idx] = False
        n = keep.sum(dim=1, keepdim=True).float()
        total = None
        for U, Tb, w in zip(users, tables, weights):
            s = U @ Tb.T
            mean = (s * keep).sum(dim=1, keepdim=True) / n
            sd = (((s - mean) ** 2 * keep).sum(dim=1, keepdim=True) / (n - 1)).sqrt()
            z = w * ((s - mean) / sd)
            total = z if total is None else total + z
        total[~keep] = NEG_INF
        st = total[tgt_user, tgt_idx]                             # -inf: the click is on its user's exclusion list
        above = torch.empty_like(tgt_idx)
        for lo in range(0, n_clicks, args.piece):
            hi = min(lo + args.piece, n_clicks)
            own, s_t, t = total[tgt_user[lo:hi]], st[lo:hi, None], tgt_idx[lo:hi, None]
            above[lo:hi] = ((own > s_t) | ((own == s_t) & (rows[None, :] < t))).sum(dim=1)
        return torch.where(st == NEG_INF, torch.zeros_like(above), 1 + above).int(), st, keep.sum(dim=1).int()

    sides = [("fused", fused), ("torch", torch_ops)]
    for _ in range(args.warmup):
        for _, fn in sides:
            fn()
    times, peaks, outs = {n: [] for n, _ in sides}, {}, {}
    for it in range(args.iters):
        for name, fn in sides:
            ms, peak, out = timed(fn)
            times[name].append(ms)
            peaks[name] = max(peaks.get(name, 0), peak)
            outs[name] = out
        print(f"[{it + 1}/{args.iters}] fused {times['fused'][-1]:.2f} ms, torch {times['torch'][-1]:.2f} ms", file=sys.stderr, flush=True)
    med = {}
    for name, _ in sides:
        t = sorted(times[name])
        med[name] = t[len(t) // 2]
        lines.append(f"  {name:6s} median {med[name]:9.3f} ms  min {t[0]:9.3f}  max {t[-1]:9.3f}   peak allocated above the inputs "
                     f"{peaks[name] / 2 ** 20:9.2f} MiB")
    lines.append(f"  fused / torch time: {med['fused'] / med['torch']:.3f}   fused / torch peak memory: "
                 f"{peaks['fused'] / max(peaks['torch'], 1):.5f}")
    fr, fs, fn_, status, _ = outs["fused"]
    tr, ts, tn = outs["torch"]
    valid = (fr > 0) & (tr > 0)
    lines.append(f"  status word {int(status)}; {n_clicks} clicks, ranks equal for {int((fr == tr).sum())}, largest rank difference "
                 f"{int((fr - tr).abs().max())}, populations equal for {int((fn_ == tn).sum())} of {B} users, largest score difference "
                 f"{float((fs[valid] - ts[valid]).abs().max()):.3e}")
    report = "\n".join(lines)
    print(report)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(report + "\n")


if __name__ == "__main__":
    main()
