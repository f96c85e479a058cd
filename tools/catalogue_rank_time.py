#!/usr/bin/env python3
"""Times the full-catalogue rank of held-out clicks two ways, in ONE process on one GPU, the two sides alternating (A, B, A, B,
...) after a shared warm-up, device-event timed (nothing is read back inside the timed region), median / min / max of --iters:

* fused: ``ops.catalogue_ranks`` (``nrl_catalogue_ranks``: the (B, V) score matrix is never written);
* torch: the same result in torch ops -- ``user @ table.T``, ``-inf`` written at the excluded positions, then per click
  ``(s > s_t) | (s == s_t & row < t)`` summed over the user's row.

Shape: --users users, --news table rows, D = 300 and 400, 1..5 clicks per user, ragged exclusion lists of 0..50 rows per user.
Peak allocated memory of each side is the allocator's high-water mark above the inputs.  The two results are compared (the torch
GEMM rounds differently, so a rank may move where scores are within rounding of each other; the report counts them).  The roof is
the exact-fp32 MFMA rate, 2 * B * V * D FLOP against 155 TF.  Needs a GPU: there is no CPU path to time."""
import argparse
import os
import socket
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ROOF_TFLOPS = 155.0


def timed(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), torch.cuda.max_memory_allocated() - base, out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--users", type=int, default=512)
    ap.add_argument("--news", type=int, default=65536)
    ap.add_argument("--iters", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("catalogue_rank_time: no GPU; a time measured anywhere else says nothing about this path")
    from newsreclib_amd import _lib, ops
    B, V = args.users, args.news
    lines = [f"catalogue_rank_time: B = {B} users, V = {V} news, 1..5 clicks per user, exclusion lists of 0..50 rows; {torch.cuda.get_device_name()} on "
             f"{socket.gethostname()}; library build id {_lib.load().nrl_build_id().decode()}; torch {torch.__version__}; "
             f"warm-up {args.warmup}, {args.iters} alternating repeats, device events"]
    for D in (300, 400):
        g = torch.Generator().manual_seed(args.seed + D)
        user, table = torch.randn(B, D, generator=g).cuda(), torch.randn(V, D, generator=g).cuda()
        sizes = torch.randint(0, 51, (B,), generator=g)
        excl_idx = torch.randint(0, V, (int(sizes.sum()),), generator=g).cuda()
        excl_off = torch.cat([torch.zeros(1, dtype=torch.int64), sizes.cumsum(0)]).cuda()
        excl_user = torch.repeat_interleave(torch.arange(B), sizes).cuda()

        clicks = torch.randint(1, 6, (B,), generator=g)
        tgt_idx = torch.randint(0, V, (int(clicks.sum()),), generator=g).cuda()
        tgt_off = torch.cat([torch.zeros(1, dtype=torch.int64), clicks.cumsum(0)]).cuda()
        tgt_user = torch.repeat_interleave(torch.arange(B), clicks).cuda()
        rows = torch.arange(V).cuda()

        def fused():
            return ops.catalogue_ranks(user, table, tgt_idx, tgt_off, excl_idx, excl_off)

        def torch_ops():
            s = user @ table.T
            s[excl_user, excl_idx] = float("-inf")
            st = s[tgt_user, tgt_idx]
            own = s[tgt_user]                           # (n_clicks, V): every click against its user's row
            above = (own > st[:, None]) | ((own == st[:, None]) & (rows[None, :] < tgt_idx[:, None]))
            rank = torch.where(st > float("-inf"), 1 + above.sum(1), torch.zeros_like(tgt_idx))
            return rank.int(), st, (s > float("-inf")).sum(1).int()

        sides = [("fused", fused), ("torch", torch_ops)]
        for _ in range(args.warmup):
            for _, fn in sides:
                fn()
        times, peaks, outs = {n: [] for n, _ in sides}, {}, {}
        for _ in range(args.iters):
            for name, fn in sides:
                ms, peak, out = timed(fn)
                times[name].append(ms)
                peaks[name] = max(peaks.get(name, 0), peak)
                outs[name] = out
        flop = 2.0 * B * V * D
        lines.append(f"D = {D}: score matrix {B * V * 4 / 2 ** 20:.1f} MiB, {flop / 1e9:.1f} GFLOP, roof {flop / ROOF_TFLOPS / 1e9:.3f} ms")
        med = {}
        for name, _ in sides:
            t = sorted(times[name])
            med[name] = t[len(t) // 2]
            lines.append(f"  {name:6s} median {med[name]:8.3f} ms  min {t[0]:8.3f}  max {t[-1]:8.3f}   {flop / med[name] / 1e9:7.1f} TFLOP/s = "
                         f"{100 * flop / med[name] / 1e9 / ROOF_TFLOPS:5.1f} % of the fp32-MFMA roof   peak allocated above the inputs "
                         f"{peaks[name] / 2 ** 20:8.2f} MiB")
        lines.append(f"  fused / torch time: {med['fused'] / med['torch']:.3f}   fused / torch peak memory: "
                     f"{peaks['fused'] / max(peaks['torch'], 1):.4f}")
        fr, fs, fn_, status = outs["fused"]
        tr, ts, tn = outs["torch"]
        valid = fr > 0
        lines.append(f"  status word {int(status)}; {int(clicks.sum())} clicks, ranks equal for {int((fr == tr).sum())}, largest rank "
                     f"difference {int((fr - tr).abs().max())}, populations equal for {int((fn_ == tn).sum())} of {B} users, largest "
                     f"score difference {float((fs[valid] - ts[valid]).abs().max()):.3e}")
    report = "\n".join(lines)
    print(report)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(report + "\n")


if __name__ == "__main__":
    main()
