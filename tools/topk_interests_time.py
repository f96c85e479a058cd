#!/usr/bin/env python3
"""Times the multi-interest full-catalogue top-k two ways, in ONE process on one GPU, the two sides alternating (A, B, A, B, ...)
after a shared warm-up, device-event timed (nothing is read back inside the timed region), median / min / max of --iters:

* fused: ``ops.topk_interest_scores`` (``nrl_topk_interest_scores``: neither the (B, V) nor the (B K, V) matrix is written);
* torch: the same result in torch ops -- ``einsum`` to (B, K, V), the aggregate over K (max / mean / softmax-weighted by the gate
  logits, a second ``einsum``), ``-inf`` written at the excluded positions, ``torch.topk``; ``--user-chunk`` users at a time
  where the (B, K, V) matrices do not fit (0: all at once).

Shape: --users users of --interests interest vectors, --news table rows, D = --dim, k = --k, ragged exclusion lists of 0..50 rows
per user, every mode of --modes.  Peak allocated memory of each side is the allocator's high-water mark above the inputs.  The two
results are compared (the torch GEMM rounds differently, so rows may swap where scores are within rounding of each other; the
report counts them).  The roof is the exact-fp32 MFMA rate, 2 * B * K * V * D FLOP against 155 TF, twice that for "weighted"
(two products).  Needs a GPU: there is no CPU path to time."""
import argparse
import os
import socket
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.topk_time import ROOF_TFLOPS, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--users", type=int, default=512)
    ap.add_argument("--interests", type=int, default=32)
    ap.add_argument("--news", type=int, default=65536)
    ap.add_argument("--dim", type=int, default=256)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--modes", default="max,mean,weighted")
    ap.add_argument("--iters", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--user-chunk", type=int, default=0, help="users per step of the torch side (0: all at once)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None, help="also write the report to this file (appended: one run per mode is possible)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("topk_interests_time: no GPU; a time measured anywhere else says nothing about this path")
    from newsreclib_amd import _lib, ops
    B, K, V, D, k = args.users, args.interests, args.news, args.dim, args.k
    step = args.user_chunk or B
    lines = [f"topk_interests_time: B = {B} users x K = {K} interests, V = {V} news, D = {D}, k = {k}, exclusion lists of 0..50 rows; "
             f"{torch.cuda.get_device_name()} on {socket.gethostname()}; library build id {_lib.load().nrl_build_id().decode()}; "
             f"torch {torch.__version__}; warm-up {args.warmup}, {args.iters} alternating repeats, device events; torch side "
             f"{step} users at a time; (B K, V) matrix {B * K * V * 4 / 2 ** 30:.2f} GiB"]
    g = torch.Generator().manual_seed(args.seed + D)
    interests, table = torch.randn(B, K, D, generator=g).cuda(), torch.randn(V, D, generator=g).cuda()
    gate = (torch.randn(B, K, D, generator=g) * D ** -0.5).cuda()          # logits of order one: the weights are spread
    sizes = torch.randint(0, 51, (B,), generator=g)
    excl_idx = torch.randint(0, V, (int(sizes.sum()),), generator=g).cuda()
    excl_off = torch.cat([torch.zeros(1, dtype=torch.int64), sizes.cumsum(0)]).cuda()
    excl_user = torch.repeat_interleave(torch.arange(B), sizes).cuda()
    for mode in args.modes.split(","):

        def fused():
            return ops.topk_interest_scores(interests, table, k, mode, gate if mode == "weighted" else None, excl_idx, excl_off)

        def torch_ops():
            parts = []
            for lo in range(0, B, step):
                s = torch.einsum("bkd,vd->bkv", interests[lo:lo + step], table)
                if mode == "max":
                    s = s.max(dim=1).values
                elif mode == "mean":
                    s = s.mean(dim=1)
                else:
                    w = torch.softmax(torch.einsum("bkd,vd->bkv", gate[lo:lo + step], table), dim=1)
                    s = (w * s).sum(dim=1)
                parts.append(s)
            s = torch.cat(parts) if len(parts) > 1 else parts[0]
            s[excl_user, excl_idx] = float("-inf")
            score, idx = torch.topk(s, k, dim=1)
            return idx, score

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
            print(f"[{mode} {it + 1}/{args.iters}] fused {times['fused'][-1]:.1f} ms, torch {times['torch'][-1]:.1f} ms", file=sys.stderr,
                  flush=True)
        flop = 2.0 * B * K * V * D * (2 if mode == "weighted" else 1)
        block = [f"mode = {mode}: {flop / 1e12:.2f} TFLOP, roof {flop / ROOF_TFLOPS / 1e9:.1f} ms"]
        med = {}
        for name, _ in sides:
            t = sorted(times[name])
            med[name] = t[len(t) // 2]
            block.append(f"  {name:6s} median {med[name]:9.2f} ms  min {t[0]:9.2f}  max {t[-1]:9.2f}   {flop / med[name] / 1e9:7.1f} TFLOP/s = "
                         f"{100 * flop / med[name] / 1e9 / ROOF_TFLOPS:5.1f} % of the fp32-MFMA roof   peak allocated above the inputs "
                         f"{peaks[name] / 2 ** 20:9.2f} MiB")
        block.append(f"  fused / torch time: {med['fused'] / med['torch']:.3f}   fused / torch peak memory: "
                     f"{peaks['fused'] / max(peaks['torch'], 1):.5f}")
        fi, fs, status = outs["fused"]
        ti, ts = outs["torch"]
        block.append(f"  status word {int(status)}; rows equal in {int((fi == ti).sum())} of {fi.numel()} slots, same row sets for "
                     f"{int((fi.sort(1).values == ti.sort(1).values).all(1).sum())} of {B} users, largest score difference "
                     f"{float((fs - ts).abs().max()):.3e}")
        del outs, fi, fs, ti, ts
        lines += block
    report = "\n".join(lines)
    print(report)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(report + "\n")


if __name__ == "__main__":
    main()
