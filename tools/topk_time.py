#!/usr/bin/env python3
"""Times the full-catalogue top-k two ways, in ONE process on one GPU, the two sides alternating (A, B, A, B, ...) after a shared
warm-up, device-event timed (nothing is read back inside the timed region), median / min / max of --iters:

* fused: ``ops.topk_scores`` (``nrl_topk_scores``: the (B, V) score matrix is never written);
* torch: the same result in torch ops -- ``user @ table.T``, ``-inf`` written at the excluded positions, ``torch.topk``.

Shape: --users users, --news table rows, D = 300 and 400, k = --k, ragged exclusion lists of 0..50 rows per user.  Peak allocated
memory of each side is the allocator's high-water mark above the inputs.  The two results are compared (the torch GEMM rounds
differently, so rows may swap where scores are within rounding of each other; the report counts them).  The roof is the exact-fp32
MFMA rate, 2 * B * V * D FLOP against 155 TF.  Needs a GPU: there is no CPU path to time."""
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
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--iters", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("topk_time: no GPU; a time measured anywhere else says nothing about this path")
    from newsreclib_amd import _lib, ops
    B, V, k = args.users, args.news, args.k
    lines = [f"topk_time: B = {B} users, V = {V} news, k = {k}, exclusion lists of 0..50 rows; {torch.cuda.get_device_name()} on "
             f"{socket.gethostname()}; library build id {_lib.load().nrl_build_id().decode()}; torch {torch.__version__}; "
             f"warm-up {args.warmup}, {args.iters} alternating repeats, device events"]
    for D in (300, 400):
        g = torch.Generator().manual_seed(args.seed + D)
        user, table = torch.randn(B, D, generator=g).cuda(), torch.randn(V, D, generator=g).cuda()
        sizes = torch.randint(0, 51, (B,), generator=g)
        excl_idx = torch.randint(0, V, (int(sizes.sum()),), generator=g).cuda()
        excl_off = torch.cat([torch.zeros(1, dtype=torch.int64), sizes.cumsum(0)]).cuda()
        excl_user = torch.repeat_interleave(torch.arange(B), sizes).cuda()

        def fused():
            return ops.topk_scores(user, table, k, excl_idx, excl_off)

        def torch_ops():
            s = user @ table.T
            s[excl_user, excl_idx] = float("-inf")
            score, idx = torch.topk(s, k, dim=1)
            return idx, score

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
        fi, fs, status = outs["fused"]
        ti, ts = outs["torch"]
        same = fi == ti
        lines.append(f"  status word {int(status)}; rows equal in {int(same.sum())} of {same.numel()} slots, same row sets for "
                     f"{int((fi.sort(1).values == ti.sort(1).values).all(1).sum())} of {B} users, largest score difference "
                     f"{float((fs - ts).abs().max()):.3e}")
    report = "\n".join(lines)
    print(report)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(report + "\n")


if __name__ == "__main__":
    main()
