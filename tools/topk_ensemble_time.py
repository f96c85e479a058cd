#!/usr/bin/env python3
"""Times the z-scored ensemble full-catalogue top-k (MANNeR) two ways, in ONE process on one GPU, the two sides alternating
(A, B, A, B, ...) after a shared warm-up, device-event timed (nothing is read back inside the timed region), median / min / max
of --iters:

* fused: ``ops.topk_ensemble_scores`` (``nrl_topk_ensemble_scores``: a statistics pass and a scores pass over the tables, no
  (B, V) matrix is written);
* torch: the same result in torch ops -- one GEMM per sub-model to (B, V), the mean and ``std`` (unbiased) over the user's
  population through a mask, the weighted sum of the z-scores, ``-inf`` written at the excluded positions, ``torch.topk``.

Shape: --users users, --news table rows, D = --dim, T = --models sub-models with the weights 1.0, 0.2, -0.25, k = --k, ragged
exclusion lists of 0..50 rows per user.  Peak allocated memory of each side is the allocator's high-water mark above the inputs.
The two results are compared (the torch GEMM and its reductions round differently, so rows may swap where scores are within
rounding of each other; the report counts them).  The roof is the exact-fp32 MFMA rate over the two passes,
2 * T * 2 B V D FLOP against 155 TF.  Needs a GPU: there is no CPU path to time."""
import argparse
import os
import socket
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.topk_time import ROOF_TFLOPS, timed  # noqa: E402

WEIGHTS = (1.0, 0.2, -0.25)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--users", type=int, default=512)
    ap.add_argument("--news", type=int, default=65536)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--models", type=int, default=3)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--iters", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("topk_ensemble_time: no GPU; a time measured anywhere else says nothing about this path")
    from newsreclib_amd import _lib, ops
    B, V, D, T, k = args.users, args.news, args.dim, args.models, args.k
    weights = list(WEIGHTS[:T])
    lines = [f"topk_ensemble_time: B = {B} users, V = {V} news, D = {D}, T = {T} sub-models (weights {weights}), k = {k}, exclusion "
             f"lists of 0..50 rows; {torch.cuda.get_device_name()} on {socket.gethostname()}; library build id "
             f"{_lib.load().nrl_build_id().decode()}; torch {torch.__version__}; warm-up {args.warmup}, {args.iters} alternating "
             f"repeats, device events; the T (B, V) fp32 matrices {T * B * V * 4 / 2 ** 20:.0f} MiB"]
    g = torch.Generator().manual_seed(args.seed + D)
    users = [torch.randn(B, D, generator=g).cuda() for _ in range(T)]
    tables = [torch.randn(V, D, generator=g).cuda() for _ in range(T)]
    sizes = torch.randint(0, 51, (B,), generator=g)
    excl_idx = torch.randint(0, V, (int(sizes.sum()),), generator=g).cuda()
    excl_off = torch.cat([torch.zeros(1, dtype=torch.int64), sizes.cumsum(0)]).cuda()
    excl_user = torch.repeat_interleave(torch.arange(B), sizes).cuda()

    def fused():
        return ops.topk_ensemble_scores(users, tables, weights, k, excl_idx, excl_off)

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
        total[~keep] = float("-inf")
        score, idx = torch.topk(total, k, dim=1)
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
        print(f"[{it + 1}/{args.iters}] fused {times['fused'][-1]:.2f} ms, torch {times['torch'][-1]:.2f} ms", file=sys.stderr, flush=True)
    flop = 2.0 * T * 2.0 * B * V * D
    lines.append(f"two passes: {flop / 1e12:.3f} TFLOP, roof {flop / ROOF_TFLOPS / 1e9:.2f} ms (the torch side runs one pass: half of it)")
    med = {}
    for name, _ in sides:
        t = sorted(times[name])
        med[name] = t[len(t) // 2]
        lines.append(f"  {name:6s} median {med[name]:9.2f} ms  min {t[0]:9.2f}  max {t[-1]:9.2f}   roof / median = "
                     f"{100 * flop / med[name] / 1e9 / ROOF_TFLOPS:5.1f} % of the fp32-MFMA roof of the two passes   peak allocated above "
                     f"the inputs {peaks[name] / 2 ** 20:9.2f} MiB")
    lines.append(f"  fused / torch time: {med['fused'] / med['torch']:.3f}   fused / torch peak memory: "
                 f"{peaks['fused'] / max(peaks['torch'], 1):.5f}")
    fi, fs, status, _ = outs["fused"]
    ti, ts = outs["torch"]
    lines.append(f"  status word {int(status)}; rows equal in {int((fi == ti).sum())} of {fi.numel()} slots, same row sets for "
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
