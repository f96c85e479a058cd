#!/usr/bin/env python3
"""Times the full-catalogue top-k by DKN's factored DNN click predictor, in ONE process on one GPU, the sides alternating
(A, B, C, A, B, C, ...) after a shared warm-up, device-event timed (nothing is read back inside the timed region), median / min /
max of --iters whole calls:

* fused: ``ops.topk_relu_scores`` (``nrl_topk_relu_scores``: neither (B, V) nor (B, V, Hd) is written);
* torch: the same result in torch ops from the same ``q`` and ``proj`` -- ``(relu(proj[None] + q[:, None]) * w2).sum(-1) + b2``,
  ``-inf`` written at the excluded positions, ``torch.topk`` -- with the (B, V, Hd) activations in one piece (the matrix-vector
  form of the second layer is refused by the BLAS library at B * V = 33.5 M rows, so this side multiplies and sums);
* torch/c: the activations in pieces of --chunk table rows, the second layer as ``relu(...) @ w2 + b2``, each piece written into
  its columns of one (B, V) matrix.

Shape: --users users, --news table rows, dim = --dim, Hd = 16 and 64, k = --k, ragged exclusion lists of 0..50 rows per user.
Peak allocated memory of each side is the allocator's high-water mark above the inputs.  The results are compared (torch rounds
the second layer differently, so rows may swap where scores are within rounding of each other; the report counts them).  The two
calls that feed the ranking are timed on their own: ``ops_dkn.dkn_cand_project`` (once per cache) and ``ops_dkn.dkn_user_query``
(once per batch, histories of 0..50 rows).  Whole calls only: no kernel is timed alone.  Needs a GPU: there is no CPU path."""
import argparse
import os
import socket
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


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


def alternate(sides, warmup, iters):
    for _ in range(warmup):
        for _, fn in sides:
            fn()
    times, peaks, outs = {n: [] for n, _ in sides}, {}, {}
    for _ in range(iters):
        for name, fn in sides:
            ms, peak, out = timed(fn)
            times[name].append(ms)
            peaks[name] = max(peaks.get(name, 0), peak)
            outs[name] = out
    return {n: sorted(t) for n, t in times.items()}, peaks, outs


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--users", type=int, default=512)
    ap.add_argument("--news", type=int, default=65536)
    ap.add_argument("--dim", type=int, default=400)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--chunk", type=int, default=1024)
    ap.add_argument("--iters", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("topk_dnn_time: no GPU; a time measured anywhere else says nothing about this path")
    from newsreclib_amd import _lib, ops, ops_dkn
    B, V, dim, k = args.users, args.news, args.dim, args.k
    lines = [f"topk_dnn_time: B = {B} users, V = {V} news, dim = {dim}, k = {k}, exclusion lists of 0..50 rows; "
             f"{torch.cuda.get_device_name()} on {socket.gethostname()}; library build id {_lib.load().nrl_build_id().decode()}; "
             f"torch {torch.__version__}; warm-up {args.warmup}, {args.iters} alternating repeats, device events, whole calls"]
    for Hd in (16, 64):
        g = torch.Generator().manual_seed(args.seed + Hd)

        def dnn():
            return [(torch.randn(Hd, 2 * dim, generator=g) / (2 * dim) ** 0.5).cuda(), (0.1 * torch.randn(Hd, generator=g)).cuda(),
                    (torch.randn(1, Hd, generator=g) / Hd ** 0.5).cuda(), (0.1 * torch.randn(1, generator=g)).cuda()]

        att, pred = dnn(), dnn()
        table = torch.randn(V, dim, generator=g).cuda()
        hsizes = torch.randint(0, 51, (B,), generator=g)
        hist = torch.randn(int(hsizes.sum()), dim, generator=g).cuda()
        hoff = torch.cat([torch.zeros(1, dtype=torch.int64), hsizes.cumsum(0)]).cuda()
        sizes = torch.randint(0, 51, (B,), generator=g)
        excl_idx = torch.randint(0, V, (int(sizes.sum()),), generator=g).cuda()
        excl_off = torch.cat([torch.zeros(1, dtype=torch.int64), sizes.cumsum(0)]).cuda()
        excl_user = torch.repeat_interleave(torch.arange(B), sizes).cuda()
        max_hist = int(hsizes.max())

        feed = [("project", lambda: ops_dkn.dkn_cand_project(table, pred)),
                ("query", lambda: ops_dkn.dkn_user_query(hist, hoff, max_hist, att, pred))]
        ft, _, fo = alternate(feed, args.warmup, args.iters)
        proj, (_, q) = fo["project"], fo["query"]
        w2, b2 = pred[2], pred[3]
        w2v = w2.reshape(-1)

        def fused():
            return ops.topk_relu_scores(q, proj, w2, b2, k, excl_idx, excl_off)

        def rank(s):
            s[excl_user, excl_idx] = float("-inf")
            score, idx = torch.topk(s, k, dim=1)
            return idx, score

        def torch_ops():
            return rank((torch.relu(proj[None, :, :] + q[:, None, :]) * w2v).sum(-1) + b2)

        def torch_chunked():
            s = torch.empty((B, V), dtype=torch.float32, device=q.device)
            for lo in range(0, V, args.chunk):
                s[:, lo:lo + args.chunk] = torch.relu(proj[None, lo:lo + args.chunk, :] + q[:, None, :]) @ w2v + b2
            return rank(s)

        sides = [("fused", fused), ("torch", torch_ops), ("torch/c", torch_chunked)]
        times, peaks, outs = alternate(sides, args.warmup, args.iters)
        lines.append(f"Hd = {Hd}: (B, V, Hd) activations {B * V * Hd * 4 / 2 ** 20:.1f} MiB, (B, V) scores {B * V * 4 / 2 ** 20:.1f} MiB, "
                     f"proj {V * Hd * 4 / 2 ** 20:.1f} MiB, {3.0 * B * V * Hd / 1e9:.2f} G add / select / fma; torch/c in pieces of "
                     f"{args.chunk} rows")
        lines.append(f"  feeding calls (not part of the ranking times): dkn_cand_project of the {V} x {dim} table median "
                     f"{ft['project'][len(ft['project']) // 2]:.3f} ms (once per cache), dkn_user_query of {B} users "
                     f"({int(hsizes.sum())} history rows) median {ft['query'][len(ft['query']) // 2]:.3f} ms")
        med = {}
        for name, _ in sides:
            t = times[name]
            med[name] = t[len(t) // 2]
            lines.append(f"  {name:8s} median {med[name]:8.3f} ms  min {t[0]:8.3f}  max {t[-1]:8.3f}   peak allocated above the inputs "
                         f"{peaks[name] / 2 ** 20:9.2f} MiB")
        fi, fs, status = outs["fused"]
        for name in ("torch", "torch/c"):
            ti, ts = outs[name]
            lines.append(f"  fused / {name} time: {med['fused'] / med[name]:.3f}   peak memory: {peaks['fused'] / max(peaks[name], 1):.5f}   "
                         f"rows equal in {int((fi == ti).sum())} of {fi.numel()} slots, same row sets for "
                         f"{int((fi.sort(1).values == ti.sort(1).values).all(1).sum())} of {B} users, largest score difference "
                         f"{float((fs - ts).abs().max()):.3e}")
        lines.append(f"  status word {int(status)}")
    report = "\n".join(lines)
    print(report)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(report + "\n")


if __name__ == "__main__":
    main()
