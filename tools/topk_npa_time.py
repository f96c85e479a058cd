#!/usr/bin/env python3
"""Times the full-catalogue top-k by NPA's personalized-pooling score, in ONE process on one GPU, the sides alternating
(A, B, A, B, ...) after a shared warm-up, device-event timed (nothing is read back inside the timed region), median / min / max of
--iters whole calls:

* fused: ``ops.topk_pooled_scores`` (``nrl_topk_pooled_scores``: neither a (B, V, L) nor the (B, V, F) array is written);
* torch: the same result in torch ops from the same ``q``, ``user`` and feature maps, in pieces of --chunk table rows sized to fit
  memory: two GEMMs to (Vp, L, B), ``softmax`` over the tokens, the weighted sum, ``-inf`` written at the excluded positions of
  the piece (their positions are prepared outside the timed region), ``torch.topk``, and a merge of the running (B, k) lists over
  the pieces.

Shape: --users users, --news table rows, L = --tokens, F = --filters, k = --k, ragged exclusion lists of 0..50 rows per user.  Peak
allocated memory of each side is the allocator's high-water mark above the inputs.  The results are compared (torch orders its
sums differently, so rows may swap where scores are within rounding of each other; the report counts them).  The share of the
fp32-MFMA roof is 4 B V L F flops over --roof-tflops.  Whole calls only: no kernel is timed alone.  Needs a GPU: there is no CPU
path."""
import argparse
import os
import socket
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.topk_dnn_time import alternate  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--users", type=int, default=512)
    ap.add_argument("--news", type=int, default=65536)
    ap.add_argument("--tokens", type=int, default=30)
    ap.add_argument("--filters", type=int, default=400)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--chunk", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--roof-tflops", type=float, default=155.0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("topk_npa_time: no GPU; a time measured anywhere else says nothing about this path")
    from newsreclib_amd import _lib, ops
    B, V, L, F, k = args.users, args.news, args.tokens, args.filters, args.k
    g = torch.Generator(device="cuda").manual_seed(args.seed)
    feat = torch.relu(torch.randn(V, L, F, generator=g, device="cuda"))
    q = torch.tanh(0.25 * torch.randn(B, F, generator=g, device="cuda"))
    user = torch.randn(B, F, generator=g, device="cuda") / F ** 0.5
    hg = torch.Generator().manual_seed(args.seed)
    sizes = torch.randint(0, 51, (B,), generator=hg)
    excl_host = torch.randint(0, V, (int(sizes.sum()),), generator=hg)
    excl_user_host = torch.repeat_interleave(torch.arange(B), sizes)
    excl_idx = excl_host.cuda()
    excl_off = torch.cat([torch.zeros(1, dtype=torch.int64), sizes.cumsum(0)]).cuda()
    pieces = []                                             # (lo, hi, users, columns of the piece) of the excluded positions
    for lo in range(0, V, args.chunk):
        hi = min(lo + args.chunk, V)
        inside = (excl_host >= lo) & (excl_host < hi)
        pieces.append((lo, hi, excl_user_host[inside].cuda(), (excl_host[inside] - lo).cuda()))
    qT, uT = q.T.contiguous(), user.T.contiguous()

    def fused():
        return ops.topk_pooled_scores(q, user, feat, k, excl_idx, excl_off)

    def torch_ops():
        best_s = best_i = None
        for lo, hi, eu, ec in pieces:
            c = feat[lo:hi]
            w = torch.softmax(c @ qT, dim=1)                 # (Vp, L, B)
            s = (w * (c @ uT)).sum(dim=1).T.contiguous()    # (B, Vp)
            s[eu, ec] = float("-inf")
            ps, pi = torch.topk(s, min(k, hi - lo), dim=1)
            pi = pi + lo
            if best_s is not None:
                ps, pi = torch.cat([best_s, ps], dim=1), torch.cat([best_i, pi], dim=1)
                ps, sel = torch.topk(ps, min(k, ps.shape[1]), dim=1)
                pi = pi.gather(1, sel)
            best_s, best_i = ps, pi
        return best_i, best_s

    sides = [("fused", fused), ("torch", torch_ops)]
    times, peaks, outs = alternate(sides, args.warmup, args.iters)
    flops = 4.0 * B * V * L * F
    roof_ms = flops / (args.roof_tflops * 1e12) * 1e3
    lines = [f"topk_npa_time: B = {B} users, V = {V} news, L = {L}, F = {F}, k = {k}, exclusion lists of 0..50 rows; "
             f"{torch.cuda.get_device_name()} on {socket.gethostname()}; library build id {_lib.load().nrl_build_id().decode()}; "
             f"torch {torch.__version__}; warm-up {args.warmup}, {args.iters} alternating repeats, device events, whole calls",
             f"feature maps {V * L * F * 4 / 2 ** 30:.2f} GiB, one (B, V, L) fp32 tensor {B * V * L * 4 / 2 ** 30:.2f} GiB, "
             f"{flops / 1e12:.2f} TFLOP = {roof_ms:.2f} ms at {args.roof_tflops:.0f} TF (fp32 MFMA); torch in pieces of {args.chunk} rows"]
    med = {}
    for name, _ in sides:
        t = times[name]
        med[name] = t[len(t) // 2]
        lines.append(f"  {name:8s} median {med[name]:8.3f} ms  min {t[0]:8.3f}  max {t[-1]:8.3f}   {100.0 * roof_ms / med[name]:5.1f} % of the roof   "
                     f"peak allocated above the inputs {peaks[name] / 2 ** 20:9.2f} MiB")
    fi, fs, status = outs["fused"]
    ti, ts = outs["torch"]
    lines.append(f"  fused / torch time: {med['fused'] / med['torch']:.3f}   peak memory: {peaks['fused'] / max(peaks['torch'], 1):.5f}   "
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
