#!/usr/bin/env python3
"""Time the MINER head (category bias + poly attention + target-aware scores + disagreement loss, forward and backward) on the
library's kernels and as the same computation written in plain torch ops, on the same GPU in the same process.

    python tools/miner_head_time.py [--batch 128] [--hist 50] [--cand 5] [--reps 7] [--iters 50]

Shapes: miner.yaml widths (D = 256, K = 32, context_code_dim = 200, category dim 100); every user has ``--hist`` clicks and
``--cand`` candidates.  Method: both variants are warmed up, then timed alternately ``--reps`` times over ``--iters`` steps
each between device synchronisations (wall clock); the line reports the median and the min-max spread of the per-step times of
each and prints one JSON object."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from newsreclib_amd import ops_miner  # noqa: E402
from newsreclib_amd.user_encoder_miner import PolyAttention, TargetAwareAttention  # noqa: E402


def torch_head(hv, cv, hc, cc, enc, taa, B, H, C):
    """miner_module.py:261-323,398-406 in torch ops (dense history, masked (B, H, n_cand) bias, K x K cosine)."""
    hist, cand = hv.view(B, H, -1), cv.view(B, C, -1)
    hh = hc / torch.linalg.norm(hc, dim=1, keepdim=True)
    ch = cc / torch.linalg.norm(cc, dim=1, keepdim=True)
    bias = (hh @ ch.t()).view(B, H, B * C)
    own = (torch.arange(B * C, device=hv.device) // C).unsqueeze(0) == torch.arange(B, device=hv.device).unsqueeze(1)
    bias = bias.masked_fill(own.unsqueeze(1), 0)
    proj = torch.tanh(hist @ enc.linear.weight.t())
    w = proj @ enc.context_codes.t() + bias.mean(dim=2).unsqueeze(2)
    w = torch.softmax(w.permute(0, 2, 1), dim=2)          # (every history is full: no masked position)
    uv = w @ hist
    S = cand @ uv.permute(0, 2, 1)
    q = torch.nn.functional.gelu(uv @ taa.linear.weight.t())
    scores = (torch.softmax(cand @ q.permute(0, 2, 1), dim=2) * S).sum(dim=2)
    xn = uv / (1e-8 + torch.linalg.norm(uv, dim=2, keepdim=True))
    d = (xn @ xn.permute(0, 2, 1)).masked_fill(torch.eye(uv.shape[1], dtype=torch.bool, device=hv.device).unsqueeze(0), 0)
    return scores, d.mean()


def kernel_head(hv, cv, hc, cc, enc, taa, B, H, C, bh, bc, ho, co):
    bias = ops_miner.CategBiasFn.apply(hc, cc, bh, bc, ho, co, B)
    uv = enc(hv, ho, B, H, bias=bias)
    scores = taa(uv, cv, co, C)
    return scores, ops_miner.disagreement_loss(uv, False)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--hist", type=int, default=50)
    ap.add_argument("--cand", type=int, default=5)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50)
    a = ap.parse_args()
    B, H, C, D, K, Cd, Dc = a.batch, a.hist, a.cand, 256, 32, 200, 100
    dev = "cuda"
    torch.manual_seed(0)
    enc, taa = PolyAttention(D, K, Cd).to(dev), TargetAwareAttention(D).to(dev)
    leaves = [(torch.randn(B * H, D, device=dev) * 0.25).requires_grad_(True), (torch.randn(B * C, D, device=dev) * 0.25).requires_grad_(True),
              torch.randn(B * H, Dc, device=dev).requires_grad_(True), torch.randn(B * C, Dc, device=dev).requires_grad_(True)]
    bh = torch.arange(B, device=dev).repeat_interleave(H)
    bc = torch.arange(B, device=dev).repeat_interleave(C)
    ho, co = torch.arange(B + 1, device=dev) * H, torch.arange(B + 1, device=dev) * C
    d_scores = torch.randn(B, C, device=dev)
    params = list(enc.parameters()) + list(taa.parameters())

    def step(fn, *extra):
        for t in leaves + params:
            t.grad = None
        scores, dis = fn(*leaves, enc, taa, B, H, C, *extra)
        ((scores * d_scores).sum() + dis).backward()
        return scores

    variants = {"kernels": lambda: step(kernel_head, bh, bc, ho, co), "torch_ops": lambda: step(torch_head)}
    ref, got = variants["torch_ops"]().detach(), variants["kernels"]().detach()
    err = float((ref - got).abs().max())
    for fn in variants.values():
        for _ in range(10):
            fn()
    times = {k: [] for k in variants}
    for _ in range(a.reps):
        for name, fn in variants.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.iters):
                fn()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / a.iters * 1e3)
    out = {"shape": dict(B=B, H=H, C=C, D=D, K=K, Cd=Cd, Dc=Dc), "max_abs_score_diff": err, "device": torch.cuda.get_device_name(0)}
    for name, ts in times.items():
        out[name] = {"median_ms": round(statistics.median(ts), 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4)}
    out["torch_over_kernels"] = round(out["torch_ops"]["median_ms"] / out["kernels"]["median_ms"], 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
