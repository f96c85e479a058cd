#!/usr/bin/env python3
"""Times the SentiDebias head -- everything outside the news encoder, the user encoder and the scorer -- forward and backward for
both phases of the train step, as the kernels of ``ops_sentidebias`` and as the reference's formulation in torch ops on the same
tensors (per-row sentiment vectors through embedding -> linear -> tanh, dense sentiment matrices, two-layer discriminator, one-hot
cross entropy), and the shared user encoder over the news history and the sentiment history as two calls against one
(2B, H, D) call.  (The one call is timed only: the NRMS user encoder attends ACROSS the rows of a call, user/nrms.py:34-36, so
stacking the two histories couples them and changes the result.)  Event-timed, median of --iters after --warmup."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--hist", type=int, default=50)
    ap.add_argument("--cand", type=int, default=5)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--engine", default="bf16x3")
    args = ap.parse_args()
    from newsreclib_amd import _lib, ops_sentidebias as SD
    from newsreclib_amd.senti_debias_module import Discriminator, SentimentEncoder
    from newsreclib_amd.user_encoder import UserEncoder
    _lib.set_gemm_engine(args.engine)
    torch.manual_seed(0)
    B, H, C, D, S = args.batch, args.hist, args.cand, 300, 4
    nh, nc = B * H, B * C
    N = nh + nc
    dev = "cuda"
    enc, disc = SentimentEncoder(3, 256, D).to(dev), Discriminator(D, 256, 3).to(dev)
    news = torch.randn(N, D, device=dev, requires_grad=True)
    ids = torch.randint(0, S, (N,), device=dev)
    hoff, coff = torch.arange(B + 1, device=dev) * H, torch.arange(B + 1, device=dev) * C
    u_free = torch.randn(B, D, device=dev, requires_grad=True)
    free = torch.randn(B, C, device=dev, requires_grad=True)
    w_u = torch.randn(B, D, device=dev)           # stands in for the user encoder: a fixed linear read-out of the history mean
    params_g, params_d = list(enc.parameters()), list(disc.parameters())

    def flags(gen):
        for p in params_g:
            p.requires_grad_(gen)
        for p in params_d:
            p.requires_grad_(not gen)
        news.requires_grad_(gen)

    def clear():
        for t in params_g + params_d + [news, u_free, free]:
            t.grad = None

    def kernels_g():
        clear()
        T = enc.table()
        cos = SD.RowCosFn.apply(news, T, ids, nh)
        sent_hist = SD.SentHistFn.apply(T, ids[:nh], hoff, B, H)
        u_aware = sent_hist.mean(dim=1) * w_u
        comb = SD.CombinedScoresFn.apply(free, u_aware, T, ids[nh:], coff)
        adv = disc.losses(news, ids, nh)
        (cos.abs().sum() + comb.sum() - 0.15 * (adv[0] + adv[1])).backward()

    def torch_g():
        clear()
        sv = torch.tanh(enc.linear(enc.embedding_layer(ids)))                      # (N, D) sentiment vectors
        cosv = (news * sv).sum(-1) / (1e-8 + torch.linalg.norm(news, dim=1) * torch.linalg.norm(sv, dim=1))
        cos = torch.stack([cosv[:nh].mean(), cosv[nh:].mean()])
        sent_hist = sv[:nh].reshape(B, H, D)                                       # (full rows: the dense batch is a reshape)
        u_aware = sent_hist.mean(dim=1) * w_u
        comb = free + torch.bmm(u_aware.unsqueeze(1), sv[nh:].reshape(B, C, D).permute(0, 2, 1)).squeeze(1)
        adv = torch_adv()
        (cos.abs().sum() + comb.sum() - 0.15 * adv).backward()

    def torch_adv():
        out = 0.0
        for lo, hi in ((0, nh), (nh, N)):
            logits = disc.linear2(torch.tanh(disc.linear1(news[lo:hi])))
            y = torch.zeros_like(logits)
            y[torch.arange(hi - lo, device=dev), ids[lo:hi] - 1] = 1.0
            out = out + torch.nn.functional.cross_entropy(logits, y)
        return out

    def kernels_d():
        clear()
        adv = disc.losses(news, ids, nh)
        (adv[0] + adv[1]).backward()

    def torch_d():
        clear()
        torch_adv().backward()

    res = {}
    flags(True)
    res["phase G kernels"], res["phase G torch ops"] = timed(kernels_g, args.warmup, args.iters), timed(torch_g, args.warmup, args.iters)
    flags(False)
    res["phase D kernels"], res["phase D torch ops"] = timed(kernels_d, args.warmup, args.iters), timed(torch_d, args.warmup, args.iters)

    ue = UserEncoder(news_embed_dim=D, num_heads=15, query_dim=200).to(dev)
    a = torch.randn(B, H, D, device=dev, requires_grad=True)
    b = torch.randn(B, H, D, device=dev, requires_grad=True)

    def two_calls():
        for p in ue.parameters():
            p.grad = None
        (ue(a).sum() + ue(b).sum()).backward()

    def one_call():
        for p in ue.parameters():
            p.grad = None
        ue(torch.cat([a, b], dim=0)).sum().backward()

    res["user encoder, two (B, H, D) calls"] = timed(two_calls, args.warmup, args.iters)
    res["user encoder, one (2B, H, D) call"] = timed(one_call, args.warmup, args.iters)
    print(f"B={B} H={H} C={C} engine={args.engine}, fwd + bwd, ms: median [min, max]")
    for k, (med, lo, hi) in res.items():
        print(f"  {k:38s} {med:7.3f} [{lo:.3f}, {hi:.3f}]")


if __name__ == "__main__":
    main()
