#!/usr/bin/env python3
"""Times the two MANNeR kernels against the same computation built from what existed before, in ONE process on one GPU, the two
sides interleaved (A, B, A, B, ...) after a shared warm-up, event-timed, median / min / max of --iters:

* ``nrl_supcon_embed_fwd_bwd`` (loss + dE) at (85, 768) and (255, 768), T = 0.9, against the torch-op formulation of the same loss
  with autograd (Gram matrix, masks, masked logsumexp, reducer, backward);
* ``nrl_manner_scores`` at the MIND-like evaluation shape (B = 512 impressions, H <= 50, C from 2 to 300, V = 65 536, D = 768) for
  k = 1 and k = 3 tables, against the path built from existing pieces: per table two ``embedding_gather`` calls, dense batching,
  ``hist_mean``, ``dot_scores`` and a torch z-score over the real candidates.

* the ``AModule`` train step (forward, loss, backward, Adam) on one batch of 85 news and the ``CRModule`` train step on 8
  impressions (--hist clicks and --cand candidates each), both over a roberta-base-SHAPED body with random weights
  (tests/helpers.PLM_FULL_CFG), texts of 96 tokens, layers 0-7 frozen; these have no counterpart to compare with and are
  reported as they are (--steps 0 skips them)."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def interleaved(fns, warmup, iters):
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(iters):
        for i, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ts[i].append(a.elapsed_time(b))
    out = []
    for t in ts:
        t.sort()
        out.append((t[len(t) // 2], t[0], t[-1]))
    return out


def torch_supcon(E, labels, T):
    x = E.detach().requires_grad_(True)
    same = labels.unsqueeze(1) == labels.unsqueeze(0)
    eye = torch.eye(E.shape[0], dtype=torch.bool, device=E.device)
    pos = (same & ~eye).float()
    keep = ~eye
    mat = (x @ x.t()) / T
    mat = mat - mat.max(dim=1, keepdim=True)[0].detach()
    den = torch.logsumexp(mat.masked_fill(~keep, torch.finfo(mat.dtype).min), dim=1, keepdim=True)
    rows = -((pos * (mat - den)).sum(1) / (pos.sum(1) + torch.finfo(mat.dtype).tiny))
    kept = (rows > 0).float()
    loss = (rows * kept).sum() / kept.sum().clamp_min(1.0)          # (no host read-back either: the fair comparison)
    loss.backward()
    return loss, x.grad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--engine", default="bf16x3")
    ap.add_argument("--steps", type=int, default=10, help="timed train steps per module (0: skip)")
    ap.add_argument("--hist", type=int, default=50)
    ap.add_argument("--cand", type=int, default=5)
    args = ap.parse_args()
    from newsreclib_amd import _lib, ops
    from newsreclib_amd.dense_batch import dense_rows
    from newsreclib_amd.ops_manner import manner_scores, supcon_embed_fwd_bwd
    _lib.set_gemm_engine(args.engine)
    dev = "cuda"
    g = torch.Generator().manual_seed(1)
    print(f"engine {args.engine}; median / min / max ms over {args.iters} interleaved iterations")
    for N, classes in ((85, 17), (255, 17)):
        E = (torch.randn(N, 768, generator=g) * 0.11).to(dev)
        labels = (torch.arange(N) % classes).to(dev)
        k, t = interleaved([lambda: supcon_embed_fwd_bwd(E, labels, 0.9), lambda: torch_supcon(E, labels, 0.9)],
                           args.warmup, args.iters)
        print(f"supcon_embed N={N} D=768: kernel {k[0]:.4f} / {k[1]:.4f} / {k[2]:.4f}   torch ops {t[0]:.4f} / {t[1]:.4f} / {t[2]:.4f}")
    B, V, D = 512, 65536, 768
    hs = torch.randint(1, 51, (B,), generator=g)
    cs = torch.randint(2, 301, (B,), generator=g)
    cs[0] = 300
    hist_idx = torch.randint(0, V, (int(hs.sum()),), generator=g).to(dev)
    cand_idx = torch.randint(0, V, (int(cs.sum()),), generator=g).to(dev)
    z = torch.zeros(1, dtype=torch.int64)
    hist_off, cand_off = torch.cat([z, hs.cumsum(0)]).to(dev), torch.cat([z, cs.cumsum(0)]).to(dev)
    ar = torch.arange(B)
    bh, bc = torch.repeat_interleave(ar, hs).to(dev), torch.repeat_interleave(ar, cs).to(dev)
    max_h, max_c = int(hs.max()), int(cs.max())
    slot = (torch.arange(max_c).unsqueeze(0) < cs.unsqueeze(1)).to(dev)
    cs_d = cs.to(dev).float().unsqueeze(1)
    tables = [(torch.randn(V, D, generator=g) / D ** 0.5).to(dev) for _ in range(3)]
    weights = [1.0, -0.3, 0.25]

    def pieces(k):
        total = None
        for t in range(k):
            hv = ops.embedding_gather(tables[t], hist_idx.reshape(-1, 1)).reshape(-1, D)
            cv = ops.embedding_gather(tables[t], cand_idx.reshape(-1, 1)).reshape(-1, D)
            ha = dense_rows(hv, bh, B, max_h, hist_off, max_is_exact=True)
            ca = dense_rows(cv, bc, B, max_c, cand_off, max_is_exact=True)
            s = ops.DotScoresFn.apply(ops.HistMeanFn.apply(ha, hist_off), ca)
            mean = s.sum(1, keepdim=True) / cs_d
            var = (((s - mean) ** 2) * slot).sum(1, keepdim=True) / (cs_d - 1)
            zt = (s - mean) / var.sqrt()
            total = zt if t == 0 else total + weights[t] * zt
        return total

    with torch.no_grad():
        for k in (1, 3):
            a = manner_scores(tables[:k], weights[:k], hist_idx, hist_off, cand_idx, cand_off, max_c)
            b = pieces(k)
            diff = float(((a - b) * slot).abs().max())
            r = interleaved([lambda: manner_scores(tables[:k], weights[:k], hist_idx, hist_off, cand_idx, cand_off, max_c),
                             lambda: pieces(k)], args.warmup, args.iters)
            print(f"manner_scores k={k} B={B} rows {int(hs.sum())}+{int(cs.sum())}: kernel {r[0][0]:.4f} / {r[0][1]:.4f} / {r[0][2]:.4f}"
                  f"   existing pieces {r[1][0]:.4f} / {r[1][1]:.4f} / {r[1][2]:.4f}   (max difference {diff:.2e})")
    if args.steps > 0:
        train_steps(args)


def train_steps(args):
    import tempfile

    import numpy as np

    from newsreclib_amd.manner_a_module import AModule
    from newsreclib_amd.manner_cr_module import CRModule
    from newsreclib_amd.synthetic import make_news_batch
    from tests.helpers import PLM_FULL_CFG, make_roberta
    dev, n_ent, De = "cuda", 30_000, 256          # 16 heads: 768 / 16 = 48 and 256 / 16 = 16 are head widths the kernels have
    path = make_roberta(tempfile.mkdtemp(), PLM_FULL_CFG, 41, 0.02)
    ents = torch.randn(n_ent, De, generator=torch.Generator().manual_seed(2)) * 0.3
    common = dict(dataset_attributes=["title", "abstract", "title_entities", "abstract_entities"],
                  attributes2encode=["title", "abstract", "title_entities", "abstract_entities"], plm_model=path,
                  frozen_layers=list(range(8)), text_embed_dim=768, num_heads=16, query_dim=200, dropout_probability=0.2,
                  use_entities=True, pretrained_entity_embeddings_path="", entity_embed_dim=De, optimizer=None, scheduler=None,
                  pretrained_entity_embeddings=ents)

    def to_dev(nd):
        return {k: ({kk: vv.to(dev) for kk, vv in v.items()} if isinstance(v, dict) else v.to(dev)) for k, v in nd.items()}

    def run(mod, step_loss, what):
        opt = torch.optim.Adam([p for p in mod.parameters() if p.requires_grad], lr=1e-5)

        def step():
            opt.zero_grad(set_to_none=True)
            loss = step_loss()
            loss.backward()
            opt.step()
        for _ in range(3):
            step()
        torch.cuda.synchronize()
        ts = []
        for _ in range(args.steps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            step()
            b.record()
            torch.cuda.synchronize()
            ts.append(a.elapsed_time(b))
        ts.sort()
        print(f"{what}: train step {ts[len(ts) // 2]:.2f} / {ts[0]:.2f} / {ts[-1]:.2f} ms (median / min / max of {args.steps})")

    nb = make_news_batch(17, 5, n_entities=n_ent, L=96, seed=3)
    a_batch = {"news": to_dev(nb["news"]), "labels": nb["labels"].to(dev)}
    a_mod = AModule(outputs={"val": [], "test": []}, temperature=0.9, labels_path="", **common).to(dev).train()
    run(a_mod, lambda: a_mod.model_step(a_batch)[0], "AModule, 85 news x 96 tokens")
    del a_mod
    B, H, C = 8, args.hist, args.cand
    rng = np.random.default_rng(5)
    labels = torch.zeros(B * C)
    labels[torch.arange(B) * C + torch.from_numpy(rng.integers(0, C, B))] = 1.0
    ar = torch.arange(B)
    c_batch = {"x_hist": to_dev(make_news_batch(B * H, 1, n_entities=n_ent, L=96, seed=6)["news"]),
               "x_cand": to_dev(make_news_batch(B * C, 1, n_entities=n_ent, L=96, seed=7)["news"]),
               "batch_hist": torch.repeat_interleave(ar, H).to(dev), "batch_cand": torch.repeat_interleave(ar, C).to(dev),
               "labels": labels.to(dev), "user_ids": (ar + 1).to(dev), "user_idx": ar.to(dev), "batch_size": B}
    c_mod = CRModule(outputs={"train": [], "val": [], "test": []}, loss="sup_con_loss", late_fusion=False, temperature=0.36,
                     top_k_list=[5, 10], num_categ_classes=18, num_sent_classes=3, save_recs=False, recs_fpath=None,
                     **common).to(dev).train()
    run(c_mod, lambda: c_mod.model_step(c_batch)[0], f"CRModule, 8 impressions ({B * H} + {B * C} news x 96 tokens)")


if __name__ == "__main__":
    main()
