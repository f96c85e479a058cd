#!/usr/bin/env python3
"""NPA evaluation on one GPU: the module's ``torch.no_grad()`` forward (every batch re-runs the title CNN on all of its history
and candidate rows) against ``evaluation.NpaFeatureCache`` (conv feature maps of the corpus cached once, impressions scored from
them by ``nrl_npa_cached_scores``), on a MIND-dev-shaped synthetic set: 65 k unique news of 30 tokens, <= 50 clicks and 2..300
candidates per impression (the distributions of tools/eval_throughput.py), reference model sizes (D 300, F 400, U 50, P 200).

Device events around alternating windows of the two paths, over several distinct batches; prints impressions/s of both, the cache
build time, the scorer's kernel-pair time and its achieved bytes/s against the byte model (n_hist + n_cand) * L * F * 4, and the
largest score difference between the two paths.  One JSON line at the end."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _events(fn, iters):
    """ms per call of fn(i), device events around `iters` calls"""
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for i in range(iters):
        fn(i)
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--news", type=int, default=65000)
    ap.add_argument("--vocab", type=int, default=70000)
    ap.add_argument("--users", type=int, default=50000)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--batches", type=int, default=6, help="distinct batches the timed windows cycle through")
    ap.add_argument("--iters", type=int, default=24, help="calls per timed window")
    ap.add_argument("--rounds", type=int, default=3, help="alternating windows per path")
    ap.add_argument("--tokens", type=int, default=30)
    ap.add_argument("--filters", type=int, default=400)
    ap.add_argument("--embed", type=int, default=300)
    ap.add_argument("--engine", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this tool measures on the GPU; there is no CPU path"
    from functools import partial

    from newsreclib_amd import _lib, ops_npa
    from newsreclib_amd.evaluation import DeviceNewsTable
    from newsreclib_amd.npa_module import NPAModule
    from newsreclib_amd.nrms_module import prepare_batch
    from newsreclib_amd.synthetic import _titles
    if args.engine:
        _lib.set_gemm_engine(args.engine)
    rng = np.random.default_rng(0)
    torch.manual_seed(0)
    L, F_, B = args.tokens, args.filters, args.batch
    mod = NPAModule(
        outputs={"train": [], "val": [], "test": []}, dual_loss_training=False, dual_loss_coef=None, loss="cross_entropy_loss",
        late_fusion=False, temperature=None, pretrained_embeddings_path=None, text_embed_dim=args.embed, user_embed_dim=50,
        num_users=args.users, num_filters=F_, window_size=3, word_pref_query_dim=200, news_pref_query_dim=200,
        dropout_probability=0.2, top_k_list=[5, 10], num_categ_classes=18, num_sent_classes=3, save_recs=False, recs_fpath=None,
        optimizer=partial(torch.optim.Adam, lr=1e-4), scheduler=None,
        pretrained_embeddings=torch.randn(args.vocab, args.embed) * 0.3).cuda().eval()
    table = DeviceNewsTable({"title": torch.from_numpy(_titles(rng, args.news, args.vocab, L))})
    nb = args.batches
    data = []
    for _ in range(nb):
        hs = np.clip(np.rint(rng.lognormal(3.0, 0.8, B)), 1, 50).astype(np.int64)
        cs = np.clip(np.rint(rng.lognormal(3.3, 0.7, B)), 2, 300).astype(np.int64)
        d = dict(hist=torch.from_numpy(rng.integers(1, args.news, int(hs.sum()))).cuda(),
                 cand=torch.from_numpy(rng.integers(1, args.news, int(cs.sum()))).cuda(),
                 hs=torch.from_numpy(hs), cs=torch.from_numpy(cs), users=torch.from_numpy(rng.integers(1, args.users, B)).cuda())
        d["batch"] = prepare_batch(table.build_batch(d["hist"], d["hs"], d["cand"], d["cs"], torch.zeros(int(cs.sum())),
                                                     d["users"]), args.vocab)
        d["rows"] = int(hs.sum() + cs.sum())
        data.append(d)
    rows = float(np.mean([d["rows"] for d in data]))
    cache = mod.feature_cache(table)

    def build(_):
        cache.build()

    with torch.no_grad():
        build(0)                                             # warm-up (allocates the table once more than needed)
        t_build = min(_events(build, 1) for _ in range(2))
        fwd = lambda i: mod(data[i % nb]["batch"])           # noqa: E731  (the batch is built and prepared outside the window)
        sc = lambda i: cache.scores(data[i % nb]["hist"], data[i % nb]["hs"], data[i % nb]["cand"], data[i % nb]["cs"],  # noqa: E731
                                    data[i % nb]["users"])
        # the kernel pair alone: queries and offsets prepared outside the window
        prep = []
        for d in data:
            zero = torch.zeros(1, dtype=torch.int64, device="cuda")
            text_q, q_news = mod.user_queries(d["users"])
            prep.append((d["hist"], torch.cat([zero, d["hs"].cuda().cumsum(0)]), d["cand"], torch.cat([zero, d["cs"].cuda().cumsum(0)]),
                         text_q[:B], text_q[B:], q_news, int(d["hs"].max()), int(d["cs"].max())))
        kern = lambda i: ops_npa.npa_cached_scores(cache.features, *prep[i % nb])  # noqa: E731
        err = max(float((fwd(i) - sc(i)).abs().max()) for i in range(nb))        # also the warm-up of every shape
        for i in range(nb):
            kern(i)
        torch.cuda.synchronize()
        t_fwd, t_sc, t_k = [], [], []
        for _ in range(args.rounds):                         # alternate the paths: other work shares the host
            t_fwd.append(_events(fwd, args.iters))
            t_sc.append(_events(sc, args.iters))
            t_k.append(_events(kern, args.iters))
    bytes_model = rows * L * F_ * 4
    res = dict(engine=_lib.get_gemm_engine(), news=args.news, tokens=L, filters=F_, batch=B, rows_per_batch=rows,
               table_gb=cache.features.numel() * 4 / 1e9, build_ms=t_build,
               forward_ms=min(t_fwd), forward_ms_all=t_fwd, scores_ms=min(t_sc), scores_ms_all=t_sc, kernels_ms=min(t_k),
               kernels_ms_all=t_k, forward_impr_per_s=B / min(t_fwd) * 1e3, scores_impr_per_s=B / min(t_sc) * 1e3,
               model_bytes=bytes_model, kernels_tb_per_s=bytes_model / (min(t_k) * 1e-3) / 1e12, max_abs_diff=err)
    print(f"engine {res['engine']}; {args.news} news x {L} tokens x {F_} filters: table {res['table_gb']:.2f} GB, "
          f"build {t_build:.0f} ms; B = {B}, {rows:.0f} history + candidate rows per batch")
    print(f"module no_grad forward : {min(t_fwd):8.3f} ms/batch  {res['forward_impr_per_s']:10.0f} impressions/s")
    print(f"NpaFeatureCache.scores : {min(t_sc):8.3f} ms/batch  {res['scores_impr_per_s']:10.0f} impressions/s")
    print(f"  kernel pair alone    : {min(t_k):8.3f} ms/batch  {res['kernels_tb_per_s']:.2f} TB/s of the byte model "
          f"({bytes_model / 1e9:.2f} GB per batch)")
    print(f"max |forward - cached| over the {nb} batches: {err:.3e}")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
