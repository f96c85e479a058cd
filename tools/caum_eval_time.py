#!/usr/bin/env python3
"""CAUM evaluation on one GPU: ``NewsVectorCache.scores`` with ``CAUMModule.factored_eval`` off (the dense (B, max_cand) slot
block, 8 slots a pass) and on (``UserEncoder.score_ragged``: the real (user, candidate) pairs only), in ONE process on the same
seeded batch, at the caum.yaml widths (400 / 20 heads, 400 filters, DenseAttention 400 / 256).

Two shapes: B users with <= 50 clicks and MIND-dev-like candidate lists (log-normal, mean about 37, one list of 300 so that
max_cand = 300), and the same users with 5 candidates each, where padding buys nothing.  The cache holds --news random vectors:
the scorer's cost does not depend on their values and the news encoder is not what is measured.

Per shape and side: median of --samples single calls between device events, the two sides alternating after a shared warm-up;
peak device memory above what is allocated before the call; the largest score difference between the sides.  With --budgets
the factored side is also timed at other ``row_budget`` values (what the default was chosen from).  One JSON line at the end."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _one(fn):
    """-> (ms, peak bytes above the allocation before the call, result) of one call"""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    out = fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop), torch.cuda.max_memory_allocated() - base, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--news", type=int, default=65536)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--samples", type=int, default=15)
    ap.add_argument("--budgets", type=int, nargs="*", default=[])
    ap.add_argument("--engine", default=None)
    ap.add_argument("--factored-only", action="store_true",
                    help="three factored calls at the ragged shape and nothing else (for a kernel trace)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this tool measures on the GPU; there is no CPU path"
    from functools import partial

    from newsreclib_amd import _lib
    from newsreclib_amd.caum_module import CAUMModule
    from newsreclib_amd.evaluation import DeviceNewsTable, NewsVectorCache
    if args.engine:
        _lib.set_gemm_engine(args.engine)
    rng = np.random.default_rng(0)
    torch.manual_seed(0)
    B, V = args.batch, args.news
    mod = CAUMModule(
        dataset_attributes=["title", "abstract", "category", "title_entities"],
        attributes2encode=["title", "category", "title_entities"], outputs={"train": [], "val": [], "test": []},
        dual_loss_training=False, dual_loss_coef=None, loss="cross_entropy_loss", late_fusion=False, temperature=None,
        use_plm=False, pretrained_word_embeddings_path=None, plm_model=None, frozen_layers=None, text_embed_dim=300,
        categ_embed_dim=100, use_entities=True, pretrained_entity_embeddings_path=None, entity_embed_dim=100,
        entity_num_heads=20, text_num_heads=20, news_embed_dim=400, query_dim=200, dropout_probability=0.2,
        user_vector_dim=400, num_filters=400, dense_att_hidden_dim1=400, dense_att_hidden_dim2=256, top_k_list=[5, 10],
        num_categ_classes=18, num_sent_classes=3, save_recs=False, recs_fpath=None,
        optimizer=partial(torch.optim.Adam, lr=1e-4), scheduler=None, pretrained_word_embeddings=torch.randn(1000, 300) * 0.3,
        pretrained_entity_embeddings=torch.randn(1000, 100) * 0.3).cuda().eval()
    cache = NewsVectorCache(mod, DeviceNewsTable({"category": torch.zeros(V, dtype=torch.int64)}))
    cache.vectors = torch.randn(V, 400, device="cuda") * 0.1           # stand-ins for the cached news vectors

    hs = np.clip(np.rint(rng.lognormal(3.0, 0.8, B)), 1, 50).astype(np.int64)
    ragged = np.clip(np.rint(rng.lognormal(3.35, 0.7, B)), 2, 300).astype(np.int64)
    ragged[0] = 300
    shapes = {"ragged": ragged, "five": np.full(B, 5, dtype=np.int64)}
    hist = torch.from_numpy(rng.integers(1, V, int(hs.sum()))).cuda()
    res = dict(engine=_lib.get_gemm_engine(), batch=B, news=V, max_hist=int(hs.max()), default_row_budget=mod.user_encoder.row_budget)
    print(f"engine {res['engine']}; B = {B}, <= {int(hs.max())} clicks, {V} cached vectors x 400; median of {args.samples} "
          f"alternating calls after {args.warmup} warm-up calls a side; row_budget {mod.user_encoder.row_budget}")
    for name, cs in shapes.items():
        cand = torch.from_numpy(rng.integers(1, V, int(cs.sum()))).cuda()
        call = (hist, torch.from_numpy(hs), cand, torch.from_numpy(cs))

        def side(on, budget=None):
            mod.factored_eval = on
            if budget is not None:
                mod.user_encoder.row_budget = budget
            return cache.scores(*call)

        if args.factored_only:
            if name == "ragged":
                for _ in range(3):
                    side(True)
                torch.cuda.synchronize()
            continue
        for _ in range(args.warmup):
            side(False), side(True)
        t, peak, out = {False: [], True: []}, {}, {}
        for _ in range(args.samples):
            for on in (False, True):
                ms, pk, out[on] = _one(lambda: side(on))
                t[on].append(ms)
                peak[on] = max(peak.get(on, 0), pk)
        diff = float((out[True] - out[False]).abs().max())
        pairs, padded = int(cs.sum()), B * int(cs.max())
        r = dict(pairs=pairs, padded_slots=padded, max_cand=int(cs.max()), default_ms=statistics.median(t[False]),
                 factored_ms=statistics.median(t[True]), default_peak_gb=peak[False] / 1e9, factored_peak_gb=peak[True] / 1e9,
                 max_abs_diff=diff, scores_absmax=float(out[False].abs().max()), status=int(mod.factored_status))
        res[name] = r
        verdict = "" if r["factored_ms"] <= r["default_ms"] else "   **the factored path loses here**"
        print(f"{name}: {pairs} real pairs of {padded} padded slots (max_cand {r['max_cand']})")
        print(f"  factored_eval off : {r['default_ms']:10.2f} ms/batch   peak {r['default_peak_gb']:6.2f} GB above the inputs")
        print(f"  factored_eval on  : {r['factored_ms']:10.2f} ms/batch   peak {r['factored_peak_gb']:6.2f} GB above the inputs"
              f"   ({r['default_ms'] / r['factored_ms']:.2f}x){verdict}")
        print(f"  max |off - on| {diff:.3e} on scores of magnitude {r['scores_absmax']:.2f}; status {r['status']}")
        keep = mod.user_encoder.row_budget
        for budget in args.budgets:
            side(True, budget)
            runs = [_one(lambda: side(True, budget))[:2] for _ in range(5)]
            r[f"budget_{budget}"] = dict(ms=statistics.median(x[0] for x in runs), peak_gb=max(x[1] for x in runs) / 1e9)
            print(f"  row_budget {budget:8d}: {r[f'budget_{budget}']['ms']:10.2f} ms/batch   peak "
                  f"{r[f'budget_{budget}']['peak_gb']:6.2f} GB")
        mod.user_encoder.row_budget = keep
    print(json.dumps(res))


if __name__ == "__main__":
    main()
