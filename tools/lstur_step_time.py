#!/usr/bin/env python3
"""Times the LSTUR (BASELINE config 5), NAML (--model naml) NPA (--model npa: title only, 45,215 users), DKN
(--model dkn: title + title entities over 30,000 entities, 4 windows x 100 filters) or CAUM (--model caum: title, category
and title entities at the caum.yaml widths), MINER (--model miner: BASELINE configs[3] shape -- roberta-base-shaped random
body from tests/helpers.make_roberta, L = 96, layers 0-7 frozen, run it with --batch 8 -- at the miner.yaml widths) or, for the
same-box comparison with it, NRMS-PLM (--model nrms_plm: configs[3] itself) train step on one GPU: B users x 50 clicks, title 30 + abstract 50
tokens, CNN 300 filters x window 3, GRU 700.  Prints ms/step and impressions/s; with --breakdown also the
per-kernel time from torch.profiler-free HIP events around the module's stages."""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--vocab", type=int, default=70000)
    ap.add_argument("--engine", default="bf16x3")
    ap.add_argument("--model", default="lstur", choices=["lstur", "naml", "cen", "mins", "npa", "dkn", "caum", "miner", "nrms_plm", "sentidebias", "nrms"])
    args = ap.parse_args()
    from functools import partial

    from newsreclib_amd import _lib
    from newsreclib_amd.lstur_module import LSTURModule
    from newsreclib_amd.nrms_module import prepare_batch
    from newsreclib_amd.synthetic import add_lstur_fields, make_batch
    from newsreclib_amd.trainer import NRMSTrainer
    _lib.set_gemm_engine(args.engine)
    torch.manual_seed(0)
    if args.model in ("miner", "nrms_plm"):
        return plm_step(args)
    if args.model in ("sentidebias", "nrms"):
        return senti_step(args)
    emb = torch.randn(args.vocab, 300) * 0.3
    mod = LSTURModule(
        dataset_attributes=["title", "abstract", "category"], attributes2encode=["title", "abstract", "category"],
        outputs={"train": [], "val": [], "test": []}, dual_loss_training=False, dual_loss_coef=None,
        loss="cross_entropy_loss", late_fusion=False, temperature=None, use_plm=False,
        pretrained_embeddings_path=None, plm_model=None, frozen_layers=None, text_embed_dim=300, num_heads=15,
        num_filters=300, window_size=3, query_dim=200, categ_embed_dim=100, dropout_probability=0.2,
        num_users=45214, user_masking_probability=0.5, long_short_term_method="ini", top_k_list=[5, 10],
        num_categ_classes=18, num_sent_classes=3, save_recs=False, recs_fpath=None,
        optimizer=partial(torch.optim.Adam, lr=1e-4), scheduler=None, pretrained_embeddings=emb).cuda()
    if args.model == "naml":   # configs/model/naml.yaml: 400 filters, category view, add_att combination
        from newsreclib_amd.naml_module import NAMLModule
        mod = NAMLModule(
            dataset_attributes=["title", "abstract", "category"], attributes2encode=["title", "abstract", "category"],
            outputs={"train": [], "val": [], "test": []}, dual_loss_training=False, dual_loss_coef=None,
            loss="cross_entropy_loss", late_fusion=False, temperature=None, use_plm=False,
            pretrained_embeddings_path=None, plm_model=None, frozen_layers=None, text_embed_dim=300, num_heads=15,
            num_filters=400, window_size=3, query_dim=200, categ_embed_dim=100, dropout_probability=0.2,
            top_k_list=[5, 10], num_categ_classes=18, num_sent_classes=3, save_recs=False, recs_fpath=None,
            optimizer=partial(torch.optim.Adam, lr=1e-4), scheduler=None, pretrained_embeddings=emb).cuda()
    if args.model == "cen":    # configs/model/cen_news_rec.yaml: title only, 400 filters, 20 heads, GRU 400 over 20 recent
        from newsreclib_amd.cen_news_rec_module import CenNewsRecModule
        mod = CenNewsRecModule(
            dataset_attributes=["title", "abstract", "category"], attributes2encode=["title"],
            outputs={"train": [], "val": [], "test": []}, dual_loss_training=False, dual_loss_coef=None,
            loss="cross_entropy_loss", late_fusion=False, temperature=None, use_plm=False,
            pretrained_embeddings_path=None, plm_model=None, frozen_layers=None, embed_dim=300, num_heads=20,
            num_filters=400, window_size=3, query_dim=200, dropout_probability=0.2, gru_hidden_dim=400,
            num_recent_news=20, top_k_list=[5, 10], num_categ_classes=18, num_sent_classes=3, save_recs=False,
            recs_fpath=None, optimizer=partial(torch.optim.Adam, lr=1e-4), scheduler=None,
            pretrained_embeddings=emb).cuda()
    if args.model == "mins":   # configs/model/mins.yaml: MHSA text encoder on title + abstract, 6 GRU channels
        from newsreclib_amd.mins_module import MINSModule
        mod = MINSModule(
            dataset_attributes=["title", "abstract", "category"], attributes2encode=["title", "abstract", "category"],
            outputs={"train": [], "val": [], "test": []}, dual_loss_training=False, dual_loss_coef=None,
            loss="cross_entropy_loss", late_fusion=False, temperature=None, use_plm=False,
            pretrained_embeddings_path=None, plm_model=None, frozen_layers=None, text_embed_dim=300,
            categ_embed_dim=100, num_heads=15, query_dim=200, dropout_probability=0.2, num_filters=300,
            num_gru_channels=6, top_k_list=[5, 10], num_categ_classes=18, num_sent_classes=3, save_recs=False,
            recs_fpath=None, optimizer=partial(torch.optim.Adam, lr=1e-4), scheduler=None,
            pretrained_embeddings=emb).cuda()
    if args.model == "npa":    # configs/model/npa.yaml
        from newsreclib_amd.npa_module import NPAModule
        mod = NPAModule(
            outputs={"train": [], "val": [], "test": []}, dual_loss_training=False, dual_loss_coef=None,
            loss="cross_entropy_loss", late_fusion=False, temperature=None, pretrained_embeddings_path=None,
            text_embed_dim=300, user_embed_dim=50, num_users=45214, num_filters=400, window_size=3,
            word_pref_query_dim=200, news_pref_query_dim=200, dropout_probability=0.2, top_k_list=[5, 10],
            num_categ_classes=18, num_sent_classes=3, save_recs=False, recs_fpath=None,
            optimizer=partial(torch.optim.Adam, lr=1e-4), scheduler=None, pretrained_embeddings=emb).cuda()
    if args.model == "dkn":    # configs/model/dkn.yaml (use_context, windows 1-4 x 100 filters, entities 100-d)
        from newsreclib_amd.dkn_module import DKNModule
        mod = DKNModule(
            outputs={"train": [], "val": [], "test": []}, dual_loss_training=False, dual_loss_coef=None,
            loss="cross_entropy_loss", late_fusion=False, temperature=None, pretrained_word_embeddings_path=None,
            text_embed_dim=300, use_context=True, pretrained_entity_embeddings_path=None, entity_embed_dim=100,
            num_filters=100, window_sizes=[1, 2, 3, 4], hidden_dim_dnn=16, top_k_list=[5, 10], num_categ_classes=18,
            num_sent_classes=3, save_recs=False, recs_fpath=None, optimizer=partial(torch.optim.Adam, lr=1e-4),
            scheduler=None, pretrained_word_embeddings=emb, pretrained_entity_embeddings=torch.randn(30000, 100) * 0.3).cuda()
    if args.model == "caum":   # configs/model/caum.yaml: title 300 / 20 heads, category 100, title entities 100 / 20 heads
        from newsreclib_amd.caum_module import CAUMModule
        mod = CAUMModule(
            dataset_attributes=["title", "abstract", "category", "title_entities"],
            attributes2encode=["title", "category", "title_entities"], outputs={"train": [], "val": [], "test": []},
            dual_loss_training=False, dual_loss_coef=None, loss="cross_entropy_loss", late_fusion=False, temperature=None,
            use_plm=False, pretrained_word_embeddings_path=None, plm_model=None, frozen_layers=None, text_embed_dim=300,
            categ_embed_dim=100, use_entities=True, pretrained_entity_embeddings_path=None, entity_embed_dim=100,
            entity_num_heads=20, text_num_heads=20, news_embed_dim=400, query_dim=200, dropout_probability=0.2,
            user_vector_dim=400, num_filters=400, dense_att_hidden_dim1=400, dense_att_hidden_dim2=256, top_k_list=[5, 10],
            num_categ_classes=18, num_sent_classes=3, save_recs=False, recs_fpath=None,
            optimizer=partial(torch.optim.Adam, lr=1e-4), scheduler=None, pretrained_word_embeddings=emb,
            pretrained_entity_embeddings=torch.randn(30000, 100) * 0.3).cuda()
    trainer = NRMSTrainer(mod, lr=1e-4)
    batch = add_lstur_fields(make_batch(args.batch, vocab=args.vocab, mode="fixed", seed=1, device="cuda"), args.vocab,
                             19, 45215, 50, seed=2)
    if args.model in ("dkn", "caum"):
        from newsreclib_amd.synthetic import add_dkn_fields
        batch = add_dkn_fields(batch, n_entities=30000, seed=3)
    batch = prepare_batch(batch)
    for _ in range(args.warmup):
        trainer.step(batch)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        loss = trainer.step(batch)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / args.steps
    print(f"{args.model} B={args.batch} engine={args.engine}: {dt * 1e3:.3f} ms/step, {args.batch / dt:.1f} impressions/s, "
          f"loss={float(loss):.4f}")


def senti_step(args):
    """--model sentidebias: the two-optimizer SentiDebias step (configs/model/senti_debias.yaml: title, 300 / 15 heads / 200,
    discriminator 300-256-3) under ``SentiDebiasTrainer``; --model nrms: the NRMS step of the same shape under ``NRMSTrainer``,
    the same-box yardstick.  Median of per-step event times."""
    from functools import partial

    from newsreclib_amd.nrms_module import NRMSModule
    from newsreclib_amd.senti_debias_module import Discriminator, Generator, SentiDebiasModule, SentimentEncoder
    from newsreclib_amd.synthetic import make_batch
    from newsreclib_amd.trainer import NRMSTrainer, SentiDebiasTrainer
    emb = torch.randn(args.vocab, 300) * 0.3
    batch = make_batch(args.batch, vocab=args.vocab, mode="fixed", seed=1, device="cuda")
    g = torch.Generator().manual_seed(5)
    for part in ("x_hist", "x_cand"):
        batch[part]["sentiment"] = torch.randint(0, 4, (batch[part]["title"].shape[0],), generator=g).cuda()
    outputs = {"train": [], "val": [], "test": []}
    if args.model == "nrms":
        mod = NRMSModule(dataset_attributes=["title", "abstract", "category"], attributes2encode=["title"], outputs=outputs,
                         dual_loss_training=False, dual_loss_coef=None, loss="cross_entropy_loss", late_fusion=False,
                         temperature=None, use_plm=False, pretrained_embeddings_path=None, plm_model=None, frozen_layers=None,
                         embed_dim=300, num_heads=15, query_dim=200, dropout_probability=0.2, top_k_list=[5, 10],
                         num_categ_classes=18, num_sent_classes=3, save_recs=False, recs_fpath=None,
                         optimizer=partial(torch.optim.Adam, lr=1e-4), scheduler=None, pretrained_embeddings=emb).cuda()
        trainer = NRMSTrainer(mod, lr=1e-4)
    else:
        gen = Generator(dataset_attributes=["title", "abstract", "category", "sentiment"], attributes2encode=["title"],
                        late_fusion=False, use_plm=False, pretrained_embeddings_path=None, plm_model=None, frozen_layers=None,
                        embed_dim=300, num_heads=15, query_dim=200, dropout_probability=0.2,
                        sentiment_encoder=SentimentEncoder(3, 256, 300), pretrained_embeddings=emb)
        mod = SentiDebiasModule(outputs=outputs, generator=gen, discriminator=Discriminator(300, 256, 3), top_k_list=[5, 10],
                                num_categ_classes=18, num_sent_classes=3, save_recs=False, recs_fpath=None, optimizer=None,
                                alpha_coefficient=0.15, beta_coefficient=10.0,
                                optimizer_generator=partial(torch.optim.Adam, lr=1e-5),
                                optimizer_discriminator=partial(torch.optim.Adam, lr=2e-5), scheduler=None).cuda()
        trainer = SentiDebiasTrainer(mod)
    batch = mod._prepare(batch)
    for _ in range(args.warmup):
        trainer.step(batch)
    times = []
    for _ in range(args.steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        loss = trainer.step(batch)
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    times.sort()
    med = times[len(times) // 2]
    loss = loss if torch.is_tensor(loss) else loss[0]
    print(f"{args.model} B={args.batch} engine={args.engine}: median {med:.3f} ms/step [min {times[0]:.3f}, max {times[-1]:.3f}] "
          f"over {len(times)} steps, loss={float(loss):.4f}")


def plm_step(args):
    """MINER / NRMS-PLM at the BASELINE configs[3] shape: B users x 50 clicks + 5 candidates, titles of 96 tokens."""
    import statistics
    import tempfile
    from functools import partial

    from newsreclib_amd.nrms_module import prepare_batch
    from newsreclib_amd.synthetic import make_batch
    from newsreclib_amd.trainer import NRMSTrainer
    from tests.helpers import PLM_FULL_CFG, make_roberta
    path = make_roberta(tempfile.mkdtemp(), PLM_FULL_CFG, 41, 0.02)
    common = dict(dataset_attributes=["title", "abstract", "category"], attributes2encode=["title"],
                  outputs={"train": [], "val": [], "test": []}, dual_loss_training=False, dual_loss_coef=None,
                  loss="cross_entropy_loss", late_fusion=False, temperature=None, use_plm=True, plm_model=path,
                  frozen_layers=list(range(8)), dropout_probability=0.2, top_k_list=[5, 10], num_categ_classes=18,
                  num_sent_classes=3, save_recs=False, recs_fpath=None, optimizer=partial(torch.optim.Adam, lr=1e-5),
                  scheduler=None)
    if args.model == "miner":      # configs/model/miner.yaml
        from newsreclib_amd.miner_module import MINERModule
        mod = MINERModule(apply_reduce_dim=True, text_embed_dim=768, news_embed_dim=256, use_categ_bias=True,
                          pretrained_categ_embeddings_path=None, num_context_codes=32, context_code_dim=200,
                          score_type="weighted", pretrained_categ_embeddings=torch.randn(19, 300) * 0.3, **common).cuda()
    else:
        from newsreclib_amd.nrms_module import NRMSModule
        mod = NRMSModule(pretrained_embeddings_path=None, embed_dim=768, num_heads=16, query_dim=200, **common).cuda()
    trainer = NRMSTrainer(mod, lr=1e-5)
    b = make_batch(args.batch, vocab=50000, mode="fixed", seed=1, L=96, device="cuda")
    rng = torch.Generator().manual_seed(2)
    for part in ("x_hist", "x_cand"):          # tokenizer-style inputs (rec_dataset.py:180-190)
        ids = b[part]["title"].clamp_min(3)
        b[part]["title"] = {"input_ids": ids, "attention_mask": torch.ones_like(ids)}
        b[part]["category"] = torch.randint(1, 19, (ids.shape[0],), generator=rng).cuda()
    batch = prepare_batch(b)
    for _ in range(args.warmup):
        trainer.step(batch)
    times = []
    for _ in range(args.steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        loss = trainer.step(batch)
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    med = statistics.median(times)
    print(f"{args.model} B={args.batch} engine={args.engine}: median {med:.2f} ms/step [min {min(times):.2f}, max {max(times):.2f}] "
          f"over {args.steps} steps, {args.batch / med * 1e3:.1f} impressions/s, loss={float(loss):.4f}")


if __name__ == "__main__":
    main()
