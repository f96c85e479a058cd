"""Model, table and batch builders that more than one test module uses.  A test module never imports from another test module:
what two of them need lives here (or in ``tests/helpers.py`` and the per-model ``*_oracle`` / ``*_helpers`` modules), so that
editing one test file cannot change what another builds or asserts.  The CPU reference of the full-catalogue contract is
``tests/catalogue_ref.py``, which imports nothing of the library; this module does."""
import json
import os

import numpy as np
import torch

from tests import miner_oracle as MO
from tests.helpers import (GOLDEN, PLM_HEADS, PLM_Q, build_cen_module, build_lstur_module, build_mins_module, build_module,
                           build_naml_module, build_sentirec_module, build_tanr_module, load_golden, make_tiny_roberta)


# ---- synthetic news tables, impressions and histories ----------------------------------------------------------------------------
def impressions(rng, n_imp, n_news, max_hist=12, max_cand=40):
    imps = []
    for i in range(n_imp):
        nh, nc = int(rng.integers(1, max_hist + 1)), int(rng.integers(2, max_cand + 1))
        lab = np.zeros(nc, dtype=np.float32)
        lab[rng.integers(0, nc)] = 1.0
        imps.append({"hist": torch.from_numpy(rng.integers(1, n_news, nh)), "cand": torch.from_numpy(rng.integers(1, n_news, nc)),
                     "labels": torch.from_numpy(lab), "user_idx": torch.tensor(i % 7)})
    return imps


def news_table(rng, n_news, vocab, L=30, n_categ=19):
    lens = rng.integers(3, L + 1, n_news)
    ids = rng.integers(1, vocab, (n_news, L))
    ids[np.arange(L)[None, :] >= lens[:, None]] = 0
    ids[0] = 0
    return {"title": torch.from_numpy(ids), "category": torch.from_numpy(rng.integers(1, n_categ, n_news)),
            "sentiment": torch.from_numpy(rng.integers(1, 4, n_news))}


def hist_batch(n_news, B=6, seed=3, full=False, sizes=None):
    rng = np.random.default_rng(seed)
    if sizes is None:
        sizes = np.full(B, 8) if full else rng.integers(1, 9, B)  # full: every history as long as the longest
    hist = [torch.from_numpy(rng.choice(np.arange(1, n_news), int(n), replace=False)) for n in sizes]
    return hist, torch.cat(hist), torch.tensor([len(h) for h in hist]), torch.arange(B) % 7


ATTRS = ["title", "abstract", "category", "sentiment_class"]


def make_frames(n_news=40, n_imp=23, seed=0):
    import pandas as pd
    rng = np.random.default_rng(seed)
    nids = [f"N{int(i)}" for i in rng.permutation(np.arange(1000, 1000 + n_news))]
    news = pd.DataFrame({
        "tokenized_title": [list(rng.integers(1, 500, rng.integers(0, 9))) for _ in nids],     # some empty, some > max
        "tokenized_abstract": [list(rng.integers(1, 500, rng.integers(1, 14))) for _ in nids],
        "category_class": rng.integers(0, 18, n_news), "subcategory_class": rng.integers(0, 200, n_news),
        "sentiment_class": rng.integers(0, 3, n_news), "sentiment_score": rng.random(n_news).astype(np.float32),
    }, index=nids)
    rows = []
    for i in range(n_imp):
        nc = int(rng.integers(2, 12))
        labels = np.zeros(nc, dtype=np.int64)
        labels[rng.choice(nc, int(rng.integers(1, max(2, nc // 3 + 1))), replace=False)] = 1
        if labels.all():
            labels[0] = 0
        rows.append({"uid": f"U{int(rng.integers(1, 99999))}", "user": int(rng.integers(0, 50)),
                     "history": list(rng.choice(nids, int(rng.integers(1, 9)))),
                     "candidates": list(rng.choice(nids, nc, replace=False)), "labels": list(labels)})
    return news, pd.DataFrame(rows)


def assert_batches_equal(a, b):
    assert set(a) >= {"batch_hist", "batch_cand", "x_hist", "x_cand", "labels", "user_ids", "user_idx"}
    for k in ("batch_hist", "batch_cand", "labels", "user_ids", "user_idx"):
        assert a[k].dtype == b[k].dtype and torch.equal(a[k].cpu(), b[k]), k
    for part in ("x_hist", "x_cand"):
        assert set(a[part]) == set(b[part]), (part, set(a[part]), set(b[part]))
        for k in b[part]:
            assert a[part][k].dtype == b[part][k].dtype and torch.equal(a[part][k].cpu(), b[part][k]), (part, k)


# ---- MANNeR ----------------------------------------------------------------------------------------------------------------------
MANNER_D, MANNER_DE, N_ENT = 96, 96, 40          # (entity heads of 96 / 6 = 16: a head width the attention kernels have)


def common_kwargs(plm_path, use_entities=True, p_drop=0.2):
    return dict(dataset_attributes=["title", "abstract", "title_entities", "abstract_entities", "category", "sentiment"],
                attributes2encode=["title", "abstract", "title_entities", "abstract_entities"] if use_entities
                else ["title", "abstract"],
                plm_model=plm_path, frozen_layers=[0], text_embed_dim=MANNER_D, num_heads=PLM_HEADS, query_dim=PLM_Q,
                dropout_probability=p_drop, use_entities=use_entities, pretrained_entity_embeddings_path="",
                entity_embed_dim=MANNER_DE, optimizer=None, scheduler=None)


def cr_kwargs(plm_path, loss="cross_entropy_loss", late_fusion=False, **kw):
    out = common_kwargs(plm_path, **kw)
    out.update(outputs={"train": ["preds", "targets", "cand_news_size"], "val": ["preds", "targets", "cand_news_size"],
                        "test": ["preds", "targets", "cand_news_size", "hist_news_size"]},
               loss=loss, late_fusion=late_fusion, temperature=0.36, top_k_list=[5, 10], num_categ_classes=18,
               num_sent_classes=3, save_recs=False, recs_fpath=None)
    return out


def a_kwargs(plm_path, temperature=0.9, **kw):
    out = common_kwargs(plm_path, **kw)
    out.update(outputs={"val": ["embeddings", "labels"], "test": ["embeddings", "labels"]}, temperature=temperature,
               labels_path="")
    return out


def entity_table(seed=3):
    return torch.randn(N_ENT, MANNER_DE, generator=torch.Generator().manual_seed(seed))


def manner_news(n, L, seed, use_entities=True):
    from newsreclib_amd.synthetic import make_news_batch
    b = make_news_batch(n, 1, vocab_size=200, n_entities=N_ENT, L=L, seed=seed, use_entities=use_entities)["news"]
    return {k: ({kk: vv.to("cuda") for kk, vv in v.items()} if isinstance(v, dict) else v.to("cuda")) for k, v in b.items()}


def manner_modules(tmp_path):
    from newsreclib_amd.manner_a_module import AModule
    from newsreclib_amd.manner_cr_module import CRModule
    plm = make_tiny_roberta(str(tmp_path))
    torch.manual_seed(11)
    cr = CRModule(**cr_kwargs(plm, late_fusion=True), pretrained_entity_embeddings=entity_table(1)).to("cuda").eval()
    ac = AModule(**a_kwargs(plm), pretrained_entity_embeddings=entity_table(2)).to("cuda").eval()
    asent = AModule(**a_kwargs(plm, use_entities=False)).to("cuda").eval()
    with torch.no_grad():                                    # three different encoders (the same tiny body otherwise)
        for i, m in enumerate((cr, ac, asent)):
            for p in m.news_encoder.combine_layer.parameters():
                p.copy_(torch.randn(p.shape, generator=torch.Generator().manual_seed(20 + i)).to("cuda") * 0.3)
    return cr, ac, asent


def manner_ensemble(cr, ac, asent, cw=0.2, sw=-0.25):
    from newsreclib_amd.manner_module import MANNERModule
    return MANNERModule.from_modules(cr, ac, asent, outputs={"test": ["preds", "targets", "cand_news_size"]}, categ_weight=cw,
                                     sent_weight=sw, top_k_list=[5, 10], num_categ_classes=4, num_sent_classes=3).eval()


def manner_table_and_impressions(n_news=40, seed=3):
    from newsreclib_amd.evaluation import DeviceNewsTable
    g = torch.Generator().manual_seed(seed)
    news = manner_news(n_news, 12, seed)
    attrs = dict(news, category=torch.randint(1, 5, (n_news,), generator=g), sentiment=torch.randint(1, 4, (n_news,), generator=g))
    imps = []
    for _ in range(9):
        h, c = int(torch.randint(1, 6, (1,), generator=g)), int(torch.randint(2, 8, (1,), generator=g))
        lab = torch.zeros(c)
        lab[int(torch.randint(0, c, (1,), generator=g))] = 1.0
        imps.append({"hist": torch.randint(0, n_news, (h,), generator=g), "cand": torch.randperm(n_news, generator=g)[:c],
                     "labels": lab})
    return DeviceNewsTable(attrs, device="cuda"), imps


# ---- tiny modules of every family, for the wiring tests --------------------------------------------------------------------------
def tiny(model, late_fusion=False, tmp_path=None, n_news=None):
    """(module in eval mode, table attributes or a DeviceNewsTable) from the synthetic builders of the existing GPU tests."""
    rng = np.random.default_rng(11)
    n_news, n_manner, vocab = n_news or 50, n_news or 40, 120      # (the MANNeR table builder's own default is 40)
    if model == "sentirec":
        from oracle import sentirec_oracle as SO
        g = load_golden("sentirec_tiny_eval")
        params = SO.make_sentirec_params(int(g["cfg_vocab"]), int(g["cfg_n_sent"]), seed=int(g["cfg_param_seed"]))
        attrs = news_table(rng, n_news, int(g["cfg_vocab"]), L=12, n_categ=7)
        return build_sentirec_module(g, params).eval(), {"title": attrs["title"]}
    if model == "manner_cr":
        from newsreclib_amd.manner_cr_module import CRModule
        torch.manual_seed(11)
        mod = CRModule(**cr_kwargs(make_tiny_roberta(str(tmp_path)), late_fusion=late_fusion),
                       pretrained_entity_embeddings=entity_table(1)).to("cuda").eval()
        return mod, manner_table_and_impressions(n_manner)[0]
    attrs = news_table(rng, n_news, vocab, L=12, n_categ=7)
    attrs["abstract"] = news_table(rng, n_news, vocab, L=20)["title"]
    if model == "nrms":
        from oracle import nrms_oracle as O
        mod = build_module(O.make_params(vocab, seed=8), late_fusion=late_fusion)
        attrs = {k: v for k, v in attrs.items() if k != "abstract"}
    elif model in ("lstur_ini", "lstur_con"):
        from oracle.lstur_oracle import make_lstur_params
        cfg = dict(vocab=vocab, n_categ=7, n_users=9, D=48, F=48, W=3, Q=32, categ_dim=16, text_attrs=("title", "abstract"),
                   text_order=("title", "abstract"), method=model[-3:], p_drop=0.2, p_mask=0.5)
        mod = build_lstur_module(cfg, make_lstur_params(vocab, 7, 9, 48, 48, 3, 32, 16, method=model[-3:], seed=5))
    elif model == "naml":
        from oracle.naml_oracle import make_naml_params
        cfg = dict(vocab=vocab, n_categ=7, D=48, F=48, W=3, Q=32, categ_dim=16, text_attrs=("title", "abstract"),
                   text_order=("title", "abstract"), p_drop=0.2)
        mod = build_naml_module(cfg, make_naml_params(vocab, 7, 48, 48, 3, 32, 16, seed=5))
    elif model == "tanr":
        from oracle.tanr_oracle import make_tanr_params
        cfg = dict(vocab=vocab, n_categ=7, D=48, F=48, W=3, Q=32, p_drop=0.2, coef=0.2)
        mod = build_tanr_module(cfg, make_tanr_params(vocab, 7, 48, 48, 3, 32, seed=5))
    elif model == "cen":
        from oracle.cen_news_rec_oracle import make_cen_news_rec_params
        cfg = dict(vocab=vocab, D=40, F=48, W=3, Q=32, heads=3, recent=3, p_drop=0.2, late_fusion=False)
        mod = build_cen_module(cfg, make_cen_news_rec_params(vocab, 40, 48, 3, 32, seed=5))
    elif model == "mins":
        from oracle.mins_oracle import make_mins_params
        cfg = dict(vocab=vocab, n_categ=7, D=48, Q=32, categ_dim=16, heads=3, channels=4,
                   text_attrs=("title", "abstract"), text_order=("title", "abstract"), p_drop=0.2)
        mod = build_mins_module(cfg, make_mins_params(vocab, 7, 48, 32, 16, 4, seed=5))
    else:
        raise AssertionError(model)
    return mod.eval(), attrs


def tiny_dkn(late_fusion=False, n_news=50, Hd=6):
    """(DKNModule in eval mode, table attributes) from the synthetic builders of the DKN tests: dim = 24."""
    from tests import dkn_oracle as DO
    cfg = dict(vocab=120, n_ent=30, D=16, Ed=8, F=8, Hd=Hd, windows=[1, 2, 3], use_context=True, late_fusion=late_fusion)
    params = DO.make_dkn_params(cfg["vocab"], cfg["n_ent"], cfg["D"], cfg["Ed"], cfg["F"], cfg["windows"], Hd,
                                use_context=True, late_fusion=late_fusion, seed=8)
    rng = np.random.default_rng(11)
    attrs = {"title": torch.from_numpy(rng.integers(1, cfg["vocab"], (n_news, 12))),
             "title_entities": torch.from_numpy(rng.integers(0, cfg["n_ent"], (n_news, 12)))}
    return DO.build_module(cfg, params).eval(), attrs


def tiny_npa(late_fusion=False, n_news=50, L=6, F_=8):
    """(NPAModule in eval mode, DeviceNewsTable) from the synthetic builders of the NPA tests."""
    from newsreclib_amd.evaluation import DeviceNewsTable
    from tests import npa_oracle as NO
    vocab, n_users = 60, 9
    cfg = dict(vocab=vocab, n_users=n_users, D=12, U=6, F=F_, W=3, Pw=8, Pn=8, late_fusion=late_fusion)
    params = NO.make_npa_params(vocab, n_users, 12, 6, F_, 3, 8, 8, late_fusion=late_fusion, seed=4)
    titles = torch.randint(1, vocab, (n_news, L), generator=torch.Generator().manual_seed(104))
    return NO.build_module(cfg, params).eval(), DeviceNewsTable({"title": titles})


def head_tols(engine):
    return (5e-5, 5e-4) if engine == "f32" else (1e-4, 1e-3)


def miner_golden_module(name, tmp_path, monkeypatch=None, **overrides):
    g = load_golden(name)
    cfg = MO.golden_cfg(g)
    over = dict(text_embed_dim=96) if name == "miner_head_full" else {}          # (the head fixture never runs the body)
    over.update(overrides)
    params = MO.golden_params(cfg)
    if name == "miner_head_full":
        params = {k: v for k, v in params.items() if not k.startswith(MO.TXT)}
        params.update({MO.TXT + "reduce_dim.weight": torch.zeros(cfg["Dn"], 96), MO.TXT + "reduce_dim.bias": torch.zeros(cfg["Dn"])})
    mod = MO.build_module(cfg, params, MO.make_body(str(tmp_path), cfg), **over)
    mod.train() if cfg["p_drop"] > 0 else mod.eval()
    mod.news_encoder.text_encoders["title"].plm_model.eval()
    if monkeypatch is not None:
        from newsreclib_amd import miner_module
        monkeypatch.setattr(miner_module, "_draw_seed", lambda: cfg["seed"])
    return g, cfg, mod


def miner_table_case(g):
    """One table row per history / candidate row of the fixture, both sides padded to one length."""
    batch = MO.golden_batch(g)
    L = max(batch["x_hist"]["title"]["input_ids"].shape[1], batch["x_cand"]["title"]["input_ids"].shape[1])

    def pad(t, value):
        return torch.nn.functional.pad(t, (0, L - t.shape[1]), value=value)

    title = {"input_ids": torch.cat([pad(batch["x_" + s]["title"]["input_ids"], 1) for s in ("hist", "cand")]),
             "attention_mask": torch.cat([pad(batch["x_" + s]["title"]["attention_mask"], 0) for s in ("hist", "cand")])}
    categ = torch.cat([batch["x_hist"]["category"], batch["x_cand"]["category"]])
    return batch, title, categ


def miner_cache(name, score_type, tmp_path):
    """(module, NewsVectorCache over one table row per history / candidate row of the fixture, host index lists)."""
    from newsreclib_amd.evaluation import DeviceNewsTable, NewsVectorCache
    if score_type is None:
        g, cfg, mod = miner_golden_module(name, tmp_path)
    else:              # (the fixture's parameters are drawn per score type: the module is built from its configuration)
        g = load_golden(name)
        cfg = dict(MO.golden_cfg(g), score_type=score_type)
        mod = MO.build_module(cfg, MO.golden_params(cfg), MO.make_body(str(tmp_path), cfg))
    batch, title, categ = miner_table_case(g)
    table = DeviceNewsTable({"title": title, "category": categ}, device="cuda")
    B = batch["batch_size"]
    nh = batch["batch_hist"].shape[0]
    hs = torch.bincount(batch["batch_hist"], minlength=B)
    return mod, cfg, NewsVectorCache(mod, table, chunk=5), torch.arange(nh), hs


def npa_contract():
    with open(os.path.join(GOLDEN, "npa_contract.json")) as f:
        return json.load(f)


def npa_contract_module(**over):
    c = npa_contract()["config"]
    cfg = dict(vocab=c["vocab"], n_users=c["num_users"] + 1, D=c["text_embed_dim"], U=c["user_embed_dim"],
               F=c["num_filters"], W=c["window_size"], Pw=c["word_pref_query_dim"], Pn=c["news_pref_query_dim"],
               late_fusion=False)
    from newsreclib_amd.npa_module import NPAModule
    kw = dict(outputs={"train": [], "val": [], "test": []}, dual_loss_training=False, dual_loss_coef=None,
              loss="cross_entropy_loss", late_fusion=False, temperature=None, pretrained_embeddings_path=None,
              text_embed_dim=cfg["D"], user_embed_dim=cfg["U"], num_users=c["num_users"], num_filters=cfg["F"],
              window_size=cfg["W"], word_pref_query_dim=cfg["Pw"], news_pref_query_dim=cfg["Pn"],
              dropout_probability=0.2, top_k_list=[5, 10], num_categ_classes=18, num_sent_classes=3, save_recs=False,
              recs_fpath=None, optimizer=None, scheduler=None,
              pretrained_embeddings=torch.zeros(cfg["vocab"], cfg["D"]))
    kw.update(over)
    return NPAModule(**kw)
