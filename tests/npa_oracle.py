"""CPU restatement of the reference NPA forward / loss (test infrastructure, beside the frozen ``oracle`` package).

``NPAModule.forward`` (npa_module.py:208-252): ``UserProjection`` (projection.py:35-50), ``CNNPersAtt`` twice
(text.py:376-392: embedding -> dropout -> Conv1d(padding=1) -> ReLU -> dropout -> personalized attention over ALL tokens),
NPA ``UserEncoder`` (user/npa.py:48-60) over the ``to_dense_batch`` history (zero rows up to the batch's longest history
take part in the softmax), dot-product scores, CE loss.  Dropout masks: the library's counter-based ones, streams as
include/newsreclib_amd.h fixes them (0: x, 1: c, 2: u, 3 / 4: history / candidate text query, 5: news query).
Pinned by tests/golden/make_golden_npa.py."""
from __future__ import annotations

from typing import Dict

import torch
import torch.nn.functional as F

from oracle.nrms_oracle import ce_loss, click_scores, dropout_multiplier, to_dense_batch

PRE = "news_encoder."
TEXT_PROJ = PRE + "text_query_projection.preference_query_projection."
TEXT_ATT = PRE + "personalized_attention.preference_query_projection."
NEWS_PROJ = "user_encoder.news_query_projection.preference_query_projection."
NEWS_ATT = "user_encoder.personalized_attention.preference_query_projection."
USER = "user_projection.user_embed"


def make_npa_params(vocab: int, num_users: int, D: int = 300, U: int = 50, F_: int = 400, W: int = 3, Pw: int = 200,
                    Pn: int = 200, late_fusion: bool = False, seed: int = 0) -> Dict[str, torch.Tensor]:
    """num_users = rows of the user table (the module's num_users + 1)."""
    g = torch.Generator().manual_seed(seed)

    def rnd(*shape, scale):
        return (torch.randn(*shape, generator=g) * scale).float()

    p = {
        USER: torch.rand(num_users, U, generator=g),
        PRE + "embedding_layer.weight": rnd(vocab, D, scale=0.3),
        PRE + "cnn.weight": rnd(F_, D, W, scale=(W * D) ** -0.5),
        PRE + "cnn.bias": rnd(F_, scale=0.05),
        TEXT_PROJ + "weight": rnd(Pw, U, scale=U ** -0.5),
        TEXT_PROJ + "bias": rnd(Pw, scale=0.05),
        TEXT_ATT + "weight": rnd(F_, Pw, scale=Pw ** -0.5),
        TEXT_ATT + "bias": rnd(F_, scale=0.05),
    }
    if not late_fusion:
        p.update({NEWS_PROJ + "weight": rnd(Pn, U, scale=U ** -0.5), NEWS_PROJ + "bias": rnd(Pn, scale=0.05),
                  NEWS_ATT + "weight": rnd(F_, Pn, scale=Pn ** -0.5), NEWS_ATT + "bias": rnd(F_, scale=0.05)})
    return p


def _query(u, params, proj, att, mask):
    h = torch.relu(u @ params[proj + "weight"].t() + params[proj + "bias"])
    if mask is not None:
        h = h * mask.to(h.dtype)
    return torch.tanh(h @ params[att + "weight"].t() + params[att + "bias"])


def _conv_features(ids, params, m1, m2):
    x = params[PRE + "embedding_layer.weight"][ids]
    if m1 is not None:
        x = x * m1.to(x.dtype)
    c = torch.relu(F.conv1d(x.permute(0, 2, 1), params[PRE + "cnn.weight"], params[PRE + "cnn.bias"], padding=1))
    c = c.permute(0, 2, 1)                                           # (N, L, F)
    return c * m2.to(c.dtype) if m2 is not None else c


def _pers_att(keys, q):
    """keys (N, S, F), q (N, F) -> (N, F): softmax over the whole S axis."""
    w = torch.softmax(torch.einsum("nsf,nf->ns", keys, q), dim=1)
    return torch.einsum("ns,nsf->nf", w, keys)


def npa_forward(batch, params, p_drop: float = 0.0, seed: int = 0, late_fusion: bool = False) -> dict:
    B = int(batch.get("batch_size", int(batch["batch_hist"].max()) + 1))
    ids_h, ids_c = batch["x_hist"]["title"], batch["x_cand"]["title"]
    nh, nc, L = ids_h.shape[0], ids_c.shape[0], ids_h.shape[1]
    table = params[USER]
    U, D = table.shape[1], params[PRE + "embedding_layer.weight"].shape[1]
    F_, Pw = params[TEXT_ATT + "weight"].shape
    m = dict(u=None, qh=None, qc=None, qn=None, x=None, c=None)
    if p_drop > 0.0:
        m["x"] = dropout_multiplier(seed, 0, p_drop, (nh + nc, L, D))
        m["c"] = dropout_multiplier(seed, 1, p_drop, (nh + nc, L, F_))
        m["u"] = dropout_multiplier(seed, 2, p_drop, (B, U))
        m["qh"] = dropout_multiplier(seed, 3, p_drop, (B, Pw))
        m["qc"] = dropout_multiplier(seed, 4, p_drop, (B, Pw))
        if not late_fusion:
            m["qn"] = dropout_multiplier(seed, 5, p_drop, (B, params[NEWS_PROJ + "weight"].shape[0]))
    u = table[batch["user_idx"]]
    if m["u"] is not None:
        u = u * m["u"].to(u.dtype)
    q_hist = _query(u, params, TEXT_PROJ, TEXT_ATT, m["qh"])
    q_cand = _query(u, params, TEXT_PROJ, TEXT_ATT, m["qc"])
    c = _conv_features(torch.cat([ids_h, ids_c]), params, m["x"], m["c"])
    hist_vec = _pers_att(c[:nh], q_hist[batch["batch_hist"]])
    cand_vec = _pers_att(c[nh:], q_cand[batch["batch_cand"]])
    hist_dense, mask_h = to_dense_batch(hist_vec, batch["batch_hist"], B)
    cand_dense, _ = to_dense_batch(cand_vec, batch["batch_cand"], B)
    if not late_fusion:
        user = _pers_att(hist_dense, _query(u, params, NEWS_PROJ, NEWS_ATT, m["qn"]))
    else:
        user = hist_dense.sum(dim=1) / mask_h.sum(dim=1, keepdim=True)
    scores = click_scores(user, cand_dense)
    y_true, _ = to_dense_batch(batch["labels"], batch["batch_cand"], B)
    return dict(hist_vec=hist_vec, cand_vec=cand_vec, user_vec=user, scores=scores, y_true=y_true,
                loss=ce_loss(scores, y_true))


def loss_and_grads(batch, params, **kw):
    leaves = {k: v.clone().requires_grad_(True) for k, v in params.items()}
    out = npa_forward(batch, leaves, **kw)
    grads = torch.autograd.grad(out["loss"], list(leaves.values()), allow_unused=True)
    g = {k: (gr if gr is not None else torch.zeros_like(leaves[k])) for k, gr in zip(leaves, grads)}
    g[PRE + "embedding_layer.weight"][0] = 0.0                       # padding_idx = 0
    return out, g


# ---- fixtures (tests/golden/npa_*.npz) --------------------------------------------------------------------------------
NPA_CASES = ["npa_tiny_eval", "npa_tiny_train", "npa16_train", "npa_tiny_late_fusion"]
MODULE_KEYS = ("vocab", "n_users", "D", "U", "F", "W", "Pw", "Pn")


def golden_cfg(g, prefix=""):
    cfg = {k: int(g[prefix + "cfg_" + k]) for k in MODULE_KEYS}
    cfg["param_seed"] = int(g["cfg_param_seed"])
    for k, conv in (("p_drop", float), ("seed", int), ("late_fusion", bool)):
        cfg[k] = conv(g["cfg_" + k]) if "cfg_" + k in g else conv(0)
    return cfg


def golden_params(cfg):
    return make_npa_params(cfg["vocab"], cfg["n_users"], cfg["D"], cfg["U"], cfg["F"], cfg["W"], cfg["Pw"], cfg["Pn"],
                           late_fusion=cfg["late_fusion"], seed=cfg["param_seed"])


def golden_batch(g, prefix="", device="cpu"):
    t = lambda a: torch.as_tensor(a).to(device)  # noqa: E731
    B = int(g[prefix + "in_batch_size"])
    return {"batch_hist": t(g[prefix + "in_batch_hist"]), "batch_cand": t(g[prefix + "in_batch_cand"]),
            "x_hist": {"title": t(g[prefix + "in_title_hist"])}, "x_cand": {"title": t(g[prefix + "in_title_cand"])},
            "labels": t(g[prefix + "in_labels"]), "user_idx": t(g[prefix + "in_user_idx"]),
            "user_ids": t(g[prefix + "in_user_idx"]) + 1, "batch_size": B}


def build_module(cfg, params, device="cuda", p_drop=None, **overrides):
    """NPAModule (the product) loaded from a reference-keyed state dict."""
    from newsreclib_amd.npa_module import NPAModule
    kw = dict(outputs={"train": ["preds", "targets", "cand_news_size"], "val": ["preds", "targets", "cand_news_size"],
                       "test": ["preds", "targets", "cand_news_size"]},
              dual_loss_training=False, dual_loss_coef=None, loss="cross_entropy_loss", late_fusion=cfg["late_fusion"],
              temperature=None, pretrained_embeddings_path=None, text_embed_dim=cfg["D"], user_embed_dim=cfg["U"],
              num_users=cfg["n_users"] - 1, num_filters=cfg["F"], window_size=cfg["W"], word_pref_query_dim=cfg["Pw"],
              news_pref_query_dim=cfg["Pn"], dropout_probability=0.2 if p_drop is None else p_drop, top_k_list=[5],
              num_categ_classes=18, num_sent_classes=3, save_recs=False, recs_fpath=None, optimizer=None,
              scheduler=None, pretrained_embeddings=params[PRE + "embedding_layer.weight"])
    kw.update(overrides)
    mod = NPAModule(**kw)
    res = mod.load_state_dict(params, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    return mod.to(device)
