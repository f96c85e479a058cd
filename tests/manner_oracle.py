"""CPU restatements for the MANNeR tests, in this project's own words (TEST INFRASTRUCTURE).

* ``supcon_embed``: pytorch-metric-learning 2.2.0 ``SupConLoss(temperature, DotProductSimilarity(normalize_embeddings=False))``
  called with embeddings and integer labels (manner_a_module.py:151-153,174): labels -> all pairs
  (``lmu.get_all_pairs_indices``: positives = equal labels off the diagonal, negatives = different labels) -> the masked loss of
  ``oracle/losses_oracle.py`` with the Gram matrix as the score matrix -> ``AvgNonZeroReducer``.  Runs in the dtype of its input
  (float64 reference, fp32 torch-op formulation) and is differentiable.
* ``ensemble_scores``: ``MANNERModule._submodel_forward`` + ``forward`` (manner_module.py:152-204) with per-impression loops.
"""
from __future__ import annotations

import torch


def label_pairs(labels: torch.Tensor):
    same = labels.unsqueeze(1) == labels.unsqueeze(0)
    diff = ~same
    same = same.clone()
    same.fill_diagonal_(False)
    a1, p = torch.where(same)
    a2, n = torch.where(diff)
    return a1, p, a2, n


def supcon_rows(E: torch.Tensor, labels: torch.Tensor, temperature: float):
    """-> per-row losses (N) or None in the "exactly zero" cases."""
    idx = label_pairs(labels)
    if all(len(x) <= 1 for x in idx):
        return None
    a1, p, a2, n = idx
    mat = E @ E.t()
    pos_mask, neg_mask = torch.zeros_like(mat), torch.zeros_like(mat)
    pos_mask[a1, p] = 1
    neg_mask[a2, n] = 1
    if not (pos_mask.bool().any() and neg_mask.bool().any()):
        return None
    mat = mat / temperature
    mat = mat - mat.max(dim=1, keepdim=True)[0].detach()
    keep = (pos_mask + neg_mask).bool()
    x = mat.masked_fill(~keep, torch.finfo(mat.dtype).min)
    den = torch.logsumexp(x, dim=1, keepdim=True).masked_fill(~keep.any(dim=1, keepdim=True), 0)
    log_prob = mat - den
    return -((pos_mask * log_prob).sum(dim=1) / (pos_mask.sum(dim=1) + torch.finfo(mat.dtype).tiny))


def supcon_embed(E: torch.Tensor, labels: torch.Tensor, temperature: float) -> torch.Tensor:
    rows = supcon_rows(E, labels, temperature)
    zero = E.sum() * 0
    if rows is None:
        return zero
    kept = rows > 0
    return rows[kept].mean() if int(kept.sum()) >= 1 else zero


def supcon_embed_with_grad(E: torch.Tensor, labels: torch.Tensor, temperature: float, dtype=torch.float64):
    x = E.detach().to(dtype).clone().requires_grad_(True)
    loss = supcon_embed(x, labels, temperature)
    loss.backward()
    return loss.detach(), x.grad.detach()


def submodel_scores(table: torch.Tensor, hist, cand) -> list:
    """z-scored scores of one sub-model: per impression a 1-D tensor over its own candidates."""
    out = []
    for h, c in zip(hist, cand):
        user = table[h].sum(dim=0) / len(h)
        s = table[c] @ user
        out.append((s - s.sum() / len(c)) / torch.std(s))
    return out


def ensemble_scores(tables, weights, hist, cand) -> list:
    total = None
    for t, (table, w) in enumerate(zip(tables, weights)):
        z = submodel_scores(table, hist, cand)
        total = z if t == 0 else [a + w * b for a, b in zip(total, z)]
    return total


# ---- inputs of the kernel checks (tests/test_gpu_manner.py, tests/sweep_inputs_sd_manner.py) --------------------------------------
def supcon_case(N, D, classes, T, seed=0, singleton=False):
    """Embeddings scaled so that the float64 row losses are exactly 0 or >= 1e-3 (the reducer's `> 0` test cannot flip within
    tolerance): seeds counted up from `seed + 1`, first hit.  ``singleton``: the last row gets a class of its own."""
    for s in range(seed + 1, seed + 50):
        g = torch.Generator().manual_seed(s)
        E = torch.randn(N, D, generator=g) * (0.6 * (T ** 0.5) / D ** 0.25)
        labels = torch.randint(0, classes, (N,), generator=g)
        if N <= classes * 2:
            labels = torch.arange(N) % classes
        if singleton:
            labels[N - 1] = classes
        rows = supcon_rows(E.double(), labels, T)
        if rows is not None and bool(((rows == 0) | (rows >= 1e-3)).all()) and bool((rows > 0).any()):
            return E, labels
    raise AssertionError("no seed satisfies the row-loss condition")


def random_tables(k, V, D, seed):
    """Unit-scale random news vectors.  Every multi-candidate impression must have std >= 1e-2 max|score| in every sub-model
    (asserted by the caller), else the z-score amplifies rounding."""
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(V, D, generator=g) / D ** 0.5 for _ in range(k)]


def min_std_ratio(tables, hist, cand, skip=()):
    """min over the sub-models and the impressions with several candidates (those in ``skip`` left out) of
    std / max|score| of the float64 raw scores."""
    worst = float("inf")
    for t in tables:
        t = t.double()
        for b, (h, c) in enumerate(zip(hist, cand)):
            if len(c) > 1 and b not in skip:
                s = t[c] @ (t[h].sum(0) / len(h))
                worst = min(worst, float(torch.std(s)) / float(s.abs().max()))
    return worst


# ---- fixtures shared by tests/golden/make_golden_manner.py and the tests ----------------------------------------------------------
TINY = dict(T=96, De=96, H=6, Q=32, n_ent=40, frozen=(0,))          # tests.helpers.make_tiny_roberta's width; heads of 16
NE = "news_encoder."
ENT = NE + "entity_encoders.entities."
SAMPLE_STRIDE = 13
ENS_WEIGHTS = ((0.0, 0.0), (-0.3, 0.0), (0.2, -0.25))
ENTITY_STREAM, CAND_STREAM_BASE = 6, 4          # news_encoder.ENTITY_STREAMS["entities"]; the candidate call's stream_base


def make_body(save_dir):
    """The tiny transformer body with its last LayerNorm scaled by 0.25 (tests/miner_oracle.make_body: the news vector is built
    from the raw CLS row, whose entries would otherwise be ~1 and push the scores out of the absolute bounds' range)."""
    from tests import miner_oracle
    return miner_oracle.make_body(save_dir, {"apply_reduce_dim": False})


def _block(prefix, D, Q, rnd):
    return {prefix + "multihead_attention.in_proj_weight": rnd(3 * D, D, scale=D ** -0.5),
            prefix + "multihead_attention.in_proj_bias": rnd(3 * D, scale=0.1),
            prefix + "multihead_attention.out_proj.weight": rnd(D, D, scale=D ** -0.5),
            prefix + "multihead_attention.out_proj.bias": rnd(D, scale=0.1),
            prefix + "additive_attention.linear.weight": rnd(Q, D, scale=D ** -0.5),
            prefix + "additive_attention.linear.bias": rnd(Q, scale=0.1),
            prefix + "additive_attention.query": rnd(Q, scale=0.5)}


def make_manner_params(seed: int, use_entities: bool = True, user_encoder: bool = False, cfg=TINY):
    """Every parameter outside the transformer body under the reference's state-dict keys, from one seed."""
    g = torch.Generator().manual_seed(seed)

    def rnd(*shape, scale):
        return (torch.randn(*shape, generator=g) * scale).float()

    T, De, Q = cfg["T"], cfg["De"], cfg["Q"]
    width = T + De if use_entities else T
    p = {NE + "combine_layer.weight": rnd(T, width, scale=width ** -0.5), NE + "combine_layer.bias": rnd(T, scale=0.1)}
    if use_entities:
        p[ENT + "embedding_layer.weight"] = rnd(cfg["n_ent"], De, scale=0.5)
        p.update(_block(ENT, De, Q, rnd))
    if user_encoder:
        p.update(_block("user_encoder.", T, Q, rnd))
    return p


def score_supcon_rows(scores, y_true, mask_cand, temperature=0.1):
    """Per-row losses of the score-matrix SupCon (oracle/losses_oracle.sup_con_loss before its reducer)."""
    from oracle.losses_oracle import indices_tuple, masked_logsumexp
    a1, p, a2, n = indices_tuple(y_true, mask_cand)
    pos_mask, neg_mask = torch.zeros_like(scores), torch.zeros_like(scores)
    pos_mask[a1, p] = 1
    neg_mask[a2, n] = 1
    mat = scores / temperature
    mat = mat - mat.max(dim=1, keepdim=True)[0]
    log_prob = mat - masked_logsumexp(mat, (pos_mask + neg_mask).bool())
    return -((pos_mask * log_prob).sum(dim=1) / (pos_mask.sum(dim=1) + torch.finfo(mat.dtype).tiny))


def dense_loops(x, batch, B):
    """``to_dense_batch`` with loops: (dense, mask)."""
    counts = [int((batch == b).sum()) for b in range(B)]
    mx = max(counts)
    dense = x.new_zeros((B, mx) + tuple(x.shape[1:]))
    mask = torch.zeros(B, mx, dtype=torch.bool)
    start = 0
    for b, c in enumerate(counts):
        dense[b, :c] = x[start:start + c]
        mask[b, :c] = True
        start += c
    return dense, mask


def cr_forward(news_encoder, user_encoder, click_predictor, batch):
    """``CRModule.forward`` (manner_cr_module.py:229-254) around given components; ``user_encoder`` None = late fusion."""
    B = batch["batch_size"]
    hist_vec = news_encoder(batch["x_hist"])
    hist_agg, mask_hist = dense_loops(hist_vec, batch["batch_hist"], B)
    cand_vec = news_encoder(batch["x_cand"])
    cand_agg, mask_cand = dense_loops(cand_vec, batch["batch_cand"], B)
    if user_encoder is not None:
        user_vector = user_encoder(hist_agg)
    else:
        hist_size = torch.tensor([int(mask_hist[i].sum()) for i in range(B)])
        user_vector = torch.div(hist_agg.sum(dim=1), hist_size.unsqueeze(dim=-1))
    scores = click_predictor(user_vector.unsqueeze(dim=1), cand_agg.permute(0, 2, 1))
    return scores, hist_vec, cand_vec, mask_cand


def cr_loss(scores, batch, mask_cand, loss: str):
    """``CRModule.model_step``'s loss (manner_cr_module.py:276-314); the SupCon temperature is the loss's default 0.1."""
    from oracle.losses_oracle import sup_con_loss
    y_true, _ = dense_loops(batch["labels"], batch["batch_cand"], batch["batch_size"])
    if loss == "cross_entropy_loss":
        return torch.nn.CrossEntropyLoss()(scores, y_true), y_true
    return sup_con_loss(scores, y_true, mask_cand, 0.1), y_true


def submodel_forward(news_encoder, click_predictor, batch):
    """``MANNERModule._submodel_forward`` (manner_module.py:152-188) around a given news encoder."""
    B = batch["batch_size"]
    hist_agg, mask_hist = dense_loops(news_encoder(batch["x_hist"]), batch["batch_hist"], B)
    cand_agg, mask_cand = dense_loops(news_encoder(batch["x_cand"]), batch["batch_cand"], B)
    hist_size = torch.tensor([int(mask_hist[i].sum()) for i in range(B)])
    user_vector = torch.div(hist_agg.sum(dim=1), hist_size.unsqueeze(dim=-1))
    scores = click_predictor(user_vector.unsqueeze(dim=1), cand_agg.permute(0, 2, 1))
    cand_size = torch.tensor([int(mask_cand[i].sum()) for i in range(B)])
    std_devs = torch.stack([torch.std(scores[i][mask_cand[i]]) for i in range(B)]).unsqueeze(-1)
    raw = scores
    scores = torch.div(scores - torch.div(torch.sum(scores, dim=1), cand_size).unsqueeze(-1).expand_as(scores), std_devs)
    return scores, raw, mask_cand


def entity_masks(seed, p, n, L, De, stream_base=0):
    """The two dropout multipliers of the entity encoder for one news-encoder call: on the embedded ids (n, L, De) and on the
    attention output, which the reference holds seq-first (L, n, De)."""
    from oracle.nrms_oracle import dropout_multiplier
    s = ENTITY_STREAM + stream_base
    return [dropout_multiplier(seed, s, p, (n, L, De)), dropout_multiplier(seed, s + 1, p, (n, L, De)).transpose(0, 1)]
