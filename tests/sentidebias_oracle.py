"""float64 CPU restatement of the SentiDebias head (senti_debias_module.py:164-263,406-411,475-530; aspect.py SentimentEncoder) and
the portable parameters of its fixtures.  Two formulations of everything that touches a sentiment vector: ROW-WISE, as the reference
writes it (one (N, D) sentiment vector per news row, dense (B, H, D) / (B, C, D) sentiment matrices), and TABLE-GATHER, as the
kernels compute it (every vector a row of the (S, D) table); ``test_oracle_sentidebias`` checks one against the other and both
against the goldens."""
import numpy as np
import torch

D, SENT_EMB, HIDDEN, N_OUT, N_SENT = 300, 256, 256, 3, 4      # configs/model/senti_debias.yaml
COS_EPS = 1e-8

HEAD_SHAPES = {
    "generator.sentiment_encoder.embedding_layer.weight": (N_SENT, SENT_EMB),
    "generator.sentiment_encoder.linear.weight": (D, SENT_EMB),
    "generator.sentiment_encoder.linear.bias": (D,),
    "discriminator.linear1.weight": (HIDDEN, D),
    "discriminator.linear1.bias": (HIDDEN,),
    "discriminator.linear2.weight": (N_OUT, HIDDEN),
    "discriminator.linear2.bias": (N_OUT,),
}


def make_head_params(seed):
    """Sentiment encoder + discriminator parameters (reference state-dict keys), numpy ``default_rng`` draws in sorted key order.
    Row 0 of the embedding is zero (padding_idx); the bias is large enough that ``tanh(bias)`` is far from the zero vector."""
    rng = np.random.default_rng(seed)
    out = {}
    for key in sorted(HEAD_SHAPES):
        shape = HEAD_SHAPES[key]
        scale = 0.3 if key.endswith("bias") else (1.0 if "embedding" in key else 1.0 / np.sqrt(shape[-1]))
        out[key] = torch.from_numpy((scale * rng.standard_normal(shape)).astype(np.float32))
    out["generator.sentiment_encoder.embedding_layer.weight"][0] = 0.0
    return out


def make_params(vocab, nrms_seed, head_seed, late_fusion=False):
    from oracle.nrms_oracle import make_params as nrms_params
    out = {"generator." + k: v for k, v in nrms_params(vocab, D, 200, seed=nrms_seed).items()
           if not (late_fusion and k.startswith("user_encoder."))}
    out.update(make_head_params(head_seed))
    return out


def sentiment_table(p):
    E, W, b = (p["generator.sentiment_encoder." + k].double() for k in ("embedding_layer.weight", "linear.weight", "linear.bias"))
    return torch.tanh(E @ W.T + b)


def dense(x, sizes):
    """to_dense_batch: (sum sizes, ...) -> (B, max, ...) zero padded."""
    B, mx = len(sizes), int(max(sizes))
    out = x.new_zeros((B, mx) + tuple(x.shape[1:]))
    o = 0
    for b, n in enumerate(sizes):
        out[b, :n] = x[o:o + n]
        o += n
    return out


def cos_rows(a, b):
    return (a * b).sum(-1) / (COS_EPS + a.norm(dim=-1) * b.norm(dim=-1))


def wrapped_target(ids, n_out):
    """:409 writes the one-hot at column ``id - 1``: id 0 indexes column -1, the last one; an id above ``n_out`` raises."""
    if int(ids.max()) > n_out:
        raise IndexError("sentiment id above output_dim")
    return torch.where(ids == 0, torch.full_like(ids, n_out - 1), ids - 1)


def adversarial_loss(logits, ids):
    col = wrapped_target(ids, logits.shape[1])
    return -torch.log_softmax(logits, dim=1).gather(1, col.reshape(-1, 1)).mean()


def discriminator_losses(p, hist_vec, cand_vec, ids_h, ids_c):
    w1, b1, w2, b2 = (p["discriminator." + k].double() for k in ("linear1.weight", "linear1.bias", "linear2.weight", "linear2.bias"))
    f = lambda x: torch.tanh(x.double() @ w1.T + b1) @ w2.T + b2  # noqa: E731
    return adversarial_loss(f(hist_vec), ids_h), adversarial_loss(f(cand_vec), ids_c)


def head_rowwise(p, hist_vec, cand_vec, user_free, user_aware_fn, ids_h, ids_c, hist_sizes, cand_sizes, late_fusion):
    """The reference's formulation: per-row sentiment vectors and dense sentiment matrices.  ``user_aware_fn`` maps the dense
    (B, H, D) sentiment history to the bias-aware user vector (the shared user encoder; unused under late fusion)."""
    T = sentiment_table(p)
    hs, cs = T[ids_h], T[ids_c]                                   # (N, D) sentiment vectors
    hs_d, cs_d, cn_d = dense(hs, hist_sizes), dense(cs, cand_sizes), dense(cand_vec.double(), cand_sizes)
    n = torch.tensor(hist_sizes, dtype=torch.float64).unsqueeze(-1)
    user_aware = hs_d.sum(1) / n if late_fusion else user_aware_fn(hs_d)
    return _finish(hist_vec, cand_vec, hs, cs, user_free, user_aware, cn_d, torch.einsum("bd,bcd->bc", user_aware, cs_d))


def head_table(p, hist_vec, cand_vec, user_free, user_aware_fn, ids_h, ids_c, hist_sizes, cand_sizes, late_fusion):
    """The kernels' formulation: T[id] read in place, class fractions under late fusion, (B, S) products gathered by class."""
    T = sentiment_table(p)
    B, S = len(hist_sizes), T.shape[0]
    if late_fusion:
        frac = torch.zeros(B, S, dtype=torch.float64)
        o = 0
        for b, n in enumerate(hist_sizes):
            frac[b] = torch.bincount(ids_h[o:o + n], minlength=S).double() / n
            o += n
        user_aware = frac @ T
    else:
        hs_d = torch.zeros(B, int(max(hist_sizes)), T.shape[1], dtype=torch.float64)
        o = 0
        for b, n in enumerate(hist_sizes):
            hs_d[b, :n] = T[ids_h[o:o + n]]                       # padded slots stay ZERO (not T[0])
            o += n
        user_aware = user_aware_fn(hs_d)
    P = user_aware @ T.T                                          # (B, S)
    aware = torch.zeros(B, int(max(cand_sizes)), dtype=torch.float64)
    o = 0
    for b, n in enumerate(cand_sizes):
        aware[b, :n] = P[b, ids_c[o:o + n]]
        o += n
    cn_d = dense(cand_vec.double(), cand_sizes)
    return _finish(hist_vec, cand_vec, T[ids_h], T[ids_c], user_free, user_aware, cn_d, aware)


def _finish(hist_vec, cand_vec, hs, cs, user_free, user_aware, cand_dense, aware_scores):
    user_free = user_free.double()
    cos_h, cos_c = cos_rows(hist_vec.double(), hs).mean(), cos_rows(cand_vec.double(), cs).mean()
    cos_u = cos_rows(user_free, user_aware).unsqueeze(1)                     # (B, 1)
    loss_orth = (cos_h.abs() + cos_c.abs() + cos_u.abs()).mean()            # scalars broadcast onto (B, 1), :241-246
    free = torch.einsum("bd,bcd->bc", user_free, cand_dense)
    return dict(combined=free + aware_scores, bias_free=free, loss_orth=loss_orth, cos_hist=cos_h, cos_cand=cos_c,
                cos_user=cos_u.reshape(-1), user_aware=user_aware)


def cross_entropy(scores, y_true):
    """nn.CrossEntropyLoss with probability targets: mean over rows of -sum(y * log_softmax)."""
    return -(y_true.double() * torch.log_softmax(scores.double(), dim=1)).sum(1).mean()
