"""float64 restatement of the factored CAUM evaluation (``UserEncoder.score_ragged``), test infrastructure beside
``tests/caum_oracle.py``.

Without dropout the CAUM user encoder (user/caum.py:81-125) is linear everywhere except the attention softmax, the two tanh of
``DenseAttention`` and its final softmax, so it factors into a part per history row, a part per candidate row and the
across-users attention whose operands are sums of one row of each.  Weight blocks: linear1 = [W1l | W1c | W1r | W1k]
(D columns each), linear2 = [W2k | W2h], linear3 = [W3c (F columns) | W3a (U columns)], DenseAttention.linear = [Wdx (U columns)
| Wdk]; Win / bin / Wo / bo the attention's projections.  Pair (b, i) is flat candidate row p = cand_offsets[b] + i.

``factored_scores`` follows those formulas literally, in the dtype of its inputs (the tests hand it float64); it is compared
slot by slot with ``caum_oracle.user_encoder_slot`` in tests/test_caum_factored_host.py."""
from __future__ import annotations

from typing import Dict

import torch

from tests.caum_oracle import UE


def factored_scores(h: torch.Tensor, c: torch.Tensor, cand_offsets, params: Dict[str, torch.Tensor], heads: int) -> torch.Tensor:
    """h (B, H, D) dense zero-padded history, c (n, D) flat ragged candidate rows, cand_offsets (B + 1) -> scores (n,)."""
    B, H, D = h.shape
    offs = [int(v) for v in cand_offsets]
    sizes = [offs[b + 1] - offs[b] for b in range(B)]
    P = {k[len(UE):]: v.to(h.dtype) for k, v in params.items() if k.startswith(UE)}
    W1, b1, W2, b2, W3, b3 = (P[k] for k in ("linear1.weight", "linear1.bias", "linear2.weight", "linear2.bias",
                                             "linear3.weight", "linear3.bias"))
    F_, U = W1.shape[0], W2.shape[0]
    W1l, W1c, W1r, W1k = W1[:, :D], W1[:, D:2 * D], W1[:, 2 * D:3 * D], W1[:, 3 * D:]
    W2k, W2h = W2[:, :D], W2[:, D:]
    W3c, W3a = W3[:, :F_], W3[:, F_:]
    Wd, bd = P["dense_att.linear.weight"], P["dense_att.linear.bias"]
    Wdx, Wdk = Wd[:, :U], Wd[:, U:]
    W2d, b2d = P["dense_att.linear2.weight"], P["dense_att.linear2.bias"]
    w3d, b3d = P["dense_att.linear3.weight"].reshape(-1), P["dense_att.linear3.bias"]
    Win, bin_ = P["multihead_attention.in_proj_weight"], P["multihead_attention.in_proj_bias"]
    Wo, bo = P["multihead_attention.out_proj.weight"], P["multihead_attention.out_proj.bias"]
    dh = U // heads

    # user side, over the B * H history rows (neighbours circular over H)
    left, right = torch.roll(h, 1, dims=1), torch.roll(h, -1, dims=1)
    Pc = left @ W1l.t() + h @ W1c.t() + right @ W1r.t() + b1
    Ps = h @ W2h.t() + b2
    qkv_h = Ps @ Win.t() + bin_                                   # (B, H, 3U)
    Xh = Pc @ W3c.t() + b3 + W3a @ bo                             # (B, H, U)
    # candidate side, over the n candidate rows
    qkv_c = (c @ W2k.t()) @ Win.t()                               # no bias
    Xc = (c @ W1k.t()) @ W3c.t()
    g1 = c @ Wdk.t() + bd
    W3aWo = W3a @ Wo

    def heads_of(t):                                              # (..., U) -> (..., heads, dh)
        return t.reshape(*t.shape[:-1], heads, dh)

    scores = torch.zeros(c.shape[0], dtype=h.dtype)
    for i in range(max(sizes) if sizes else 0):
        # keys / values of slot i: every user, with its candidate row where it has one
        kv = qkv_h.clone()                                        # (B, H, 3U)
        for b in range(B):
            if i < sizes[b]:
                kv[b] = kv[b] + qkv_c[offs[b] + i]
        k, v = heads_of(kv[..., U:2 * U]), heads_of(kv[..., 2 * U:])          # (B', H, heads, dh)
        for b in range(B):
            if i >= sizes[b]:
                continue
            p = offs[b] + i
            q = heads_of(qkv_h[b, :, :U] + qkv_c[p, :U])                      # (H, heads, dh)
            s = torch.einsum("thd,bthd->thb", q, k) / dh ** 0.5               # softmax over the users b'
            o = torch.einsum("thb,bthd->thd", torch.softmax(s, dim=-1), v).reshape(H, U)
            x = Xh[b] + Xc[p] + o @ W3aWo.t()                                 # (H, U)
            z1 = torch.tanh(x @ Wdx.t() + g1[p])
            z2 = torch.tanh(z1 @ W2d.t() + b2d)
            alpha = torch.softmax(z2 @ w3d + b3d, dim=0)                      # over all H positions, padded ones included
            scores[p] = c[p] @ (alpha @ x)
    return scores
