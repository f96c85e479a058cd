"""CAUM user encoder (reference user/caum.py:10-125, layers/attention.py:169-209) on HIP kernels, every candidate slot in
one pass.  The module holds the parameters under the reference's keys (``linear1..3``, ``dense_att.linear/linear2/linear3``,
``multihead_attention.*``); ``forward`` runs them through ``ops_caum``.

The reference calls the encoder once per candidate slot (caum_module.py:342-344).  Here the slots are rows of one call:
r = (b, i, t) for user b, slot i, history position t.  ``linear1``, ``linear2`` and ``DenseAttention.linear`` split into a
history part, a candidate part and a bias:
  * training (fresh dropout masks per slot): the history part runs over the B * C * H per-slot dropped-out rows;
  * evaluation (no dropout): once over the B * H rows, shared by every slot; the candidate part runs once per (b, i).
The neighbours of the candi-CNN come from the circular shift of the dense, zero-padded history, as in the reference.  The
seq-first ``nn.MultiheadAttention`` attends ACROSS THE USERS of the batch for every (slot, history position); padded history
rows and padded candidate slots take part, as in the reference.  Evaluation runs the slots in chunks of ``slot_chunk``
(exact: the attention couples users within a slot, never slots).  ``score_ragged`` is the evaluation without the padded
slots: the same computation factored so that only the real (user, candidate) pairs are visited."""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn as nn

from . import ops_caum
from .ops_blocks import LinearActFn, LinearFn


class DenseAttention(nn.Module):
    """Parameter container of the reference's ``DenseAttention`` (Linear -> tanh -> Linear -> tanh -> Linear)."""

    def __init__(self, input_dim: int, hidden_dim1: int, hidden_dim2: int) -> None:
        super().__init__()
        for name, v in (("input_dim", input_dim), ("hidden_dim1", hidden_dim1), ("hidden_dim2", hidden_dim2)):
            if not isinstance(v, int):
                raise ValueError(f"Expected keyword argument `{name}` to be an `int` but got {v}")
        self.linear = nn.Linear(input_dim, hidden_dim1)
        self.tanh1 = nn.Tanh()
        self.linear2 = nn.Linear(hidden_dim1, hidden_dim2)
        self.tanh2 = nn.Tanh()
        self.linear3 = nn.Linear(hidden_dim2, 1)


def _zeros(n: int, like: torch.Tensor) -> torch.Tensor:
    return torch.zeros(n, dtype=torch.float32, device=like.device)


class UserEncoder(nn.Module):
    slot_chunk = 8          # candidate slots per evaluation pass (None: all at once)

    def __init__(self, news_embed_dim: int, num_filters: int, dense_att_hidden_dim1: int, dense_att_hidden_dim2: int,
                 user_vector_dim: int, num_heads: int, dropout_probability: float) -> None:
        super().__init__()
        if not isinstance(news_embed_dim, int):
            raise ValueError(f"Expected keyword argument `news_embed_dim` to be an `int` but got {news_embed_dim}")
        if not isinstance(num_filters, int):
            raise ValueError(f"Expected keyword argument `num_filters` to be an `int` but got {num_filters}")
        if not isinstance(dropout_probability, float):
            raise ValueError(
                f"Expected keyword argument `dropout_probability` to be a `float` but got {dropout_probability}")
        if news_embed_dim != user_vector_dim:
            # DenseAttention takes 2 * user_vector_dim but receives [user_vector_dim, news_embed_dim] (user/caum.py:116)
            raise ValueError("CAUM needs news_embed_dim == user_vector_dim (the reference's DenseAttention input width)")
        for name, v in (("news_embed_dim", news_embed_dim), ("num_filters", num_filters),
                        ("dense_att_hidden_dim1", dense_att_hidden_dim1), ("dense_att_hidden_dim2", dense_att_hidden_dim2)):
            if v % 4:
                raise NotImplementedError(f"the CAUM kernels take {name} as a multiple of 4 (got {v})")
        self.dropout1 = nn.Dropout(p=dropout_probability)     # hold p; the kernels draw the masks
        self.dropout2 = nn.Dropout(p=dropout_probability)
        self.dropout3 = nn.Dropout(p=dropout_probability)
        self.linear1 = nn.Linear(in_features=news_embed_dim * 4, out_features=num_filters)
        self.linear2 = nn.Linear(in_features=news_embed_dim * 2, out_features=user_vector_dim)
        self.linear3 = nn.Linear(in_features=num_filters + user_vector_dim, out_features=user_vector_dim)
        self.dense_att = DenseAttention(input_dim=user_vector_dim * 2, hidden_dim1=dense_att_hidden_dim1,
                                        hidden_dim2=dense_att_hidden_dim2)
        self.multihead_attention = nn.MultiheadAttention(embed_dim=user_vector_dim, num_heads=num_heads)
        self.num_heads = num_heads
        ops_caum.padded_attention_params(self.multihead_attention, num_heads)     # raises on a head dim beyond 64

    def forward(self, hist: torch.Tensor, cand: torch.Tensor, cand_offsets: torch.Tensor, seed: int = 0,
                slot_chunk: Optional[int] = -1) -> torch.Tensor:
        """hist (B, H, D) dense zero-padded history, cand (B, C, D) dense candidates, cand_offsets (B + 1) -> scores (B, C),
        exactly 0 at padded slots.  ``seed``: the step's dropout seed (streams: ``ops_caum``)."""
        p = float(self.dropout1.p) if self.training else 0.0
        C = cand.shape[1]
        chunk = self.slot_chunk if slot_chunk == -1 else slot_chunk
        if p > 0.0 or chunk is None or chunk >= C:
            return self._slots(hist, cand, cand_offsets, p, seed, 0)
        parts = [self._slots(hist, cand[:, i:i + chunk].contiguous(), cand_offsets, 0.0, 0, i) for i in range(0, C, chunk)]
        return torch.cat(parts, dim=1)

    # compact (pair, position) rows per pass of ``score_ragged``: about 7.4 KB of intermediates a row at the caum.yaml
    # widths (o, x, a1 / z1, z2), i.e. ~1 GB a pass; the measured peak is in DESIGN 7p
    row_budget = 131072

    @torch.no_grad()
    def score_ragged(self, hist: torch.Tensor, cand_rows: torch.Tensor, cand_offsets: torch.Tensor,
                     row_budget: Optional[int] = None):
        """Evaluation scores of the REAL (user, candidate) pairs only: hist (B, H, D) dense zero-padded history, cand_rows
        (n, D) the candidates of all users one after the other, cand_offsets (B + 1) int64 -> (scores (n,) in the order of
        ``cand_rows``, status (1,) int32).

        Without dropout the encoder is linear up to the attention softmax and DenseAttention's tanh, so it factors into a part
        per history row (B * H rows), a part per candidate row (n rows) and the across-users attention, whose q|k|v rows are
        sums of one row of each (``nrl_caum_eval_attn``); only the n * H rows of real pairs go through the tail
        (linear3's attention block folded into the out-projection, DenseAttention, the score).  A user with fewer candidates
        than the slot still is a key of that slot's attention, with a zero candidate, as in the reference.  The pairs are
        visited slot by slot (the attention couples the users of a slot) in passes of at most ``row_budget`` compact rows
        (default: the class attribute); a pass may end inside a slot.  Equal to ``forward`` within rounding (the products are
        reassociated; the folded weights are formed in float64 from the parameters on every call and nothing is kept).

        Inference only (``torch.no_grad``); ``ValueError`` in training mode with dropout.  ONE device-to-host read per call:
        the per-slot pair counts, which size the passes.  status: 0, or ``ops_caum.STATUS_BAD_OFFSETS`` (the candidate sizes
        do not add up to n: nothing was launched) | ``ops_caum.STATUS_BAD_INDEX`` (a kernel met an index out of range); with
        a non-zero status every score is 0."""
        if self.training and float(self.dropout1.p) > 0.0:
            raise ValueError("UserEncoder.score_ragged is the evaluation path: call .eval() first (dropout draws a fresh mask "
                             "per slot, which does not factor)")
        B, H, D = hist.shape
        n = cand_rows.shape[0]
        dev = hist.device
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        if n == 0 or B == 0:
            return torch.zeros(n, dtype=torch.float32, device=dev), status
        offs = cand_offsets.to(torch.int64)
        F_, U, heads = self.linear1.out_features, self.linear2.out_features, self.num_heads
        # ---- the slot-major pair list (device, n entries) and the per-slot pair counts (the one read-back)
        rows = torch.arange(n, device=dev)
        user = torch.searchsorted(offs[1:].contiguous(), rows, right=True).clamp_(max=B - 1)
        order = torch.argsort((rows - offs[user]) * B + user)            # pair j of the list is candidate row order[j]
        pair_user = user[order]
        sizes = offs[1:] - offs[:-1]
        counts = (B - torch.searchsorted(torch.sort(sizes).values, rows, right=True)).cpu().tolist()
        slot_counts = counts[:counts.index(0)] if 0 in counts else counts
        if sum(slot_counts) != n:                                        # offsets that are no partition of the n rows
            return torch.zeros(n, dtype=torch.float32, device=dev), status.fill_(ops_caum.STATUS_BAD_OFFSETS)
        # ---- folded weights, float64 -> float32, from the parameters of this call
        f64 = lambda t: t.detach().double()  # noqa: E731
        f32 = lambda t: t.float().contiguous()  # noqa: E731
        w_in, b_in, w_o, dhp, scale = ops_caum.padded_attention_params(self.multihead_attention, heads)
        w1, w2, w3 = f64(self.linear1.weight), f64(self.linear2.weight), f64(self.linear3.weight)
        w_in, w3c, w3a = f64(w_in), w3[:, :F_], w3[:, F_:]
        w_xh = f32(w3c @ w1[:, :3 * D])                                                          # (U, 3D): [left|centre|right]
        b_xh = f32(w3c @ f64(self.linear1.bias) + f64(self.linear3.bias) + w3a @ f64(self.multihead_attention.out_proj.bias))
        w_qh, b_qh = f32(w_in @ w2[:, D:]), f32(w_in @ f64(self.linear2.bias) + f64(b_in))
        w_qc, w_xc, w_y = f32(w_in @ w2[:, :D]), f32(w3c @ w1[:, 3 * D:]), f32(w3a @ f64(w_o))
        da = self.dense_att
        wd = da.linear.weight.detach()
        w_dx, w_dk = wd[:, :U].contiguous(), wd[:, U:].contiguous()
        h1 = wd.shape[0]
        # ---- user side (B * H rows) and candidate side (n rows), once
        hist = hist.detach()
        hist3 = torch.cat([torch.roll(hist, 1, dims=1), hist, torch.roll(hist, -1, dims=1)], dim=-1).reshape(B * H, 3 * D)
        xh = LinearFn.apply(hist3, w_xh, b_xh, None)
        qkv_h = LinearFn.apply(hist.reshape(B * H, D), w_qh, b_qh, None)
        del hist3
        cand_rows = cand_rows.detach()
        qkv_c = LinearFn.apply(cand_rows, w_qc, _zeros(w_qc.shape[0], hist), None)               # flat candidate order
        c_sm = cand_rows.index_select(0, order)                                                  # pair-list order from here on
        xc = LinearFn.apply(c_sm, w_xc, _zeros(U, hist), None)
        g1 = LinearFn.apply(c_sm, w_dk, da.linear.bias, None)
        # ---- the real pairs, pass by pass
        budget = self.row_budget if row_budget is None else row_budget
        chunks = ops_caum.plan_pair_chunks(slot_counts, H, budget)
        unit = torch.arange(max(j1 - j0 for j0, j1 in chunks) + 1, device=dev)
        zero_u, zero_h1 = _zeros(U, hist), _zeros(h1, hist)
        parts = []
        for j0, j1 in chunks:
            tab, n_items = ops_caum.pair_chunk_table(slot_counts, j0, j1, H, heads)
            tab = torch.tensor(tab, dtype=torch.int32).pin_memory().to(dev, non_blocking=True)
            o = ops_caum.caum_eval_attn(qkv_h, qkv_c, offs, order, pair_user, tab, n_items, B, H, j0, j1, heads, dhp, scale,
                                        status)
            x = LinearFn.apply(o, w_y, zero_u, None)
            del o
            ops_caum.caum_eval_add_(x, xh, xc, pair_user, j0, B, H, status)
            a1 = LinearFn.apply(x, w_dx, zero_h1, None)
            z1 = ops_caum.GroupTanhFn.apply(a1, g1[j0:j1], H)
            del a1
            z2 = LinearActFn.apply(z1, da.linear2.weight, da.linear2.bias, "tanh", None)
            del z1
            pairs = j1 - j0
            parts.append(ops_caum.ScoreFn.apply(z2, da.linear3.weight, da.linear3.bias, x, c_sm[j0:j1], unit[:pairs + 1],
                                                pairs, 1, 0, None).reshape(pairs))
            del z2, x
        scores = torch.zeros(n, dtype=torch.float32, device=dev).index_copy_(0, order, torch.cat(parts))
        return torch.where(status == 0, scores, torch.zeros_like(scores)), status

    def _slots(self, hist, cand, cand_offsets, p, seed, slot0):
        B, H, D = hist.shape
        C = cand.shape[1]
        F_ = self.linear1.out_features
        U = self.linear2.out_features
        base = ops_caum.USER_STREAM_BASE
        w1, w2 = self.linear1.weight, self.linear2.weight
        # linear1 = [left | centre | right | cand] blocks, linear2 = [cand | hist] (user/caum.py:97-110)
        w_hist = torch.cat([w1[:, :D], w1[:, D:2 * D], w1[:, 2 * D:3 * D], w2[:, D:]], dim=0)          # (3F + U, D)
        b_hist = torch.cat([self.linear1.bias, _zeros(2 * F_, hist), self.linear2.bias])
        w_cand = torch.cat([w1[:, 3 * D:], w2[:, :D]], dim=0)                                          # (F + U, D)
        if p > 0.0:
            hd, cd = ops_caum.ExpandFn.apply(hist, cand, p, seed, base)       # per-slot dropout2 / dropout1
            hs = C
        else:
            hd, cd, hs = hist, cand, 1
        P = LinearFn.apply(hd.reshape(-1, D), w_hist, b_hist, None)
        cd2 = cd.reshape(B * C, D)
        Q = LinearFn.apply(cd2, w_cand, _zeros(F_ + U, hist), None)
        cnn, s = ops_caum.CombineFn.apply(P, Q, B, C, H, F_, U, hs)
        # nn.MultiheadAttention without batch_first over (B, H, U): sequence = the B users, batch = every (slot, position)
        a = ops_caum.padded_attention(s, self.multihead_attention, self.num_heads, C * H, B, seq_first=True)
        z = ops_caum.ConcatDropoutFn.apply(cnn, a, B, C, H, p, seed, base)
        x = LinearFn.apply(z, self.linear3.weight, self.linear3.bias, None)                           # (R, U)
        da = self.dense_att
        wd = da.linear.weight                                                                           # [x | cand]
        a1 = LinearFn.apply(x, wd[:, :U].contiguous(), _zeros(wd.shape[0], hist), None)
        g1 = LinearFn.apply(cd2, wd[:, U:].contiguous(), da.linear.bias, None)
        z1 = ops_caum.GroupTanhFn.apply(a1, g1, H)
        z2 = LinearActFn.apply(z1, da.linear2.weight, da.linear2.bias, "tanh", None)
        return ops_caum.ScoreFn.apply(z2, da.linear3.weight, da.linear3.bias, x, cd2, cand_offsets, B, C, slot0, None)
