"""``torch.autograd.Function`` wrappers of the CAUM entry points (``nrl_caum.hip``).  Same conventions as ``ops.py``.

Dropout streams (``nrl_caum_dropout`` / the user-encoder calls) follow the library's counter-based mask spec
(``oracle/nrms_oracle.py``): the flat row-major index of the masked tensor, one stream per mask.  The CAUM module's map:
news encoder title 0 (embedding) / 1 (attention output), category 4, title entities 6 / 7 (abstract entities 8 / 9); user
encoder ``USER_STREAM_BASE + 3 i + {0, 1, 2}`` for dropout1 / dropout2 / dropout3 of candidate slot i."""
from __future__ import annotations

import torch

from . import _lib, ops
from .ops import GradAwareFunction, _chk, _grad_targets, _stream, saving

USER_STREAM_BASE = 16


def _check(rc, name):
    _lib.check(rc, name)


class AttnFn(GradAwareFunction):
    """Softmax attention over a packed q|k|v buffer (rows, 3 * heads * dh) -> (rows, heads * dh): every (outer, head) group
    attends over ``seq`` positions.  ``seq_first``: row = s * outer + n (``nn.MultiheadAttention``, batch_first=False), else
    row = n * seq + s.  ``scale`` multiplies q (0: 1/sqrt(dh))."""

    @staticmethod
    def forward(ctx, qkv, outer, seq, heads, dh, seq_first, scale):
        lib = _lib.load()
        qkv = _chk(qkv, torch.float32, "qkv")
        rows = qkv.shape[0]
        if qkv.shape != (rows, 3 * heads * dh) or rows != outer * seq:
            raise ValueError("newsreclib_amd: inconsistent packed attention shapes")
        o = torch.empty((rows, heads * dh), dtype=torch.float32, device=qkv.device)
        lse = torch.empty((outer * heads * seq,), dtype=torch.float32, device=qkv.device)
        cfg = (int(outer), int(seq), int(heads), int(dh), int(bool(seq_first)), float(scale))
        _check(lib.nrl_caum_attn_fwd(qkv.data_ptr(), o.data_ptr(), lse.data_ptr(), *cfg, _stream()), "nrl_caum_attn_fwd")
        if saving(ctx):
            ctx.save_for_backward(qkv, o, lse)
            ctx.cfg = cfg
        return o

    @staticmethod
    def backward(ctx, d_o):
        lib = _lib.load()
        qkv, o, lse = ctx.saved_tensors
        d_o = _chk(d_o, torch.float32, "d_out")
        dqkv = torch.empty_like(qkv)
        _check(lib.nrl_caum_attn_bwd(qkv.data_ptr(), o.data_ptr(), d_o.data_ptr(), lse.data_ptr(), dqkv.data_ptr(), *ctx.cfg,
                                     _stream()), "nrl_caum_attn_bwd")
        return dqkv, None, None, None, None, None, None


def _dropout(lib, x, p, seed, stream_id):
    y = torch.empty_like(x)
    _check(lib.nrl_caum_dropout(x.data_ptr(), y.data_ptr(), x.numel(), float(p), int(seed), int(stream_id), _stream()),
           "nrl_caum_dropout")
    return y


class DropoutFn(GradAwareFunction):
    """Element dropout under the library's mask spec (flat row-major index, one stream)."""

    @staticmethod
    def forward(ctx, x, p, seed, stream_id):
        x = _chk(x, torch.float32, "input")
        ctx.cfg = (float(p), int(seed), int(stream_id))
        return _dropout(_lib.load(), x, *ctx.cfg)

    @staticmethod
    def backward(ctx, d_y):
        return _dropout(_lib.load(), _chk(d_y, torch.float32, "d_out"), *ctx.cfg), None, None, None


def dropout(x, p: float, seed: int, stream_id: int):
    return DropoutFn.apply(x, p, seed, stream_id) if p > 0.0 else x


class ExpandFn(GradAwareFunction):
    """Per-slot dropout1 / dropout2 (user/caum.py:88-89): h (B, H, D), c (B, C, D) -> hd (B, C, H, D), cd (B, C, D)."""

    @staticmethod
    def forward(ctx, h, c, p, seed, base):
        lib = _lib.load()
        h, c = _chk(h, torch.float32, "hist"), _chk(c, torch.float32, "cand")
        B, H, D = h.shape
        C = c.shape[1]
        hd = torch.empty((B, C, H, D), dtype=torch.float32, device=h.device)
        cd = torch.empty((B, C, D), dtype=torch.float32, device=h.device)
        ctx.cfg = (B, C, H, D, float(p), int(seed), int(base))
        _check(lib.nrl_caum_expand_fwd(h.data_ptr(), c.data_ptr(), *ctx.cfg, hd.data_ptr(), cd.data_ptr(), _stream()),
               "nrl_caum_expand_fwd")
        return hd, cd

    @staticmethod
    def backward(ctx, d_hd, d_cd):
        lib = _lib.load()
        B, C, H, D = ctx.cfg[:4]
        dev = (d_hd if d_hd is not None else d_cd).device
        d_hd = _chk(d_hd, torch.float32, "d_hd") if d_hd is not None else torch.zeros((B, C, H, D), device=dev)
        d_cd = _chk(d_cd, torch.float32, "d_cd") if d_cd is not None else torch.zeros((B, C, D), device=dev)
        d_h = torch.empty((B, H, D), dtype=torch.float32, device=dev)
        d_c = torch.empty((B, C, D), dtype=torch.float32, device=dev)
        _check(lib.nrl_caum_expand_bwd(d_hd.data_ptr(), d_cd.data_ptr(), *ctx.cfg, d_h.data_ptr(), d_c.data_ptr(), _stream()),
               "nrl_caum_expand_bwd")
        return d_h, d_c, None, None, None


class CombineFn(GradAwareFunction):
    """candi-CNN and linear2 from their parts (user/caum.py:97-110), P (B * hs * H, 3F + U), Q (B * C, F + U) ->
    cnn (B * C * H, F), s (B * C * H, U); see ``nrl_caum_combine_fwd``."""

    @staticmethod
    def forward(ctx, P, Q, B, C, H, F, U, hs):
        lib = _lib.load()
        P, Q = _chk(P, torch.float32, "P"), _chk(Q, torch.float32, "Q")
        if P.shape != (B * hs * H, 3 * F + U) or Q.shape != (B * C, F + U):
            raise ValueError("newsreclib_amd: inconsistent CAUM combine shapes")
        R = B * C * H
        cnn = torch.empty((R, F), dtype=torch.float32, device=P.device)
        s = torch.empty((R, U), dtype=torch.float32, device=P.device)
        ctx.cfg = (B, C, H, F, U, hs)
        _check(lib.nrl_caum_combine_fwd(P.data_ptr(), Q.data_ptr(), *ctx.cfg, cnn.data_ptr(), s.data_ptr(), _stream()),
               "nrl_caum_combine_fwd")
        return cnn, s

    @staticmethod
    def backward(ctx, d_cnn, d_s):
        lib = _lib.load()
        B, C, H, F, U, hs = ctx.cfg
        dev = (d_cnn if d_cnn is not None else d_s).device
        R = B * C * H
        d_cnn = _chk(d_cnn, torch.float32, "d_cnn") if d_cnn is not None else torch.zeros((R, F), device=dev)
        d_s = _chk(d_s, torch.float32, "d_s") if d_s is not None else torch.zeros((R, U), device=dev)
        d_P = torch.empty((B * hs * H, 3 * F + U), dtype=torch.float32, device=dev)
        d_Q = torch.empty((B * C, F + U), dtype=torch.float32, device=dev)
        _check(lib.nrl_caum_combine_bwd(d_cnn.data_ptr(), d_s.data_ptr(), *ctx.cfg, d_P.data_ptr(), d_Q.data_ptr(), _stream()),
               "nrl_caum_combine_bwd")
        return d_P, d_Q, None, None, None, None, None, None


class ConcatDropoutFn(GradAwareFunction):
    """dropout3([cnn, self]) (user/caum.py:112-113): (R, F), (R, U) -> (R, F + U)."""

    @staticmethod
    def forward(ctx, cnn, a, B, C, H, p, seed, base):
        lib = _lib.load()
        cnn, a = _chk(cnn, torch.float32, "cnn"), _chk(a, torch.float32, "self")
        F, U = cnn.shape[1], a.shape[1]
        z = torch.empty((cnn.shape[0], F + U), dtype=torch.float32, device=cnn.device)
        ctx.cfg = (B, C, H, F, U, float(p), int(seed), int(base))
        _check(lib.nrl_caum_concat_dropout_fwd(cnn.data_ptr(), a.data_ptr(), *ctx.cfg, z.data_ptr(), _stream()),
               "nrl_caum_concat_dropout_fwd")
        return z

    @staticmethod
    def backward(ctx, d_z):
        lib = _lib.load()
        B, C, H, F, U = ctx.cfg[:5]
        d_z = _chk(d_z, torch.float32, "d_z")
        d_cnn = torch.empty((d_z.shape[0], F), dtype=torch.float32, device=d_z.device)
        d_a = torch.empty((d_z.shape[0], U), dtype=torch.float32, device=d_z.device)
        _check(lib.nrl_caum_concat_dropout_bwd(d_z.data_ptr(), *ctx.cfg, d_cnn.data_ptr(), d_a.data_ptr(), _stream()),
               "nrl_caum_concat_dropout_bwd")
        return d_cnn, d_a, None, None, None, None, None, None


class GroupTanhFn(GradAwareFunction):
    """tanh(a + g[row // rows_per_group]): DenseAttention's first layer from its history part a (R, N) and candidate part
    g (R / rows_per_group, N)."""

    @staticmethod
    def forward(ctx, a, g, rows_per_group):
        lib = _lib.load()
        a, g = _chk(a, torch.float32, "a"), _chk(g, torch.float32, "g")
        G, N = g.shape
        if a.shape != (G * rows_per_group, N):
            raise ValueError("newsreclib_amd: inconsistent grouped-tanh shapes")
        z = torch.empty_like(a)
        _check(lib.nrl_caum_group_tanh_fwd(a.data_ptr(), g.data_ptr(), G, int(rows_per_group), N, z.data_ptr(), _stream()),
               "nrl_caum_group_tanh_fwd")
        if saving(ctx):
            ctx.save_for_backward(z)
            ctx.cfg = (G, int(rows_per_group), N)
        return z

    @staticmethod
    def backward(ctx, d_z):
        lib = _lib.load()
        (z,) = ctx.saved_tensors
        G, rpg, N = ctx.cfg
        d_z = _chk(d_z, torch.float32, "d_z")
        d_a = torch.empty_like(z)
        d_g = torch.empty((G, N), dtype=torch.float32, device=z.device)
        _check(lib.nrl_caum_group_tanh_bwd(d_z.data_ptr(), z.data_ptr(), G, rpg, N, d_a.data_ptr(), d_g.data_ptr(), _stream()),
               "nrl_caum_group_tanh_bwd")
        return d_a, d_g, None


class ScoreFn(GradAwareFunction):
    """DenseAttention's last layer, the softmax over the H history slots, the user vector and the score
    (user/caum.py:116-125) for every (b, i): z2 (R, N2), x (R, U), cd (B * C, U) -> scores (B, C), 0 at padded slots."""

    @staticmethod
    def forward(ctx, z2, w3, b3, x, cd, cand_offsets, B, C, slot0, grad_bufs):
        lib = _lib.load()
        z2, x, cd = _chk(z2, torch.float32, "z2"), _chk(x, torch.float32, "x"), _chk(cd, torch.float32, "cand")
        w3, b3 = _chk(w3, torch.float32, "dense_att.linear3.weight"), _chk(b3, torch.float32, "dense_att.linear3.bias")
        offs = _chk(cand_offsets, torch.int64, "cand_offsets")
        R, N2 = z2.shape
        U = x.shape[1]
        H = R // (B * C)
        if R != B * C * H or x.shape[0] != R or cd.shape != (B * C, U) or w3.numel() != N2 or b3.numel() != 1:
            raise ValueError("newsreclib_amd: inconsistent CAUM score shapes")
        scores = torch.empty((B, C), dtype=torch.float32, device=z2.device)
        alpha = torch.empty((R,), dtype=torch.float32, device=z2.device)
        user = torch.empty((B * C, U), dtype=torch.float32, device=z2.device)
        _check(lib.nrl_caum_score_fwd(z2.data_ptr(), w3.data_ptr(), b3.data_ptr(), x.data_ptr(), cd.data_ptr(), offs.data_ptr(),
                                      B, C, int(slot0), H, N2, U, scores.data_ptr(), alpha.data_ptr(), user.data_ptr(),
                                      _stream()), "nrl_caum_score_fwd")
        if saving(ctx):
            ctx.save_for_backward(z2, w3, b3, x, cd, offs, alpha, user)
            ctx.cfg, ctx.grad_bufs = (B, C, int(slot0), H, N2, U), grad_bufs
        return scores

    @staticmethod
    def backward(ctx, d_scores):
        lib = _lib.load()
        z2, w3, b3, x, cd, offs, alpha, user = ctx.saved_tensors
        B, C, slot0, H, N2, U = ctx.cfg
        d_scores = _chk(d_scores, torch.float32, "d_scores")
        bufs, rets = _grad_targets([w3, b3], ctx.grad_bufs)
        d_z2, d_x, d_cd = torch.empty_like(z2), torch.empty_like(x), torch.empty_like(cd)
        ws = ops.workspace(lib.nrl_caum_score_workspace_bytes(B, C, H, N2), z2.device)
        _check(lib.nrl_caum_score_bwd(d_scores.data_ptr(), z2.data_ptr(), w3.data_ptr(), x.data_ptr(), cd.data_ptr(),
                                      alpha.data_ptr(), user.data_ptr(), offs.data_ptr(), B, C, slot0, H, N2, U,
                                      d_z2.data_ptr(), d_x.data_ptr(), d_cd.data_ptr(), bufs[0].data_ptr(), bufs[1].data_ptr(),
                                      ws.data_ptr(), ws.numel(), _stream()), "nrl_caum_score_bwd")
        return d_z2, rets[0], rets[1], d_x, d_cd, None, None, None, None, None


HEAD_DIMS = (16, 20, 32, 48, 64)          # what the attention kernels are instantiated for


def padded_attention_params(mha, heads: int):
    """-> (in-projection (3 Dp, D), its bias (3 Dp), out-projection (D, Dp), padded head dim, q scale) of ``mha``
    (``nn.MultiheadAttention``, D = embed_dim) with each head's dh features padded to the next built head dim with zero rows
    / columns.  Zero features change neither q k^T nor the softmax nor p v; the scale stays 1/sqrt(dh).  Built from the
    parameters on every call (autograd maps the gradients back to the reference's layout), so no copy can go stale."""
    D = mha.embed_dim
    dh = D // heads
    dhp = next((d for d in HEAD_DIMS if d >= dh), None)
    if dhp is None or dh * heads != D:
        raise NotImplementedError(f"head dim {D}/{heads} is not built (at most 64)")
    w_in, b_in, w_o = mha.in_proj_weight, mha.in_proj_bias, mha.out_proj.weight
    scale = 1.0 / float(dh) ** 0.5
    if dhp == dh:
        return w_in, b_in, w_o, dh, scale
    Dp = heads * dhp
    dev = w_in.device
    col = torch.arange(heads, device=dev).repeat_interleave(dh) * dhp + torch.arange(dh, device=dev).repeat(heads)
    rows = torch.cat([col, col + Dp, col + 2 * Dp])
    w_in_p = w_in.new_zeros(3 * Dp, D).index_copy(0, rows, w_in)
    b_in_p = b_in.new_zeros(3 * Dp).index_copy(0, rows, b_in)
    w_o_p = w_o.new_zeros(D, Dp).index_copy(1, col, w_o)
    return w_in_p, b_in_p, w_o_p, dhp, scale


EVAL_QUERY_TILE = 64                      # queries per work item of ``nrl_caum_eval_attn``
STATUS_BAD_INDEX = 1                      # set by the kernels: an offset / pair-list entry failed its range check
STATUS_BAD_OFFSETS = 2                    # set by ``score_ragged``: the candidate sizes do not add up to the candidate rows


def plan_pair_chunks(slot_counts, H: int, row_budget: int):
    """The factored evaluation's passes over the slot-major pair list (slot 0's pairs, then slot 1's ...; ``slot_counts[i]`` =
    users with more than i candidates): -> [(j0, j1)] contiguous, disjoint, covering every pair once, each with
    ``(j1 - j0) * H <= row_budget`` -- except that a chunk always holds at least one pair.  A chunk takes whole slots while
    they fit and ends inside a slot only where that slot alone exceeds what is left of an empty chunk."""
    per = max(1, int(row_budget) // max(1, int(H)))
    chunks, j0, j = [], 0, 0
    for cnt in (int(c) for c in slot_counts):
        while cnt > 0:
            room = per - (j - j0)
            if cnt <= room:
                j, cnt = j + cnt, 0
            elif j > j0:                  # the slot does not fit behind what the chunk holds: close the chunk
                chunks.append((j0, j))
                j0 = j
            else:                         # an empty chunk and a slot larger than the budget: split the slot
                chunks.append((j0, j0 + per))
                j0 = j = j0 + per
                cnt -= per
    if j > j0:
        chunks.append((j0, j))
    return chunks


def pair_chunk_table(slot_counts, j0: int, j1: int, H: int, heads: int):
    """-> (rows [slot, first pair, pair count, first work item], work items) of the pair range [j0, j1): what
    ``nrl_caum_eval_attn`` takes as ``slot_tab`` / ``n_items``."""
    rows, items, start = [], 0, 0
    for slot, cnt in enumerate(int(c) for c in slot_counts):
        lo, hi = max(start, j0), min(start + cnt, j1)
        if lo < hi:
            rows.append([slot, lo, hi - lo, items])
            items += -(-(hi - lo) // EVAL_QUERY_TILE) * H * heads
        start += cnt
    return rows, items


def caum_eval_attn(qkv_h, qkv_c, cand_offsets, pair_row, pair_user, slot_tab, n_items: int, B: int, H: int, j0: int, j1: int,
                   heads: int, dh: int, scale: float, status):
    """``nrl_caum_eval_attn``: qkv_h (B * H, 3 * heads * dh), qkv_c (n, 3 * heads * dh) in flat candidate order -> the attention
    output ((j1 - j0) * H, heads * dh) of the pairs [j0, j1) of the slot-major pair list (``pair_row`` / ``pair_user`` int64 (n),
    ``slot_tab`` int32 (entries, 4): ``pair_chunk_table``).  ``status`` int32 (1): bit 0 is ORed in when an index fails its
    range check on the device (that pair's rows are zeros)."""
    lib = _lib.load()
    qkv_h, qkv_c = _chk(qkv_h, torch.float32, "qkv_h"), _chk(qkv_c, torch.float32, "qkv_c")
    offs, pair_row = _chk(cand_offsets, torch.int64, "cand_offsets"), _chk(pair_row, torch.int64, "pair_row")
    pair_user, slot_tab = _chk(pair_user, torch.int64, "pair_user"), _chk(slot_tab, torch.int32, "slot_tab")
    status = _chk(status, torch.int32, "status")
    n, W = qkv_c.shape[0], 3 * heads * dh
    if qkv_h.shape != (B * H, W) or qkv_c.shape != (n, W) or offs.numel() != B + 1 or pair_row.numel() != n or \
            pair_user.numel() != n or slot_tab.dim() != 2 or slot_tab.shape[1] != 4 or status.numel() != 1 or \
            not status.is_contiguous():
        raise ValueError("newsreclib_amd: inconsistent CAUM factored-attention shapes")
    o = torch.empty(((j1 - j0) * H, heads * dh), dtype=torch.float32, device=qkv_h.device)
    _check(lib.nrl_caum_eval_attn(qkv_h.data_ptr(), qkv_c.data_ptr(), offs.data_ptr(), pair_row.data_ptr(),
                                  pair_user.data_ptr(), slot_tab.data_ptr(), slot_tab.shape[0], int(n_items), B, H, n, int(j0),
                                  int(j1), heads, dh, float(scale), o.data_ptr(), status.data_ptr(), _stream()),
           "nrl_caum_eval_attn")
    return o


def caum_eval_add_(y, xh, xc, pair_user, j0: int, B: int, H: int, status):
    """In place: y ((pairs) * H, U) += xh[(user of pair j0 + jj) * H + t] + xc[j0 + jj] (``nrl_caum_eval_add``)."""
    lib = _lib.load()
    U = y.shape[1]
    pairs = y.shape[0] // H
    if not y.is_contiguous() or y.shape[0] != pairs * H or xh.shape != (B * H, U) or xc.shape != (pair_user.numel(), U):
        raise ValueError("newsreclib_amd: inconsistent CAUM factored-add shapes")
    xh, xc = _chk(xh, torch.float32, "xh"), _chk(xc, torch.float32, "xc")
    _check(lib.nrl_caum_eval_add(y.data_ptr(), xh.data_ptr(), xc.data_ptr(), pair_user.data_ptr(), pair_user.numel(), int(j0),
                                 pairs, B, H, U, y.data_ptr(), status.data_ptr(), _stream()), "nrl_caum_eval_add")
    return y


def padded_attention(x, mha, heads: int, outer: int, seq: int, seq_first: bool):
    """``mha(x, x, x)[0]`` on rows x (outer * seq, D) laid out as ``AttnFn`` describes, at any head dim the padding reaches:
    in-projection and out-projection on the GEMM engines (``LinearFn``), the attention on ``nrl_caum_attn_*``."""
    from .ops_blocks import LinearFn
    w_in, b_in, w_o, dhp, scale = padded_attention_params(mha, heads)
    qkv = LinearFn.apply(x, w_in, b_in, None)
    o = AttnFn.apply(qkv, outer, seq, heads, dhp, seq_first, scale)
    return LinearFn.apply(o, w_o, mha.out_proj.bias, None)
