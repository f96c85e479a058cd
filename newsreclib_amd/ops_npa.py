"""``torch.autograd.Function`` wrappers around the NPA part of the C ABI (include/newsreclib_amd.h): the CNN text encoder
with personalized attention, the per-user queries, and the personalized user attention.  Same conventions as ``ops.py``
(no eager fallback; optional ``grad_bufs`` to accumulate parameter gradients in place)."""
from __future__ import annotations

import ctypes

import torch

from . import _lib, ops
from ._lib import NrlCnnGrads, NrlCnnParams, NrlNpaQueryGrads, NrlNpaQueryParams
from .ops import GradAwareFunction, _chk, _grad_targets, _stream, saving
from .ops import sort_positions as _sort_positions

# dropout streams of an NPA step (include/newsreclib_amd.h): the encoder takes 0 and 1, the user queries 2..5
ENCODER_STREAM0 = 0
QUERY_STREAM0 = 2


class NpaEncoderFn(GradAwareFunction):
    """``CNNPersAtt.forward`` (reference text.py:376-392) over history and candidate rows in one call: ids (N, L) ->
    (N, F).  ``queries`` (Q, F) holds one attention query per (user, call); row n uses ``queries[owner[n]]``; the rows of
    query i are ``[offsets[i], offsets[i+1])``.  ``w_c`` in the (F, 1, W, D) layout of ``CnnEncoderFn``."""

    @staticmethod
    def forward(ctx, ids, emb, w_c, b_c, queries, owner, offsets, p_drop, seed, stream0, grad_bufs, order=None):
        lib = _lib.load()
        ids = _chk(ids, torch.int64, "ids")
        emb, w_c, b_c, queries = [_chk(t, torch.float32, n) for t, n in zip(
            (emb, w_c, b_c, queries), ("embedding", "cnn.weight", "cnn.bias", "queries"))]
        owner = _chk(owner, torch.int32, "owner")
        offsets = _chk(offsets, torch.int64, "offsets")
        if ids.dim() != 2:
            raise ValueError("newsreclib_amd: token ids must be (num_news, num_tokens)")
        N, L = ids.shape
        V, D = emb.shape
        if w_c.dim() != 4 or w_c.shape[1] != 1 or w_c.shape[3] != D:
            raise ValueError("newsreclib_amd: cnn.weight must be (num_filters, 1, window, embed_dim)")
        F_, _, W, _ = w_c.shape
        nq = queries.shape[0]
        if b_c.shape != (F_,) or queries.shape != (nq, F_) or owner.shape != (N,) or offsets.shape != (nq + 1,):
            raise ValueError("newsreclib_amd: inconsistent NPA encoder shapes")
        cp = NrlCnnParams(w_c.data_ptr(), b_c.data_ptr(), None, None, None, D, F_, W, 16)
        save = saving(ctx)
        ws = ops.workspace(lib.nrl_npa_encoder_workspace_bytes(N, L, D, F_, W), ids.device)
        out = torch.empty((N, F_), dtype=torch.float32, device=ids.device)
        _lib.check(lib.nrl_npa_encoder_fwd(ctypes.byref(cp), emb.data_ptr(), V, ids.data_ptr(), N, L, queries.data_ptr(),
                                           owner.data_ptr(), nq, float(p_drop), int(seed), int(stream0), int(save),
                                           out.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "nrl_npa_encoder_fwd")
        if save:
            if order is None:
                order = _sort_positions(ids, V)     # counting sort over the vocabulary (ops.sort_positions)
            from .ops import order_event
            ctx.order_ready = order_event(order)
            ctx.save_for_backward(ids, _chk(order, torch.int64, "order"), emb, w_c, b_c, queries, owner, offsets)
            ctx.ws, ctx.cfg, ctx.grad_bufs = ws, (float(p_drop), int(seed), int(stream0)), grad_bufs
            ctx.engine, ctx.options = _lib.engine_code(), _lib.options_mask()
        return out

    @staticmethod
    def backward(ctx, d_out):
        lib = _lib.load()
        _lib.require_engine(ctx.engine, "the NPA text encoder")
        _lib.require_options(ctx.options, "the NPA text encoder")
        ids, order, emb, w_c, b_c, queries, owner, offsets = ctx.saved_tensors
        from .ops import wait_order
        wait_order(ctx.order_ready)
        p_drop, seed, stream0 = ctx.cfg
        N, L = ids.shape
        V, D = emb.shape
        F_, _, W, _ = w_c.shape
        nq = queries.shape[0]
        d_out = _chk(d_out, torch.float32, "d_out")
        cp = NrlCnnParams(w_c.data_ptr(), b_c.data_ptr(), None, None, None, D, F_, W, 16)
        bufs, rets = _grad_targets([emb, w_c, b_c], ctx.grad_bufs)
        cg = NrlCnnGrads(bufs[1].data_ptr(), bufs[2].data_ptr(), None, None, None)
        d_queries = torch.empty_like(queries)
        _lib.check(lib.nrl_npa_encoder_bwd(ctypes.byref(cp), ctypes.byref(cg), bufs[0].data_ptr(), V, ids.data_ptr(),
                                           order.data_ptr(), N, L, queries.data_ptr(), owner.data_ptr(),
                                           offsets.data_ptr(), nq, p_drop, seed, stream0, d_out.data_ptr(),
                                           d_queries.data_ptr(), ctx.ws.data_ptr(), ctx.ws.numel(), _stream()),
                   "nrl_npa_encoder_bwd")
        ctx.ws = None
        return (None, *rets, d_queries, None, None, None, None, None, None, None)


def _query_params(table, text, news, num_filters):
    """text / news: (proj.weight, proj.bias, att.weight, att.bias); news None under late fusion."""
    tp_w, tp_b, ta_w, ta_b = text
    U, Pw = table.shape[1], tp_w.shape[0]
    if tp_w.shape != (Pw, U) or tp_b.shape != (Pw,) or ta_w.shape != (num_filters, Pw) or ta_b.shape != (num_filters,):
        raise ValueError("newsreclib_amd: inconsistent text-query parameter shapes")
    Pn = 0
    if news is not None:
        np_w, np_b, na_w, na_b = news
        Pn = np_w.shape[0]
        if np_w.shape != (Pn, U) or np_b.shape != (Pn,) or na_w.shape != (num_filters, Pn) or na_b.shape != (num_filters,):
            raise ValueError("newsreclib_amd: inconsistent news-query parameter shapes")
    ptrs = [t.data_ptr() for t in text] + ([t.data_ptr() for t in news] if news is not None else [None] * 4)
    return NrlNpaQueryParams(table.data_ptr(), *ptrs, table.shape[0], U, Pw, Pn, num_filters)


class NpaUserQueriesFn(GradAwareFunction):
    """Every per-user query of an NPA step (npa_module.py:223-242): ``UserProjection`` (projection.py:35-50), the text
    query of both ``CNNPersAtt`` calls (text.py:385, attention.py:244, two dropout draws) and the user encoder's news
    query (user/npa.py:52-58).  -> (text queries (2B, F): rows [history; candidates], news queries (B, F) or None)."""

    @staticmethod
    def forward(ctx, user_idx, table, tp_w, tp_b, ta_w, ta_b, np_w, np_b, na_w, na_b, p_drop, seed, stream0, grad_bufs):
        lib = _lib.load()
        user_idx = _chk(user_idx, torch.int64, "user_idx")
        table = _chk(table, torch.float32, "user_embed")
        text = [_chk(t, torch.float32, "text query parameter") for t in (tp_w, tp_b, ta_w, ta_b)]
        news = None if np_w is None else [_chk(t, torch.float32, "news query parameter") for t in (np_w, np_b, na_w, na_b)]
        F_ = ta_w.shape[0]
        B = user_idx.shape[0]
        qp = _query_params(table, text, news, F_)
        text_q = torch.empty((2 * B, F_), dtype=torch.float32, device=table.device)
        news_q = torch.empty((B, F_), dtype=torch.float32, device=table.device) if news is not None else None
        _lib.check(lib.nrl_npa_user_queries_fwd(ctypes.byref(qp), user_idx.data_ptr(), B, float(p_drop), int(seed),
                                                int(stream0), text_q.data_ptr(),
                                                news_q.data_ptr() if news_q is not None else None, _stream()),
                   "nrl_npa_user_queries_fwd")
        if saving(ctx):
            ctx.save_for_backward(user_idx, table, *text, *(news or ()))
            ctx.has_news, ctx.cfg, ctx.grad_bufs = news is not None, (float(p_drop), int(seed), int(stream0)), grad_bufs
        if news_q is None:
            return text_q
        return text_q, news_q

    @staticmethod
    def backward(ctx, d_text, d_news=None):
        lib = _lib.load()
        user_idx, table, *params = ctx.saved_tensors
        text, news = params[:4], (params[4:] if ctx.has_news else None)
        p_drop, seed, stream0 = ctx.cfg
        F_ = text[2].shape[0]
        B = user_idx.shape[0]
        qp = _query_params(table, text, news, F_)
        all_params = [table, *text, *(news or ())]
        bufs, rets = _grad_targets(all_params, ctx.grad_bufs)
        ptrs = [b.data_ptr() for b in bufs] + ([] if news is not None else [None] * 4)
        qg = NrlNpaQueryGrads(*ptrs)
        d_text = _chk(d_text.contiguous() if d_text is not None else torch.zeros((2 * B, F_), device=table.device),
                      torch.float32, "d_text_queries")
        if news is not None:
            d_news = _chk(d_news.contiguous() if d_news is not None else torch.zeros((B, F_), device=table.device),
                          torch.float32, "d_news_queries")
        ws = ops.workspace(lib.nrl_npa_user_queries_workspace_bytes(ctypes.byref(qp), B), table.device)
        _lib.check(lib.nrl_npa_user_queries_bwd(ctypes.byref(qp), ctypes.byref(qg), user_idx.data_ptr(), B, p_drop, seed,
                                                stream0, d_text.data_ptr(),
                                                d_news.data_ptr() if news is not None else None, ws.data_ptr(),
                                                ws.numel(), _stream()), "nrl_npa_user_queries_bwd")
        rets = list(rets) + ([] if news is not None else [None] * 4)
        return (None, *rets, None, None, None, None)


class PersonalizedUserAttentionFn(GradAwareFunction):
    """NPA ``UserEncoder`` attention (user/npa.py:48-60) on the ragged history rows (n_hist, F) with their offsets (B + 1):
    the reference's softmax also counts the ``max_hist - n_b`` zero rows of ``to_dense_batch``.  -> (B, F)."""

    @staticmethod
    def forward(ctx, hist, offsets, max_hist, queries):
        lib = _lib.load()
        hist = _chk(hist, torch.float32, "hist_news_vector")
        offsets = _chk(offsets, torch.int64, "hist_offsets")
        queries = _chk(queries, torch.float32, "news queries")
        B, F_ = queries.shape
        if hist.dim() != 2 or hist.shape[1] != F_ or offsets.shape != (B + 1,):
            raise ValueError("newsreclib_amd: inconsistent personalized-attention shapes")
        out = torch.empty((B, F_), dtype=torch.float32, device=queries.device)
        _lib.check(lib.nrl_personalized_user_attention_fwd(hist.data_ptr(), offsets.data_ptr(), B, int(max_hist), F_,
                                                           queries.data_ptr(), out.data_ptr(), _stream()),
                   "nrl_personalized_user_attention_fwd")
        if saving(ctx):
            ctx.save_for_backward(hist, offsets, queries)
            ctx.max_hist = int(max_hist)
        return out

    @staticmethod
    def backward(ctx, d_out):
        lib = _lib.load()
        hist, offsets, queries = ctx.saved_tensors
        B, F_ = queries.shape
        d_out = _chk(d_out, torch.float32, "d_out")
        d_hist = torch.empty_like(hist)
        d_q = torch.empty_like(queries)
        _lib.check(lib.nrl_personalized_user_attention_bwd(hist.data_ptr(), offsets.data_ptr(), B, ctx.max_hist, F_,
                                                           queries.data_ptr(), d_out.data_ptr(), d_hist.data_ptr(),
                                                           d_q.data_ptr(), _stream()),
                   "nrl_personalized_user_attention_bwd")
        return d_hist, None, None, d_q


MAX_FILTERS = 1024      # the pooling kernels keep a row's F columns as float4 chunks over one wave: F % 4 == 0, F <= 1024


def _conv_weight_image(w_c: torch.Tensor) -> torch.Tensor:
    """``nn.Conv1d.weight`` (F, D, W) or the kernels' (F, 1, W, D) image -> the (F, 1, W, D) image."""
    if w_c.dim() == 3:
        return w_c.permute(0, 2, 1).contiguous().unsqueeze(1)
    return w_c


@torch.no_grad()
def npa_conv_features(ids: torch.Tensor, emb: torch.Tensor, w_c: torch.Tensor, b_c: torch.Tensor,
                      out: torch.Tensor = None) -> torch.Tensor:
    """The eval-mode conv feature maps ``relu(conv1d(emb[ids]) + b)`` of ``CNNPersAtt`` (text.py:377-383, dropout off):
    ids (N, L) -> (N, L, F) fp32, the same lookup and convolution launches as ``NpaEncoderFn`` under the current engine.
    ``out``: a contiguous (N, L, F) buffer to fill (a slice of a preallocated table), else one is allocated."""
    lib = _lib.load()
    ids = _chk(ids, torch.int64, "ids")
    emb, w_c, b_c = [_chk(t, torch.float32, n) for t, n in zip((emb, _conv_weight_image(w_c), b_c),
                                                              ("embedding", "cnn.weight", "cnn.bias"))]
    if ids.dim() != 2:
        raise ValueError("newsreclib_amd: token ids must be (num_news, num_tokens)")
    N, L = ids.shape
    V, D = emb.shape
    if w_c.dim() != 4 or w_c.shape[1] != 1 or w_c.shape[3] != D:
        raise ValueError("newsreclib_amd: cnn.weight must be (num_filters, 1, window, embed_dim)")
    F_, _, W, _ = w_c.shape
    if b_c.shape != (F_,):
        raise ValueError("newsreclib_amd: inconsistent NPA encoder shapes")
    if out is None:
        out = torch.empty((N, L, F_), dtype=torch.float32, device=ids.device)
    else:
        if not out.is_cuda or out.dtype != torch.float32 or out.shape != (N, L, F_) or not out.is_contiguous():
            raise ValueError(f"newsreclib_amd: `out` must be a contiguous float32 GPU tensor of shape {(N, L, F_)}")
    cp = NrlCnnParams(w_c.data_ptr(), b_c.data_ptr(), None, None, None, D, F_, W, 16)
    ws = ops.workspace(lib.nrl_npa_conv_features_workspace_bytes(N, L, D, F_, W), ids.device)
    _lib.check(lib.nrl_npa_conv_features(ctypes.byref(cp), emb.data_ptr(), V, ids.data_ptr(), N, L, out.data_ptr(),
                                         ws.data_ptr(), ws.numel(), _stream()), "nrl_npa_conv_features")
    return out


@torch.no_grad()
def npa_cached_scores(table: torch.Tensor, hist_idx: torch.Tensor, hist_offsets: torch.Tensor, cand_idx: torch.Tensor,
                      cand_offsets: torch.Tensor, q_hist: torch.Tensor, q_cand: torch.Tensor, q_news, max_hist: int,
                      max_cand: int, return_user_vectors: bool = False):
    """``NPAModule.forward`` in eval mode from the cached feature table (num_news, L, F) of ``npa_conv_features``:
    hist_idx / cand_idx flat int64 table rows, hist_offsets / cand_offsets (B + 1) int64, q_hist / q_cand (B, F) the tanh'd
    text queries, q_news (B, F) the news query or None (late fusion), max_hist / max_cand the batch maxima (plain ints).
    -> scores (B, max_cand), 0 at padded slots [, user vectors (B, F)].  An index outside the table reads as an all-zero
    feature map."""
    lib = _lib.load()
    table = _chk(table, torch.float32, "feature table")
    hist_idx, cand_idx = _chk(hist_idx, torch.int64, "hist_idx"), _chk(cand_idx, torch.int64, "cand_idx")
    hist_offsets, cand_offsets = _chk(hist_offsets, torch.int64, "hist_offsets"), _chk(cand_offsets, torch.int64, "cand_offsets")
    q_hist, q_cand = _chk(q_hist, torch.float32, "q_hist"), _chk(q_cand, torch.float32, "q_cand")
    if q_news is not None:
        q_news = _chk(q_news, torch.float32, "q_news")
    if table.dim() != 3:
        raise ValueError("newsreclib_amd: the feature table must be (num_news, num_tokens, num_filters)")
    V, L, F_ = table.shape
    if F_ % 4 or not 4 <= F_ <= MAX_FILTERS:
        raise ValueError(f"newsreclib_amd: num_filters must be a multiple of 4 up to {MAX_FILTERS}, got {F_}")
    B = int(hist_offsets.numel()) - 1
    if B < 0 or hist_idx.dim() != 1 or cand_idx.dim() != 1 or cand_offsets.shape != (B + 1,) or q_hist.shape != (B, F_) or \
            q_cand.shape != (B, F_) or (q_news is not None and q_news.shape != (B, F_)) or int(max_hist) < 0 or int(max_cand) < 0:
        raise ValueError("newsreclib_amd: inconsistent cached-score shapes")
    scores = torch.empty((B, int(max_cand)), dtype=torch.float32, device=table.device)
    user = torch.empty((B, F_), dtype=torch.float32, device=table.device)
    _lib.check(lib.nrl_npa_cached_scores(table.data_ptr(), V, L, F_, hist_idx.data_ptr(), hist_idx.numel(),
                                         hist_offsets.data_ptr(), cand_idx.data_ptr(), cand_idx.numel(),
                                         cand_offsets.data_ptr(), B, q_hist.data_ptr(), q_cand.data_ptr(),
                                         q_news.data_ptr() if q_news is not None else None, int(max_hist), int(max_cand),
                                         user.data_ptr(), scores.data_ptr(), _stream()), "nrl_npa_cached_scores")
    return (scores, user) if return_user_vectors else scores
