"""``torch.autograd.Function`` wrappers around the DKN part of the C ABI (include/newsreclib_amd.h): the knowledge-aware CNN
news encoder and the candidate-aware user attention with the DNN click predictor.  Same conventions as ``ops.py`` (no eager
fallback; optional ``grad_bufs`` to accumulate parameter gradients in place)."""
from __future__ import annotations

import ctypes
from typing import Optional, Sequence

import torch

from . import _lib, ops
from ._lib import NrlDknClickGrads, NrlDknClickParams, NrlDknGrads, NrlDknParams
from .ops import GradAwareFunction, _chk, _grad_targets, _stream, order_event, saving, wait_order
from .ops import sort_positions as _sort_positions


def _ptr(t: Optional[torch.Tensor]):
    return t.data_ptr() if t is not None else None


def _encoder_params(word, ent, ctx_t, T, b, images, biases, windows) -> NrlDknParams:
    nw = len(windows)
    img = (ctypes.c_void_p * 4)(*([t.data_ptr() for t in images] + [None] * (4 - nw)))
    bias = (ctypes.c_void_p * 4)(*([t.data_ptr() for t in biases] + [None] * (4 - nw)))
    win = (ctypes.c_int32 * 4)(*(list(windows) + [0] * (4 - nw)))
    return NrlDknParams(word.data_ptr(), ent.data_ptr(), _ptr(ctx_t), T.data_ptr(), b.data_ptr(), img, bias, win, nw,
                        word.shape[1], ent.shape[1], biases[0].shape[0])


class DknEncoderFn(GradAwareFunction):
    """``KCNN.forward`` (reference news.py:255-299): title ids and title entity ids (N, L) -> (N, len(windows) * F).
    ``images[i]`` is the (F, W, C, D) repacked image of ``convs[2 i]`` (the (F, C, W, D) ``conv_filters.{W}.weight``), kept by
    the caller; ``convs`` = (weight, bias) per window, in ``windows`` order.  ``ctx_table`` None: ``use_context=False``."""

    @staticmethod
    def forward(ctx, ids, entity_ids, order, windows, images, grad_bufs, word, ent, ctx_table, T, b, *convs):
        lib = _lib.load()
        ids = _chk(ids, torch.int64, "title")
        entity_ids = _chk(entity_ids, torch.int64, "title_entities")
        if ids.dim() != 2 or entity_ids.shape != ids.shape:
            raise ValueError("newsreclib_amd: title and title_entities must both be (num_news, num_tokens)")
        word, ent, T, b = [_chk(t, torch.float32, n) for t, n in zip((word, ent, T, b), (
            "text_embedding_layer.weight", "entity_embedding_layer.weight", "transform_matrix", "transform_bias"))]
        if ctx_table is not None:
            ctx_table = _chk(ctx_table, torch.float32, "context_embedding_layer.weight")
        weights = [_chk(t, torch.float32, "conv_filters weight") for t in convs[0::2]]
        biases = [_chk(t, torch.float32, "conv_filters bias") for t in convs[1::2]]
        images = [_chk(t, torch.float32, "conv image") for t in images]
        N, L = ids.shape
        p = _encoder_params(word, ent, ctx_table, T, b, images, biases, windows)
        nbytes = lib.nrl_dkn_encoder_workspace_bytes(ctypes.byref(p), N, L)
        if nbytes == 0:
            raise ValueError("newsreclib_amd: unsupported DKN encoder shapes")
        ws = ops.workspace(nbytes, ids.device)
        F_ = biases[0].shape[0]
        out = torch.empty((N, len(windows) * F_), dtype=torch.float32, device=ids.device)
        am = torch.empty((N, len(windows) * F_), dtype=torch.uint8, device=ids.device)
        _lib.check(lib.nrl_dkn_encoder_fwd(ctypes.byref(p), ids.data_ptr(), entity_ids.data_ptr(), N, L, out.data_ptr(),
                                           am.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "nrl_dkn_encoder_fwd")
        if saving(ctx):
            if order is None:
                order = _sort_positions(ids, word.shape[0])
            ctx.order_ready = order_event(order)
            ent_order = _sort_positions(entity_ids, ent.shape[0])     # one order, shared by both entity tables
            ctx.save_for_backward(ids, entity_ids, _chk(order, torch.int64, "order"), ent_order, out, am, word, ent,
                                  *([ctx_table] if ctx_table is not None else []), T, b, *images, *weights, *biases)
            ctx.has_ctx, ctx.windows, ctx.ws, ctx.grad_bufs = ctx_table is not None, tuple(windows), ws, grad_bufs
            ctx.engine, ctx.options = _lib.engine_code(), _lib.options_mask()
        return out

    @staticmethod
    def backward(ctx, d_out):
        lib = _lib.load()
        _lib.require_engine(ctx.engine, "the DKN news encoder")
        _lib.require_options(ctx.options, "the DKN news encoder")
        saved = list(ctx.saved_tensors)
        ids, entity_ids, order, ent_order, out, am, word, ent = saved[:8]
        rest = saved[8:]
        ctx_table = rest.pop(0) if ctx.has_ctx else None
        T, b = rest[:2]
        nw = len(ctx.windows)
        images, weights, biases = rest[2:2 + nw], rest[2 + nw:2 + 2 * nw], rest[2 + 2 * nw:2 + 3 * nw]
        wait_order(ctx.order_ready)
        N, L = ids.shape
        d_out = _chk(d_out, torch.float32, "d_out")
        params = [word, ent] + ([ctx_table] if ctx_table is not None else []) + [T, b]
        convs = [t for pair in zip(weights, biases) for t in pair]
        bufs, rets = _grad_targets(params + convs, ctx.grad_bufs)
        pb, cb = bufs[:len(params)], bufs[len(params):]
        if ctx_table is None:
            pb = pb[:2] + [None] + pb[2:]
        g = NrlDknGrads(_ptr(pb[0]), _ptr(pb[1]), _ptr(pb[2]), _ptr(pb[3]), _ptr(pb[4]),
                        (ctypes.c_void_p * 4)(*([t.data_ptr() for t in cb[0::2]] + [None] * (4 - nw))),
                        (ctypes.c_void_p * 4)(*([t.data_ptr() for t in cb[1::2]] + [None] * (4 - nw))))
        p = _encoder_params(word, ent, ctx_table, T, b, images, biases, ctx.windows)
        _lib.check(lib.nrl_dkn_encoder_bwd(ctypes.byref(p), ctypes.byref(g), ids.data_ptr(), order.data_ptr(),
                                           entity_ids.data_ptr(), ent_order.data_ptr(), N, L, out.data_ptr(), am.data_ptr(),
                                           d_out.data_ptr(), ctx.ws.data_ptr(), ctx.ws.numel(), _stream()),
                   "nrl_dkn_encoder_bwd")
        ctx.ws = None
        rp, rc = rets[:len(params)], rets[len(params):]
        if ctx_table is None:
            rp = rp[:2] + [None] + rp[2:]
        return (None, None, None, None, None, None, *rp, *rc)


def _click_params(att: Sequence[torch.Tensor], pred: Sequence[torch.Tensor]) -> NrlDknClickParams:
    return NrlDknClickParams(*[t.data_ptr() for t in att], *[t.data_ptr() for t in pred], int(att[0].shape[0]))


class DknClickFn(GradAwareFunction):
    """DKN ``UserEncoder`` (user/dkn.py:59-107) + ``DNNPredictor`` (click_predictor.py:40-45) + the padded-candidate mask
    (dkn_module.py:237-238) on the ragged rows: hist (n_hist, dim), cand (n_cand, dim) with their offsets (B + 1).
    ``att`` / ``pred``: (w1, b1, w2, b2) of ``user_encoder.dnn`` / ``click_predictor.dnn``.  -> scores (B, max_cand)."""

    @staticmethod
    def forward(ctx, hist, hist_offsets, max_hist, cand, cand_offsets, max_cand, aw1, ab1, aw2, ab2, pw1, pb1, pw2, pb2):
        lib = _lib.load()
        hist = _chk(hist, torch.float32, "hist_news_vector")
        cand = _chk(cand, torch.float32, "cand_news_vector")
        hist_offsets = _chk(hist_offsets, torch.int64, "hist_offsets")
        cand_offsets = _chk(cand_offsets, torch.int64, "cand_offsets")
        att = [_chk(t, torch.float32, "user_encoder.dnn") for t in (aw1, ab1, aw2, ab2)]
        pred = [_chk(t, torch.float32, "click_predictor.dnn") for t in (pw1, pb1, pw2, pb2)]
        B, dim = cand_offsets.shape[0] - 1, cand.shape[1]
        Hd = att[0].shape[0]
        if hist.dim() != 2 or hist.shape[1] != dim or att[0].shape != (Hd, 2 * dim) or pred[0].shape != (Hd, 2 * dim) \
                or hist_offsets.shape != (B + 1,) or att[2].numel() != Hd or pred[2].numel() != Hd:
            raise ValueError("newsreclib_amd: inconsistent DKN user-encoder / click-predictor shapes")
        p = _click_params(att, pred)
        scores = torch.empty((B, int(max_cand)), dtype=torch.float32, device=cand.device)
        user = torch.empty((B, dim), dtype=torch.float32, device=cand.device)
        _lib.check(lib.nrl_dkn_click_fwd(ctypes.byref(p), hist.data_ptr(), hist_offsets.data_ptr(), int(max_hist),
                                         cand.data_ptr(), cand_offsets.data_ptr(), B, int(max_cand), dim, scores.data_ptr(),
                                         user.data_ptr(), _stream()), "nrl_dkn_click_fwd")
        if saving(ctx):
            ctx.save_for_backward(hist, hist_offsets, cand, cand_offsets, user, *att, *pred)
            ctx.dims = (int(max_hist), int(max_cand))
        return scores

    @staticmethod
    def backward(ctx, d_scores):
        lib = _lib.load()
        hist, hist_offsets, cand, cand_offsets, user, *params = ctx.saved_tensors
        att, pred = params[:4], params[4:]
        max_hist, max_cand = ctx.dims
        B, dim = user.shape
        d_scores = _chk(d_scores, torch.float32, "d_scores")
        bufs, rets = _grad_targets(att + pred, None)
        g = NrlDknClickGrads(*[t.data_ptr() for t in bufs])
        d_hist, d_cand = torch.empty_like(hist), torch.empty_like(cand)
        ws = ops.workspace(lib.nrl_dkn_click_workspace_bytes(B, max_cand, dim, att[0].shape[0]), cand.device)
        p = _click_params(att, pred)
        _lib.check(lib.nrl_dkn_click_bwd(ctypes.byref(p), ctypes.byref(g), hist.data_ptr(), hist_offsets.data_ptr(),
                                         max_hist, cand.data_ptr(), cand_offsets.data_ptr(), B, max_cand, dim,
                                         user.data_ptr(), d_scores.data_ptr(), d_hist.data_ptr(), d_cand.data_ptr(),
                                         ws.data_ptr(), ws.numel(), _stream()), "nrl_dkn_click_bwd")
        return (d_hist, None, None, d_cand, None, None, *rets)


# ---- the click predictor factored for a full-catalogue ranking (ops.topk_relu_scores) -------------------------------------------
def _pred_params(pred: Sequence[torch.Tensor], dim: int):
    pred = [_chk(t, torch.float32, "click_predictor.dnn") for t in pred]
    Hd = pred[0].shape[0]
    if pred[0].shape != (Hd, 2 * dim) or pred[1].numel() != Hd or pred[2].numel() != Hd or pred[3].numel() != 1:
        raise ValueError("newsreclib_amd: inconsistent DKN click-predictor shapes")
    return pred, int(Hd)


def dkn_user_query(hist: torch.Tensor, hist_offsets: torch.Tensor, max_hist: int, att: Sequence[torch.Tensor],
                   pred: Sequence[torch.Tensor]):
    """``nrl_dkn_user_query``: hist (n_hist, dim) with hist_offsets (B + 1) -> (user (B, dim), q (B, Hd)).  ``user`` is the DKN
    user vector, the bits ``DknClickFn`` computes for the same histories; ``q = user Wu^T + b1`` is the user's share of the click
    predictor's first layer (``pred[0] = [Wc | Wu]``).  An empty history gives ``user = 0`` and ``q = b1``.  No gradient."""
    lib = _lib.load()
    hist = _chk(hist, torch.float32, "hist_news_vector")
    hist_offsets = _chk(hist_offsets, torch.int64, "hist_offsets")
    if hist.dim() != 2 or hist_offsets.dim() != 1 or hist_offsets.numel() < 1:
        raise ValueError("newsreclib_amd: hist (n_hist, dim) and hist_offsets (B + 1) expected")
    B, dim = int(hist_offsets.numel()) - 1, int(hist.shape[1])
    att = [_chk(t, torch.float32, "user_encoder.dnn") for t in att]
    pred, Hd = _pred_params(pred, dim)
    if att[0].shape != (Hd, 2 * dim) or att[2].numel() != Hd:
        raise ValueError("newsreclib_amd: inconsistent DKN user-encoder / click-predictor shapes")
    user = torch.empty((B, dim), dtype=torch.float32, device=hist.device)
    q = torch.empty((B, Hd), dtype=torch.float32, device=hist.device)
    p = _click_params(att, pred)
    _lib.check(lib.nrl_dkn_user_query(ctypes.byref(p), hist.data_ptr(), hist_offsets.data_ptr(), int(max_hist), B, dim,
                                      user.data_ptr(), q.data_ptr(), _stream()), "nrl_dkn_user_query")
    return user, q


def dkn_cand_project(rows: torch.Tensor, pred: Sequence[torch.Tensor]) -> torch.Tensor:
    """``nrl_dkn_cand_project``: rows (N, dim) -> (N, Hd) = rows Wc^T, the news' share of the click predictor's first layer
    (``pred[0] = [Wc | Wu]``), without the bias.  A row's result does not depend on the other rows.  No gradient."""
    lib = _lib.load()
    rows = _chk(rows, torch.float32, "rows")
    if rows.dim() != 2:
        raise ValueError("newsreclib_amd: rows (N, dim) expected")
    N, dim = int(rows.shape[0]), int(rows.shape[1])
    pred, Hd = _pred_params(pred, dim)
    out = torch.empty((N, Hd), dtype=torch.float32, device=rows.device)
    # (the attention half of the parameter struct is not read by this entry: the predictor's own tensors stand in)
    p = _click_params(pred, pred)
    _lib.check(lib.nrl_dkn_cand_project(ctypes.byref(p), rows.data_ptr(), N, dim, out.data_ptr(), _stream()),
               "nrl_dkn_cand_project")
    return out
