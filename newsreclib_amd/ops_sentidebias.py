"""``torch.autograd.Function`` wrappers of the SentiDebias entry points (``nrl_sentidebias.hip``).  Same conventions as ``ops.py``.

Every sentiment vector of the model is a row of the ``(S, D)`` table ``T = tanh(E W^T + b)`` (``sentiment_table``: ``S`` rows, torch
ops); everything that scales with the news rows or the history slots is a kernel here, and every function skips the outputs its
inputs' ``requires_grad`` flags do not ask for (phase G of the adversarial step wants activation gradients and no discriminator
weight gradients, phase D the reverse).  The gradients of ``T``, ``linear2.weight`` and ``linear2.bias`` are per-64-row slabs added
in order (``nrl_miner_slab_sum``): bit-reproducible."""
from __future__ import annotations

import torch

from . import _lib, ops
from .ops import GradAwareFunction, _chk, _stream, saving

MAX_CLASSES = 8


def _f32(shape, like):
    return torch.empty(shape, dtype=torch.float32, device=like.device)


def _slab_sum(lib, slabs, n_slabs, width, out):
    _lib.check(lib.nrl_miner_slab_sum(slabs.data_ptr(), n_slabs, width, 1.0, out.data_ptr(), _stream()), "nrl_miner_slab_sum")


def sentiment_table(encoder) -> torch.Tensor:
    """``SentimentEncoder.forward`` on its ``S`` ids (aspect.py: ``tanh(linear(embedding(id)))``): the (S, D) table.  Row
    ``padding_idx`` of the embedding is detached: the reference's embedding backward leaves it without a gradient (the vector of
    that id still moves through ``linear.weight`` / ``linear.bias``)."""
    w = encoder.embedding_layer.weight
    pad = getattr(encoder.embedding_layer, "padding_idx", None)
    if pad is not None:
        w = torch.cat([w[:pad], w[pad:pad + 1].detach(), w[pad + 1:]], dim=0)
    return torch.tanh(torch.nn.functional.linear(w, encoder.linear.weight, encoder.linear.bias))


class RowCosFn(GradAwareFunction):
    """news (N, D), T (S, D), ids (N) with the history rows first -> (2): the mean over the history rows and over the candidate
    rows of ``cos(news_r, T[id_r])`` with the reference's ``dot / (1e-8 + |a| |b|)`` (senti_debias_module.py:208-229)."""

    @staticmethod
    def forward(ctx, news, T, ids, n_hist):
        lib = _lib.load()
        news, T, ids = _chk(news, torch.float32, "news vectors"), _chk(T, torch.float32, "sentiment table"), \
            _chk(ids, torch.int64, "sentiment ids")
        N, D = news.shape
        S = T.shape[0]
        if T.shape != (S, D) or ids.shape != (N,) or not 0 <= n_hist <= N:
            raise ValueError("newsreclib_amd: inconsistent SentiDebias row-cosine shapes")
        partial, out = _f32((2 * lib.nrl_sd_num_slabs(N),), news), _f32((2,), news)
        _lib.check(lib.nrl_sd_rowcos_fwd(news.data_ptr(), ids.data_ptr(), T.data_ptr(), N, int(n_hist), D, S, partial.data_ptr(),
                                         out.data_ptr(), _stream()), "nrl_sd_rowcos_fwd")
        if saving(ctx):
            ctx.save_for_backward(news, T, ids)
            ctx.n_hist = int(n_hist)
        return out

    @staticmethod
    def backward(ctx, d_out):
        lib = _lib.load()
        news, T, ids = ctx.saved_tensors
        N, D = news.shape
        S = T.shape[0]
        d_out = _chk(d_out, torch.float32, "d_out")
        need_news, need_T = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        d_news = torch.empty_like(news) if need_news else None
        n_slabs = lib.nrl_sd_num_slabs(N)
        slabs = _f32((n_slabs, S * D), news) if need_T else None
        _lib.check(lib.nrl_sd_rowcos_bwd(news.data_ptr(), ids.data_ptr(), T.data_ptr(), d_out.data_ptr(), N, ctx.n_hist, D, S,
                                         d_news.data_ptr() if need_news else None, slabs.data_ptr() if need_T else None,
                                         _stream()), "nrl_sd_rowcos_bwd")
        d_T = None
        if need_T:
            d_T = torch.empty_like(T)
            _slab_sum(lib, slabs, n_slabs, S * D, d_T)
        return d_news, d_T, None, None


class SentHistFn(GradAwareFunction):
    """The dense sentiment history (B, H, D) of ``to_dense_batch(sentiment_encoder(ids), batch_hist)`` (:176-177) from ids and T:
    ``T[id]`` at real slots -- id 0 included: ``tanh(linear.bias)`` -- and ZERO at padded slots."""

    @staticmethod
    def forward(ctx, T, ids, hist_off, B, H):
        lib = _lib.load()
        T, ids, off = _chk(T, torch.float32, "sentiment table"), _chk(ids, torch.int64, "sentiment ids"), \
            _chk(hist_off, torch.int64, "hist_offsets")
        S, D = T.shape
        if off.numel() != B + 1:
            raise ValueError("newsreclib_amd: inconsistent SentiDebias history shapes")
        out = _f32((B, H, D), T)
        _lib.check(lib.nrl_sd_hist_fwd(ids.data_ptr(), off.data_ptr(), T.data_ptr(), B, H, D, S, ids.numel(), out.data_ptr(),
                                       _stream()), "nrl_sd_hist_fwd")
        if saving(ctx):
            ctx.save_for_backward(ids, off)
            ctx.cfg = (int(B), int(H), int(D), int(S))
        return out

    @staticmethod
    def backward(ctx, d_out):
        lib = _lib.load()
        ids, off = ctx.saved_tensors
        B, H, D, S = ctx.cfg
        d_out = _chk(d_out, torch.float32, "d_out")
        n_slabs = lib.nrl_sd_num_slabs(B * H)
        slabs = _f32((n_slabs, S * D), d_out)
        _lib.check(lib.nrl_sd_hist_bwd(d_out.data_ptr(), ids.data_ptr(), off.data_ptr(), B, H, D, S, ids.numel(), slabs.data_ptr(),
                                       _stream()), "nrl_sd_hist_bwd")
        d_T = _f32((S, D), d_out)
        _slab_sum(lib, slabs, n_slabs, S * D, d_T)
        return d_T, None, None, None, None


class LateUserFn(GradAwareFunction):
    """Late fusion (:197-205): the history sum of the sentiment vectors divided by the history size =
    ``(class counts / n_b) @ T``, with no dense tensor.  T (S, D) -> (B, D)."""

    @staticmethod
    def forward(ctx, T, ids, hist_off, B):
        lib = _lib.load()
        T, ids, off = _chk(T, torch.float32, "sentiment table"), _chk(ids, torch.int64, "sentiment ids"), \
            _chk(hist_off, torch.int64, "hist_offsets")
        S, D = T.shape
        if off.numel() != B + 1:
            raise ValueError("newsreclib_amd: inconsistent SentiDebias history shapes")
        frac, u = _f32((B, S), T), _f32((B, D), T)
        _lib.check(lib.nrl_sd_late_fwd(ids.data_ptr(), off.data_ptr(), T.data_ptr(), B, D, S, ids.numel(), frac.data_ptr(),
                                       u.data_ptr(), _stream()), "nrl_sd_late_fwd")
        if saving(ctx):
            ctx.save_for_backward(frac)
        return u

    @staticmethod
    def backward(ctx, d_u):
        lib = _lib.load()
        (frac,) = ctx.saved_tensors
        B, S = frac.shape
        d_u = _chk(d_u, torch.float32, "d_user")
        D = d_u.shape[1]
        d_T = _f32((S, D), d_u)
        _lib.check(lib.nrl_sd_bt_matmul(frac.data_ptr(), d_u.data_ptr(), B, S, D, d_T.data_ptr(), _stream()), "nrl_sd_bt_matmul")
        return d_T, None, None, None


class CombinedScoresFn(GradAwareFunction):
    """``bias_free_scores + DotProduct(u_aware, dense candidate sentiment vectors)`` (:249-255): the bias-aware part is
    ``(u_aware @ T^T)[b, class of candidate c]`` at real slots and 0 at padded ones (their sentiment vectors are zero rows).
    free (B, C), u_aware (B, D), T (S, D), ids (n_cand) -> (B, C)."""

    @staticmethod
    def forward(ctx, free, u, T, ids, cand_off):
        lib = _lib.load()
        free, u, T = _chk(free, torch.float32, "bias-free scores"), _chk(u, torch.float32, "bias-aware user"), \
            _chk(T, torch.float32, "sentiment table")
        ids, off = _chk(ids, torch.int64, "sentiment ids"), _chk(cand_off, torch.int64, "cand_offsets")
        B, C = free.shape
        S, D = T.shape
        if u.shape != (B, D) or off.numel() != B + 1:
            raise ValueError("newsreclib_amd: inconsistent SentiDebias score shapes")
        out = _f32((B, C), free)
        _lib.check(lib.nrl_sd_scores_fwd(u.data_ptr(), T.data_ptr(), ids.data_ptr(), off.data_ptr(), free.data_ptr(), B, C, D, S,
                                         ids.numel(), None, out.data_ptr(), _stream()), "nrl_sd_scores_fwd")
        if saving(ctx):
            ctx.save_for_backward(u, T, ids, off)
            ctx.C = int(C)
        return out

    @staticmethod
    def backward(ctx, d_out):
        lib = _lib.load()
        u, T, ids, off = ctx.saved_tensors
        B, D = u.shape
        S = T.shape[0]
        d_out = _chk(d_out, torch.float32, "d_scores")
        d_u = d_T = None
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            dP, d_u = _f32((B, S), u), torch.empty_like(u)
            _lib.check(lib.nrl_sd_scores_bwd(d_out.data_ptr(), T.data_ptr(), ids.data_ptr(), off.data_ptr(), B, ctx.C, D, S,
                                             ids.numel(), dP.data_ptr(), d_u.data_ptr(), _stream()), "nrl_sd_scores_bwd")
            if ctx.needs_input_grad[2]:
                d_T = torch.empty_like(T)
                _lib.check(lib.nrl_sd_bt_matmul(dP.data_ptr(), u.data_ptr(), B, S, D, d_T.data_ptr(), _stream()), "nrl_sd_bt_matmul")
        return (d_out if ctx.needs_input_grad[0] else None), d_u, d_T, None, None


class DiscriminatorLossFn(GradAwareFunction):
    """``Discriminator`` + ``adversarial_loss`` of both sides (senti_debias_module.py:45-51,406-411,495-496): news (N, D) with the
    history rows first -> (2) = [adv(hist), adv(cand)].  ``tanh(linear1)`` runs on the GEMM engine (``nrl_linear_act_fwd``); the
    fused tail takes the hidden rows through linear2, log-softmax and the cross entropy against the one-hot the reference writes
    at column ``id - 1`` (:409: id 0 wraps to the last column), each side averaged over its own rows.  The backward's tail hands
    ``d_pre`` (the ``1 - h^2`` factor applied) to the engine's ``nrl_linear_bwd_img``, which is asked for the activation gradient
    only when the news rows need one and for the weight gradients only when linear1 does."""

    @staticmethod
    def forward(ctx, news, w1, b1, w2, b2, ids, n_hist):
        lib = _lib.load()
        news, ids = _chk(news, torch.float32, "news vectors"), _chk(ids, torch.int64, "sentiment ids")
        w1, b1, w2, b2 = (_chk(t, torch.float32, n) for t, n in zip((w1, b1, w2, b2), ("linear1.weight", "linear1.bias",
                                                                                       "linear2.weight", "linear2.bias")))
        N, D = news.shape
        Hd, O = w1.shape[0], w2.shape[0]
        if w1.shape != (Hd, D) or b1.shape != (Hd,) or w2.shape != (O, Hd) or b2.shape != (O,) or ids.shape != (N,) or \
                not 0 <= n_hist <= N:
            raise ValueError("newsreclib_amd: inconsistent SentiDebias discriminator shapes")
        if O > MAX_CLASSES:
            raise NotImplementedError(f"newsreclib_amd: the discriminator tail takes at most {MAX_CLASSES} outputs")
        ws = ops.workspace(lib.nrl_linear_act_workspace_bytes(N, Hd, D), news.device)
        h = _f32((N, Hd), news)
        _lib.check(lib.nrl_linear_act_fwd(news.data_ptr(), w1.data_ptr(), b1.data_ptr(), N, Hd, D, 1, h.data_ptr(), ws.data_ptr(),
                                          ws.numel(), _stream()), "nrl_linear_act_fwd")
        partial, out = _f32((2 * lib.nrl_sd_num_slabs(N),), news), _f32((2,), news)
        _lib.check(lib.nrl_sd_disc_tail_fwd(h.data_ptr(), w2.data_ptr(), b2.data_ptr(), ids.data_ptr(), N, int(n_hist), Hd, O,
                                            partial.data_ptr(), out.data_ptr(), _stream()), "nrl_sd_disc_tail_fwd")
        if saving(ctx):
            ctx.save_for_backward(news, w1, h, w2, b2, ids)
            ctx.n_hist, ctx.engine = int(n_hist), _lib.engine_code()
        return out

    @staticmethod
    def backward(ctx, d_out):
        lib = _lib.load()
        _lib.require_engine(ctx.engine, "the SentiDebias discriminator")
        news, w1, h, w2, b2, ids = ctx.saved_tensors
        N, D = news.shape
        Hd, O = w1.shape[0], w2.shape[0]
        d_out = _chk(d_out, torch.float32, "d_out")
        need_x, need_1 = ctx.needs_input_grad[0], ctx.needs_input_grad[1] or ctx.needs_input_grad[2]
        need_2 = ctx.needs_input_grad[3] or ctx.needs_input_grad[4]
        d_pre = torch.empty_like(h)
        n_slabs, width = lib.nrl_sd_num_slabs(N), lib.nrl_sd_disc_slab_width(Hd, O)
        slabs = _f32((n_slabs, width), news) if need_2 else None
        _lib.check(lib.nrl_sd_disc_tail_bwd(h.data_ptr(), w2.data_ptr(), b2.data_ptr(), ids.data_ptr(), d_out.data_ptr(), N,
                                            ctx.n_hist, Hd, O, d_pre.data_ptr(), slabs.data_ptr() if need_2 else None, _stream()),
                   "nrl_sd_disc_tail_bwd")
        d_w2 = d_b2 = d_x = d_w1 = d_b1 = None
        if need_2:
            both = _f32((width,), news)
            _slab_sum(lib, slabs, n_slabs, width, both)
            d_w2, d_b2 = both[:O * Hd].view(O, Hd), both[O * Hd:O * Hd + O]
        if need_x or need_1:
            if need_x:
                d_x = torch.empty_like(news)
            if need_1:                                   # (the engine ADDS its weight gradients)
                d_w1, d_b1 = torch.zeros_like(w1), torch.zeros((Hd,), dtype=torch.float32, device=news.device)
            ws = ops.workspace(lib.nrl_linear_workspace_bytes(Hd, D), news.device)
            ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
            _lib.check(lib.nrl_linear_bwd_img(news.data_ptr(), w1.data_ptr(), d_pre.data_ptr(), N, Hd, D, ptr(d_x), ptr(d_w1),
                                              ptr(d_b1), ws.data_ptr(), ws.numel(), 0, _stream()), "nrl_linear_bwd")
        return d_x, d_w1, d_b1, d_w2, d_b2, None, None
