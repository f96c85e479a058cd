"""``torch.autograd.Function`` wrappers of the MINER entry points (``nrl_miner.hip``).  Same conventions as ``ops.py``.

History and candidate rows are FLAT here (``(n_hist, D)`` / ``(n_cand, D)`` with the ``(B + 1)`` offsets of ``attach_layout``):
the padded rows of the reference's dense history only add a closed-form term to the poly-attention softmax (``PolyFn``).

Dropout streams of the MINER module (the library's counter-based mask spec, ``oracle/nrms_oracle.py``; flat row-major index
of the masked tensor, one stream per mask).  Every other model draws from 0-9 (news encoders) and 16 + 3 i (CAUM's candidate
slots); MINER's four masks sit at ``0x4D49 + k`` so that no configuration of another model shares a stream with them:
  * ``REDUCE_HIST`` / ``REDUCE_CAND``: the dropout after ``reduce_dim`` of the history / candidate call, over (rows, news_embed_dim);
  * ``CATEG_HIST`` / ``CATEG_CAND``: the category encoder's dropout of the history / candidate call, over (rows, categ_dim)."""
from __future__ import annotations

import torch

from . import _lib, ops
from .ops import GradAwareFunction, _chk, _stream, saving

STREAM_BASE = 0x4D49
REDUCE_HIST, REDUCE_CAND, CATEG_HIST, CATEG_CAND = (STREAM_BASE + k for k in range(4))

SCORE_MODES = {"max": 0, "mean": 1, "weighted": 2}
COS_EPS = 1e-8          # components/utils.py:29-30


def _check(rc, name):
    _lib.check(rc, name)


def _f32(shape, like):
    return torch.empty(shape, dtype=torch.float32, device=like.device)


class BiasFreeLinearFn(GradAwareFunction):
    """``act(x W^T)`` of a bias-free ``nn.Linear`` (``PolyAttention.linear`` with tanh, ``TargetAwareAttention.linear`` without):
    x (M, K), w (N, K) -> (M, N).  Forward and activation gradient run on the GEMM engines through the existing entries with a
    zero bias vector passed in (their behaviour for other callers is unchanged); the WEIGHT gradient does not: the engines add
    split partial sums atomically, so it runs on ``nrl_miner_wgrad`` (slabs of 64 rows, then the slabs in order) and is
    bit-reproducible."""

    @staticmethod
    def forward(ctx, x, w, act):
        lib = _lib.load()
        x, w = _chk(x, torch.float32, "input"), _chk(w, torch.float32, "weight")
        if x.dim() != 2 or w.dim() != 2 or x.shape[1] != w.shape[1] or act not in (None, "tanh"):
            raise ValueError("newsreclib_amd: inconsistent bias-free linear arguments")
        M, K = x.shape
        N = w.shape[0]
        zeros = torch.zeros((N,), dtype=torch.float32, device=x.device)
        c = _f32((M, N), x)
        if act == "tanh":
            ws = ops.workspace(lib.nrl_linear_act_workspace_bytes(M, N, K), x.device)
            _check(lib.nrl_linear_act_fwd(x.data_ptr(), w.data_ptr(), zeros.data_ptr(), M, N, K, 1, c.data_ptr(), ws.data_ptr(),
                                          ws.numel(), _stream()), "nrl_linear_act_fwd")
        else:
            ws = ops.workspace(lib.nrl_linear_workspace_bytes(N, K), x.device)
            _check(lib.nrl_linear_fwd_img(x.data_ptr(), w.data_ptr(), zeros.data_ptr(), M, N, K, c.data_ptr(), ws.data_ptr(),
                                          ws.numel(), 0, _stream()), "nrl_linear_fwd")
        if saving(ctx):
            ctx.save_for_backward(x, w, c if act == "tanh" else None)
            ctx.engine = _lib.engine_code()
        return c

    @staticmethod
    def backward(ctx, d_c):
        lib = _lib.load()
        _lib.require_engine(ctx.engine, "bias-free linear")
        x, w, c = ctx.saved_tensors
        M, K = x.shape
        N = w.shape[0]
        d_pre = _chk(d_c, torch.float32, "d_out")
        if c is not None:
            d_c, d_pre = d_pre, torch.empty_like(c)
            _check(lib.nrl_miner_tanh_grad(d_c.data_ptr(), c.data_ptr(), c.numel(), d_pre.data_ptr(), _stream()),
                   "nrl_miner_tanh_grad")
        d_x = d_w = None
        if ctx.needs_input_grad[0]:
            d_x = torch.empty_like(x)
            ws = ops.workspace(lib.nrl_linear_workspace_bytes(N, K), x.device)
            _check(lib.nrl_linear_bwd_img(None, w.data_ptr(), d_pre.data_ptr(), M, N, K, d_x.data_ptr(), None, None,
                                          ws.data_ptr(), ws.numel(), 0, _stream()), "nrl_linear_bwd")
        if ctx.needs_input_grad[1]:
            d_w = torch.empty_like(w)
            ws = ops.workspace(lib.nrl_miner_wgrad_workspace_bytes(M, N, K), x.device)
            _check(lib.nrl_miner_wgrad(d_pre.data_ptr(), x.data_ptr(), M, N, K, d_w.data_ptr(), ws.data_ptr(), ws.numel(),
                                       _stream()), "nrl_miner_wgrad")
        return d_x, d_w, None


class CategBiasFn(GradAwareFunction):
    """Category bias per flat history row (miner_module.py:270-285 + the ``mean(dim=2)`` of attention.py:113): the mean over
    ALL candidate rows of the batch of cos(h_t, c), the user's own candidates counted as 0 -- as
    ``hh_t . (S_all - S_own[user]) / n_cand`` over the unit rows (no epsilon).  hc (n_hist, Dc), cc (n_cand, Dc) -> (n_hist)."""

    @staticmethod
    def forward(ctx, hc, cc, batch_hist, batch_cand, hist_off, cand_off, B):
        lib = _lib.load()
        hc, cc = _chk(hc, torch.float32, "history category rows"), _chk(cc, torch.float32, "candidate category rows")
        bh, bc = _chk(batch_hist, torch.int64, "batch_hist"), _chk(batch_cand, torch.int64, "batch_cand")
        ho, co = _chk(hist_off, torch.int64, "hist_offsets"), _chk(cand_off, torch.int64, "cand_offsets")
        nh, Dc = hc.shape
        nc = cc.shape[0]
        if cc.shape[1] != Dc or bh.shape[0] != nh or bc.shape[0] != nc or ho.numel() != B + 1 or co.numel() != B + 1:
            raise ValueError("newsreclib_amd: inconsistent MINER category-bias shapes")
        ws = ops.workspace(lib.nrl_miner_categ_bias_workspace_bytes(B, nh, nc, Dc), hc.device)
        bias = _f32((nh,), hc)
        _check(lib.nrl_miner_categ_bias_fwd(hc.data_ptr(), cc.data_ptr(), bh.data_ptr(), co.data_ptr(), B, nh, nc, Dc,
                                            bias.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "nrl_miner_categ_bias_fwd")
        if saving(ctx):
            ctx.save_for_backward(hc, cc, bc, ho, bias)
            ctx.ws, ctx.B = ws, B
        return bias

    @staticmethod
    def backward(ctx, d_bias):
        lib = _lib.load()
        hc, cc, bc, ho, bias = ctx.saved_tensors
        d_bias = _chk(d_bias, torch.float32, "d_bias")
        d_hc, d_cc = torch.empty_like(hc), torch.empty_like(cc)
        _check(lib.nrl_miner_categ_bias_bwd(d_bias.data_ptr(), hc.data_ptr(), cc.data_ptr(), ho.data_ptr(), bc.data_ptr(),
                                            bias.data_ptr(), ctx.B, hc.shape[0], cc.shape[0], hc.shape[1], d_hc.data_ptr(),
                                            d_cc.data_ptr(), ctx.ws.data_ptr(), ctx.ws.numel(), _stream()),
               "nrl_miner_categ_bias_bwd")
        return d_hc, d_cc, None, None, None, None, None


class PolyFn(GradAwareFunction):
    """``PolyAttention`` after its projection (attention.py:110-122): E (n_hist, D), P = tanh(E W^T) (n_hist, Cd),
    codes (K, Cd), bias (n_hist) or None -> user_vector (B, K, D).  The reference fills the ``max_hist - n_b`` padded positions
    of user b with 1e-30 (not -inf), so they take part in the softmax; their embeddings are zero, so they only add
    ``(max_hist - n_b) * exp(1e-30 - max)`` to the denominator."""

    @staticmethod
    def forward(ctx, E, P, codes, bias, hist_off, B, max_hist):
        lib = _lib.load()
        E, P, codes = _chk(E, torch.float32, "embeddings"), _chk(P, torch.float32, "projection"), \
            _chk(codes, torch.float32, "context_codes")
        bias = _chk(bias, torch.float32, "bias") if bias is not None else None
        ho = _chk(hist_off, torch.int64, "hist_offsets")
        nh, D = E.shape
        K, Cd = codes.shape
        if P.shape != (nh, Cd) or ho.numel() != B + 1 or (bias is not None and bias.shape != (nh,)):
            raise ValueError("newsreclib_amd: inconsistent MINER poly-attention shapes")
        uv, A = _f32((B, K, D), E), _f32((B, K, max_hist), E)
        cfg = (int(B), int(max_hist), int(D), int(Cd), int(K))
        _check(lib.nrl_miner_poly_fwd(E.data_ptr(), P.data_ptr(), codes.data_ptr(), bias.data_ptr() if bias is not None else None,
                                      ho.data_ptr(), *cfg, uv.data_ptr(), A.data_ptr(), _stream()), "nrl_miner_poly_fwd")
        if saving(ctx):
            ctx.save_for_backward(E, P, codes, ho, A)
            ctx.cfg, ctx.has_bias = cfg, bias is not None
        return uv

    @staticmethod
    def backward(ctx, d_uv):
        lib = _lib.load()
        E, P, codes, ho, A = ctx.saved_tensors
        B, max_hist, D, Cd, K = ctx.cfg
        d_uv = _chk(d_uv, torch.float32, "d_user_vector")
        d_E, d_P, d_codes = torch.empty_like(E), torch.empty_like(P), torch.empty_like(codes)
        d_bias = _f32((E.shape[0],), E) if ctx.has_bias else None
        ws = ops.workspace(lib.nrl_miner_poly_workspace_bytes(B, K, Cd), E.device)
        _check(lib.nrl_miner_poly_bwd(d_uv.data_ptr(), E.data_ptr(), P.data_ptr(), codes.data_ptr(), A.data_ptr(), ho.data_ptr(),
                                      *ctx.cfg, d_E.data_ptr(), d_P.data_ptr(), d_codes.data_ptr(),
                                      d_bias.data_ptr() if d_bias is not None else None, ws.data_ptr(), ws.numel(), _stream()),
               "nrl_miner_poly_bwd")
        return d_E, d_P, d_codes, d_bias, None, None, None


class ScoreFn(GradAwareFunction):
    """Matching scores and their aggregation (miner_module.py:298-308, attention.py:162-166): cand (n_cand, D),
    user_vector (B, K, D), Z = user_vector Wt^T (B, K, D) for ``weighted`` (None otherwise) -> scores (B, max_cand), exactly 0
    at padded slots.  ``max`` routes its gradient to the (lowest) index of the maximum, as ``torch.max`` does."""

    @staticmethod
    def forward(ctx, cand, uv, Z, cand_off, B, max_cand, mode):
        lib = _lib.load()
        cand, uv = _chk(cand, torch.float32, "candidates"), _chk(uv, torch.float32, "user_vector")
        co = _chk(cand_off, torch.int64, "cand_offsets")
        code = SCORE_MODES[mode]
        nc, D = cand.shape
        K = uv.shape[1]
        if uv.shape != (B, K, D) or co.numel() != B + 1:
            raise ValueError("newsreclib_amd: inconsistent MINER score shapes")
        if K > 255:
            raise NotImplementedError("newsreclib_amd: the MINER score kernels take at most 255 context codes")
        if code == 2:
            Z = _chk(Z, torch.float32, "target-aware projection")
            if Z.shape != uv.shape:
                raise ValueError("newsreclib_amd: inconsistent MINER target-aware projection shape")
        save = saving(ctx)
        scores = _f32((B, max_cand), cand)
        G = S = W = arg = None
        if save and code == 2:
            G, S, W = torch.empty_like(uv), _f32((nc, K), cand), _f32((nc, K), cand)
        if save and code == 0:
            arg = torch.empty((nc,), dtype=torch.uint8, device=cand.device)
        ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
        cfg = (int(B), int(max_cand), int(D), int(K), code)
        _check(lib.nrl_miner_score_fwd(cand.data_ptr(), uv.data_ptr(), ptr(Z if code == 2 else None), co.data_ptr(), *cfg,
                                       scores.data_ptr(), ptr(G), ptr(S), ptr(W), ptr(arg), _stream()), "nrl_miner_score_fwd")
        if save:
            ctx.save_for_backward(cand, uv, Z if code == 2 else None, co, scores, G, S, W, arg)
            ctx.cfg = cfg
        return scores

    @staticmethod
    def backward(ctx, d_scores):
        lib = _lib.load()
        cand, uv, Z, co, scores, G, S, W, arg = ctx.saved_tensors
        d_scores = _chk(d_scores, torch.float32, "d_scores")
        d_cand, d_uv = torch.empty_like(cand), torch.empty_like(uv)
        d_Z = torch.empty_like(uv) if ctx.cfg[4] == 2 else None
        ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
        _check(lib.nrl_miner_score_bwd(d_scores.data_ptr(), scores.data_ptr(), cand.data_ptr(), uv.data_ptr(), ptr(Z), ptr(G),
                                       ptr(S), ptr(W), ptr(arg), co.data_ptr(), *ctx.cfg, d_cand.data_ptr(), d_uv.data_ptr(),
                                       ptr(d_Z), _stream()), "nrl_miner_score_bwd")
        return d_cand, d_uv, d_Z, None, None, None, None


class CosDisagreementFn(GradAwareFunction):
    """Mean over all groups * R * R entries of the per-group R x R cosine matrix of x (groups, R, D) with a zeroed diagonal,
    rows divided by ``norm + eps`` (miner_module.py:398-406): the MINER disagreement loss (eps 1e-8, one group per user) and,
    with one group of the B mean vectors and eps 0, its late-fusion form.  Two passes in a fixed order: per-group sums, then
    their sum."""

    @staticmethod
    def forward(ctx, x, eps):
        lib = _lib.load()
        x = _chk(x, torch.float32, "user_vector")
        G, R, D = x.shape
        partial, loss = _f32((G,), x), _f32((1,), x)
        scale = 1.0 / float(G * R * R)
        _check(lib.nrl_miner_cos_fwd(x.data_ptr(), G, R, D, float(eps), partial.data_ptr(), _stream()), "nrl_miner_cos_fwd")
        _check(lib.nrl_miner_slab_sum(partial.data_ptr(), G, 1, scale, loss.data_ptr(), _stream()), "nrl_miner_slab_sum")
        if saving(ctx):
            ctx.save_for_backward(x)
            ctx.cfg = (float(eps), scale)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, d_loss):
        lib = _lib.load()
        (x,) = ctx.saved_tensors
        G, R, D = x.shape
        eps, scale = ctx.cfg
        d_loss = _chk(d_loss.reshape(1), torch.float32, "d_loss")
        d_x = torch.empty_like(x)
        _check(lib.nrl_miner_cos_bwd(x.data_ptr(), G, R, D, eps, d_loss.data_ptr(), scale, d_x.data_ptr(), _stream()),
               "nrl_miner_cos_bwd")
        return d_x, None


def disagreement_loss(user_vector: torch.Tensor, late_fusion: bool) -> torch.Tensor:
    if late_fusion:          # torchmetrics' 2-D cosine across the users' mean vectors: plain L2 norm, no epsilon
        return CosDisagreementFn.apply(user_vector.unsqueeze(0), 0.0)
    return CosDisagreementFn.apply(user_vector, COS_EPS)
