"""``torch.autograd.Function`` wrappers around the C ABI (include/newsreclib_amd.h).

PyTorch is plumbing here: it owns device memory, streams and the autograd tape; every FLOP of the
path runs in the HIP library.  There is deliberately no eager fallback.

Parameter-gradient convention: when a ``grad_bufs`` tuple is supplied (the persistent ``.grad`` /
flat data-parallel gradient buffer of each parameter, see ``trainer.FlatParams``), the kernels
accumulate straight into those buffers and autograd receives ``None`` for the parameters --
no 84 MB zero-fill + add per encoder call.  Without it the functions return ordinary gradients.
"""
from __future__ import annotations

import ctypes
import math
import os
from typing import NamedTuple, Optional, Sequence, Tuple

import torch

from . import _lib
from ._lib import NrlBlockGrads, NrlBlockParams


_RAW_STREAM = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_GET_DEVICE = getattr(torch._C, "_cuda_getDevice", None)


def _stream() -> int:
    """Raw handle of the current HIP stream of the current device.  (Through the private fast path when this torch has it:
    ``torch.cuda.current_stream()`` builds a Stream object per call, ~9 us, and every ctypes wrapper asks once -- 16 calls = 0.15 ms
    of host time per train step, a sixth of the whole issue time at B = 32 where host and device are neck and neck.)"""
    if _RAW_STREAM is not None and _GET_DEVICE is not None:
        return _RAW_STREAM(_GET_DEVICE())
    return torch.cuda.current_stream().cuda_stream


def workspace(nbytes: int, device) -> torch.Tensor:
    """The one place a native workspace is allocated: a uint8 buffer of at least 256 bytes (never empty, so never a null pointer).
    The wrappers of the sibling modules call it as ``ops.workspace`` so that replacing this attribute reaches every call."""
    return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)


def _chk(t: torch.Tensor, dtype, name: str) -> torch.Tensor:
    if not t.is_cuda:
        raise RuntimeError(f"newsreclib_amd: `{name}` must live on the GPU (got {t.device}); "
                           "there is no CPU path")
    if t.dtype != dtype:
        raise TypeError(f"newsreclib_amd: `{name}` must be {dtype}, got {t.dtype}")
    return t if t.is_contiguous() else t.contiguous()


def _block_params(tensors: Sequence[torch.Tensor], heads: int, engine: int = 0, options: int = 0) -> NrlBlockParams:
    w_in, b_in, w_o, b_o, w_a, b_a, q_a = tensors
    D, Q = w_o.shape[0], w_a.shape[0]
    if w_in.shape != (3 * D, D) or b_in.shape != (3 * D,) or b_o.shape != (D,) or \
            w_a.shape != (Q, D) or b_a.shape != (Q,) or q_a.shape != (Q,):
        raise ValueError("newsreclib_amd: inconsistent MHSA/additive-attention parameter shapes")
    return NrlBlockParams(w_in.data_ptr(), b_in.data_ptr(), w_o.data_ptr(), b_o.data_ptr(),
                          w_a.data_ptr(), b_a.data_ptr(), q_a.data_ptr(), D, heads, Q, int(engine), int(options))


def _block_grads(bufs: Sequence[torch.Tensor]) -> NrlBlockGrads:
    return NrlBlockGrads(*[b.data_ptr() for b in bufs])


def _grad_targets(params: Sequence[torch.Tensor], grad_bufs: Optional[Sequence[Optional[torch.Tensor]]]):
    """-> (buffers the kernels add into, gradients to hand back to autograd)."""
    bufs, rets = [], []
    for i, p in enumerate(params):
        gb = grad_bufs[i] if grad_bufs is not None else None
        if gb is not None:
            if gb.shape != p.shape or not gb.is_contiguous() or gb.dtype != torch.float32:
                raise ValueError("newsreclib_amd: bad grad buffer")
            bufs.append(gb)
            rets.append(None)
        else:
            z = torch.zeros_like(p)
            bufs.append(z)
            rets.append(z)
    return bufs, rets


class deferred_weight_grads:
    """While active, ``UserEncoderFn.backward`` issues its three weight gradients (phase 2 of ``nrl_user_encoder_bwd_phase``)
    on ``stream`` instead of the caller's: they are ~100 us of few-row launches that nothing in the rest of the backward reads,
    so they run beside the chip-filling news-encoder backward instead of in front of it.  Leaving the context makes the
    current stream wait for ``stream`` (the join) -- do it before anything reads the gradient buffers (all-reduce, Adam).
    Only calls that accumulate into caller-owned ``grad_bufs`` defer (gradients handed back to autograd are consumed on the
    caller's stream right after the backward returns).  Used by ``trainer.NRMSTrainer``; off everywhere else."""

    _active = None

    def __init__(self, stream: "torch.cuda.Stream"):
        self.stream = stream
        self.keep = []          # tensors the side stream still reads: kept alive until the join

    def __enter__(self):
        deferred_weight_grads._active = self
        return self

    def __exit__(self, *exc):
        deferred_weight_grads._active = None
        self.joined = bool(self.keep)      # (the caller's stream now waits for everything issued on `stream` so far)
        if self.keep:
            torch.cuda.current_stream().wait_stream(self.stream)
            self.keep = []
        return False


import threading

_TLS = threading.local()


class GradAwareFunction(torch.autograd.Function):
    """``torch.autograd.Function`` whose ``forward`` can tell whether the CALLER had gradients enabled.  Inside ``forward``
    autograd has switched grad mode off, and ``ctx.needs_input_grad`` only reflects the inputs' ``requires_grad`` flags -- so
    a forward under ``torch.no_grad()`` over trainable parameters looked like a training forward and ran the training shapes of
    the kernels (activations saved, 0.57 + 0.23 ms instead of 0.41 + 0.18 ms for the two news-encoder launches of an evaluation
    batch: found in round 4 with a kernel trace of the evaluation forward).  ``apply`` records the caller's grad mode;
    ``saving(ctx)`` = "a backward can follow"."""

    @classmethod
    def apply(cls, *args, **kwargs):
        prev = getattr(_TLS, "grad", True)
        _TLS.grad = torch.is_grad_enabled()
        try:
            return super().apply(*args, **kwargs)
        finally:
            _TLS.grad = prev


def saving(ctx, inputs=None) -> bool:
    """True when the forward must keep what its backward needs: the caller has gradients enabled AND some (listed) input
    requires one."""
    need = ctx.needs_input_grad if inputs is None else ctx.needs_input_grad[inputs]
    return bool(getattr(_TLS, "grad", True)) and any(need)


class NewsEncoderFn(GradAwareFunction):
    """``MHSAAddAtt.forward`` (reference text.py:222-236): ids (N, L) -> (N, D)."""

    @staticmethod
    def forward(ctx, ids, emb, w_in, b_in, w_o, b_o, w_a, b_a, q_a, heads, p_drop, seed, stream0,
                grad_bufs, order=None, table_grad_hook=None):
        lib = _lib.load()
        ids = _chk(ids, torch.int64, "ids")
        params = [_chk(t, torch.float32, n) for t, n in zip(
            (emb, w_in, b_in, w_o, b_o, w_a, b_a, q_a),
            ("embedding", "in_proj_weight", "in_proj_bias", "out_proj.weight", "out_proj.bias",
             "linear.weight", "linear.bias", "query"))]
        emb = params[0]
        if ids.dim() != 2:
            raise ValueError("newsreclib_amd: token ids must be (num_news, num_tokens)")
        N, L = ids.shape
        V, D = emb.shape
        engine, options = _lib.engine_code(), _lib.options_word()
        bp = _block_params(params[1:], heads, engine, options)
        save = saving(ctx)
        ws_bytes = lib.nrl_news_encoder_workspace_bytes(N, L, D, heads, bp.query_dim)
        ws = workspace(ws_bytes, ids.device)
        out = torch.empty((N, D), dtype=torch.float32, device=ids.device)
        _lib.check(lib.nrl_news_encoder_fwd(ctypes.byref(bp), emb.data_ptr(), V, ids.data_ptr(), N, L,
                                            float(p_drop), int(seed), int(stream0), int(save),
                                            out.data_ptr(), ws.data_ptr(), ws.numel(), _stream()),
                   "nrl_news_encoder_fwd")
        if save:
            if order is None:
                # id-sorted visiting order for the table gradient (index bookkeeping on the int64 ids;
                # `prepare_batch` precomputes it once per batch so the step does not pay the sort)
                order = sort_positions_async(ids, V) if os.environ.get("NRL_SORT_ASYNC", "1") == "2" else sort_positions(ids, V)
            ctx.order_ready = order_event(order)      # (side-stream sort: the backward waits for it)
            order = _chk(order, torch.int64, "order")
            if order.numel() == ids.numel():          # an order from elsewhere (argsort): append the count of id-0 positions
                order = torch.cat([order.reshape(-1), (ids == 0).sum().reshape(1)])
            ctx.save_for_backward(ids, order, *params)
            ctx.ws, ctx.cfg, ctx.grad_bufs = ws, (heads, float(p_drop), int(seed), int(stream0)), grad_bufs
            ctx.table_grad_hook, ctx.engine, ctx.options = table_grad_hook, engine, options
        return out

    @staticmethod
    def backward(ctx, d_out):
        lib = _lib.load()
        ids, order, *params = ctx.saved_tensors
        emb = params[0]
        heads, p_drop, seed, stream0 = ctx.cfg
        N, L = ids.shape
        V, D = emb.shape
        d_out = _chk(d_out, torch.float32, "d_out")
        # the engine and the kernel-selection switches the forward ran under travel with the call: the backward reads the
        # workspace in the format the forward wrote, whatever the process defaults are by now
        bp = _block_params(params[1:], heads, ctx.engine, ctx.options)
        bufs, rets = _grad_targets(params, ctx.grad_bufs)
        bg = _block_grads(bufs[1:])
        ws = ctx.ws
        wait_order(ctx.order_ready)
        def run(phase):
            _lib.check(lib.nrl_news_encoder_bwd(ctypes.byref(bp), ctypes.byref(bg), emb.data_ptr(), bufs[0].data_ptr(), V,
                                                ids.data_ptr(), order.data_ptr(), N, L, p_drop, seed, stream0,
                                                d_out.data_ptr(), phase, ws.data_ptr(), ws.numel(), _stream()),
                       "nrl_news_encoder_bwd")

        hook = ctx.table_grad_hook
        if hook is None:
            run(0)
        else:
            # the embedding-table gradient (>96 % of all gradient bytes) is complete after phase 1: let the
            # data-parallel trainer start its all-reduce now, under the weight-gradient GEMMs of phase 2
            run(1)
            _call_table_grad_hook(hook, bufs[0], ids)
            run(2)
        ctx.ws = None
        return (None, *rets, None, None, None, None, None, None, None)


def _call_table_grad_hook(hook, grad: torch.Tensor, ids: torch.Tensor) -> None:
    """``hook(grad, ids)`` -- or ``hook(grad)`` for a callable that takes one positional argument (the signature the hook had
    before the touched-row exchange needed the ids)."""
    import inspect
    try:
        params = [p for p in inspect.signature(hook).parameters.values()
                  if p.kind in (p.POSITIONAL_ONLY, p.POSITIONAL_OR_KEYWORD, p.VAR_POSITIONAL)]
        two = any(p.kind == p.VAR_POSITIONAL for p in params) or len(params) >= 2
    except (TypeError, ValueError):
        two = True
    if two:
        hook(grad, ids)
    else:
        hook(grad)


class UserEncoderFn(GradAwareFunction):
    """NRMS ``UserEncoder.forward`` (reference user/nrms.py:32-41): hist (B, H, D) -> (B, D)."""

    @staticmethod
    def forward(ctx, hist, w_in, b_in, w_o, b_o, w_a, b_a, q_a, heads, grad_bufs, p_drop=0.0, seed=0,
                input_dropout=True, stream0=0):
        lib = _lib.load()
        hist = _chk(hist, torch.float32, "hist_news_vector")
        params = [_chk(t, torch.float32, "user encoder parameter") for t in (w_in, b_in, w_o, b_o, w_a, b_a, q_a)]
        if hist.dim() != 3:
            raise ValueError("newsreclib_amd: hist_news_vector must be (batch, history, dim)")
        B, H, D = hist.shape
        engine = _lib.engine_code()
        options = _lib.options_word()
        bp = _block_params(params, heads, engine, options)
        if bp.embed_dim != D:
            raise ValueError("newsreclib_amd: hist feature dim does not match the encoder")
        save = saving(ctx)
        ws_bytes = lib.nrl_user_encoder_workspace_bytes(B, H, D, heads, bp.query_dim)
        ws = workspace(ws_bytes, hist.device)
        out = torch.empty((B, D), dtype=torch.float32, device=hist.device)
        _lib.check(lib.nrl_user_encoder_fwd(ctypes.byref(bp), hist.data_ptr(), B, H, float(p_drop), int(seed),
                                            int(stream0), int(bool(input_dropout)), int(save), out.data_ptr(),
                                            ws.data_ptr(), ws.numel(), _stream()), "nrl_user_encoder_fwd")
        if save:
            ctx.save_for_backward(hist, *params)
            ctx.ws, ctx.heads, ctx.grad_bufs, ctx.engine = ws, heads, grad_bufs, engine
            ctx.options = options
            ctx.drop = (float(p_drop), int(seed), int(stream0), int(bool(input_dropout)))
        return out

    @staticmethod
    def backward(ctx, d_out):
        lib = _lib.load()
        hist, *params = ctx.saved_tensors
        B, H, D = hist.shape
        d_out = _chk(d_out, torch.float32, "d_out")
        bp = _block_params(params, ctx.heads, ctx.engine, ctx.options)   # (engine and switches of the forward)
        bufs, rets = _grad_targets(params, ctx.grad_bufs)
        bg = _block_grads(bufs)
        d_hist = torch.empty_like(hist)
        ws = ctx.ws

        def run(phase):
            _lib.check(lib.nrl_user_encoder_bwd_phase(ctypes.byref(bp), ctypes.byref(bg), hist.data_ptr(), B, H,
                                                      ctx.drop[0], ctx.drop[1], ctx.drop[2], ctx.drop[3], d_out.data_ptr(),
                                                      d_hist.data_ptr(), phase, ws.data_ptr(), ws.numel(), _stream()),
                       "nrl_user_encoder_bwd_phase")

        defer = deferred_weight_grads._active
        if defer is None or any(r is not None for r in rets):
            run(0)
        else:
            run(1)
            defer.stream.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(defer.stream):
                run(2)
            defer.keep.append((ws, hist, params, bufs))
        ctx.ws = None
        return (d_hist, *rets, None, None, None, None, None, None)


class ToDenseBatchFn(GradAwareFunction):
    """``to_dense_batch`` values (torch_geometric; nrms_module.py:233,237): (N, D) -> (B, max_len, D)."""

    @staticmethod
    def forward(ctx, x, offsets, batch_size, max_len):
        lib = _lib.load()
        x = _chk(x, torch.float32, "x")
        offsets = _chk(offsets, torch.int64, "offsets")
        N, D = x.shape
        dense = torch.empty((batch_size, max_len, D), dtype=torch.float32, device=x.device)
        _lib.check(lib.nrl_to_dense_batch_fwd(x.data_ptr(), offsets.data_ptr(), batch_size, max_len, D,
                                              dense.data_ptr(), _stream()), "nrl_to_dense_batch_fwd")
        ctx.save_for_backward(offsets)
        ctx.shape = (N, D, batch_size, max_len)
        return dense

    @staticmethod
    def backward(ctx, d_dense):
        lib = _lib.load()
        (offsets,) = ctx.saved_tensors
        N, D, B, max_len = ctx.shape
        d_dense = _chk(d_dense, torch.float32, "d_dense")
        d_x = torch.empty((N, D), dtype=torch.float32, device=d_dense.device)
        _lib.check(lib.nrl_to_dense_batch_bwd(d_dense.data_ptr(), offsets.data_ptr(), B, max_len, D, N,
                                              d_x.data_ptr(), _stream()), "nrl_to_dense_batch_bwd")
        return d_x, None, None, None


class HistMeanFn(GradAwareFunction):
    """late fusion (nrms_module.py:243-248): (B, max_len, D) zero-padded history -> (B, D) mean over the TRUE
    number of clicks."""

    @staticmethod
    def forward(ctx, hist, offsets):
        lib = _lib.load()
        hist = _chk(hist, torch.float32, "hist_news_vector")
        offsets = _chk(offsets, torch.int64, "offsets")
        B, H, D = hist.shape
        user = torch.empty((B, D), dtype=torch.float32, device=hist.device)
        _lib.check(lib.nrl_hist_mean_fwd(hist.data_ptr(), offsets.data_ptr(), B, H, D, user.data_ptr(), _stream()),
                   "nrl_hist_mean_fwd")
        ctx.save_for_backward(offsets)
        ctx.shape = (B, H, D)
        return user

    @staticmethod
    def backward(ctx, d_user):
        lib = _lib.load()
        (offsets,) = ctx.saved_tensors
        B, H, D = ctx.shape
        d_user = _chk(d_user, torch.float32, "d_user")
        d_hist = torch.empty((B, H, D), dtype=torch.float32, device=d_user.device)
        _lib.check(lib.nrl_hist_mean_bwd(d_user.data_ptr(), offsets.data_ptr(), B, H, D, d_hist.data_ptr(), _stream()),
                   "nrl_hist_mean_bwd")
        return d_hist, None


class DotScoresFn(GradAwareFunction):
    """``DotProduct.forward`` (click_predictor.py:9-11): user (B, D) x cand (B, C, D) -> (B, C)."""

    @staticmethod
    def forward(ctx, user, cand):
        lib = _lib.load()
        user = _chk(user, torch.float32, "user_vec")
        cand = _chk(cand, torch.float32, "cand_news_vector")
        B, C, D = cand.shape
        scores = torch.empty((B, C), dtype=torch.float32, device=user.device)
        _lib.check(lib.nrl_dot_scores_fwd(user.data_ptr(), cand.data_ptr(), B, C, D, scores.data_ptr(),
                                          _stream()), "nrl_dot_scores_fwd")
        ctx.save_for_backward(user, cand)
        return scores

    @staticmethod
    def backward(ctx, d_scores):
        lib = _lib.load()
        user, cand = ctx.saved_tensors
        B, C, D = cand.shape
        d_scores = _chk(d_scores, torch.float32, "d_scores")
        d_user, d_cand = torch.empty_like(user), torch.empty_like(cand)
        _lib.check(lib.nrl_dot_scores_bwd(d_scores.data_ptr(), user.data_ptr(), cand.data_ptr(), B, C, D,
                                          d_user.data_ptr(), d_cand.data_ptr(), _stream()),
                   "nrl_dot_scores_bwd")
        return d_user, d_cand


class CrossEntropyFn(GradAwareFunction):
    """``CrossEntropyLoss()(scores, y_true)`` with float targets (nrms_module.py:287-288)."""

    @staticmethod
    def forward(ctx, scores, y_true, grad_scale):
        lib = _lib.load()
        scores = _chk(scores, torch.float32, "scores")
        y_true = _chk(y_true, torch.float32, "y_true")
        B, C = scores.shape
        loss = torch.empty((), dtype=torch.float32, device=scores.device)
        d_scores = torch.empty_like(scores)
        _lib.check(lib.nrl_ce_loss_fwd_bwd(scores.data_ptr(), y_true.data_ptr(), B, C, float(grad_scale),
                                           loss.data_ptr(), d_scores.data_ptr(), _stream()),
                   "nrl_ce_loss_fwd_bwd")
        ctx.save_for_backward(d_scores)
        return loss

    @staticmethod
    def backward(ctx, g):
        (d_scores,) = ctx.saved_tensors
        if g.data_ptr() in _UNIT_GRADS:      # the root gradient of a trainer (a registered tensor holding 1.0): d_scores as is
            return d_scores, None, None
        return d_scores * g, None, None


# Root gradients known to hold exactly 1.0 (``register_unit_grad``): a loss that receives one of them as its incoming gradient
# IS the root of the backward and hands its stored gradient on without the multiply (one small launch per step; autograd's own
# ``ones_like`` fill is the other one a trainer saves by passing the tensor to ``loss.backward(gradient=...)``).  The registry
# keeps the tensors alive, so an address can never come back as some other tensor's.
_UNIT_GRADS = {}


def register_unit_grad(t: torch.Tensor) -> torch.Tensor:
    _UNIT_GRADS[t.data_ptr()] = t
    return t


class SupConFn(GradAwareFunction):
    """``SupConLoss()(embeddings=scores, indices_tuple=...)`` as called at nrms_module.py:289-318: scores, y_true
    (B, C) dense, cand_sizes (B,) int64 = real candidates per row."""

    @staticmethod
    def forward(ctx, scores, y_true, cand_sizes, temperature):
        lib = _lib.load()
        scores = _chk(scores, torch.float32, "scores")
        y_true = _chk(y_true, torch.float32, "y_true")
        cand_sizes = _chk(cand_sizes, torch.int64, "cand_sizes")
        B, C = scores.shape
        if y_true.shape != (B, C) or cand_sizes.shape != (B,):
            raise ValueError("newsreclib_amd: inconsistent sup-con loss shapes")
        loss = torch.empty((), dtype=torch.float32, device=scores.device)
        d_scores = torch.empty_like(scores)
        _lib.check(lib.nrl_supcon_loss_fwd_bwd(scores.data_ptr(), y_true.data_ptr(), cand_sizes.data_ptr(), B, C,
                                               float(temperature), 1.0, loss.data_ptr(), d_scores.data_ptr(),
                                               _stream()), "nrl_supcon_loss_fwd_bwd")
        ctx.save_for_backward(d_scores)
        return loss

    @staticmethod
    def backward(ctx, g):
        (d_scores,) = ctx.saved_tensors
        return d_scores * g, None, None, None


class SplitRowsFn(GradAwareFunction):
    """(x[:n], x[n:]) whose backward is ONE concatenation.  (Plain slicing makes autograd zero-fill two full-size
    gradients, copy a slice into each and add them: five launches where one does.)"""

    @staticmethod
    def forward(ctx, x, n):
        ctx.n = int(n)
        return x[:n], x[n:]

    @staticmethod
    def backward(ctx, g_head, g_tail):
        return torch.cat((g_head, g_tail), dim=0), None


def split_rows(x: torch.Tensor, n: int):
    return SplitRowsFn.apply(x, n) if x.requires_grad else (x[:n], x[n:])


# ---- evaluation forwards of the news encoder from a per-token q|k|v table (include/newsreclib_amd.h, ABI v16) ------------
def token_table_supported(seq_len: int, embed_dim: int, heads: int, query_dim: int) -> bool:
    return _lib.engine_code() == 2 and bool(_lib.load().nrl_token_table_supported(int(seq_len), int(embed_dim), int(heads),
                                                                                 int(query_dim)))


def token_table_build(params: Sequence[torch.Tensor], heads: int, buf: Optional[torch.Tensor] = None) -> Optional[torch.Tensor]:
    """``params`` = (embedding table, in_proj_weight, in_proj_bias, out_proj.weight, out_proj.bias, linear.weight, linear.bias,
    query) of an ``MHSAAddAtt``: runs the in-projection once per vocabulary id and builds the back half's weight images into
    ``buf`` (reused when large enough).  None when the geometry has no table (``nrl_token_table_bytes`` == 0)."""
    lib = _lib.load()
    params = [_chk(t.detach(), torch.float32, "parameter") for t in params]
    emb = params[0]
    V, D = emb.shape
    bp = _block_params(params[1:], heads, _lib.engine_code(), _lib.options_word())
    nbytes = int(lib.nrl_token_table_bytes(V, D, int(heads), bp.query_dim))
    if nbytes == 0:
        return None
    if buf is None or buf.numel() < nbytes or buf.device != emb.device:
        buf = torch.empty(nbytes, dtype=torch.uint8, device=emb.device)
    _lib.check(lib.nrl_token_table_build(ctypes.byref(bp), emb.data_ptr(), V, buf.data_ptr(), buf.numel(), _stream()),
               "nrl_token_table_build")
    return buf


def news_encoder_fwd_table(ids: torch.Tensor, table: torch.Tensor, vocab: int, params: Sequence[torch.Tensor],
                           heads: int) -> torch.Tensor:
    """``MHSAAddAtt.forward`` in evaluation mode from a table of ``token_table_build`` (``params`` without the embedding table:
    the seven block parameters): ids (N, L) -> (N, D), EQUAL to the table-less evaluation forward."""
    lib = _lib.load()
    ids = _chk(ids, torch.int64, "ids")
    if ids.dim() != 2:
        raise ValueError("newsreclib_amd: token ids must be (num_news, num_tokens)")
    N, L = ids.shape
    params = [_chk(t.detach(), torch.float32, "parameter") for t in params]
    bp = _block_params(params, heads, _lib.engine_code(), _lib.options_word())
    out = torch.empty((N, bp.embed_dim), dtype=torch.float32, device=ids.device)
    ws = workspace(lib.nrl_news_encoder_fwd_table_workspace_bytes(N, L, int(heads)), ids.device)
    _lib.check(lib.nrl_news_encoder_fwd_table(ctypes.byref(bp), table.data_ptr(), table.numel(), int(vocab), ids.data_ptr(), N, L,
                                              out.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "nrl_news_encoder_fwd_table")
    return out


# ---- plain (non-autograd) entry points ----------------------------------------------------------
def embedding_gather(table: torch.Tensor, ids: torch.Tensor) -> torch.Tensor:
    lib = _lib.load()
    table, ids = _chk(table, torch.float32, "table"), _chk(ids, torch.int64, "ids")
    out = torch.empty(tuple(ids.shape) + (table.shape[1],), dtype=torch.float32, device=table.device)
    _lib.check(lib.nrl_embedding_gather(table.data_ptr(), ids.data_ptr(), ids.numel(), table.shape[1],
                                        out.data_ptr(), _stream()), "nrl_embedding_gather")
    return out


def linear(a: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    lib = _lib.load()
    a, w = _chk(a, torch.float32, "a"), _chk(w, torch.float32, "w")
    M, K = a.shape
    N = w.shape[0]
    c = torch.empty((M, N), dtype=torch.float32, device=a.device)
    b = _chk(bias, torch.float32, "bias").data_ptr() if bias is not None else None
    ws = workspace(lib.nrl_linear_workspace_bytes(N, K), a.device)
    _lib.check(lib.nrl_linear_fwd(a.data_ptr(), w.data_ptr(), b, M, N, K, c.data_ptr(), ws.data_ptr(), ws.numel(),
                                  _stream()), "nrl_linear_fwd")
    return c


def dropout_mask(n: int, p: float, seed: int, stream: int, device) -> torch.Tensor:
    lib = _lib.load()
    keep = torch.empty(n, dtype=torch.uint8, device=device)
    _lib.check(lib.nrl_dropout_mask(keep.data_ptr(), n, float(p), int(seed), int(stream), _stream()),
               "nrl_dropout_mask")
    return keep


def adam_step_(param: torch.Tensor, grad: torch.Tensor, exp_avg: torch.Tensor, exp_avg_sq: torch.Tensor,
               step: int, lr: float = 1e-4, betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8,
               grad_scale: float = 1.0, zero_grad: bool = False) -> None:
    lib = _lib.load()
    for t in (param, grad, exp_avg, exp_avg_sq):
        if not (t.is_cuda and t.is_contiguous() and t.dtype == torch.float32):
            raise ValueError("newsreclib_amd.adam_step_: contiguous float32 GPU tensors required")
    _lib.check(lib.nrl_adam_step(param.data_ptr(), grad.data_ptr(), exp_avg.data_ptr(),
                                 exp_avg_sq.data_ptr(), param.numel(), lr, betas[0], betas[1], eps,
                                 int(step), float(grad_scale), int(zero_grad), _stream()), "nrl_adam_step")


def adam_rows_mark_(ids: torch.Tensor, mark: torch.Tensor, step: int) -> None:
    """mark[id] = step for the ids of a step's batch (``nrl_adam_rows_mark``; lazy table Adam, trainer.LazyTableAdam)."""
    lib = _lib.load()
    ids = _chk(ids, torch.int64, "ids").reshape(-1)
    _lib.check(lib.nrl_adam_rows_mark(ids.data_ptr(), ids.numel(), mark.numel(), mark.data_ptr(), int(step), _stream()),
               "nrl_adam_rows_mark")


def adam_rows_advance_(param: torch.Tensor, grad: torch.Tensor, exp_avg: torch.Tensor, exp_avg_sq: torch.Tensor,
                       last_step: torch.Tensor, mark: Optional[torch.Tensor], status: torch.Tensor, upto_step: int,
                       with_grad, lr: float, betas: Tuple[float, float], eps: float, grad_scale: float = 1.0,
                       stride: int = 1, offset: int = 0, exclude_mark: Optional[torch.Tensor] = None, exclude_tag: int = 0) -> None:
    """``nrl_adam_rows_advance`` over a (rows, dim) table and its flat gradient / moment views (see include/newsreclib_amd.h)."""
    lib = _lib.load()
    rows, dim = param.shape
    for t in (param, grad, exp_avg, exp_avg_sq):
        if not (t.is_cuda and t.is_contiguous() and t.dtype == torch.float32 and tuple(t.shape) == (rows, dim)):
            raise ValueError("newsreclib_amd.adam_rows_advance_: contiguous float32 GPU tensors of one (rows, dim) shape required")
    _lib.check(lib.nrl_adam_rows_advance(param.data_ptr(), grad.data_ptr(), exp_avg.data_ptr(), exp_avg_sq.data_ptr(), rows, dim,
                                         last_step.data_ptr(), mark.data_ptr() if mark is not None else None,
                                         status.data_ptr(), int(stride), int(offset), int(upto_step), int(with_grad),
                                         lr, betas[0], betas[1], eps, float(grad_scale),
                                         exclude_mark.data_ptr() if exclude_mark is not None else None, int(exclude_tag),
                                         _stream()), "nrl_adam_rows_advance")


def sort_positions(ids: torch.Tensor, vocab: Optional[int] = None) -> torch.Tensor:
    """Positions of the flat id vector grouped by ascending id: the visiting order of the embedding-table gradient
    (what ``embedding_dense_backward`` gets from its own sort).  With ``vocab`` (exclusive upper bound of the ids) a
    three-launch counting sort in the HIP library; the order INSIDE one id's run is unspecified.  Without it,
    ``torch.argsort`` (index bookkeeping on int64, no arithmetic).  The result has n + 1 entries: the last one is the number
    of positions holding id 0 (they sort first), which lets the news-encoder backward skip the rows of the padding id."""
    flat = _chk(ids, torch.int64, "ids").reshape(-1)
    n = flat.numel()
    if not vocab or vocab > (1 << 20):
        # (n + 1) entries like the library's sort: the positions by ascending id, then the number of id-0 positions
        return torch.cat([torch.argsort(flat, stable=True), (flat == 0).sum().reshape(1)])
    lib = _lib.load()
    order = torch.empty(n + 1, dtype=torch.int64, device=flat.device)
    ws = workspace(lib.nrl_sort_positions_workspace_bytes(n, int(vocab)), flat.device)
    _lib.check(lib.nrl_sort_positions(flat.data_ptr(), n, int(vocab), order.data_ptr(), ws.data_ptr(), ws.numel(),
                                      _stream()), "nrl_sort_positions")
    return order


_SIDE_STREAMS = {}


def sort_positions_async(ids: torch.Tensor, vocab: Optional[int] = None) -> torch.Tensor:
    """``sort_positions`` on a side stream: the visiting order is needed by the news encoder's BACKWARD only, so the three
    small, latency-bound launches of the counting sort (~45 us at B = 128) run beside the forward instead of in front of
    it.  The completion event travels WITH the tensor (``order._nrl_ready``): every autograd forward that receives the
    tensor reads it (``order_event``, which does not consume it) and its backward waits for it on the launch stream
    (``wait_order``) -- a second encoder call on the same order, or a re-forwarded prepared batch, waits just the same.
    Ids that are not on a GPU are sorted in place (no stream to fork from)."""
    dev = ids.device
    if dev.type != "cuda":
        return sort_positions(ids, vocab)
    main = torch.cuda.current_stream(dev)
    side = _SIDE_STREAMS.get(dev.index)
    if side is None:
        side = _SIDE_STREAMS[dev.index] = torch.cuda.Stream(dev)
    side.wait_stream(main)                       # the ids were produced on the launch stream
    with torch.cuda.stream(side):
        order = sort_positions(ids, vocab)
        ready = torch.cuda.Event()
        ready.record(side)
    ids.record_stream(side)                      # allocator: neither tensor may be recycled under the other stream
    order.record_stream(main)
    order._nrl_ready = ready                     # lives and dies with the tensor: no stale event can meet a recycled address
    return order


def order_event(order: Optional[torch.Tensor]):
    """The side-stream completion event of an order tensor (None for an order computed on the launch stream)."""
    return getattr(order, "_nrl_ready", None) if order is not None else None


def wait_order(event) -> None:
    if event is not None:
        torch.cuda.current_stream().wait_event(event)


def offsets_from_sorted_batch(batch: torch.Tensor, batch_size: int) -> torch.Tensor:
    """Prefix sums of the sorted assignment vector (``rec_dataset.py:289-293``) -> (B + 1,) int64."""
    counts = torch.bincount(batch, minlength=batch_size)
    off = torch.zeros(batch_size + 1, dtype=torch.int64, device=batch.device)
    torch.cumsum(counts, 0, out=off[1:])
    return off


# ---- streaming evaluation metrics (nrl_metrics.hip) -----------------------------------------------
METRICS_MAX_CAND, METRICS_MAX_CLASSES, METRICS_MAX_K, METRICS_MAX_NK = 4096, 1024, 1024, 4
METRICS_FLAGS = {1: f"an impression has more than {METRICS_MAX_CAND} candidates",
                 2: "an aspect id is negative or >= num_classes",
                 4: "an offset vector is not non-decreasing inside its buffer"}


def metrics_columns(top_k: Sequence[int], prefixes: Sequence[str] = ()) -> list:
    """Column names of the rows / sums of ``impression_metrics`` (the key names of ``metrics.ranking_metrics`` /
    ``metrics.aspect_metrics``; the per-impression reciprocal rank stands under "mrr")."""
    cols = ["mrr"] + [f"ndcg@{k}" for k in top_k]
    for p in prefixes:
        cols += [f"{p}_div@{k}" for k in top_k] + [f"{p}_pers@{k}" for k in top_k]
    return cols


def impression_metrics(preds: torch.Tensor, targets: torch.Tensor, cand_offsets: torch.Tensor, top_k: Sequence[int],
                       aspects: Sequence[Tuple[torch.Tensor, torch.Tensor, int]] = (), hist_offsets: Optional[torch.Tensor] = None,
                       status: Optional[torch.Tensor] = None, sums: Optional[torch.Tensor] = None,
                       count: Optional[torch.Tensor] = None, want_rank: bool = True, want_rows: bool = True):
    """``nrl_impression_metrics`` over one batch of ragged impressions -> (rank (N) int32 | None, rows (B, cols) fp32 | None, status).
    ``aspects``: up to two (cand_aspects (N) int64, hist_aspects (n_hist) int64, num_classes) sharing ``hist_offsets`` (B + 1).
    ``sums`` (cols float64) / ``count`` (1 int64) are accumulated into; ``status`` (1 int32) is OR-ed into (``METRICS_FLAGS``) and
    must be read by the caller -- nothing here synchronises with the host."""
    lib = _lib.load()
    preds, targets = _chk(preds, torch.float32, "preds"), _chk(targets, torch.float32, "targets")
    cand_offsets = _chk(cand_offsets, torch.int64, "cand_offsets")
    N, B = int(preds.numel()), int(cand_offsets.numel()) - 1
    top_k = [int(k) for k in top_k]
    if targets.numel() != N or B < 0 or preds.dim() != 1:
        raise ValueError("newsreclib_amd: flat preds / targets of one length and cand_offsets of B + 1 entries expected")
    if len(top_k) > METRICS_MAX_NK or any(not 1 <= k <= METRICS_MAX_K for k in top_k):
        raise ValueError(f"newsreclib_amd: at most {METRICS_MAX_NK} top_k values, each in [1, {METRICS_MAX_K}]; got {top_k}")
    if len(aspects) > 2:
        raise ValueError("newsreclib_amd: at most two aspects per call")
    asp, n_hist = [], 0
    if aspects:
        if hist_offsets is None:
            raise ValueError("newsreclib_amd: aspects need hist_offsets")
        hist_offsets = _chk(hist_offsets, torch.int64, "hist_offsets")
        if hist_offsets.numel() != B + 1:
            raise ValueError("newsreclib_amd: hist_offsets must have B + 1 entries")
        n_hist = int(aspects[0][1].numel())
        for ca, ha, ncls in aspects:
            ca, ha = _chk(ca, torch.int64, "cand_aspects"), _chk(ha, torch.int64, "hist_aspects")
            if ca.numel() != N or ha.numel() != n_hist or not 2 <= int(ncls) <= METRICS_MAX_CLASSES:
                raise ValueError(f"newsreclib_amd: every aspect needs N candidate ids, one history length and 2 <= num_classes <= "
                                 f"{METRICS_MAX_CLASSES}; got {ca.numel()} / {ha.numel()} ids, num_classes {ncls}")
            asp.append((ca, ha, int(ncls)))
    dev = preds.device
    cols = 1 + len(top_k) * (1 + 2 * len(asp))
    if status is None:
        status = torch.zeros(1, dtype=torch.int32, device=dev)
    status = _chk(status, torch.int32, "status")
    if (sums is None) != (count is None):
        raise ValueError("newsreclib_amd: sums and count go together")
    if sums is not None:
        sums, count = _chk(sums, torch.float64, "sums"), _chk(count, torch.int64, "count")
        if sums.numel() != cols or count.numel() != 1:
            raise ValueError(f"newsreclib_amd: sums must have {cols} entries and count one")
    rank = torch.empty(N, dtype=torch.int32, device=dev) if want_rank else None
    rows = torch.zeros((B, cols), dtype=torch.float32, device=dev) if want_rows else None
    if B == 0:
        return rank, rows, status
    ws = workspace(lib.nrl_impression_metrics_workspace_bytes(N, B, len(asp), len(top_k)), dev)
    ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
    a0 = asp[0] if len(asp) > 0 else (None, None, 0)
    a1 = asp[1] if len(asp) > 1 else (None, None, 0)
    ks = (ctypes.c_int32 * max(len(top_k), 1))(*top_k)
    _lib.check(lib.nrl_impression_metrics(preds.data_ptr(), targets.data_ptr(), cand_offsets.data_ptr(), N, B, len(asp),
                                          ptr(a0[0]), ptr(a0[1]), a0[2], ptr(a1[0]), ptr(a1[1]), a1[2], ptr(hist_offsets) if asp else None,
                                          n_hist, ks, len(top_k), ptr(rank), ptr(rows), ptr(sums), ptr(count), status.data_ptr(),
                                          ws.data_ptr(), ws.numel(), _stream()), "nrl_impression_metrics")
    return rank, rows, status


# ---- a grid of ensemble weights in one pass (nrl_metrics.hip: mt_grid_kernel) ---------------------------------------------------
GRID_MAX_COMPONENTS, GRID_MAX_CONFIGS = 4, 4096


def grid_weights(weights, n_components: Optional[int] = None) -> torch.Tensor:
    """The weight rows of a grid, checked on the HOST -> (G, T) fp32 CPU tensor.  ``ValueError`` for a row of zeros (it would
    score every candidate 0: no ranking to evaluate), a non-finite weight or rows of the wrong length; ``NotImplementedError``
    beyond ``GRID_MAX_COMPONENTS`` / ``GRID_MAX_CONFIGS``."""
    w = torch.as_tensor(weights, dtype=torch.float32).detach().cpu()
    if w.dim() != 2 or w.shape[0] < 1 or w.shape[1] < 1:
        raise ValueError(f"newsreclib_amd: weights must be (G, T) with at least one row and one component, got {tuple(w.shape)}")
    G, T = w.shape
    if n_components is not None and T != int(n_components):
        raise ValueError(f"newsreclib_amd: every weight row needs one entry per component: {int(n_components)}, got {T}")
    if T > GRID_MAX_COMPONENTS or G > GRID_MAX_CONFIGS:
        raise NotImplementedError(f"newsreclib_amd: a weight grid takes at most {GRID_MAX_COMPONENTS} components and "
                                  f"{GRID_MAX_CONFIGS} rows per call; got ({G}, {T})")
    if not bool(torch.isfinite(w).all()):
        raise ValueError("newsreclib_amd: non-finite weight in the grid")
    zero = (w == 0).all(1)
    if bool(zero.any()):
        raise ValueError(f"newsreclib_amd: weight row {int(zero.nonzero()[0])} of the grid is all zeros")
    return w.contiguous()


def grid_metrics(comp: torch.Tensor, weights, targets: torch.Tensor, cand_offsets: torch.Tensor, top_k: Sequence[int],
                 aspects: Sequence[Tuple[torch.Tensor, torch.Tensor, int]] = (), hist_offsets: Optional[torch.Tensor] = None,
                 status: Optional[torch.Tensor] = None, sums: Optional[torch.Tensor] = None, count: Optional[torch.Tensor] = None,
                 want_rows: bool = False, want_preds: bool = False, configs_per_block: int = 0):
    """``nrl_grid_metrics``: ``impression_metrics`` for the G score vectors ``weights[g] . comp`` of one batch of ragged impressions
    -> (rows (G, B, cols) fp32 | None, preds (G, N) fp32 | None, status).  ``comp`` (T, N): the components (``manner_zscores``);
    ``weights`` (G, T): a host tensor or nested list, checked by ``grid_weights`` and uploaded, or a GPU fp32 tensor that the
    caller has checked that way (nothing here reads the device).  A term with weight 0 is skipped, so a NaN component does not
    reach a row that does not use it.  ``sums`` (G, cols float64) / ``count`` (1 int64) are accumulated into: ``sums[g]`` gets what
    ``impression_metrics`` adds when fed row g's scores, to the bit; ``count`` once.  Everything else as ``impression_metrics``.
    ``configs_per_block`` overrides the launch plan (0: from G and B); it changes no result."""
    lib = _lib.load()
    comp, targets = _chk(comp, torch.float32, "comp"), _chk(targets, torch.float32, "targets")
    cand_offsets = _chk(cand_offsets, torch.int64, "cand_offsets")
    if comp.dim() != 2 or targets.dim() != 1:
        raise ValueError("newsreclib_amd: comp (T, N) and flat targets (N) expected")
    T, N = int(comp.shape[0]), int(comp.shape[1])
    B = int(cand_offsets.numel()) - 1
    if targets.numel() != N or B < 0:
        raise ValueError("newsreclib_amd: comp (T, N), targets of N entries and cand_offsets of B + 1 entries expected")
    dev = comp.device
    if torch.is_tensor(weights) and weights.is_cuda:
        weights = _chk(weights, torch.float32, "weights")
        if weights.dim() != 2 or weights.shape[1] != T:
            raise ValueError(f"newsreclib_amd: every weight row needs one entry per component: {T}, got {tuple(weights.shape)}")
        if T > GRID_MAX_COMPONENTS or weights.shape[0] > GRID_MAX_CONFIGS or weights.shape[0] < 1:
            raise NotImplementedError(f"newsreclib_amd: a weight grid takes at most {GRID_MAX_COMPONENTS} components and 1 to "
                                      f"{GRID_MAX_CONFIGS} rows per call; got {tuple(weights.shape)}")
    else:
        weights = grid_weights(weights, T).pin_memory().to(dev, non_blocking=True)      # (a pageable copy would synchronise)
    G = int(weights.shape[0])
    top_k = [int(k) for k in top_k]
    if len(top_k) > METRICS_MAX_NK or any(not 1 <= k <= METRICS_MAX_K for k in top_k):
        raise ValueError(f"newsreclib_amd: at most {METRICS_MAX_NK} top_k values, each in [1, {METRICS_MAX_K}]; got {top_k}")
    if len(aspects) > 2:
        raise ValueError("newsreclib_amd: at most two aspects per call")
    asp, n_hist = [], 0
    if aspects:
        if hist_offsets is None:
            raise ValueError("newsreclib_amd: aspects need hist_offsets")
        hist_offsets = _chk(hist_offsets, torch.int64, "hist_offsets")
        if hist_offsets.numel() != B + 1:
            raise ValueError("newsreclib_amd: hist_offsets must have B + 1 entries")
        n_hist = int(aspects[0][1].numel())
        for ca, ha, ncls in aspects:
            ca, ha = _chk(ca, torch.int64, "cand_aspects"), _chk(ha, torch.int64, "hist_aspects")
            if ca.numel() != N or ha.numel() != n_hist or not 2 <= int(ncls) <= METRICS_MAX_CLASSES:
                raise ValueError(f"newsreclib_amd: every aspect needs N candidate ids, one history length and 2 <= num_classes <= "
                                 f"{METRICS_MAX_CLASSES}; got {ca.numel()} / {ha.numel()} ids, num_classes {ncls}")
            asp.append((ca, ha, int(ncls)))
    cols = 1 + len(top_k) * (1 + 2 * len(asp))
    if status is None:
        status = torch.zeros(1, dtype=torch.int32, device=dev)
    status = _chk(status, torch.int32, "status")
    if (sums is None) != (count is None):
        raise ValueError("newsreclib_amd: sums and count go together")
    if sums is not None:
        sums, count = _chk(sums, torch.float64, "sums"), _chk(count, torch.int64, "count")
        if tuple(sums.shape) != (G, cols) or count.numel() != 1:
            raise ValueError(f"newsreclib_amd: sums must be ({G}, {cols}) and count one entry")
    if int(configs_per_block) < 0:
        raise ValueError("newsreclib_amd: configs_per_block >= 0 (0: the plan)")
    rows = torch.zeros((G, B, cols), dtype=torch.float32, device=dev) if want_rows else None
    preds = torch.zeros((G, N), dtype=torch.float32, device=dev) if want_preds else None
    if B == 0:
        return rows, preds, status
    ws = workspace(lib.nrl_grid_metrics_workspace_size(B, G, len(asp), len(top_k), int(want_rows)), dev)
    ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
    a0 = asp[0] if len(asp) > 0 else (None, None, 0)
    a1 = asp[1] if len(asp) > 1 else (None, None, 0)
    ks = (ctypes.c_int32 * max(len(top_k), 1))(*top_k)
    _lib.check(lib.nrl_grid_metrics(comp.data_ptr(), T, weights.data_ptr(), G, targets.data_ptr(), cand_offsets.data_ptr(), N, B,
                                    len(asp), ptr(a0[0]), ptr(a0[1]), a0[2], ptr(a1[0]), ptr(a1[1]), a1[2],
                                    ptr(hist_offsets) if asp else None, n_hist, ks, len(top_k), int(configs_per_block), ptr(rows),
                                    ptr(preds), ptr(sums), ptr(count), status.data_ptr(), ws.data_ptr(), ws.numel(), _stream()),
               "nrl_grid_metrics")
    return rows, preds, status


# ---- full-catalogue top-k recommendation (nrl_topk.hip) ------------------------------------------------------------------------
TOPK_MAX_K, TOPK_MAX_D = 128, 1024
TOPK_FLAGS = {1: "an exclusion index is outside [0, V) (ignored)",
              2: "excl_off decreases or leaves its range (that user's row is all -1 / -inf)",
              4: "a NaN score of an eligible, not excluded row (that row is left out for that user)",
              8: "a user's scores of some table cannot be standardised: zero, non-finite or undefined standard deviation (that "
                 "user's row is all -1 / -inf)"}


def _topk_masks(excl_idx, excl_off, eligible, B: int, V: int):
    """The exclusion lists and the eligibility mask as every top-k entry takes them, checked."""
    if (excl_idx is None) != (excl_off is None):
        raise ValueError("newsreclib_amd: excl_idx and excl_off go together")
    if excl_idx is not None:
        excl_idx, excl_off = _chk(excl_idx, torch.int64, "excl_idx"), _chk(excl_off, torch.int64, "excl_off")
        if excl_off.numel() != B + 1:
            raise ValueError("newsreclib_amd: excl_off must have B + 1 entries")
        # the kernel trusts excl_off[B] as the length of excl_idx: an offset beyond the list is turned into one it rejects
        excl_off = torch.where(excl_off > excl_idx.numel(), torch.full_like(excl_off, -1), excl_off)
    if eligible is not None:
        if eligible.dtype == torch.bool and eligible.is_cuda:
            eligible = eligible.to(torch.uint8)
        eligible = _chk(eligible, torch.uint8, "eligible")
        if eligible.numel() != V:
            raise ValueError("newsreclib_amd: eligible must have one entry per table row")
    return excl_idx, excl_off, eligible


def _ptr(t):
    """An optional tensor as a native entry takes it."""
    return t.data_ptr() if t is not None else None


def _topk_outputs(B: int, k: int, dev):
    return (torch.empty((B, max(k, 0)), dtype=torch.int64, device=dev), torch.empty((B, max(k, 0)), dtype=torch.float32, device=dev),
            torch.zeros(1, dtype=torch.int32, device=dev))


def _rank_targets(tgt_idx, tgt_off, B: int):
    """The target lists as every rank entry takes them, checked (``catalogue_ranks`` documents them)."""
    tgt_idx, tgt_off = _chk(tgt_idx, torch.int64, "tgt_idx"), _chk(tgt_off, torch.int64, "tgt_off")
    if tgt_off.numel() != B + 1:
        raise ValueError("newsreclib_amd: tgt_off must have B + 1 entries")
    n_tgt = int(tgt_idx.numel())
    # (the kernel validates the offsets against n_tgt itself; as for excl_off, one beyond the list is turned into one it rejects)
    return tgt_idx, torch.where(tgt_off > n_tgt, torch.full_like(tgt_off, -1), tgt_off), n_tgt


def _rank_outputs(n_tgt: int, B: int, dev):
    return (torch.empty(n_tgt, dtype=torch.int32, device=dev), torch.empty(n_tgt, dtype=torch.float32, device=dev),
            torch.empty(B, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev))


class _Scorer(NamedTuple):
    """A scorer's inputs, checked once for its top-k wrapper and its rank wrapper: the sizes, the D its workspace is sized with and
    its own arguments of the native call, those before ``k`` / the targets (``lead``) and those after (``trail``); ``keep`` holds
    what the pointers among them point into."""
    B: int
    V: int
    D: int
    dev: torch.device
    lead: tuple
    trail: tuple
    keep: tuple


def _run_topk(entry: str, s: _Scorer, k: int, excl_idx, excl_off, eligible, slices: int, extra=()):
    """The top-k entry ``entry`` under scorer ``s``; ``extra``: the outputs of its own between ``score`` and ``status``."""
    lib = _lib.load()
    k = int(k)
    excl_idx, excl_off, eligible = _topk_masks(excl_idx, excl_off, eligible, s.B, s.V)
    idx, score, status = _topk_outputs(s.B, k, s.dev)
    ws = workspace(lib.nrl_topk_scores_workspace_bytes(s.B, s.V, s.D, k, int(slices)), s.dev)
    _lib.check(getattr(lib, entry)(*s.lead, k, *s.trail, _ptr(excl_idx), _ptr(excl_off), _ptr(eligible), int(slices), idx.data_ptr(),
                                   score.data_ptr(), *(t.data_ptr() for t in extra), status.data_ptr(), ws.data_ptr(), ws.numel(),
                                   _stream()), entry)
    return idx, score, status


def _run_ranks(entry: str, s: _Scorer, tgt_idx, tgt_off, excl_idx, excl_off, eligible, slices: int, extra=(), ws_lead=(), after=()):
    """The rank entry ``entry`` under scorer ``s``; ``extra``: the outputs of its own between ``ranked`` and ``status``; ``ws_lead``
    (with it the entry has a workspace function of its own): that function's arguments before B; ``after``: the inputs of its own
    between the targets and the exclusion lists."""
    lib = _lib.load()
    tgt_idx, tgt_off, n_tgt = _rank_targets(tgt_idx, tgt_off, s.B)
    excl_idx, excl_off, eligible = _topk_masks(excl_idx, excl_off, eligible, s.B, s.V)
    rank, score, ranked, status = _rank_outputs(n_tgt, s.B, s.dev)
    ws_size = getattr(lib, entry + "_workspace_size") if ws_lead else lib.nrl_catalogue_ranks_workspace_size
    ws = workspace(ws_size(*ws_lead, s.B, s.V, s.D, n_tgt, int(slices)), s.dev)
    _lib.check(getattr(lib, entry)(*s.lead, *s.trail, tgt_idx.data_ptr(), tgt_off.data_ptr(), n_tgt, *after, _ptr(excl_idx),
                                   _ptr(excl_off), _ptr(eligible), int(slices), rank.data_ptr(), score.data_ptr(), ranked.data_ptr(),
                                   *(t.data_ptr() for t in extra), status.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), entry)
    return rank, score, ranked, status


def _dot_scorer(user_vec, table) -> _Scorer:
    user_vec, table = _chk(user_vec, torch.float32, "user_vec"), _chk(table, torch.float32, "table")
    if user_vec.dim() != 2 or table.dim() != 2 or user_vec.shape[1] != table.shape[1]:
        raise ValueError(f"newsreclib_amd: user_vec (B, D) and table (V, D) expected, got {tuple(user_vec.shape)} and "
                         f"{tuple(table.shape)}")
    B, D, V = int(user_vec.shape[0]), int(user_vec.shape[1]), int(table.shape[0])
    return _Scorer(B, V, D, user_vec.device, (user_vec.data_ptr(), table.data_ptr(), B, V, D), (), (user_vec, table))


def topk_scores(user_vec: torch.Tensor, table: torch.Tensor, k: int, excl_idx: Optional[torch.Tensor] = None,
                excl_off: Optional[torch.Tensor] = None, eligible: Optional[torch.Tensor] = None, slices: int = 0):
    """``nrl_topk_scores``: for each row of ``user_vec`` (B, D) the ``k`` rows of ``table`` (V, D) of highest dot product ->
    (idx (B, k) int64, score (B, k) fp32, status (1) int32), score descending, equal scores by ascending row, ``-1`` / ``-inf``
    where fewer than ``k`` rows qualify.  ``excl_idx`` (int64) / ``excl_off`` (B + 1 int64): ragged per-user rows that are never
    returned (the history); ``eligible`` (V uint8 or bool): 0 = never returned for anyone.  The (B, V) score matrix is never
    materialised.  ``status`` (``TOPK_FLAGS``) stays on the device and must be read by the caller -- nothing here synchronises
    with the host."""
    return _run_topk("nrl_topk_scores", _dot_scorer(user_vec, table), k, excl_idx, excl_off, eligible, slices)


TOPK_CAP_MAX_K = 64


def _capped(s: _Scorer, row_class: torch.Tensor, max_per_class: int) -> _Scorer:
    """Scorer ``s`` with the class cap behind ``k``: ``row_class`` checked (one int32 per table row; int64 converted by one device
    op); the native entry checks ``k`` and ``max_per_class`` before it launches anything."""
    if row_class is None:
        raise ValueError("newsreclib_amd: row_class (one class id per table row) is required")
    if row_class.dtype == torch.int64 and row_class.is_cuda:
        row_class = row_class.to(torch.int32)
    row_class = _chk(row_class, torch.int32, "row_class")
    if row_class.dim() != 1 or row_class.numel() != s.V:
        raise ValueError(f"newsreclib_amd: row_class must have one entry per table row ({s.V}), got {tuple(row_class.shape)}")
    m = max(min(int(max_per_class), 2 ** 31 - 1), 0)                          # (as an int32; anything below 1 is refused natively)
    return s._replace(trail=(*s.trail, row_class.data_ptr(), m), keep=(*s.keep, row_class))


def topk_scores_capped(user_vec: torch.Tensor, table: torch.Tensor, k: int, row_class: torch.Tensor, max_per_class: int,
                       excl_idx: Optional[torch.Tensor] = None, excl_off: Optional[torch.Tensor] = None,
                       eligible: Optional[torch.Tensor] = None, slices: int = 0):
    """``nrl_topk_scores_capped``: ``topk_scores`` with at most ``max_per_class`` rows of any one class in a user's list.
    ``row_class`` (V int32, or int64: converted by one device op) gives every table row its class (a category, a subcategory, a
    sentiment class; any value is a class of its own).  Walking a user's rows that are eligible, not excluded and not NaN-scored
    in ``topk_scores``' order, a row is taken while fewer than ``max_per_class`` rows of its class have been; the first ``k``
    (at most ``TOPK_CAP_MAX_K``) are returned, ``-1`` / ``-inf`` beyond them.  Returns, flags and the rest of the arguments are
    those of ``topk_scores``; with ``max_per_class >= k`` so are the bits.  Nothing here synchronises with the host."""
    s = _capped(_dot_scorer(user_vec, table), row_class, max_per_class)
    return _run_topk("nrl_topk_scores_capped", s, k, excl_idx, excl_off, eligible, slices)


RANK_MAX_TARGETS = 32
# the status word of ``catalogue_ranks``: the flags of ``topk_scores`` it shares, in its own words, and its two own bits
RANK_FLAGS = {1: TOPK_FLAGS[1],
              2: "excl_off decreases or leaves its range (that user's ranks and population are 0)",
              4: "a NaN score of an eligible, not excluded row (that row is left out of that user's population)",
              16: "tgt_off decreases or leaves its range, or a user owns more than 32 targets (that user's ranks are 0)",
              32: "a target index is outside [0, V) (its rank is 0)"}


def catalogue_ranks(user_vec: torch.Tensor, table: torch.Tensor, tgt_idx: torch.Tensor, tgt_off: torch.Tensor,
                    excl_idx: Optional[torch.Tensor] = None, excl_off: Optional[torch.Tensor] = None,
                    eligible: Optional[torch.Tensor] = None, slices: int = 0):
    """``nrl_catalogue_ranks``: where the held-out rows ``tgt_idx`` (int64) / ``tgt_off`` (B + 1 int64, ragged per user, at most
    ``RANK_MAX_TARGETS`` per user) land when each row of ``user_vec`` (B, D) is ranked against the whole ``table`` (V, D) ->
    (rank int32 (n_tgt), score fp32 (n_tgt), ranked int32 (B), status (1) int32).  ``rank`` is 1 + the number of rows of the
    user's population (eligible, not excluded, not NaN-scored) that ``topk_scores`` orders above the target, 0 when the target
    is not itself in the population (its ``score`` is then ``-inf``); ``ranked`` is the size of the population.  Scores, order,
    ``excl_idx`` / ``excl_off`` and ``eligible`` are those of ``topk_scores``, bit for bit: ``rank <= k`` exactly when the target is
    slot ``rank - 1`` of the user's top-k list.  The (B, V) score matrix is never materialised.  ``status`` (``RANK_FLAGS``)
    stays on the device -- nothing here synchronises with the host."""
    return _run_ranks("nrl_catalogue_ranks", _dot_scorer(user_vec, table), tgt_idx, tgt_off, excl_idx, excl_off, eligible, slices)


INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1


def _window(user_vec, table, row_time, win_lo, win_hi):
    """The three int32 arrays of a windowed entry: dtype (``TypeError``) and lengths (``ValueError``) are refused before anything
    looks at a device, then the scorer's own checks and ``_chk`` -> (the scorer, the arrays' pointers, the tensors to keep alive)."""
    B = int(user_vec.shape[0]) if user_vec.dim() else -1
    V = int(table.shape[0]) if table.dim() else -1
    named = ((row_time, "row_time", V, "table row"), (win_lo, "win_lo", B, "user"), (win_hi, "win_hi", B, "user"))
    for t, name, n, what in named:
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int32:
            raise TypeError(f"newsreclib_amd: `{name}` must be an int32 tensor, got "
                            f"{t.dtype if isinstance(t, torch.Tensor) else type(t).__name__}")
    for t, name, n, what in named:
        if t.dim() != 1 or t.numel() != n:
            raise ValueError(f"newsreclib_amd: `{name}` must have one entry per {what} ({n}), got {tuple(t.shape)}")
    s = _dot_scorer(user_vec, table)
    keep = tuple(_chk(t, torch.int32, name) for t, name, _, _ in named)
    return s._replace(keep=(*s.keep, *keep)), tuple(t.data_ptr() for t in keep)


def topk_window_scores(user_vec: torch.Tensor, table: torch.Tensor, k: int, row_time: torch.Tensor, win_lo: torch.Tensor,
                       win_hi: torch.Tensor, excl_idx: Optional[torch.Tensor] = None, excl_off: Optional[torch.Tensor] = None,
                       eligible: Optional[torch.Tensor] = None, slices: int = 0):
    """``nrl_topk_window_scores``: ``topk_scores`` with a time window of its own per user.  Row ``v`` can be returned for user ``u``
    only when ``win_lo[u] <= row_time[v] <= win_hi[u]`` -- ``row_time`` (V) and ``win_lo`` / ``win_hi`` (B) int32 in any one unit,
    the interval closed, ``(INT32_MIN, INT32_MAX)`` no window, ``win_lo[u] > win_hi[u]`` an empty one (a row of ``-1`` / ``-inf``,
    no flag).  Returns, order, masks, flags (``TOPK_FLAGS``) and the score bits are those of ``topk_scores``; a NaN score is
    flagged only for a row inside that user's window.  A table tile outside the windows of all 64 users of a workgroup is neither
    read nor multiplied, so on a table in time order the cost falls with the windows.  Nothing here synchronises with the host."""
    s, ptrs = _window(user_vec, table, row_time, win_lo, win_hi)
    return _run_topk("nrl_topk_window_scores", s._replace(trail=ptrs), k, excl_idx, excl_off, eligible, slices)


def catalogue_window_ranks(user_vec: torch.Tensor, table: torch.Tensor, tgt_idx: torch.Tensor, tgt_off: torch.Tensor,
                           row_time: torch.Tensor, win_lo: torch.Tensor, win_hi: torch.Tensor,
                           excl_idx: Optional[torch.Tensor] = None, excl_off: Optional[torch.Tensor] = None,
                           eligible: Optional[torch.Tensor] = None, slices: int = 0):
    """``nrl_catalogue_window_ranks``: ``catalogue_ranks`` against the population of ``topk_window_scores`` -> (rank int32 (n_tgt),
    score fp32 (n_tgt), ranked int32 (B), status (1) int32).  A target outside its owner's window has rank 0 and score ``-inf``
    without a flag, like an ineligible one; ``ranked`` counts the rows inside the window.  ``rank <= k`` exactly when the target is
    slot ``rank - 1`` of ``topk_window_scores(k)``, with the same score bits.  Flags: ``RANK_FLAGS``.  Nothing here synchronises
    with the host."""
    s, ptrs = _window(user_vec, table, row_time, win_lo, win_hi)
    return _run_ranks("nrl_catalogue_window_ranks", s, tgt_idx, tgt_off, excl_idx, excl_off, eligible, slices, after=ptrs)


def _sample_args(user_key, n: int, seed, inv_temp=None):
    """The arguments of the Gumbel entries, refused before anything looks at a device: an int64 key tensor of ``n`` entries
    (``TypeError`` / ``ValueError``), a seed in [0, 2^64) and a finite ``inv_temp >= 0`` (``ValueError``) -> (seed, inv_temp)."""
    if not isinstance(user_key, torch.Tensor) or user_key.dtype != torch.int64:
        raise TypeError(f"newsreclib_amd: `user_key` must be an int64 tensor, got "
                        f"{user_key.dtype if isinstance(user_key, torch.Tensor) else type(user_key).__name__}")
    if user_key.dim() != 1 or user_key.numel() != n:
        raise ValueError(f"newsreclib_amd: `user_key` must have one entry per user ({n}), got {tuple(user_key.shape)}")
    if isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed < 2 ** 64:
        raise ValueError(f"newsreclib_amd: `seed` must be an integer in [0, 2^64), got {seed!r}")
    if inv_temp is not None:
        inv_temp = float(inv_temp)
        if not math.isfinite(inv_temp) or inv_temp < 0 or inv_temp > 3.4028234663852886e38:
            raise ValueError(f"newsreclib_amd: `inv_temp` must be finite (in fp32) and >= 0, got {inv_temp!r}")
    return seed, inv_temp


def gumbel_noise(user_key: torch.Tensor, row: torch.Tensor, seed: int):
    """``nrl_gumbel_noise``: the noise of ``topk_sampled_scores`` for the pairs ``(user_key[i], row[i])`` (int64, equal lengths) under
    ``seed`` -> (u, g) fp32: ``u = (2 m + 1) 2^-24`` with ``m`` the top 23 bits of the pair's hash, ``g = -log(-log(u))``.  The
    device function the sampled walk calls: the same bits."""
    if not isinstance(row, torch.Tensor) or row.dtype != torch.int64:
        raise TypeError(f"newsreclib_amd: `row` must be an int64 tensor, got "
                        f"{row.dtype if isinstance(row, torch.Tensor) else type(row).__name__}")
    if row.dim() != 1:
        raise ValueError(f"newsreclib_amd: `row` must be one-dimensional, got {tuple(row.shape)}")
    n = int(row.numel())
    seed, _ = _sample_args(user_key, n, seed)
    user_key, row = _chk(user_key, torch.int64, "user_key"), _chk(row, torch.int64, "row")
    u = torch.empty(n, dtype=torch.float32, device=row.device)
    g = torch.empty(n, dtype=torch.float32, device=row.device)
    _lib.check(_lib.load().nrl_gumbel_noise(user_key.data_ptr(), row.data_ptr(), n, seed, u.data_ptr(), g.data_ptr(), _stream()),
               "nrl_gumbel_noise")
    return u, g


def topk_sampled_scores(user_vec: torch.Tensor, table: torch.Tensor, k: int, user_key: torch.Tensor, seed: int,
                        inv_temp: float = 1.0, excl_idx: Optional[torch.Tensor] = None, excl_off: Optional[torch.Tensor] = None,
                        eligible: Optional[torch.Tensor] = None, slices: int = 0):
    """``nrl_topk_sampled_scores``: Gumbel top-k, one Plackett-Luce draw without replacement from ``softmax(score * inv_temp)`` per
    user -> (idx (B, k) int64, key (B, k) fp32, score (B, k) fp32, status (1) int32).  The list is ``topk_scores``' over the
    perturbed key ``z = fl(fl(score * inv_temp) + g)``, ``g`` the Gumbel noise of ``(seed, user_key[b], row)`` (``gumbel_noise``),
    generated where the score is consumed: neither the (B, V) scores nor a (B, V) noise matrix is materialised.  ``key`` is ``z``
    (descending; equal ``z`` -- 23 random bits per pair, so it happens -- by ascending row), ``score`` the raw score with the bits
    ``topk_scores`` reports for that (user, row), ``-1`` / ``-inf`` / ``-inf`` beyond the population.  ``user_key`` (B int64) names
    the users: a user's lists depend on ``(seed, its key, its vector, the table, its masks, inv_temp)`` and on nothing else -- not
    on B, its place in the batch, ``slices`` or earlier calls.  ``inv_temp = 0`` is a uniformly random ordered k-subset.  Masks and
    flags (``TOPK_FLAGS``) are those of ``topk_scores``.  Nothing here synchronises with the host."""
    B = int(user_vec.shape[0]) if isinstance(user_vec, torch.Tensor) and user_vec.dim() else -1
    seed, inv_temp = _sample_args(user_key, B, seed, inv_temp)
    s = _dot_scorer(user_vec, table)
    user_key = _chk(user_key, torch.int64, "user_key")
    score = torch.empty((s.B, max(int(k), 0)), dtype=torch.float32, device=s.dev)
    s = s._replace(trail=(user_key.data_ptr(), seed, inv_temp), keep=(*s.keep, user_key))
    idx, key, status = _run_topk("nrl_topk_sampled_scores", s, k, excl_idx, excl_off, eligible, slices, extra=(score,))
    return idx, key, score, status


TOPK_MAX_DRAWS = 32


def _draws_arg(k, draws) -> int:
    """``draws`` of ``topk_sampled_draws`` against ``k``, refused before anything looks at a device -> draws."""
    if isinstance(draws, bool) or not isinstance(draws, int):
        raise TypeError(f"newsreclib_amd: `draws` must be an integer, got {type(draws).__name__}")
    if not 1 <= draws <= TOPK_MAX_DRAWS:
        raise ValueError(f"newsreclib_amd: `draws` must be in [1, {TOPK_MAX_DRAWS}], got {draws}")
    if isinstance(k, bool) or not isinstance(k, int):
        raise TypeError(f"newsreclib_amd: `k` must be an integer, got {type(k).__name__}")
    if k >= 1 and draws * k > TOPK_MAX_K:
        raise ValueError(f"newsreclib_amd: `draws * k` must be at most {TOPK_MAX_K}, got {draws} * {k}")
    return draws


def topk_sampled_draws(user_vec: torch.Tensor, table: torch.Tensor, k: int, draws: int, user_key: torch.Tensor, seed: int,
                       inv_temp: float = 1.0, excl_idx: Optional[torch.Tensor] = None, excl_off: Optional[torch.Tensor] = None,
                       eligible: Optional[torch.Tensor] = None, slices: int = 0):
    """``nrl_topk_sampled_draws``: ``draws`` Gumbel top-k lists per user from ONE walk over the table -> (idx (B, draws, k) int64,
    key (B, draws, k) fp32, score (B, draws, k) fp32, status (1) int32).  Draw ``r`` is, bit for bit in all three outputs, what
    ``topk_sampled_scores`` returns under ``(seed + r) mod 2^64`` with everything else equal, and ``status`` is the OR of those
    calls' words: the dot products are computed once per table tile and perturbed ``draws`` times.  ``draws`` in
    ``[1, TOPK_MAX_DRAWS]`` and ``draws * k <= TOPK_MAX_K``; the other arguments, their checks and the flags (``TOPK_FLAGS``) are
    those of ``topk_sampled_scores``.  Nothing here synchronises with the host."""
    draws = _draws_arg(k, draws)
    B = int(user_vec.shape[0]) if isinstance(user_vec, torch.Tensor) and user_vec.dim() else -1
    seed, inv_temp = _sample_args(user_key, B, seed, inv_temp)
    s = _dot_scorer(user_vec, table)
    user_key = _chk(user_key, torch.int64, "user_key")
    lib = _lib.load()
    excl_idx, excl_off, eligible = _topk_masks(excl_idx, excl_off, eligible, s.B, s.V)
    shape = (s.B, draws, max(k, 0))
    idx = torch.empty(shape, dtype=torch.int64, device=s.dev)
    key, score = (torch.empty(shape, dtype=torch.float32, device=s.dev) for _ in range(2))
    status = torch.zeros(1, dtype=torch.int32, device=s.dev)
    ws = workspace(lib.nrl_topk_sampled_draws_workspace_size(s.B, s.V, s.D, k, draws, int(slices)), s.dev)
    _lib.check(lib.nrl_topk_sampled_draws(*s.lead, k, draws, _ptr(excl_idx), _ptr(excl_off), _ptr(eligible), user_key.data_ptr(), seed,
                                          inv_temp, int(slices), idx.data_ptr(), key.data_ptr(), score.data_ptr(), status.data_ptr(),
                                          ws.data_ptr(), ws.numel(), _stream()), "nrl_topk_sampled_draws")
    return idx, key, score, status


# the status word of ``list_class_exposure`` (a dictionary of its own: the key sets of the other flag dictionaries are pinned)
EXPOSURE_FLAGS = {1: "a listed row other than -1 is outside [0, V) (it counts for no class)",
                  64: "a class id is outside [0, S) (that row counts for no class)"}


def list_class_exposure(list_idx: torch.Tensor, row_class: torch.Tensor, pos_weight: torch.Tensor, S: int):
    """``nrl_list_class_exposure``: the position-weighted exposure that ``L`` lists per user give each of ``S`` classes ->
    (exposure (B, S) fp32, status (1) int32).  ``list_idx`` (B, L, k) int64, ``-1`` an empty slot (the draws of
    ``topk_sampled_draws``; (B, k) is taken as L = 1); ``row_class`` (V int32, or int64: converted by one device op); ``pos_weight``
    (k) fp32.  ``exposure[b, s]`` is the sum, over the lists in order and their slots in order, of ``pos_weight[j]`` where the
    slot's row has class ``s``, accumulated in float64, divided by ``L`` and rounded once.  ``S`` in ``[1, TOPK_MAX_BIAS_CLASSES]``,
    ``k`` in ``[1, TOPK_MAX_K]``.  A row outside the table or a class outside ``[0, S)`` counts for no class and is flagged
    (``EXPOSURE_FLAGS``).  Nothing here synchronises with the host."""
    if not isinstance(list_idx, torch.Tensor) or list_idx.dtype != torch.int64:
        raise TypeError(f"newsreclib_amd: `list_idx` must be an int64 tensor, got "
                        f"{list_idx.dtype if isinstance(list_idx, torch.Tensor) else type(list_idx).__name__}")
    if not isinstance(row_class, torch.Tensor) or row_class.dtype not in (torch.int32, torch.int64):
        raise TypeError(f"newsreclib_amd: `row_class` must be an int32 tensor, got "
                        f"{row_class.dtype if isinstance(row_class, torch.Tensor) else type(row_class).__name__}")
    if not isinstance(pos_weight, torch.Tensor) or pos_weight.dtype != torch.float32:
        raise TypeError(f"newsreclib_amd: `pos_weight` must be a float32 tensor, got "
                        f"{pos_weight.dtype if isinstance(pos_weight, torch.Tensor) else type(pos_weight).__name__}")
    if list_idx.dim() == 2:
        list_idx = list_idx.unsqueeze(1)
    if list_idx.dim() != 3:
        raise ValueError(f"newsreclib_amd: `list_idx` must be (B, L, k), got {tuple(list_idx.shape)}")
    B, L, k = (int(n) for n in list_idx.shape)
    S = int(S)
    if not 1 <= S <= TOPK_MAX_BIAS_CLASSES:
        raise ValueError(f"newsreclib_amd: `S` must be in [1, {TOPK_MAX_BIAS_CLASSES}], got {S}")
    if L < 1 or not 1 <= k <= TOPK_MAX_K:
        raise ValueError(f"newsreclib_amd: `list_idx` must hold L >= 1 lists of 1 <= k <= {TOPK_MAX_K} slots, got {tuple(list_idx.shape)}")
    if row_class.dim() != 1:
        raise ValueError(f"newsreclib_amd: `row_class` must be one-dimensional, got {tuple(row_class.shape)}")
    if pos_weight.dim() != 1 or pos_weight.numel() != k:
        raise ValueError(f"newsreclib_amd: `pos_weight` must have one entry per slot ({k}), got {tuple(pos_weight.shape)}")
    if row_class.dtype == torch.int64 and row_class.is_cuda:
        row_class = row_class.to(torch.int32)
    list_idx, row_class = _chk(list_idx, torch.int64, "list_idx"), _chk(row_class, torch.int32, "row_class")
    pos_weight = _chk(pos_weight, torch.float32, "pos_weight")
    out = torch.empty((B, S), dtype=torch.float32, device=list_idx.device)
    status = torch.zeros(1, dtype=torch.int32, device=list_idx.device)
    _lib.check(_lib.load().nrl_list_class_exposure(list_idx.data_ptr(), row_class.data_ptr(), pos_weight.data_ptr(), B, L, k,
                                                   int(row_class.numel()), S, out.data_ptr(), status.data_ptr(), _stream()),
               "nrl_list_class_exposure")
    return out, status


# the status word of ``catalogue_logz`` / ``list_logprob``: the flags of ``topk_scores`` they share, in their own words, and their
# two own bits (a dictionary of its own: the key set of ``TOPK_FLAGS`` is pinned)
POLICY_FLAGS = {1: TOPK_FLAGS[1],
                2: "excl_off decreases or leaves its range (that user's population is empty)",
                4: "a NaN scaled score of an eligible, not excluded row (that row is left out of that user's sums)",
                128: "an invalid list: a hole before a row, a row outside [0, V), a row twice or a row outside the user's population "
                     "(that user's log-probabilities are NaN)",
                256: "an infinite scaled score of an eligible, not excluded row (that row is left out of that user's sums)"}


def _policy_args(inv_temp, lists, name: str, user_vec):
    """The arguments of the policy entries, refused before anything looks at a device: a finite ``inv_temp >= 0`` (``ValueError``)
    and, when given, an int64 tensor ``lists`` (``TypeError``) of shape (B, k <= TOPK_MAX_K) (``ValueError``) -> inv_temp."""
    if not isinstance(user_vec, torch.Tensor) or user_vec.dtype != torch.float32:
        raise TypeError(f"newsreclib_amd: `user_vec` must be a float32 tensor, got "
                        f"{user_vec.dtype if isinstance(user_vec, torch.Tensor) else type(user_vec).__name__}")
    if lists is not None:
        if not isinstance(lists, torch.Tensor) or lists.dtype != torch.int64:
            raise TypeError(f"newsreclib_amd: `{name}` must be an int64 tensor, got "
                            f"{lists.dtype if isinstance(lists, torch.Tensor) else type(lists).__name__}")
        B = int(user_vec.shape[0]) if user_vec.dim() else -1
        if lists.dim() != 2 or lists.shape[0] != B:
            raise ValueError(f"newsreclib_amd: `{name}` must be (B, k) with one list per user ({B}), got {tuple(lists.shape)}")
        if lists.shape[1] > TOPK_MAX_K:
            raise ValueError(f"newsreclib_amd: `{name}` holds at most {TOPK_MAX_K} rows per user, got {int(lists.shape[1])}")
    inv_temp = float(inv_temp)
    if not math.isfinite(inv_temp) or inv_temp < 0 or inv_temp > 3.4028234663852886e38:
        raise ValueError(f"newsreclib_amd: `inv_temp` must be finite (in fp32) and >= 0, got {inv_temp!r}")
    return inv_temp


def catalogue_logz(user_vec: torch.Tensor, table: torch.Tensor, inv_temp: float = 1.0, excl_idx: Optional[torch.Tensor] = None,
                   excl_off: Optional[torch.Tensor] = None, eligible: Optional[torch.Tensor] = None,
                   drop_idx: Optional[torch.Tensor] = None):
    """``nrl_catalogue_logz``: the log-partition of the policy ``topk_sampled_scores`` draws from, ``softmax(t)`` with
    ``t = fl(score * inv_temp)`` over each user's population (eligible, not excluded, ``t`` finite) minus the rows of
    ``drop_idx`` ((B, kd) int64, ``-1`` an empty slot) -> (max (B) fp32, logsum (B) fp32: ``log sum exp(t - max)``, entropy (B)
    fp32 in nats, pop (B) int32, dropped (B) int32: the rows of ``drop_idx`` found in the population, status (1) int32).
    ``log Z = max + logsum``; ``log p(row) = (t - max) - logsum``.  The (B, V) score matrix is never materialised, and a user's
    outputs do not depend on B, its place in the batch or the form of the mask, bit for bit.  An empty population gives
    ``-inf, -inf, 0, 0``.  ``status`` (``POLICY_FLAGS``) stays on the device -- nothing here synchronises with the host."""
    inv_temp = _policy_args(inv_temp, drop_idx, "drop_idx", user_vec)
    s = _dot_scorer(user_vec, table)
    lib = _lib.load()
    excl_idx, excl_off, eligible = _topk_masks(excl_idx, excl_off, eligible, s.B, s.V)
    kd = 0
    if drop_idx is not None:
        drop_idx, kd = _chk(drop_idx, torch.int64, "drop_idx"), int(drop_idx.shape[1])
    mx, ls, ent = (torch.empty(s.B, dtype=torch.float32, device=s.dev) for _ in range(3))
    pop = torch.empty(s.B, dtype=torch.int32, device=s.dev)
    dropped = torch.zeros(s.B, dtype=torch.int32, device=s.dev)
    status = torch.zeros(1, dtype=torch.int32, device=s.dev)
    ws = workspace(lib.nrl_catalogue_logz_workspace_size(s.B, s.V, s.D), s.dev)
    _lib.check(lib.nrl_catalogue_logz(*s.lead, inv_temp, _ptr(excl_idx), _ptr(excl_off), _ptr(eligible), _ptr(drop_idx) if kd else None,
                                      kd, mx.data_ptr(), ls.data_ptr(), ent.data_ptr(), pop.data_ptr(), dropped.data_ptr(),
                                      status.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "nrl_catalogue_logz")
    return mx, ls, ent, pop, dropped, status


def list_logprob(user_vec: torch.Tensor, table: torch.Tensor, list_idx: torch.Tensor, inv_temp: float = 1.0,
                 excl_idx: Optional[torch.Tensor] = None, excl_off: Optional[torch.Tensor] = None,
                 eligible: Optional[torch.Tensor] = None):
    """The Plackett-Luce log-probability of given lists under the policy ``topk_sampled_scores`` draws from: ``list_idx`` (B, k)
    int64, ``-1`` in trailing empty slots -> (logp (B, k) fp32: slot j's log-probability given the slots before it, total (B)
    fp32: the list's, score (B, k) fp32: the raw scores with the bits ``topk_scores`` reports, status (1) int32).
    ``catalogue_logz`` with ``drop_idx = list_idx`` gives the tail -- the population without the listed rows -- and
    ``nrl_list_logprob`` adds the listed rows back from the last slot, in float64: positive terms only, so a slot keeps its
    precision when the slots before it hold almost all the mass.  An empty slot has logp ``+0`` and score ``-inf``.  A list with a
    hole, a row outside the table, a row twice or a row outside the user's population (excluded, ineligible, non-finite) makes
    that user's ``logp`` and ``total`` NaN and sets bit 128 of ``status`` (``POLICY_FLAGS``).  Nothing here synchronises with the
    host."""
    if list_idx is None:
        raise TypeError("newsreclib_amd: `list_idx` must be an int64 tensor, got NoneType")
    inv_temp = _policy_args(inv_temp, list_idx, "list_idx", user_vec)
    if list_idx.shape[1] < 1:
        raise ValueError("newsreclib_amd: `list_idx` must hold at least one slot per user")
    mx, ls, _, pop, dropped, status = catalogue_logz(user_vec, table, inv_temp, excl_idx, excl_off, eligible, list_idx)
    s = _dot_scorer(user_vec, table)
    list_idx = _chk(list_idx, torch.int64, "list_idx")
    k = int(list_idx.shape[1])
    score, logp = (torch.empty((s.B, k), dtype=torch.float32, device=s.dev) for _ in range(2))
    total = torch.empty(s.B, dtype=torch.float32, device=s.dev)
    _lib.check(_lib.load().nrl_list_logprob(*s.lead, inv_temp, list_idx.data_ptr(), k, mx.data_ptr(), ls.data_ptr(), pop.data_ptr(),
                                            dropped.data_ptr(), score.data_ptr(), logp.data_ptr(), total.data_ptr(),
                                            status.data_ptr(), _stream()), "nrl_list_logprob")
    return logp, total, score, status


TOPK_MAX_BIAS_CLASSES = 64
# the status words of the class-biased entries: the flags of ``topk_scores`` / ``catalogue_ranks`` and one more (bit 64).  They are
# dictionaries of their own, as ``ENSEMBLE_RANK_FLAGS`` is: the key sets of ``TOPK_FLAGS`` and ``RANK_FLAGS`` are pinned.
TOPK_BIAS_FLAGS = {**TOPK_FLAGS, 64: "a class id is outside [0, S) (that row is scored with bias 0)"}
RANK_BIAS_FLAGS = {**RANK_FLAGS, 64: TOPK_BIAS_FLAGS[64]}


def _bias_scorer(user_vec, table, bias, row_class) -> _Scorer:
    """The dot-product scorer with ``(bias, row_class, S)`` behind ``D``: ``bias`` (B, S) fp32 and ``row_class`` checked (one int32
    per table row; int64 converted by one device op).  The class ids themselves are checked on the device (``TOPK_BIAS_FLAGS[64]``)."""
    s = _dot_scorer(user_vec, table)
    if bias is None or row_class is None:
        raise ValueError("newsreclib_amd: bias (B, S) and row_class (one class id per table row) are required")
    bias = _chk(bias, torch.float32, "bias")
    if bias.dim() != 2 or bias.shape[0] != s.B or bias.shape[1] < 1:
        raise ValueError(f"newsreclib_amd: bias (B, S) with B = {s.B} and S >= 1 expected, got {tuple(bias.shape)}")
    S = int(bias.shape[1])
    if S > TOPK_MAX_BIAS_CLASSES:
        raise NotImplementedError(f"newsreclib_amd: a class bias takes at most {TOPK_MAX_BIAS_CLASSES} classes (got {S})")
    if row_class.dtype == torch.int64 and row_class.is_cuda:
        row_class = row_class.to(torch.int32)
    row_class = _chk(row_class, torch.int32, "row_class")
    if row_class.dim() != 1 or row_class.numel() != s.V:
        raise ValueError(f"newsreclib_amd: row_class must have one entry per table row ({s.V}), got {tuple(row_class.shape)}")
    return s._replace(lead=(*s.lead, bias.data_ptr(), row_class.data_ptr(), S), keep=(*s.keep, bias, row_class))


def topk_bias_scores(user_vec: torch.Tensor, table: torch.Tensor, bias: torch.Tensor, row_class: torch.Tensor, k: int,
                     excl_idx: Optional[torch.Tensor] = None, excl_off: Optional[torch.Tensor] = None,
                     eligible: Optional[torch.Tensor] = None, slices: int = 0):
    """``nrl_topk_bias_scores``: ``topk_scores`` by ``user_vec[u] . table[v] + bias[u, row_class[v]]`` -- ``bias`` (B, S) fp32, a
    per-user additive term per class (a category-affinity prior, a sentiment penalty, SentiDebias's ``u_aware T^T``), ``S`` at
    most ``TOPK_MAX_BIAS_CLASSES``; ``row_class`` (V int32, or int64: converted by one device op).  The dot product has the bits
    of ``topk_scores`` and the bias is one fp32 add behind it, so an all-zero bias returns ``topk_scores``' rows and scores.  A
    class id outside [0, S) is scored with bias 0 and flagged (``TOPK_BIAS_FLAGS[64]``); a NaN sum is dropped and flagged as any NaN
    score.  Returns, order, masks and the other flags (``TOPK_BIAS_FLAGS``) are those of ``topk_scores``.  Nothing here
    synchronises with the host."""
    return _run_topk("nrl_topk_bias_scores", _bias_scorer(user_vec, table, bias, row_class), k, excl_idx, excl_off, eligible, slices)


def topk_bias_scores_capped(user_vec: torch.Tensor, table: torch.Tensor, bias: torch.Tensor, row_class: torch.Tensor, k: int,
                            cap_class: torch.Tensor, max_per_class: int, excl_idx: Optional[torch.Tensor] = None,
                            excl_off: Optional[torch.Tensor] = None, eligible: Optional[torch.Tensor] = None, slices: int = 0):
    """``nrl_topk_bias_scores_capped``: ``topk_bias_scores`` with at most ``max_per_class`` rows of any one class of ``cap_class``
    in a user's list, as ``topk_scores_capped`` caps ``topk_scores``.  ``cap_class`` (V) is an array of its own: the cap may go by
    category while the bias goes by sentiment.  With ``max_per_class >= k`` the bits are those of ``topk_bias_scores``."""
    s = _capped(_bias_scorer(user_vec, table, bias, row_class), cap_class, max_per_class)
    return _run_topk("nrl_topk_bias_scores_capped", s, k, excl_idx, excl_off, eligible, slices)


def catalogue_bias_ranks(user_vec: torch.Tensor, table: torch.Tensor, bias: torch.Tensor, row_class: torch.Tensor,
                         tgt_idx: torch.Tensor, tgt_off: torch.Tensor, excl_idx: Optional[torch.Tensor] = None,
                         excl_off: Optional[torch.Tensor] = None, eligible: Optional[torch.Tensor] = None, slices: int = 0):
    """``nrl_catalogue_bias_ranks``: ``catalogue_ranks`` by the scores of ``topk_bias_scores`` -> (rank int32 (n_tgt), score fp32
    (n_tgt), ranked int32 (B), status (1) int32) with the targets, population, order, masks and flags (``RANK_BIAS_FLAGS``) of
    ``catalogue_ranks`` and the score bits of ``topk_bias_scores``: ``rank <= k`` exactly when the target is slot ``rank - 1`` of
    that call's list.  Nothing here synchronises with the host."""
    return _run_ranks("nrl_catalogue_bias_ranks", _bias_scorer(user_vec, table, bias, row_class), tgt_idx, tgt_off, excl_idx,
                      excl_off, eligible, slices)


# ---- greedy MMR re-ranking of a top-k pool (nrl_topk.hip: mmr_rerank_kernel) ------------------------------------------------------
MMR_MAX_POOL = 128
MMR_SIMILARITIES = {"cosine": 0, "dot": 1}
# the status word of ``mmr_rerank``; a dictionary of its own: bit 1 means something else in ``TOPK_FLAGS``, whose key set is pinned
MMR_FLAGS = {1: "a pool row other than -1 is outside [0, V) (that slot is dead)",
             4: "a non-finite score, or a non-finite self-similarity, in a slot with a valid row (that slot is dead)"}


def mmr_rerank(pool_idx: torch.Tensor, pool_score: torch.Tensor, table: torch.Tensor, k: int, lam: float,
               similarity: str = "cosine", normalize: bool = True):
    """``nrl_mmr_rerank``: greedy Maximal Marginal Relevance over a pool of table rows per user -> (idx (B, k) int64, score (B, k)
    fp32, mmr (B, k) fp32, status (1) int32).  ``pool_idx`` (B, N) int64 (``-1``: an empty slot) and ``pool_score`` (B, N) fp32 are
    what any ``topk_*`` wrapper returns, N at most ``MMR_MAX_POOL``; ``table`` (V, D) fp32 holds the news vectors.  Step by step
    the live, unselected slot of largest ``lam * rel_i - (1 - lam) * max_{c selected} sim(c, i)`` is taken (ties: the lower slot);
    ``similarity``: ``"cosine"`` or ``"dot"`` of the table rows, with the bits of ``topk_scores``' chain; ``normalize``: ``rel``
    is the score min-max scaled over the user's live slots, else the score itself.  ``score`` is the slot's pool score unchanged,
    ``mmr`` the objective it won with; ``-1`` / ``-inf`` / ``-inf`` once the live slots run out.  ``lam = 1`` without ``normalize``
    returns the pool's first ``k`` entries.  The native header states every rounding.  ``status``: ``MMR_FLAGS``; it stays on the
    device -- nothing here synchronises with the host."""
    for t, dt, name in ((pool_idx, torch.int64, "pool_idx"), (pool_score, torch.float32, "pool_score"), (table, torch.float32, "table")):
        if t.dtype != dt:
            raise ValueError(f"newsreclib_amd: `{name}` must be {dt}, got {t.dtype}")
    if pool_idx.dim() != 2 or pool_score.shape != pool_idx.shape or table.dim() != 2:
        raise ValueError(f"newsreclib_amd: pool_idx (B, N), pool_score (B, N) and table (V, D) expected, got {tuple(pool_idx.shape)}, "
                         f"{tuple(pool_score.shape)} and {tuple(table.shape)}")
    if similarity not in MMR_SIMILARITIES:
        raise ValueError(f"newsreclib_amd: similarity is one of {sorted(MMR_SIMILARITIES)}, got {similarity!r}")
    B, N, V, D, k = int(pool_idx.shape[0]), int(pool_idx.shape[1]), int(table.shape[0]), int(table.shape[1]), int(k)
    if N > MMR_MAX_POOL:
        raise NotImplementedError(f"newsreclib_amd: mmr_rerank takes a pool of at most {MMR_MAX_POOL} slots (got {N})")
    if not 1 <= k <= N:
        raise ValueError(f"newsreclib_amd: k in [1, N = {N}] expected, got {k}")
    if not 0.0 <= float(lam) <= 1.0:
        raise ValueError(f"newsreclib_amd: lam in [0, 1] expected, got {lam}")
    pool_idx, pool_score, table = _chk(pool_idx, torch.int64, "pool_idx"), _chk(pool_score, torch.float32, "pool_score"), \
        _chk(table, torch.float32, "table")
    lib = _lib.load()
    dev = pool_idx.device
    idx, score, status = _topk_outputs(B, k, dev)
    mmr = torch.empty((B, k), dtype=torch.float32, device=dev)
    _lib.check(lib.nrl_mmr_rerank(pool_idx.data_ptr(), pool_score.data_ptr(), table.data_ptr() if V else None, B, N, V, D, k,
                                  float(lam), MMR_SIMILARITIES[similarity], int(bool(normalize)), idx.data_ptr(), score.data_ptr(),
                                  mmr.data_ptr(), status.data_ptr(), _stream()), "nrl_mmr_rerank")
    return idx, score, mmr, status


# ---- calibrated greedy re-ranking of a top-k pool (nrl_topk.hip: cal_rerank_kernel) ---------------------------------------------------
CAL_MAX_CLASSES = 64
# the status word of ``calibrated_rerank``; a dictionary of its own: the key sets of ``MMR_FLAGS`` and ``TOPK_FLAGS`` are pinned
CAL_FLAGS = {1: MMR_FLAGS[1], 4: MMR_FLAGS[4],
             64: "a class id outside [0, S) (that slot stays in the pool with a calibration term of 0 and counts for no class)",
             128: "a negative, NaN or infinite target entry (taken as 0)"}


def calibrated_rerank(pool_idx: torch.Tensor, pool_score: torch.Tensor, table: Optional[torch.Tensor], row_class: torch.Tensor,
                      target: torch.Tensor, k: int, lam: float, mu: float, gamma: float, similarity: str = "cosine",
                      normalize: bool = True):
    """``nrl_calibrated_rerank``: greedy re-ranking of a pool of table rows per user by ``lam * rel_i - mu * max_{c selected}
    sim(c, i) + gamma * cal(class_i)`` -> (idx (B, k) int64, score (B, k) fp32, obj (B, k) fp32, cal (B, k) fp32, status (1)
    int32).  ``pool_idx`` / ``pool_score`` / ``table`` / ``similarity`` / ``normalize`` as for ``mmr_rerank``; ``row_class`` (V
    int32, or int64: converted by one device op) gives every table row its class, ``target`` (B, S) fp32 every user's class target
    (``class_targets``), S at most ``CAL_MAX_CLASSES``.  ``cal(c)`` is the generalised Jaccard overlap ``sum(min) / sum(max)``
    between the class counts of the list with a slot of class ``c`` added and the target: with the history's class counts as the
    target, the list's Personalization@k.  ``lam``, ``mu``, ``gamma`` each in [0, 1].  ``mu == 0`` needs no news vectors: ``table``
    may be ``None`` and no similarity is computed.  ``gamma = 0`` with ``mu = 1 - lam`` is ``mmr_rerank``.  ``obj`` is the objective
    a slot won with, ``cal`` its calibration term; ``-1`` / ``-inf`` / ``-inf`` / ``-inf`` once the live slots run out.  The native
    header states every rounding.  ``status``: ``CAL_FLAGS``; it stays on the device -- nothing here synchronises with the host."""
    checked = [(pool_idx, torch.int64, "pool_idx"), (pool_score, torch.float32, "pool_score"), (target, torch.float32, "target")]
    if table is not None:
        checked.append((table, torch.float32, "table"))
    for t, dt, name in checked:
        if t.dtype != dt:
            raise ValueError(f"newsreclib_amd: `{name}` must be {dt}, got {t.dtype}")
    if row_class is None or row_class.dtype not in (torch.int32, torch.int64):
        raise ValueError("newsreclib_amd: row_class (one int32 or int64 class id per table row) is required")
    if pool_idx.dim() != 2 or pool_score.shape != pool_idx.shape or (table is not None and table.dim() != 2) or row_class.dim() != 1:
        raise ValueError(f"newsreclib_amd: pool_idx (B, N), pool_score (B, N), table (V, D) and row_class (V) expected, got "
                         f"{tuple(pool_idx.shape)}, {tuple(pool_score.shape)}, {None if table is None else tuple(table.shape)} and "
                         f"{tuple(row_class.shape)}")
    B, N, V, k = int(pool_idx.shape[0]), int(pool_idx.shape[1]), int(row_class.numel()), int(k)
    if target.dim() != 2 or int(target.shape[0]) != B:
        raise ValueError(f"newsreclib_amd: target (B = {B}, S) expected, got {tuple(target.shape)}")
    S = int(target.shape[1])
    if table is not None and int(table.shape[0]) != V:
        raise ValueError(f"newsreclib_amd: row_class must have one entry per table row ({int(table.shape[0])}), got {V}")
    if similarity not in MMR_SIMILARITIES:
        raise ValueError(f"newsreclib_amd: similarity is one of {sorted(MMR_SIMILARITIES)}, got {similarity!r}")
    if N > MMR_MAX_POOL:
        raise NotImplementedError(f"newsreclib_amd: calibrated_rerank takes a pool of at most {MMR_MAX_POOL} slots (got {N})")
    if S > CAL_MAX_CLASSES:
        raise NotImplementedError(f"newsreclib_amd: calibrated_rerank takes at most {CAL_MAX_CLASSES} classes (got {S})")
    if S < 1:
        raise ValueError("newsreclib_amd: target needs at least one class column")
    if not 1 <= k <= N:
        raise ValueError(f"newsreclib_amd: k in [1, N = {N}] expected, got {k}")
    for name, value in (("lam", lam), ("mu", mu), ("gamma", gamma)):
        if not 0.0 <= float(value) <= 1.0:
            raise ValueError(f"newsreclib_amd: {name} in [0, 1] expected, got {value}")
    if float(mu) != 0.0 and table is None:
        raise ValueError("newsreclib_amd: mu != 0 penalises the similarity of news vectors: it needs the table")
    pool_idx, pool_score, target = _chk(pool_idx, torch.int64, "pool_idx"), _chk(pool_score, torch.float32, "pool_score"), \
        _chk(target, torch.float32, "target")
    if table is not None:
        table = _chk(table, torch.float32, "table")
    if row_class.dtype == torch.int64 and row_class.is_cuda:
        row_class = row_class.to(torch.int32)
    row_class = _chk(row_class, torch.int32, "row_class")
    lib = _lib.load()
    dev = pool_idx.device
    idx, score, status = _topk_outputs(B, k, dev)
    obj, cal = torch.empty((B, k), dtype=torch.float32, device=dev), torch.empty((B, k), dtype=torch.float32, device=dev)
    D = int(table.shape[1]) if table is not None else 0
    _lib.check(lib.nrl_calibrated_rerank(pool_idx.data_ptr(), pool_score.data_ptr(), table.data_ptr() if table is not None and V else None,
                                         B, N, V, D, row_class.data_ptr() if V else None, target.data_ptr(), S, k, float(lam),
                                         float(mu), float(gamma), MMR_SIMILARITIES[similarity], int(bool(normalize)), idx.data_ptr(),
                                         score.data_ptr(), obj.data_ptr(), cal.data_ptr(), status.data_ptr(), _stream()),
               "nrl_calibrated_rerank")
    return idx, score, obj, cal, status


# ---- greedy DPP re-ranking of a top-k pool (nrl_topk.hip: dpp_rerank_kernel) ----------------------------------------------------------
DPP_MAX_K = 64
# the status word of ``dpp_rerank``; a dictionary of its own: the key sets of ``MMR_FLAGS``, ``CAL_FLAGS`` and ``TOPK_FLAGS`` are pinned
DPP_FLAGS = {1: MMR_FLAGS[1], 4: MMR_FLAGS[4],
             256: "a negative, NaN or infinite quality entry (that slot is dead)",
             512: "the pool's kernel matrix ran out of rank before the list was full (the rest is listed by pool score, gain 0)"}


def dpp_rerank(pool_idx: torch.Tensor, pool_score: torch.Tensor, table: torch.Tensor, k: int, alpha: float = 1.0,
               similarity: str = "cosine", normalize: bool = True, quality: Optional[torch.Tensor] = None, eps: float = 1e-4):
    """``nrl_dpp_rerank``: greedy MAP inference of a determinantal point process over a pool of table rows per user (Chen, Zhang,
    Zhou 2018) -> (idx (B, k) int64, score (B, k) fp32, gain (B, k) fp32, status (1) int32).  ``pool_idx`` / ``pool_score`` /
    ``table`` / ``similarity`` / ``normalize`` as for ``mmr_rerank``, ``k`` at most ``DPP_MAX_K``.  The kernel matrix is
    ``L = diag(q) sim diag(q)``; step by step the slot that multiplies ``det L_S`` of the listed set by the most is taken (ties:
    the lower slot), so a news that is a mixture of listed ones is penalised even where it is close to none of them, which MMR's
    pairwise penalty cannot see.  ``quality`` (B, N) fp32 gives ``q`` itself (finite and >= 0); without it ``q_i = exp(alpha *
    rel_i)``, ``rel`` the score min-max scaled over the user's live slots (``normalize``) or the score itself:
    ``alpha = theta / (2 (1 - theta))`` is the paper's trade-off, 0 diversity alone.  A slot whose remaining gain is not above
    ``eps`` times its own ``L_ii`` is never taken by gain: once no slot is, the rest of the list is filled by pool score with gain
    0 and flag 512.  ``gain`` is the determinant ratio a slot won with; ``-1`` / ``-inf`` / ``-inf`` once the live slots run out.
    The native header states every rounding.  ``status``: ``DPP_FLAGS``; it stays on the device -- nothing here synchronises with
    the host."""
    checked = [(pool_idx, torch.int64, "pool_idx"), (pool_score, torch.float32, "pool_score"), (table, torch.float32, "table")]
    if quality is not None:
        checked.append((quality, torch.float32, "quality"))
    for t, dt, name in checked:
        if t.dtype != dt:
            raise ValueError(f"newsreclib_amd: `{name}` must be {dt}, got {t.dtype}")
    if pool_idx.dim() != 2 or pool_score.shape != pool_idx.shape or table.dim() != 2:
        raise ValueError(f"newsreclib_amd: pool_idx (B, N), pool_score (B, N) and table (V, D) expected, got {tuple(pool_idx.shape)}, "
                         f"{tuple(pool_score.shape)} and {tuple(table.shape)}")
    if quality is not None and quality.shape != pool_idx.shape:
        raise ValueError(f"newsreclib_amd: quality {tuple(pool_idx.shape)} expected, one entry per pool slot, got {tuple(quality.shape)}")
    if similarity not in MMR_SIMILARITIES:
        raise ValueError(f"newsreclib_amd: similarity is one of {sorted(MMR_SIMILARITIES)}, got {similarity!r}")
    B, N, V, D, k = int(pool_idx.shape[0]), int(pool_idx.shape[1]), int(table.shape[0]), int(table.shape[1]), int(k)
    if N > MMR_MAX_POOL:
        raise NotImplementedError(f"newsreclib_amd: dpp_rerank takes a pool of at most {MMR_MAX_POOL} slots (got {N})")
    if k > DPP_MAX_K:
        raise NotImplementedError(f"newsreclib_amd: dpp_rerank lists at most {DPP_MAX_K} news (got k = {k})")
    if not 1 <= k <= N:
        raise ValueError(f"newsreclib_amd: k in [1, N = {N}] expected, got {k}")
    if not 0.0 <= float(alpha) < float("inf"):
        raise ValueError(f"newsreclib_amd: alpha finite and >= 0 expected, got {alpha}")
    if not 0.0 <= float(eps) < 1.0:
        raise ValueError(f"newsreclib_amd: eps in [0, 1) expected, got {eps}")
    pool_idx, pool_score, table = _chk(pool_idx, torch.int64, "pool_idx"), _chk(pool_score, torch.float32, "pool_score"), \
        _chk(table, torch.float32, "table")
    if quality is not None:
        quality = _chk(quality, torch.float32, "quality")
    lib = _lib.load()
    dev = pool_idx.device
    idx, score, status = _topk_outputs(B, k, dev)
    gain = torch.empty((B, k), dtype=torch.float32, device=dev)
    _lib.check(lib.nrl_dpp_rerank(pool_idx.data_ptr(), pool_score.data_ptr(), quality.data_ptr() if quality is not None else None,
                                  table.data_ptr() if V else None, B, N, V, D, k, float(alpha), float(eps),
                                  MMR_SIMILARITIES[similarity], int(bool(normalize)), idx.data_ptr(), score.data_ptr(), gain.data_ptr(),
                                  status.data_ptr(), _stream()), "nrl_dpp_rerank")
    return idx, score, gain, status


def class_targets(hist_idx: torch.Tensor, hist_off: torch.Tensor, row_class: torch.Tensor, S: int, k: Optional[int] = None):
    """The class targets ``calibrated_rerank`` takes -> (B, S) fp32: the class counts of each user's ragged history (``hist_idx``:
    the concatenated table rows, ``hist_off`` (B + 1) its offsets; ``row_class`` (V) the class of every row).  A history row
    outside the table, or whose class is outside [0, S), counts for nothing.  ``k``: the counts times ``k`` over ``max(1, history
    size)`` -- the history's class proportions as quotas of a list of ``k`` (Steck, 2018) -- instead of the integer counts, which
    make ``calibrated_rerank``'s term the list's Personalization@k.  Torch ops on the tensors' device; nothing is read back."""
    dev = hist_idx.device
    S, V = int(S), int(row_class.numel())
    hist_idx, hist_off, row_class = hist_idx.long(), hist_off.to(dev).long(), row_class.to(dev).long()
    B = int(hist_off.numel()) - 1
    sizes = hist_off[1:] - hist_off[:-1]
    owner = torch.repeat_interleave(torch.arange(B, device=dev), sizes, output_size=int(hist_idx.numel()))
    row_ok = (hist_idx >= 0) & (hist_idx < V)
    cls = row_class[hist_idx.clamp(0, max(V - 1, 0))] if V else torch.full_like(hist_idx, -1)
    ok = row_ok & (cls >= 0) & (cls < S)
    counts = torch.zeros(B * S, dtype=torch.float32, device=dev)
    counts.index_put_((owner * S + torch.where(ok, cls, torch.zeros_like(cls)),), ok.float(), accumulate=True)
    counts = counts.view(B, S)
    if k is not None:
        counts = (counts * float(k)) / sizes.clamp_min(1).float()[:, None]      # (count * k is exact: one rounding per entry)
    return counts


TOPK_MAX_INTERESTS = 64


def _interest_scorer(who: str, interests, table, mode, gate) -> _Scorer:
    from .ops_miner import SCORE_MODES
    interests, table = _chk(interests, torch.float32, "interests"), _chk(table, torch.float32, "table")
    if interests.dim() != 3 or table.dim() != 2 or interests.shape[2] != table.shape[1]:
        raise ValueError(f"newsreclib_amd: interests (B, K, D) and table (V, D) expected, got {tuple(interests.shape)} and "
                         f"{tuple(table.shape)}")
    if mode not in SCORE_MODES:
        raise ValueError(f"newsreclib_amd: mode must be one of {sorted(SCORE_MODES)} (got {mode!r})")
    B, K, D, V = int(interests.shape[0]), int(interests.shape[1]), int(interests.shape[2]), int(table.shape[0])
    if K > TOPK_MAX_INTERESTS:
        raise NotImplementedError(f"newsreclib_amd: {who} takes at most {TOPK_MAX_INTERESTS} interest vectors per user (got {K})")
    if mode == "weighted":
        if gate is None:
            raise ValueError("newsreclib_amd: mode 'weighted' needs `gate` (B, K, D) = gelu(user_vector Wt^T)")
        gate = _chk(gate, torch.float32, "gate")
        if gate.shape != interests.shape:
            raise ValueError(f"newsreclib_amd: gate must have the shape of interests, got {tuple(gate.shape)}")
    else:
        gate = None
    return _Scorer(B, V, D, interests.device, (interests.data_ptr(), _ptr(gate), table.data_ptr(), B, K, V, D), (SCORE_MODES[mode],),
                   (interests, gate, table))


def topk_interest_scores(interests: torch.Tensor, table: torch.Tensor, k: int, mode: str, gate: Optional[torch.Tensor] = None,
                         excl_idx: Optional[torch.Tensor] = None, excl_off: Optional[torch.Tensor] = None,
                         eligible: Optional[torch.Tensor] = None, slices: int = 0):
    """``nrl_topk_interest_scores``: ``topk_scores`` where a user is ``K`` interest vectors -- ``interests`` (B, K, D) -- and a
    table row's score is their aggregate ``mode`` (``ops_miner.SCORE_MODES``): "max" ``max_j s_j``, "mean" ``sum_j s_j / K``,
    "weighted" ``sum_j softmax_j(l)_j s_j`` with ``s_j = interests[u, j] . table[v]`` and ``l_j = gate[u, j] . table[v]``
    (``gate`` (B, K, D) = gelu(user_vector Wt^T), required by "weighted" alone).  -> (idx (B, k) int64, score (B, k) fp32,
    status (1) int32) with the ordering, exclusion, eligibility and status flags of ``topk_scores``; neither the (B, V) nor the
    (B K, V) matrix is materialised.  The workspace is sized by ``nrl_topk_scores_workspace_bytes`` with B in users, which always
    suffices.  Nothing here synchronises with the host."""
    s = _interest_scorer("topk_interest_scores", interests, table, mode, gate)
    return _run_topk("nrl_topk_interest_scores", s, k, excl_idx, excl_off, eligible, slices)


def catalogue_interest_ranks(interests: torch.Tensor, table: torch.Tensor, tgt_idx: torch.Tensor, tgt_off: torch.Tensor, mode: str,
                             gate: Optional[torch.Tensor] = None, excl_idx: Optional[torch.Tensor] = None,
                             excl_off: Optional[torch.Tensor] = None, eligible: Optional[torch.Tensor] = None, slices: int = 0):
    """``nrl_catalogue_interest_ranks``: ``catalogue_ranks`` by the scores of ``topk_interest_scores`` -- ``interests`` (B, K, D),
    ``mode`` "max" / "mean" / "weighted" (``gate`` (B, K, D), required by "weighted" alone) -> (rank int32 (n_tgt), score fp32
    (n_tgt), ranked int32 (B), status (1) int32) with the targets, population, order, masks and flags (``RANK_FLAGS``) of
    ``catalogue_ranks`` and the score bits of ``topk_interest_scores``: ``rank <= k`` exactly when the target is slot ``rank - 1``
    of that call's list.  Neither the (B, V) nor the (B K, V) matrix is materialised; nothing here synchronises with the host."""
    s = _interest_scorer("catalogue_interest_ranks", interests, table, mode, gate)
    return _run_ranks("nrl_catalogue_interest_ranks", s, tgt_idx, tgt_off, excl_idx, excl_off, eligible, slices)


TOPK_MAX_MODELS, TOPK_STAT_CHUNKS = 3, 64


def _ensemble_scorer(users, tables, weights):
    """-> the scorer and the two outputs of its own: stats (B, T, 2) and the moments scratch."""
    users, tables = list(users), list(tables)
    T = len(tables)
    if not 1 <= T <= TOPK_MAX_MODELS or len(users) != T or len(weights) != T:
        raise ValueError(f"newsreclib_amd: 1 to {TOPK_MAX_MODELS} sub-models with one user matrix, one table and one weight each "
                         f"(got {len(users)}, {T} and {len(weights)})")
    if users[0].dim() != 2 or tables[0].dim() != 2 or users[0].shape[1] != tables[0].shape[1] or \
            any(u.shape != users[0].shape for u in users) or any(t.shape != tables[0].shape for t in tables):
        raise ValueError(f"newsreclib_amd: users (B, D) and tables (V, D) of one shape each expected, got "
                         f"{[tuple(u.shape) for u in users]} and {[tuple(t.shape) for t in tables]}")
    users = [_chk(u, torch.float32, "users") for u in users]
    tables = [_chk(t, torch.float32, "tables") for t in tables]
    B, D, V, dev = int(users[0].shape[0]), int(users[0].shape[1]), int(tables[0].shape[0]), users[0].device
    uptr = (ctypes.c_void_p * T)(*[u.data_ptr() for u in users])
    tptr = (ctypes.c_void_p * T)(*[t.data_ptr() for t in tables])
    wts = (ctypes.c_float * T)(*[float(w) for w in weights])
    stats = torch.empty((B, T, 2), dtype=torch.float32, device=dev)
    moments = torch.empty((B, TOPK_STAT_CHUNKS, T, 3), dtype=torch.float32, device=dev)
    return _Scorer(B, V, D, dev, (uptr, tptr, wts, T, B, V, D), (), (users, tables)), stats, moments


def topk_ensemble_scores(users: Sequence[torch.Tensor], tables: Sequence[torch.Tensor], weights: Sequence[float], k: int,
                         excl_idx: Optional[torch.Tensor] = None, excl_off: Optional[torch.Tensor] = None,
                         eligible: Optional[torch.Tensor] = None, slices: int = 0):
    """``nrl_topk_ensemble_scores``: ``topk_scores`` by MANNeR's ensemble of standardised scores.  ``users[t]`` (B, D),
    ``tables[t]`` (V, D) and ``weights[t]`` for T in {1, 2, 3} sub-models; the score of a table row is
    ``sum_t weights[t] * (s_t - mu_t) / sd_t`` with ``s_t = users[t][u] . tables[t][v]`` and ``mu_t`` / ``sd_t`` the mean and the
    unbiased standard deviation of ``s_t`` over the user's population: the eligible rows that are not on its exclusion list.
    -> (idx (B, k) int64, score (B, k) fp32, status (1) int32, stats (B, T, 2) fp32: mean, sd) with the ordering, exclusion,
    eligibility and status flags of ``topk_scores`` and one flag more (``TOPK_FLAGS[8]``): a user whose scores cannot be
    standardised gets ``-1`` / ``-inf``.  No (B, V) matrix is materialised; nothing here synchronises with the host."""
    s, stats, moments = _ensemble_scorer(users, tables, weights)
    return (*_run_topk("nrl_topk_ensemble_scores", s, k, excl_idx, excl_off, eligible, slices, extra=(stats, moments)), stats)


def topk_ensemble_scores_capped(users: Sequence[torch.Tensor], tables: Sequence[torch.Tensor], weights: Sequence[float], k: int,
                                row_class: torch.Tensor, max_per_class: int, excl_idx: Optional[torch.Tensor] = None,
                                excl_off: Optional[torch.Tensor] = None, eligible: Optional[torch.Tensor] = None, slices: int = 0):
    """``nrl_topk_ensemble_scores_capped``: ``topk_ensemble_scores`` with at most ``max_per_class`` rows of any one class of
    ``row_class`` in a user's list, as ``topk_scores_capped`` caps ``topk_scores``.  The statistics do not know the cap: they are
    those of ``topk_ensemble_scores``, bit for bit, and so is every returned score.  -> (idx, score, status, stats) as there."""
    s, stats, moments = _ensemble_scorer(users, tables, weights)
    s = _capped(s, row_class, max_per_class)
    return (*_run_topk("nrl_topk_ensemble_scores_capped", s, k, excl_idx, excl_off, eligible, slices, extra=(stats, moments)), stats)


# the status word of ``catalogue_ensemble_ranks``: the flags of ``catalogue_ranks`` and, worded for ranks, the one of the ensemble
ENSEMBLE_RANK_FLAGS = {**RANK_FLAGS,
                       8: "a user's scores of some table cannot be standardised: zero, non-finite or undefined standard deviation "
                          "(that user's ranks and population are 0)"}


def catalogue_ensemble_ranks(users: Sequence[torch.Tensor], tables: Sequence[torch.Tensor], weights: Sequence[float],
                             tgt_idx: torch.Tensor, tgt_off: torch.Tensor, excl_idx: Optional[torch.Tensor] = None,
                             excl_off: Optional[torch.Tensor] = None, eligible: Optional[torch.Tensor] = None, slices: int = 0):
    """``nrl_catalogue_ensemble_ranks``: ``catalogue_ranks`` by the scores of ``topk_ensemble_scores`` -- ``users[t]`` (B, D),
    ``tables[t]`` (V, D) and ``weights[t]`` for T in {1, 2, 3} sub-models -> (rank int32 (n_tgt), score fp32 (n_tgt), ranked int32
    (B), status (1) int32, stats (B, T, 2) fp32: mean, sd) with the targets, population, order and masks of ``catalogue_ranks`` and
    the statistics and score bits of ``topk_ensemble_scores``: ``rank <= k`` exactly when the target is slot ``rank - 1`` of that
    call's list.  ``status`` (``ENSEMBLE_RANK_FLAGS``): the flags of ``catalogue_ranks`` and one more -- a user whose scores cannot
    be standardised has ranks 0, scores ``-inf`` and ``ranked`` 0.  No (B, V) matrix is materialised; nothing here synchronises
    with the host."""
    s, stats, moments = _ensemble_scorer(users, tables, weights)
    return (*_run_ranks("nrl_catalogue_ensemble_ranks", s, tgt_idx, tgt_off, excl_idx, excl_off, eligible, slices,
                        extra=(stats, moments), ws_lead=(stats.shape[1],)), stats)


TOPK_MAX_HIDDEN = 64


def _relu_scorer(who: str, q, proj, w2, b2) -> _Scorer:
    """(D = 4 sizes the workspace: the partial lists and the counts do not depend on it, and nothing is gathered)"""
    if q.dim() != 2 or proj.dim() != 2 or q.shape[1] != proj.shape[1] or w2.numel() != q.shape[1] or b2.numel() != 1:
        raise ValueError(f"newsreclib_amd: q (B, Hd), proj (V, Hd), w2 (Hd) and b2 (1) expected, got {tuple(q.shape)}, "
                         f"{tuple(proj.shape)}, {tuple(w2.shape)} and {tuple(b2.shape)}")
    q, proj = _chk(q, torch.float32, "q"), _chk(proj, torch.float32, "proj")
    w2, b2 = _chk(w2, torch.float32, "w2"), _chk(b2, torch.float32, "b2")
    B, Hd, V = int(q.shape[0]), int(q.shape[1]), int(proj.shape[0])
    if not 1 <= Hd <= TOPK_MAX_HIDDEN:
        raise NotImplementedError(f"newsreclib_amd: {who} takes a hidden width in [1, {TOPK_MAX_HIDDEN}] (got {Hd})")
    return _Scorer(B, V, 4, q.device, (q.data_ptr(), proj.data_ptr(), w2.data_ptr(), b2.data_ptr(), B, V, Hd), (), (q, proj, w2, b2))


def topk_relu_scores(q: torch.Tensor, proj: torch.Tensor, w2: torch.Tensor, b2: torch.Tensor, k: int,
                     excl_idx: Optional[torch.Tensor] = None, excl_off: Optional[torch.Tensor] = None,
                     eligible: Optional[torch.Tensor] = None, slices: int = 0):
    """``nrl_topk_relu_scores``: ``topk_scores`` by DKN's DNN click predictor with its first layer split by columns: the score of
    table row ``v`` for user ``u`` is ``b2 + sum_j w2[j] * relu(proj[v, j] + q[u, j])`` with ``q`` (B, Hd) the user's share and the
    bias (``ops_dkn.dkn_user_query``) and ``proj`` (V, Hd) the table's (``ops_dkn.dkn_cand_project``); ``w2`` (Hd values) and
    ``b2`` (one value) are the second layer's parameters, on the device.  Hd in [1, 64].  -> (idx (B, k) int64, score (B, k)
    fp32, status (1) int32) with the ordering, exclusion, eligibility and status flags of ``topk_scores``; neither the (B, V) nor
    the (B, V, Hd) array is materialised.  The workspace is sized by ``nrl_topk_scores_workspace_bytes(B, V, 4, k, slices)``: the
    partial lists are those of ``topk_scores``, whose size does not depend on D.  Nothing here synchronises with the host."""
    s = _relu_scorer("topk_relu_scores", q, proj, w2, b2)
    return _run_topk("nrl_topk_relu_scores", s, k, excl_idx, excl_off, eligible, slices)


def catalogue_relu_ranks(q: torch.Tensor, proj: torch.Tensor, w2: torch.Tensor, b2: torch.Tensor, tgt_idx: torch.Tensor,
                         tgt_off: torch.Tensor, excl_idx: Optional[torch.Tensor] = None, excl_off: Optional[torch.Tensor] = None,
                         eligible: Optional[torch.Tensor] = None, slices: int = 0):
    """``nrl_catalogue_relu_ranks``: ``catalogue_ranks`` by the scores of ``topk_relu_scores`` -- ``q`` (B, Hd), ``proj`` (V, Hd),
    ``w2`` (Hd values), ``b2`` (one value), Hd in [1, 64] -> (rank int32 (n_tgt), score fp32 (n_tgt), ranked int32 (B), status (1)
    int32) with the targets, population, order, masks and flags (``RANK_FLAGS``) of ``catalogue_ranks`` and the score bits of
    ``topk_relu_scores``: ``rank <= k`` exactly when the target is slot ``rank - 1`` of that call's list.  Neither the (B, V) nor
    the (B, V, Hd) array is materialised; nothing here synchronises with the host."""
    s = _relu_scorer("catalogue_relu_ranks", q, proj, w2, b2)
    return _run_ranks("nrl_catalogue_relu_ranks", s, tgt_idx, tgt_off, excl_idx, excl_off, eligible, slices)


TOPK_MAX_TOKENS = 128


def _pooled_scorer(who: str, q, user, features) -> _Scorer:
    """(D = 4 sizes the workspace, as for ``_relu_scorer``: the targets' feature maps are read in place)"""
    if q.dim() != 2 or features.dim() != 3 or user.shape != q.shape or q.shape[1] != features.shape[2]:
        raise ValueError(f"newsreclib_amd: q (B, F), user (B, F) and features (V, L, F) expected, got {tuple(q.shape)}, "
                         f"{tuple(user.shape)} and {tuple(features.shape)}")
    q, user, features = _chk(q, torch.float32, "q"), _chk(user, torch.float32, "user"), _chk(features, torch.float32, "features")
    B, F_, V, L = int(q.shape[0]), int(q.shape[1]), int(features.shape[0]), int(features.shape[1])
    if not 1 <= L <= TOPK_MAX_TOKENS:
        raise NotImplementedError(f"newsreclib_amd: {who} takes feature maps of 1 to {TOPK_MAX_TOKENS} tokens (got {L})")
    return _Scorer(B, V, 4, q.device, (q.data_ptr(), user.data_ptr(), features.data_ptr(), B, V, L, F_), (), (q, user, features))


def topk_pooled_scores(q: torch.Tensor, user: torch.Tensor, features: torch.Tensor, k: int,
                       excl_idx: Optional[torch.Tensor] = None, excl_off: Optional[torch.Tensor] = None,
                       eligible: Optional[torch.Tensor] = None, slices: int = 0):
    """``nrl_topk_pooled_scores``: ``topk_scores`` by NPA's eval-mode score from the cached conv feature maps ``features``
    (V, L, F) (``ops_npa.npa_conv_features``): the score of table row ``v`` for user ``u`` is
    ``sum_t softmax_t(features[v] @ q[u])[t] * (features[v] @ user[u])[t]`` -- the user vector ``user`` (B, F) dotted with the news
    vector pooled by the user's own text query ``q`` (B, F), the softmax over all L tokens.  L in [1, 128], F a multiple of 4 up to
    1024.  -> (idx (B, k) int64, score (B, k) fp32, status (1) int32) with the ordering, exclusion, eligibility and status flags of
    ``topk_scores``; neither a (B, V, L) nor the (B, V, F) array is materialised.  The workspace is sized by
    ``nrl_topk_scores_workspace_bytes(B, V, 4, k, slices)``: the partial lists are those of ``topk_scores``.  Nothing here
    synchronises with the host."""
    s = _pooled_scorer("topk_pooled_scores", q, user, features)
    return _run_topk("nrl_topk_pooled_scores", s, k, excl_idx, excl_off, eligible, slices)


def catalogue_pooled_ranks(q: torch.Tensor, user: torch.Tensor, features: torch.Tensor, tgt_idx: torch.Tensor, tgt_off: torch.Tensor,
                           excl_idx: Optional[torch.Tensor] = None, excl_off: Optional[torch.Tensor] = None,
                           eligible: Optional[torch.Tensor] = None, slices: int = 0):
    """``nrl_catalogue_pooled_ranks``: ``catalogue_ranks`` by the scores of ``topk_pooled_scores`` -- ``q`` (B, F), ``user`` (B, F),
    ``features`` (V, L, F), L in [1, 128], F a multiple of 4 up to 1024 -> (rank int32 (n_tgt), score fp32 (n_tgt), ranked int32
    (B), status (1) int32) with the targets, population, order, masks and flags (``RANK_FLAGS``) of ``catalogue_ranks`` and the
    score bits of ``topk_pooled_scores``: ``rank <= k`` exactly when the target is slot ``rank - 1`` of that call's list.  The
    targets' feature maps are read in place: no (B, V), (B, V, L) or (n_tgt, L, F) array is materialised; nothing here
    synchronises with the host."""
    s = _pooled_scorer("catalogue_pooled_ranks", q, user, features)
    return _run_ranks("nrl_catalogue_pooled_ranks", s, tgt_idx, tgt_off, excl_idx, excl_off, eligible, slices)
