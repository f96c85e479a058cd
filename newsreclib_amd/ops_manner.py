"""``torch.autograd.Function`` wrappers of the MANNeR entry points (``nrl_manner.hip``, ``nrl_manner_zscores.hip``).  Same
conventions as ``ops.py``: GPU tensors only, no eager fallback, nothing synchronises with the host.

``SupConEmbedFn`` / ``SupConEmbedLoss``  the A-Module loss (manner_a_module.py:151-153): pytorch-metric-learning's ``SupConLoss``
    over ``DotProductSimilarity(normalize_embeddings=False)`` of a batch of embeddings with integer labels; loss and gradient come
    from one call, the backward scales the saved gradient.
``manner_scores``                        the ensemble scorer (manner_module.py:152-204) over up to three cached news-vector tables.
``manner_zscores``                       its per-table z-scores, flat and uncombined: the components of a weight grid (``ops.grid_metrics``).
"""
from __future__ import annotations

import ctypes
from typing import Optional, Sequence

import torch

from . import _lib, ops
from .ops import GradAwareFunction, _chk, _stream

MAX_ANCHORS = 1024
MAX_DIM = 1024
MAX_CAND = 2048
MAX_TABLES = 3


def supcon_embed_fwd_bwd(embeddings: torch.Tensor, labels: torch.Tensor, temperature: float, grad_scale: float = 1.0):
    """-> (loss (), d_embeddings (N, D)) of ``nrl_supcon_embed_fwd_bwd``."""
    lib = _lib.load()
    E = _chk(embeddings, torch.float32, "embeddings")
    labels = _chk(labels, torch.int64, "labels")
    if E.dim() != 2 or labels.shape != (E.shape[0],):
        raise ValueError("newsreclib_amd: embeddings (N, D) and labels (N) expected")
    N, D = E.shape
    if not 1 <= N <= MAX_ANCHORS or D % 4 or not 4 <= D <= MAX_DIM:
        raise ValueError(f"newsreclib_amd: the embedding SupCon kernel takes 1 <= N <= {MAX_ANCHORS} rows of a width that is a "
                         f"multiple of 4 up to {MAX_DIM}; got ({N}, {D})")
    loss = torch.empty((), dtype=torch.float32, device=E.device)
    d_E = torch.empty_like(E)
    ws = ops.workspace(lib.nrl_supcon_embed_workspace_bytes(N, D), E.device)
    _lib.check(lib.nrl_supcon_embed_fwd_bwd(E.data_ptr(), labels.data_ptr(), N, D, float(temperature), float(grad_scale),
                                            loss.data_ptr(), d_E.data_ptr(), ws.data_ptr(), ws.numel(), _stream()),
               "nrl_supcon_embed_fwd_bwd")
    return loss, d_E


class SupConEmbedFn(GradAwareFunction):
    """embeddings (N, D), labels (N) int64 -> scalar loss."""

    @staticmethod
    def forward(ctx, embeddings, labels, temperature):
        loss, d_E = supcon_embed_fwd_bwd(embeddings, labels, temperature)
        ctx.save_for_backward(d_E)
        return loss

    @staticmethod
    def backward(ctx, g):
        (d_E,) = ctx.saved_tensors
        return d_E * g, None, None


class SupConEmbedLoss(torch.nn.Module):
    """``SupConLoss(temperature=..., distance=DotProductSimilarity(normalize_embeddings=False))(embeddings, labels)``."""

    def __init__(self, temperature: float) -> None:
        super().__init__()
        self.temperature = float(temperature)

    def forward(self, embeddings: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
        return SupConEmbedFn.apply(embeddings, labels, self.temperature)


def manner_scores(tables: Sequence[torch.Tensor], weights: Sequence[float], hist_idx: torch.Tensor, hist_offsets: torch.Tensor,
                  cand_idx: torch.Tensor, cand_offsets: torch.Tensor, max_cand: int,
                  out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(B, max_cand) ensemble scores ``sum_t weights[t] * zscore(mean(tables[t][hist]) . tables[t][cand])``; 0 at padded slots.
    ``max_cand`` must be the largest candidate count (a plain int: the caller knows it from how it built the batch)."""
    lib = _lib.load()
    k = len(tables)
    if not 1 <= k <= MAX_TABLES or len(weights) != k:
        raise ValueError(f"newsreclib_amd: 1 to {MAX_TABLES} news-vector tables with one weight each")
    tables = [_chk(t, torch.float32, "news-vector table") for t in tables]
    V, D = tables[0].shape
    if any(t.shape != (V, D) for t in tables) or D % 4 or not 4 <= D <= MAX_DIM:
        raise ValueError(f"newsreclib_amd: the tables must share one (V, D) shape with D a multiple of 4 up to {MAX_DIM}")
    hist_idx, cand_idx = _chk(hist_idx, torch.int64, "hist_idx"), _chk(cand_idx, torch.int64, "cand_idx")
    hist_offsets, cand_offsets = _chk(hist_offsets, torch.int64, "hist_offsets"), _chk(cand_offsets, torch.int64, "cand_offsets")
    B = int(hist_offsets.numel()) - 1
    if B < 0 or cand_offsets.numel() != B + 1 or not 1 <= int(max_cand) <= MAX_CAND:
        raise ValueError(f"newsreclib_amd: offsets of B + 1 entries each and 1 <= max_cand <= {MAX_CAND}")
    if out is None:
        out = torch.empty((B, int(max_cand)), dtype=torch.float32, device=tables[0].device)
    ptrs = (ctypes.c_void_p * k)(*[t.data_ptr() for t in tables])
    wts = (ctypes.c_float * k)(*[float(w) for w in weights])
    _lib.check(lib.nrl_manner_scores(ptrs, wts, k, V, hist_idx.data_ptr(), hist_offsets.data_ptr(), cand_idx.data_ptr(),
                                     cand_offsets.data_ptr(), B, int(max_cand), D, out.data_ptr(), _stream()), "nrl_manner_scores")
    return out


def manner_zscores(tables: Sequence[torch.Tensor], hist_idx: torch.Tensor, hist_offsets: torch.Tensor, cand_idx: torch.Tensor,
                   cand_offsets: torch.Tensor, max_cand: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(T, N) per-table z-scores ``zscore(mean(tables[t][hist]) . tables[t][cand])``, flat and ragged in ``cand_offsets`` order
    (N = ``cand_idx.numel()``): what ``manner_scores`` combines, written out instead -- row t has the bits of ``manner_scores``
    with table t alone and weight 1.  The components ``ops.grid_metrics`` evaluates a grid of weight rows over.  ``max_cand`` as
    in ``manner_scores``; a fresh ``out`` starts at zero (candidates beyond ``max_cand`` are not written)."""
    lib = _lib.load()
    k = len(tables)
    if not 1 <= k <= MAX_TABLES:
        raise ValueError(f"newsreclib_amd: 1 to {MAX_TABLES} news-vector tables")
    tables = [_chk(t, torch.float32, "news-vector table") for t in tables]
    V, D = tables[0].shape
    if any(t.shape != (V, D) for t in tables) or D % 4 or not 4 <= D <= MAX_DIM:
        raise ValueError(f"newsreclib_amd: the tables must share one (V, D) shape with D a multiple of 4 up to {MAX_DIM}")
    hist_idx, cand_idx = _chk(hist_idx, torch.int64, "hist_idx"), _chk(cand_idx, torch.int64, "cand_idx")
    hist_offsets, cand_offsets = _chk(hist_offsets, torch.int64, "hist_offsets"), _chk(cand_offsets, torch.int64, "cand_offsets")
    B, N = int(hist_offsets.numel()) - 1, int(cand_idx.numel())
    if B < 0 or cand_offsets.numel() != B + 1 or not 1 <= int(max_cand) <= MAX_CAND:
        raise ValueError(f"newsreclib_amd: offsets of B + 1 entries each and 1 <= max_cand <= {MAX_CAND}")
    if out is None:
        out = torch.zeros((k, N), dtype=torch.float32, device=tables[0].device)
    elif _chk(out, torch.float32, "out").shape != (k, N):
        raise ValueError(f"newsreclib_amd: out must be ({k}, {N})")
    ptrs = (ctypes.c_void_p * k)(*[t.data_ptr() for t in tables])
    _lib.check(lib.nrl_manner_zscores(ptrs, k, V, hist_idx.data_ptr(), hist_offsets.data_ptr(), cand_idx.data_ptr(),
                                      cand_offsets.data_ptr(), N, B, int(max_cand), D, out.data_ptr(), _stream()), "nrl_manner_zscores")
    return out
