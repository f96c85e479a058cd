"""MINER's poly-attention user encoder and target-aware scorer (reference layers/attention.py:45-166) on HIP kernels.  The
modules hold the parameters under the reference's keys (``linear.weight``, ``context_codes``); ``forward`` runs them through
``ops_miner`` over FLAT history / candidate rows (see ``ops_miner.PolyFn``).

Both ``nn.Linear`` layers are bias-free.  Their GEMMs run on the library's engines through the existing entries with a zero
bias vector passed in (one code path for those entries); their weight gradients are fixed-order two-pass reductions
(``ops_miner.BiasFreeLinearFn``)."""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn as nn

from . import ops_miner


class PolyAttention(nn.Module):
    def __init__(self, input_dim: int, num_context_codes: int, context_code_dim: int) -> None:
        super().__init__()
        if not isinstance(input_dim, int):
            raise ValueError(f"Expected keyword argument `input_dim` to be an `int` but got {input_dim}")
        if not isinstance(num_context_codes, int):
            raise ValueError(f"Expected keyword argument `num_context_codes` to be an `int` but got {num_context_codes}")
        if not isinstance(context_code_dim, int):
            raise ValueError(f"Expected keyword argument `context_code_dim` to be an `int` but got {context_code_dim}")
        if input_dim % 4 or context_code_dim % 4:
            raise NotImplementedError("the MINER kernels take input_dim and context_code_dim as multiples of 4 "
                                      f"(got {input_dim}, {context_code_dim})")
        if num_context_codes > 255:
            raise NotImplementedError(f"the MINER kernels take at most 255 context codes (got {num_context_codes})")
        self.linear = nn.Linear(in_features=input_dim, out_features=context_code_dim, bias=False)
        self.context_codes = nn.Parameter(nn.init.xavier_uniform_(torch.empty(num_context_codes, context_code_dim),
                                                                  gain=nn.init.calculate_gain("tanh")))

    def forward(self, embeddings: torch.Tensor, hist_offsets: torch.Tensor, batch_size: int, max_hist: int,
                bias: Optional[torch.Tensor] = None) -> torch.Tensor:
        """embeddings (n_hist, D) flat history rows, hist_offsets (B + 1), bias (n_hist) per-row category bias (already the
        mean over the candidate axis) -> (B, K, D).  ``max_hist``: the dense history length of the reference's batch; the
        ``max_hist - n_b`` padded positions of a user dilute its weights (1e-30 fill)."""
        w = self.linear.weight
        proj = ops_miner.BiasFreeLinearFn.apply(embeddings, w, "tanh")
        return ops_miner.PolyFn.apply(embeddings, proj, self.context_codes, bias, hist_offsets, batch_size, max_hist)


UserEncoder = PolyAttention


class TargetAwareAttention(nn.Module):
    def __init__(self, input_dim: int) -> None:
        super().__init__()
        if not isinstance(input_dim, int):
            raise ValueError(f"Expected keyword argument `input_dim` to be an `int` but got {input_dim}")
        self.linear = nn.Linear(in_features=input_dim, out_features=input_dim, bias=False)

    def forward(self, query: torch.Tensor, key: torch.Tensor, cand_offsets: torch.Tensor, max_cand: int) -> torch.Tensor:
        """query (B, K, D) the user's interest vectors, key (n_cand, D) flat candidate rows -> scores (B, max_cand); the
        ``value`` of the reference (key . query) is formed inside the kernel."""
        B, K, D = query.shape
        w = self.linear.weight
        z = ops_miner.BiasFreeLinearFn.apply(query.reshape(B * K, D), w, None).view(B, K, D)
        return ops_miner.ScoreFn.apply(key, query, z, cand_offsets, B, max_cand, "weighted")
