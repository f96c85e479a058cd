"""DKN user encoder (reference user/dkn.py:10-107): candidate-aware attention over the clicked news, ``dnn = Linear(2 dim,
hidden) -> Linear(hidden, 1)`` on ``[cand, hist]``.  The module holds the parameters under the reference's keys; the
computation runs fused with the click predictor in ``ops_dkn.DknClickFn`` (see ``dkn_module.DKNModule.forward``)."""
from __future__ import annotations

import torch.nn as nn


class UserEncoder(nn.Module):
    def __init__(self, input_dim: int, hidden_dim: int) -> None:
        super().__init__()
        if not isinstance(input_dim, int):
            raise ValueError(f"Expected keyword argument `input_dim` to be an `int` but got {input_dim}")
        if not isinstance(hidden_dim, int):
            raise ValueError(f"Expected keyword argument `hidden_dim` to be an `int` but got {hidden_dim}")
        self.dnn = nn.Sequential(nn.Linear(in_features=input_dim * 2, out_features=hidden_dim),
                                 nn.Linear(in_features=hidden_dim, out_features=1))

    def params(self):
        """(w1, b1, w2, b2) as the kernels read them."""
        return self.dnn[0].weight, self.dnn[0].bias, self.dnn[1].weight, self.dnn[1].bias
