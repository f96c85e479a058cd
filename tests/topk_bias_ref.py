"""What the host and the GPU tests of the class-biased full-catalogue top-k and rank (``nrl_topk_bias_scores`` /
``nrl_topk_bias_scores_capped`` / ``nrl_catalogue_bias_ranks``) share, on the CPU in float64.

* ``scores``: ``U T^T + bias[u, row_class[v]]`` in float64; a class id outside [0, S) adds 0 and is reported (flag 64).

Population, order, ranks and the capped walk are those of ``tests/catalogue_ref.py`` and ``tests/topk_capped_ref.py``; the inputs
stay numpy (the generators of the tests are numpy's) and ``scores`` hands torch over.
"""
import numpy as np
import torch

E_CLASS = 64


def scores(U, T, bias, row_class):
    """-> ((B, V) float64 tensor, flags): the class ids outside [0, S) add 0 and set E_CLASS"""
    U, T, bias = np.asarray(U, dtype=np.float64), np.asarray(T, dtype=np.float64), np.asarray(bias, dtype=np.float64)
    cls = np.asarray(row_class, dtype=np.int64)
    S = bias.shape[1]
    ok = (cls >= 0) & (cls < S)
    add = np.where(ok[None, :], bias[:, np.where(ok, cls, 0)], 0.0)
    with np.errstate(invalid="ignore"):
        return torch.from_numpy(U @ T.T + add), (E_CLASS if (~ok).any() else 0)
