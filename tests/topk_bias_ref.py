"""What the host and the GPU tests of the class-biased full-catalogue top-k and rank (``nrl_topk_bias_scores`` /
``nrl_topk_bias_scores_capped`` / ``nrl_catalogue_bias_ranks``) share: a float64 / numpy restatement, all on the CPU.

* ``scores``: ``U T^T + bias[u, row_class[v]]`` in float64; a class id outside [0, S) adds 0 and is reported (flag 64).
* ``population``: which (user, row) pairs may be returned or counted: inside V, eligible, not on the user's exclusion list
  (entries outside [0, V) are ignored), score not NaN (reported: flag 4).
* ``topk``: the strict total order -- score descending, equal scores by ascending row, ``-0.0 == 0.0`` -- cut at ``k``; ``-1`` /
  ``-inf`` where the population runs out.
* ``ranks``: per target 1 + the number of rows of the population ordered above it, 0 (score ``-inf``) when the target is not
  itself in the population; and the population's size.
* ``capped``: the greedy walk of ``tests/topk_capped_ref.py`` over the same order.
"""
import numpy as np
import torch

from tests import topk_capped_ref

E_NAN, E_CLASS = 4, 64


def scores(U, T, bias, row_class):
    """-> ((B, V) float64, flags): the class ids outside [0, S) add 0 and set E_CLASS"""
    U, T, bias = np.asarray(U, dtype=np.float64), np.asarray(T, dtype=np.float64), np.asarray(bias, dtype=np.float64)
    cls = np.asarray(row_class, dtype=np.int64)
    S = bias.shape[1]
    ok = (cls >= 0) & (cls < S)
    add = np.where(ok[None, :], bias[:, np.where(ok, cls, 0)], 0.0)
    with np.errstate(invalid="ignore"):
        return U @ T.T + add, (E_CLASS if (~ok).any() else 0)


def population(s, excl=None, eligible=None):
    """-> ((B, V) bool, flags): E_NAN where a NaN score was dropped from an otherwise returnable position"""
    B, V = s.shape
    pop = np.ones((B, V), dtype=bool)
    if eligible is not None:
        pop &= np.asarray(eligible).astype(bool)[None, :]
    if excl is not None:
        for b, rows in enumerate(excl):
            for r in rows:
                if 0 <= r < V:
                    pop[b, r] = False
    nan = np.isnan(s) & pop
    return pop & ~nan, (E_NAN if nan.any() else 0)


def _order(s, pop):
    """per user the population's rows, best first"""
    key = np.where(pop, -s, np.inf)
    order = np.argsort(key, axis=1, kind="stable")             # (-0.0 == 0.0: the stable sort leaves such rows in ascending order)
    return order, pop.sum(1)


def topk(s, pop, k):
    """-> idx (B, k) int64, score (B, k) float32"""
    B, V = s.shape
    idx = np.full((B, k), -1, dtype=np.int64)
    score = np.full((B, k), -np.inf, dtype=np.float32)
    order, n = _order(s, pop)
    for b in range(B):
        m = min(k, int(n[b]))
        idx[b, :m] = order[b, :m]
        score[b, :m] = s[b, order[b, :m]].astype(np.float32) + np.float32(0.0)      # (-0 is returned as +0)
    return idx, score


def ranks(s, pop, targets):
    """``targets``: per user a list of rows -> rank (n) int32, score (n) float32, ranked (B) int32, in the users' order"""
    B, V = s.shape
    rank, score = [], []
    for b, rows in enumerate(targets):
        for r in rows:
            if not (0 <= r < V) or not pop[b, r]:
                rank.append(0)
                score.append(-np.inf)
                continue
            x = s[b, r]
            above = pop[b] & ((s[b] > x) | ((s[b] == x) & (np.arange(V) < r)))
            rank.append(1 + int(above.sum()))
            score.append(np.float32(x) + np.float32(0.0))
    return np.asarray(rank, dtype=np.int32), np.asarray(score, dtype=np.float32), pop.sum(1).astype(np.int32)


def capped(s, pop, cap_class, k, m):
    """the greedy walk of ``topk_capped_ref.reference`` -> idx (B, k) int64, score (B, k) float32 (numpy)"""
    masked = torch.from_numpy(np.where(pop, s, -np.inf))
    idx, score = topk_capped_ref.reference(masked, torch.as_tensor(np.asarray(cap_class)), k, m)
    return idx.numpy(), (score + 0.0).numpy()
