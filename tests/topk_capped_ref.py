"""What the host and the GPU tests of the class-capped top-k (``nrl_topk_scores_capped`` / ``nrl_topk_ensemble_scores_capped``)
share, all on the CPU:

* ``greedy``: the DEFINITION.  A user's rows that may be returned (score not ``None``), in the family's strict total order --
  score descending, equal scores by ascending row (``-0.0 == 0.0`` in Python as in the kernel's key) -- are walked from the
  best down and a row is taken iff fewer than ``m`` rows of its class have been taken; the walk stops at ``k``.
* ``CapList``: a restatement of the kernel's list (``TkCapList`` in ``nrl_topk.hip``): 64 positions with a class tag each, the
  threshold against position ``k - 1``, the count ``g`` of better entries of the candidate's class, the eviction of the class's
  worst entry at ``w`` (63 when the class is not full) and the one lane-select that shifts the positions ``pos .. w``.
  Positions from ``k`` on hold what fell off and are masked out of every count.
* ``stream`` / ``merge``: a list fed in any order, and the slices' first ``k`` positions fed into a fresh list.
* ``reference``: ``greedy`` over a (B, V) float64 score matrix and its population, in the order of ``tests/catalogue_ref.py``,
  as (idx (B, k) int64, score (B, k) float32) with ``-1`` / ``-inf`` where the walk runs out.
"""
import torch

from tests import catalogue_ref as C

LANES = 64


def _better(a, b):
    """entry a = (score, row) ranks above entry b"""
    return a[0] > b[0] or (a[0] == b[0] and a[1] < b[1])


def greedy(scores, classes, k, m):
    """rows taken, best first; ``scores[v]`` None: row v may not be returned"""
    order = sorted((v for v in range(len(scores)) if scores[v] is not None), key=lambda v: (-scores[v], v))
    taken, out = {}, []
    for v in order:
        if len(out) == k:
            break
        c = classes[v]
        if taken.get(c, 0) < m:
            taken[c] = taken.get(c, 0) + 1
            out.append(v)
    return out


class CapList:
    def __init__(self, k, m):
        assert 1 <= k <= LANES and m >= 1
        self.k, self.m = k, m
        self.e = [None] * LANES                 # (score, row) or None = the empty slot (entry 0: below everything)
        self.tag = [0] * LANES

    def offer(self, score, row, cls):
        x, k, m = (score, row), self.k, self.m
        kth = self.e[k - 1]
        if kth is not None and not _better(x, kth):             # the threshold pruning
            return False
        g = [e is not None and _better(e, x) for e in self.e]
        same = [p < k and self.e[p] is not None and self.tag[p] == cls for p in range(LANES)]
        if sum(1 for p in range(LANES) if same[p] and g[p]) >= m:
            return False
        pos = sum(g)
        held = [p for p in range(LANES) if same[p]]
        w = held[-1] if len(held) >= m else LANES - 1
        assert pos <= w
        old_e, old_t = list(self.e), list(self.tag)
        for p in range(LANES):                  # the lane-select
            if p < pos or p > w:
                continue
            self.e[p], self.tag[p] = (x, cls) if p == pos else (old_e[p - 1], old_t[p - 1])
        return True

    def rows(self):
        return [e[1] for e in self.e[:self.k] if e is not None]


def stream(scores, classes, k, m, order):
    """the list after the rows ``order`` (those that may be returned) have streamed past it"""
    L = CapList(k, m)
    for v in order:
        if scores[v] is not None:
            L.offer(scores[v], v, classes[v])
    return L


def merge(lists, scores, classes, k, m):
    """the slices' lists (their first k positions, tags re-read from ``classes``) merged by the same insertion"""
    out = CapList(k, m)
    for L in lists:
        for v in L.rows():
            out.offer(scores[v], v, classes[v])
    return out


def reference(s, pop, row_class, k, m):
    """``greedy`` over s (B, V) float64 and the population ``pop`` -> idx (B, k) int64, score (B, k) float32"""
    return walk_listed(*C.topk(s, pop, s.shape[1]), row_class, k, m)[:2]


def walk_listed(idx, score, row_class, k, m):
    """``greedy`` over lists that are already in the family's order (an uncapped top-k' result, k' >= k: idx (B, k'), -1 = empty)
    -> idx (B, k), score (B, k), and whether every user's walk was DECIDED inside its list: it reached k rows, or the list had
    empty slots left (so it holds the user's whole population)."""
    B, kk = idx.shape
    out_idx = torch.full((B, k), -1, dtype=torch.int64)
    out_score = torch.full((B, k), float("-inf"), dtype=torch.float32)
    cls = [int(c) for c in row_class.tolist()]
    decided = True
    for b in range(B):
        taken, n = {}, 0
        rows = idx[b].tolist()
        for j, v in enumerate(rows):
            if n == k or v < 0:
                break
            c = cls[v]
            if taken.get(c, 0) < m:
                taken[c] = taken.get(c, 0) + 1
                out_idx[b, n], out_score[b, n] = v, score[b, j]
                n += 1
        decided = decided and (n == k or not rows or rows[-1] < 0)
    return out_idx, out_score, decided
