"""CPU float64 reference of the full-catalogue rank of held-out rows (``nrl_catalogue_ranks``).

Masked scores as ``test_gpu_topk.py::_masked_scores``: ``s = U64 @ T64.T`` with the positions that are ineligible, on the user's
exclusion list or NaN at ``-inf``.  A target's rank is 1 + the number of qualifying rows with a higher score, or an equal score
and a lower row; 0 (and score ``-inf``) when the target is outside the table or does not qualify itself.  The population is the
count of finite entries."""
import torch


def ragged(lists):
    off = torch.tensor([0] + [len(x) for x in lists]).cumsum(0)
    idx = torch.tensor([v for x in lists for v in x], dtype=torch.int64)
    return idx, off


def masked_scores(U, T, excl=None, eligible=None):
    """(B, V) float64 scores; -inf where the row may not be returned for the user or its score is NaN."""
    s = U.double() @ T.double().T
    V = T.shape[0]
    s[torch.isnan(s)] = float("-inf")
    if eligible is not None:
        s[:, ~eligible.bool()] = float("-inf")
    if excl is not None:
        for b, rows in enumerate(excl):
            rows = [r for r in rows if 0 <= r < V]
            if rows:
                s[b, torch.tensor(rows)] = float("-inf")
    return s


def ranks_from_scores(s, targets):
    """rank int32 (n), score float32 (n), ranked int32 (B) of the masked scores ``s`` (B, V) and per-user target lists."""
    B, V = s.shape
    rows = torch.arange(V)
    rank, score = [], []
    for b, tl in enumerate(targets):
        ok = torch.isfinite(s[b])
        for t in tl:
            if not 0 <= t < V or not bool(ok[t]):
                rank.append(0)
                score.append(float("-inf"))
                continue
            above = ok & ((s[b] > s[b, t]) | ((s[b] == s[b, t]) & (rows < t)))
            rank.append(1 + int(above.sum()))
            score.append(float(s[b, t]))
    ranked = torch.isfinite(s).sum(1).to(torch.int32) if V else torch.zeros(B, dtype=torch.int32)
    return torch.tensor(rank, dtype=torch.int32), torch.tensor(score, dtype=torch.float64).float(), ranked


def reference(U, T, targets, excl=None, eligible=None):
    return ranks_from_scores(masked_scores(U, T, excl, eligible), targets)
