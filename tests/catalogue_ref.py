"""The full-catalogue contract, stated once for every test of the top-k and rank entries: which (user, row) pairs may be
returned, in what order, and what a target's rank is.  CPU only, torch in float64; ``newsreclib_amd`` is not imported.

* population: a row counts for a user iff it is eligible, not on the user's exclusion list (entries outside [0, V) are ignored,
  duplicates are harmless) and its score is not NaN (a NaN dropped from an otherwise allowed position is reported: status bit 4);
* order: score descending, equal scores by ascending row, ``-0.0 == +0.0``; scores come back as ``+0`` for ``-0``;
* rank: 1 + the rows of the population ordered above the target; 0 (score ``-inf``) for a target outside the table or the
  population.

Where the copies this module replaced differed, it takes the stricter reading: NaN is dropped everywhere; ``topk`` and ``ranks``
return ``+0`` for ``-0`` (``topk_capped_ref.reference`` used to pass ``-0`` on); ``topk`` refuses a ``-inf`` score inside the
population (the empty slot's value); ``check_floor`` checks membership in the population, not only in the exclusion list; ``same``
compares shapes, types and, for float32, bits where the rank files compared values.

Each scorer's ref module (``topk_*_ref``, ``catalogue_rank_*_ref``) keeps only its own scores, bounds and case builders.
The ``engine`` fixture the GPU files repeat belongs in ``conftest.py``, which stays as it is: do not import it from here."""
import numpy as np
import torch

NEG_INF = float("-inf")


def ragged(lists):
    """per-user lists -> (flat idx int64, offsets int64 (B + 1))"""
    off = torch.tensor([0] + [len(x) for x in lists]).cumsum(0)
    idx = torch.tensor([v for x in lists for v in x], dtype=torch.int64)
    return idx, off


def int_vectors(seed, B, V, D):
    """Integer-valued user and table vectors in [-4, 4]: every fp32 dot product of them is exact in any order, and ties abound."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(-4, 5, (B, D), generator=g).float(), torch.randint(-4, 5, (V, D), generator=g).float())


def dot_bound(U, T):
    """(B, V) worst-case error of an fp32 dot product of length D in any order: ``D 2^-23 |U| |T|^T`` (derived, not measured)."""
    return U.shape[1] * 2.0 ** -23 * (U.double().abs() @ T.double().abs().T)


def allowed(B, V, excl=None, eligible=None):
    """(B, V) bool: the eligible rows that are not on the user's exclusion list."""
    ok = torch.ones(B, V, dtype=torch.bool)
    if eligible is not None:
        ok &= torch.as_tensor(eligible).bool()[None, :]
    if excl is not None:
        for b, rows in enumerate(excl):
            rows = [r for r in rows if 0 <= r < V]
            if rows:
                ok[b, torch.tensor(rows)] = False
    return ok


def population(s, excl=None, eligible=None):
    """-> ((B, V) bool, whether a NaN score was dropped from an otherwise allowed position)"""
    ok, nan = allowed(*s.shape, excl, eligible), torch.isnan(s)
    return ok & ~nan, bool((ok & nan).any())


def masked(s, pop):
    """a copy of ``s`` with -inf outside the population"""
    return torch.where(pop, s, torch.full_like(s, NEG_INF))


def topk(s, pop, k):
    """-> idx (B, k) int64, score (B, k) float32; -1 / -inf where the population runs out"""
    B, V = s.shape
    assert not bool((pop & (s == NEG_INF)).any())           # (a score of -inf is the empty slot's)
    idx = torch.full((B, k), -1, dtype=torch.int64)
    score = torch.full((B, k), NEG_INF, dtype=torch.float32)
    n = min(k, V)
    if n:
        key = torch.where(pop, -s.double(), torch.full((), float("inf"), dtype=torch.float64))
        order = torch.sort(key, dim=1, stable=True)[1][:, :n]          # (-0.0 == 0.0: such rows stay in ascending order)
        keep = pop.gather(1, order)
        idx[:, :n] = torch.where(keep, order, torch.full_like(order, -1))
        score[:, :n] = masked(s, pop).gather(1, order).float() + 0.0
    return idx, score


def expected_topk(s, k, excl=None, eligible=None):
    """``topk`` over the population of the float64 scores ``s`` (B, V)"""
    return topk(s, population(s, excl, eligible)[0], k)


def ranks(s, pop, targets):
    """``targets``: per user a list of rows -> rank int32 (n), score float32 (n), ranked int32 (B), in the users' order"""
    B, V = s.shape
    rows = torch.arange(V)
    rank, score = [], []
    for b, tl in enumerate(targets):
        for t in tl:
            if not 0 <= t < V or not bool(pop[b, t]):
                rank.append(0)
                score.append(NEG_INF)
                continue
            above = pop[b] & ((s[b] > s[b, t]) | ((s[b] == s[b, t]) & (rows < t)))
            rank.append(1 + int(above.sum()))
            score.append(float(s[b, t]))
    return (torch.tensor(rank, dtype=torch.int32), torch.tensor(score, dtype=torch.float64).float() + 0.0,
            pop.sum(1).to(torch.int32))


def expected_ranks(s, targets, excl=None, eligible=None):
    """``ranks`` over the population of the float64 scores ``s`` (B, V)"""
    return ranks(s, population(s, excl, eligible)[0], targets)


def rank_intervals(s, bound, pop, targets):
    """Per target in flat order ``(lo, hi)``, None for a target outside its user's population.  With ``bound`` the worst-case
    error of a computed score, a row v != t is certainly above the target t when ``s[v] - bound[v] > s[t] + bound[t]`` and
    possibly above it when ``s[v] + bound[v] >= s[t] - bound[t]``: ``1 + #certain <= rank <= 1 + #possible``."""
    V = s.shape[1]
    out = []
    for b, tl in enumerate(targets):
        for t in tl:
            if not 0 <= t < V or not bool(pop[b, t]):
                out.append(None)
                continue
            others = pop[b].clone()
            others[t] = False
            certain = others & (s[b] - bound[b] > s[b, t] + bound[b, t])
            possible = others & (s[b] + bound[b] >= s[b, t] - bound[b, t])
            out.append((1 + int(certain.sum()), 1 + int(possible.sum())))
    return out


def check_floor(idx, score, raw, bound, pop, k):
    """The floor form of a real-valued comparison: the gap between the k-th and the (k + 1)-th score can be below the bound, so row
    sets are never compared.  Every returned score is within its bound of float64, the order is descending with ties by ascending
    row, the k rows are distinct and of the population, and no left-out row of the population exceeds the k-th by more than twice
    its bound."""
    for b in range(raw.shape[0]):
        rows = idx[b]
        assert bool((rows >= 0).all()), b
        got = score[b].double()
        err = (got - raw[b, rows]).abs()
        print(f"user {b}: max |score - float64| = {float(err.max()):.3e}, bound >= {float(bound[b, rows].min()):.3e}, "
              f"worst err / bound = {float((err / bound[b, rows]).max()):.3f}")
        assert bool((err <= bound[b, rows]).all()), b
        assert bool((got[1:] <= got[:-1]).all()), b
        tie = got[1:] == got[:-1]
        assert bool((rows[1:][tie] > rows[:-1][tie]).all()), b
        assert len(set(rows.tolist())) == k and bool(pop[b, rows].all()), b
        rest = pop[b].clone()
        rest[rows] = False
        assert bool((raw[b][rest] <= raw[b, rows].min() + 2 * bound[b][rest]).all()), b


def bits(x):
    return x.contiguous().view(torch.int32)


def same(got, want):
    """A result against its expectation (tensors, numpy arrays or sequences of them): equal shapes, types and values, and for
    float32 equal bits."""
    if isinstance(got, (tuple, list)):
        return len(got) == len(want) and all(same(g, w) for g, w in zip(got, want))
    got = got.cpu()
    want = torch.from_numpy(np.ascontiguousarray(want)) if isinstance(want, np.ndarray) else want.cpu()
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    return torch.equal(bits(got), bits(want)) if got.dtype == torch.float32 else torch.equal(got, want)


def sync_debug_honoured():
    """whether this torch build raises on synchronising calls under ``torch.cuda.set_sync_debug_mode("error")``"""
    try:
        float(torch.ones(1, device="cuda").sum())
    except RuntimeError:
        return True
    return False
