"""Restatements of ``nrl_mmr_rerank`` (``include/newsreclib_amd.h`` states the semantics) for ONE user's pool.

``mmr_f64``: the definition in float64 numpy -- real arithmetic for every purpose of the tests.
``mmr_f32``: the same with every operation one numpy float32 operation in the header's order, the pool's Gram matrix given: it
reproduces the kernel's bits whenever ``G`` has the kernel's bits (on eighth-grid tables the Gram matrix is exact).
Both return ``(idx (k) int64, score (k) float32, mmr (k), flags, steps)``; ``steps[t]`` is ``(slot chosen, objective of every
slot: NaN where the slot is dead or already selected)``.  ``forced``: follow these slots instead of choosing (the objectives are
still those of the definition): what the greedy-validity check of a kernel's own prefix needs.
"""
import numpy as np

E_ROW, E_NAN = 1, 4
F = np.float32


def live_slots(pool_idx, pool_score, V, diag):
    """(live (N) bool, flags) from the rows, the scores and the Gram diagonal (``diag[i]`` is read for slots live so far)."""
    pool_idx = np.asarray(pool_idx, dtype=np.int64)
    row_ok = (pool_idx >= 0) & (pool_idx < V)
    fin = np.isfinite(np.asarray(pool_score, dtype=np.float64))
    flags = 0
    if ((pool_idx != -1) & ~row_ok).any():
        flags |= E_ROW
    if (row_ok & ~fin).any():
        flags |= E_NAN
    live = row_ok & fin
    bad_diag = live & ~np.isfinite(np.asarray(diag, dtype=np.float64))
    if bad_diag.any():
        flags |= E_NAN
    return live & ~bad_diag, flags


def _pick(obj, avail):
    """The available slot of largest objective; equal objectives: the lower slot; NaN below every number; -1: none left."""
    cand = np.nonzero(avail)[0]
    if cand.size == 0:
        return -1
    numbers = cand[~np.isnan(obj[cand])]
    if numbers.size == 0:
        return int(cand[0])
    return int(numbers[np.argmax(obj[numbers])])            # (argmax: the first of equal maxima; -0 == +0)


def _greedy(pool_idx, pool_score, live, flags, rel, sim, lam, one_minus, k, dtype, forced):
    N = len(pool_idx)
    idx = np.full(k, -1, dtype=np.int64)
    score = np.full(k, -np.inf, dtype=np.float32)
    mmr = np.full(k, -np.inf, dtype=dtype)
    pen = np.zeros(N, dtype=dtype)
    sel = np.zeros(N, dtype=bool)
    steps = []
    with np.errstate(all="ignore"):
        for t in range(k):
            obj = (lam * rel - one_minus * pen).astype(dtype)        # (two products, each rounded, then one subtraction)
            avail = live & ~sel
            c = _pick(obj, avail) if forced is None else (int(forced[t]) if t < len(forced) else -1)
            steps.append((c, np.where(avail, obj, np.nan)))
            if c < 0:
                break
            idx[t], score[t], mmr[t] = pool_idx[c], pool_score[c], obj[c]
            sel[c] = True
            pen = sim[c].copy() if t == 0 else np.fmax(pen, sim[c])
    return idx, score, mmr, flags, steps


def mmr_f32(pool_idx, pool_score, G, V, k, lam, similarity="cosine", normalize=True, forced=None):
    """Every operation in float32, in the header's order.  ``G`` (N, N) float32: the Gram matrix of the pool's table rows (any
    value where a row is outside the table)."""
    pool_idx = np.asarray(pool_idx, dtype=np.int64)
    pool_score = np.asarray(pool_score, dtype=F)
    G = np.asarray(G, dtype=F)
    N = len(pool_idx)
    live, flags = live_slots(pool_idx, pool_score, V, np.diagonal(G))
    lam = F(lam)
    with np.errstate(all="ignore"):
        if similarity == "cosine":
            d = np.diagonal(G).astype(F)
            r = np.where(live & (d != 0), F(1) / np.sqrt(np.where(live, d, F(1)), dtype=F), F(0)).astype(F)
            sim = (G * (r[:, None] * r[None, :]).astype(F)).astype(F)
        else:
            sim = G
        rel = pool_score.copy()
        if normalize:
            rel = np.zeros(N, dtype=F)
            if live.any():
                s_min, s_max = pool_score[live].min() + F(0), pool_score[live].max() + F(0)      # (+0: a -0 extreme counts as +0)
                if s_max != s_min:
                    rel = ((pool_score - s_min).astype(F) / F(s_max - s_min)).astype(F)
        return _greedy(pool_idx, pool_score, live, flags, rel, sim, lam, F(F(1) - lam), k, F, forced)


def mmr_f64(pool_idx, pool_score, table, k, lam, similarity="cosine", normalize=True, forced=None):
    """The definition with real (float64) arithmetic over ``table`` (V, D)."""
    pool_idx = np.asarray(pool_idx, dtype=np.int64)
    score32 = np.asarray(pool_score, dtype=F)
    pool_score = score32.astype(np.float64)
    table = np.asarray(table, dtype=np.float64)
    V, N = table.shape[0], len(pool_idx)
    row_ok = (pool_idx >= 0) & (pool_idx < V)
    rows = table[np.where(row_ok, pool_idx, 0)] * row_ok[:, None]
    with np.errstate(all="ignore"):
        G = rows @ rows.T
        live, flags = live_slots(pool_idx, pool_score, V, np.diagonal(G))
        lam = float(F(lam))
        if similarity == "cosine":
            d = np.diagonal(G)
            r = np.where(live & (d != 0), 1.0 / np.sqrt(np.where(live & (d > 0), d, 1.0)), 0.0)
            sim = G * (r[:, None] * r[None, :])
        else:
            sim = G
        rel = pool_score.copy()
        if normalize:
            rel = np.zeros(N)
            if live.any():
                s_min, s_max = pool_score[live].min(), pool_score[live].max()
                if s_max != s_min:
                    rel = (pool_score - s_min) / (s_max - s_min)
        idx, _, mmr, flags, steps = _greedy(pool_idx, pool_score, live, flags, rel, sim, lam, 1.0 - lam, k, np.float64, forced)
    score = np.where(idx >= 0, 0, -np.inf).astype(F)
    for t, (c, _) in enumerate(steps):
        if c >= 0:
            score[t] = score32[c]
    return idx, score, mmr, flags, steps


def gram_f32(pool_idx, table):
    """The pool's Gram matrix from an eighth-grid table, where the float64 product is exact and fits float32 unchanged."""
    pool_idx = np.asarray(pool_idx, dtype=np.int64)
    table = np.asarray(table, dtype=np.float64)
    ok = (pool_idx >= 0) & (pool_idx < table.shape[0])
    rows = table[np.where(ok, pool_idx, 0)] * ok[:, None]
    G = rows @ rows.T
    assert np.array_equal(G.astype(F).astype(np.float64), G), "the table is not on a grid where the Gram matrix is exact in float32"
    return G.astype(F)
