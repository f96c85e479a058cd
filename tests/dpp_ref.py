"""Restatements of ``nrl_dpp_rerank`` (``include/newsreclib_amd.h`` states the semantics) for ONE user's pool.

``dpp_f64``: the definition in float64 numpy.  The marginal gain of slot i over the listed set S is computed from scratch at every
step, ``L_ii - L_iS L_SS^-1 L_Si`` by a solve against ``L_S``: it shares nothing with the incremental Cholesky rows under test.
``dpp_f32``: the kernel's recurrence with every operation one numpy float32 operation in the header's order, the pool's Gram matrix
and the slots' qualities given: it reproduces the kernel's bits whenever ``G`` has the kernel's bits (on eighth-grid tables the
Gram matrix is exact).
Both return ``(idx (k) int64, score (k) float32, gain (k), flags, steps)``; ``steps[t]`` is ``(slot chosen, gain of every slot:
NaN where the slot is dead or already listed, whether the step belonged to the DPP phase)``.  ``forced`` (``dpp_f64``): follow
these slots instead of choosing (the gains are still those of the definition): what the greedy-validity check of a kernel's own
prefix needs.
"""
import numpy as np

from tests.mmr_ref import E_NAN, E_ROW, gram_f32, live_slots  # noqa: F401  (gram_f32, E_ROW: for the tests that import this module)

E_QUALITY, E_RANK = 256, 512
F = np.float32


def _live(pool_idx, pool_score, V, diag, quality):
    """(live, flags) in the kernel's order: rows and scores, then the quality of the slots live so far, then the Gram diagonal."""
    first, flags = live_slots(pool_idx, pool_score, V, np.zeros(len(pool_idx)))
    bad_q = np.zeros(len(pool_idx), dtype=bool)
    if quality is not None:
        with np.errstate(invalid="ignore"):
            bad_q = first & ~(np.isfinite(quality) & (quality >= 0))
        if bad_q.any():
            flags |= E_QUALITY
    live, more = live_slots(pool_idx, pool_score, V, np.where(bad_q, 0, diag))
    return live & ~bad_q, flags | more


def _fill_order(live, sel, pool_score):
    """the live, unlisted slots by (pool score descending, slot ascending); -0 == +0"""
    return sorted((int(i) for i in np.nonzero(live & ~sel)[0]), key=lambda i: (-float(pool_score[i]), i))


def dpp_f32(pool_idx, pool_score, G, V, k, quality, eps=1e-4, similarity="cosine"):
    """Every operation in float32, in the header's order.  ``G`` (N, N) float32: the Gram matrix of the pool's table rows (any
    value where a row is outside the table); ``quality`` (N): the slots' qualities (the header does not fix the bits of expf, so
    the restatement takes q as given)."""
    pool_idx = np.asarray(pool_idx, dtype=np.int64)
    pool_score = np.asarray(pool_score, dtype=F)
    G, quality, eps = np.asarray(G, dtype=F), np.asarray(quality, dtype=F), F(eps)
    N = len(pool_idx)
    idx, score, gain = np.full(k, -1, dtype=np.int64), np.full(k, -np.inf, dtype=F), np.full(k, -np.inf, dtype=F)
    steps = []
    with np.errstate(all="ignore"):
        live, flags = _live(pool_idx, pool_score, V, np.diagonal(G), quality)
        if similarity == "cosine":
            d = np.diagonal(G).astype(F)
            r = np.where(live & (d != 0), F(1) / np.sqrt(np.where(live, d, F(1)), dtype=F), F(0)).astype(F)
            sim = (G * (r[:, None] * r[None, :]).astype(F)).astype(F)
        else:
            sim = G
        q = np.where(live, quality, F(0)).astype(F)
        L = ((q[:, None] * q[None, :]).astype(F) * sim).astype(F)
        bad = live & ~np.isfinite(np.diagonal(L))
        if bad.any():
            flags |= E_NAN
            live = live & ~bad
        d2 = np.diagonal(L).astype(F).copy()
        thr = (eps * d2).astype(F)
        sel = np.zeros(N, dtype=bool)
        cv = []
        t = 0
        while t < k:
            elig = live & ~sel & (d2 > 0) & (d2 >= thr)
            if not elig.any():
                break
            c = int(np.argmax(np.where(elig, d2, F(-np.inf))))      # (argmax: the first of equal maxima)
            steps.append((c, np.where(live & ~sel, d2, np.nan), True))
            idx[t], score[t], gain[t] = pool_idx[c], pool_score[c], d2[c]
            sel[c] = True
            acc = np.zeros(N, dtype=F)
            for row in cv:                                          # ascending s; one product and one sum, each rounded
                acc = (acc + (row[c] * row).astype(F)).astype(F)
            e = ((L[c] - acc).astype(F) / np.sqrt(d2[c], dtype=F)).astype(F)
            cv.append(e)
            rest = live & ~sel
            d2 = np.where(rest, (d2 - (e * e).astype(F)).astype(F), d2)
            t += 1
        for c in _fill_order(live, sel, pool_score)[:k - t]:
            steps.append((c, np.where(live & ~sel, F(0), np.nan), False))
            idx[t], score[t], gain[t] = pool_idx[c], pool_score[c], F(0)
            sel[c] = True
            flags |= E_RANK
            t += 1
    return idx, score, gain, flags, steps


def relevance_f64(pool_score, live, normalize):
    """rel of nrl_mmr_rerank in real arithmetic"""
    pool_score = np.asarray(pool_score, dtype=np.float64)
    if not normalize:
        return pool_score.copy()
    rel = np.zeros(len(pool_score))
    if live.any():
        s_min, s_max = pool_score[live].min(), pool_score[live].max()
        if s_max != s_min:
            with np.errstate(all="ignore"):
                rel = (pool_score - s_min) / (s_max - s_min)
    return rel


def kernel_matrix_f64(pool_idx, pool_score, table, quality=None, alpha=1.0, similarity="cosine", normalize=True):
    """(L (N, N) float64, live, flags, q) of the definition over ``table`` (V, D)"""
    pool_idx = np.asarray(pool_idx, dtype=np.int64)
    score = np.asarray(pool_score, dtype=F).astype(np.float64)
    table = np.asarray(table, dtype=np.float64)
    V = table.shape[0]
    row_ok = (pool_idx >= 0) & (pool_idx < V)
    rows = table[np.where(row_ok, pool_idx, 0)] * row_ok[:, None]
    with np.errstate(all="ignore"):
        G = rows @ rows.T
        live, flags = _live(pool_idx, score, V, np.diagonal(G), None if quality is None else np.asarray(quality, dtype=np.float64))
        if similarity == "cosine":
            d = np.diagonal(G)
            r = np.where(live & (d != 0), 1.0 / np.sqrt(np.where(live & (d > 0), d, 1.0)), 0.0)
            sim = G * (r[:, None] * r[None, :])
        else:
            sim = G
        if quality is None:
            q = np.exp(float(F(alpha)) * relevance_f64(score, live, normalize))
        else:
            q = np.asarray(quality, dtype=np.float64)
        q = np.where(live, q, 0.0)
        L = (q[:, None] * q[None, :]) * sim
        bad = live & ~np.isfinite(np.diagonal(L))
        if bad.any():
            flags |= E_NAN
            live = live & ~bad
    return L, live, flags, q


def marginal_gains_f64(L, listed):
    """det L_{S + i} / det L_S for every slot i, S = ``listed``: the Schur complement by a solve against L_S"""
    d = np.diagonal(L).copy()
    if not listed:
        return d
    S = list(listed)
    with np.errstate(all="ignore"):
        return d - np.einsum("si,si->i", L[S, :], np.linalg.solve(L[np.ix_(S, S)], L[S, :]))


def dpp_f64(pool_idx, pool_score, table, k, quality=None, alpha=1.0, eps=1e-4, similarity="cosine", normalize=True, forced=None):
    """The definition with real (float64) arithmetic over ``table`` (V, D)."""
    pool_idx = np.asarray(pool_idx, dtype=np.int64)
    score32 = np.asarray(pool_score, dtype=F)
    L, live, flags, _ = kernel_matrix_f64(pool_idx, score32, table, quality, alpha, similarity, normalize)
    N = len(pool_idx)
    idx, score, gain = np.full(k, -1, dtype=np.int64), np.full(k, -np.inf, dtype=F), np.full(k, -np.inf)
    sel = np.zeros(N, dtype=bool)
    steps, listed = [], []
    eps = float(F(eps))
    t = 0
    while t < k:
        g = marginal_gains_f64(L, listed)
        with np.errstate(invalid="ignore"):
            elig = live & ~sel & (g > 0) & (g >= eps * np.diagonal(L))
        if forced is not None:
            c = int(forced[t]) if t < len(forced) else -1
        else:
            c = int(np.argmax(np.where(elig, g, -np.inf))) if elig.any() else -1
        if c < 0:
            break
        steps.append((c, np.where(live & ~sel, g, np.nan), True))
        idx[t], score[t], gain[t] = pool_idx[c], score32[c], g[c]
        sel[c] = True
        listed.append(c)
        t += 1
    if forced is None:
        for c in _fill_order(live, sel, score32)[:k - t]:
            steps.append((c, np.where(live & ~sel, 0.0, np.nan), False))
            idx[t], score[t], gain[t] = pool_idx[c], score32[c], 0.0
            sel[c] = True
            flags |= E_RANK
            t += 1
    return idx, score, gain, flags, steps
