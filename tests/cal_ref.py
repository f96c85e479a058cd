"""Restatements of ``nrl_calibrated_rerank`` (``include/newsreclib_amd.h`` states the semantics) for ONE user's pool.

``cal_f64``: the definition in float64 numpy -- real arithmetic for every purpose of the tests.
``cal_f32``: the same with every operation one numpy float32 operation in the header's order, the pool's Gram matrix given
(``None`` with ``mu == 0``, where none is computed): it reproduces the kernel's bits whenever ``G`` has the kernel's bits.
Both return ``(idx (k) int64, score (k) float32, obj (k), cal (k), flags, steps)``; ``steps[t]`` is ``(slot chosen, objective of
every slot: NaN where the slot is dead or already selected)``.  ``forced``: follow these slots instead of choosing, as in
``mmr_ref``.  Live slots, relevance, similarity, tie order and NaN order are ``mmr_ref``'s own code.
"""
import numpy as np

from tests import mmr_ref as M

E_ROW, E_NAN, E_CLASS, E_TARGET = 1, 4, 64, 128
MAX_CLASSES = 64
F = np.float32


def clean_target(target, dtype):
    """(the target with every negative, NaN or infinite entry as +0, flags)"""
    raw = np.asarray(target, dtype=F)
    ok = np.isfinite(raw) & (raw >= 0)
    return np.where(ok, raw, F(0)).astype(dtype), (0 if ok.all() else E_TARGET)


def cal_terms(counts, target, dtype):
    """cal_c for every class c: two chains of single additions in ascending j from +0, one division."""
    S = len(target)
    classes = np.arange(S)
    m, x = np.zeros(S, dtype=dtype), np.zeros(S, dtype=dtype)           # (entry c: the chains of class c)
    for j in range(S):
        n1 = (counts[j] + (classes == j)).astype(dtype)
        m = (m + np.minimum(n1, target[j])).astype(dtype)
        x = (x + np.maximum(n1, target[j])).astype(dtype)
    return (m / x).astype(dtype)


def count_formula(classes, target, dtype=F):
    """sum(min(cnt, t)) / sum(max(cnt, t)) over the class counts of a finished list (header, property 5)."""
    S = len(target)
    cnt = np.bincount(np.asarray(classes, dtype=np.int64), minlength=S)
    m, x = dtype(0), dtype(0)
    for j in range(S):
        m = dtype(m + min(dtype(cnt[j]), dtype(target[j])))
        x = dtype(x + max(dtype(cnt[j]), dtype(target[j])))
    return dtype(m / x)


def _greedy(pool_idx, pool_score, live, flags, rel, sim, slot_class, target, lam, mu, gamma, k, dtype, forced):
    N, S = len(pool_idx), len(target)
    idx = np.full(k, -1, dtype=np.int64)
    score = np.full(k, -np.inf, dtype=np.float32)
    obj_out = np.full(k, -np.inf, dtype=dtype)
    cal_out = np.full(k, -np.inf, dtype=dtype)
    pen = np.zeros(N, dtype=dtype)
    sel = np.zeros(N, dtype=bool)
    counts = np.zeros(S, dtype=np.int64)
    in_range = live & (slot_class >= 0) & (slot_class < S)
    if (live & ~in_range).any():
        flags |= E_CLASS
    steps = []
    with np.errstate(all="ignore"):
        for t in range(k):
            cal = cal_terms(counts, target, dtype)
            term = np.where(in_range, cal[np.where(in_range, slot_class, 0)], dtype(0)).astype(dtype)
            base = (lam * rel).astype(dtype) if mu == 0 else ((lam * rel).astype(dtype) - (mu * pen).astype(dtype)).astype(dtype)
            obj = (base + (gamma * term).astype(dtype)).astype(dtype)
            avail = live & ~sel
            c = M._pick(obj, avail) if forced is None else (int(forced[t]) if t < len(forced) else -1)
            steps.append((c, np.where(avail, obj, np.nan)))
            if c < 0:
                break
            idx[t], score[t], obj_out[t], cal_out[t] = pool_idx[c], pool_score[c], obj[c], term[c]
            sel[c] = True
            if in_range[c]:
                counts[slot_class[c]] += 1
            if mu != 0:
                pen = sim[c].copy() if t == 0 else np.fmax(pen, sim[c])
    return idx, score, obj_out, cal_out, flags, steps


def _slot_classes(pool_idx, row_class, V):
    pool_idx = np.asarray(pool_idx, dtype=np.int64)
    ok = (pool_idx >= 0) & (pool_idx < V)
    return np.where(ok, np.asarray(row_class, dtype=np.int64)[np.where(ok, pool_idx, 0)], -1)


def _relevance(pool_score, live, normalize, dtype):
    rel = pool_score.astype(dtype)
    if normalize:
        rel = np.zeros(len(pool_score), dtype=dtype)
        if live.any():
            s_min, s_max = pool_score[live].min() + dtype(0), pool_score[live].max() + dtype(0)   # (+0: a -0 extreme counts as +0)
            if s_max != s_min:
                rel = ((pool_score - s_min).astype(dtype) / dtype(s_max - s_min)).astype(dtype)
    return rel


def cal_f32(pool_idx, pool_score, G, V, row_class, target, k, lam, mu, gamma, similarity="cosine", normalize=True, forced=None):
    """Every operation in float32, in the header's order.  ``G`` (N, N) float32: the Gram matrix of the pool's table rows; with
    ``mu == 0`` it is not looked at (``None`` will do)."""
    pool_idx = np.asarray(pool_idx, dtype=np.int64)
    pool_score = np.asarray(pool_score, dtype=F)
    N = len(pool_idx)
    lam, mu, gamma = F(lam), F(mu), F(gamma)
    target, tflag = clean_target(target, F)
    with np.errstate(all="ignore"):
        sim = None
        if mu != 0:
            G = np.asarray(G, dtype=F)
            live, flags = M.live_slots(pool_idx, pool_score, V, np.diagonal(G))
            if similarity == "cosine":
                d = np.diagonal(G).astype(F)
                r = np.where(live & (d != 0), F(1) / np.sqrt(np.where(live, d, F(1)), dtype=F), F(0)).astype(F)
                sim = (G * (r[:, None] * r[None, :]).astype(F)).astype(F)
            else:
                sim = G
        else:
            live, flags = M.live_slots(pool_idx, pool_score, V, np.zeros(N))
        rel = _relevance(pool_score, live, normalize, F)
        return _greedy(pool_idx, pool_score, live, flags | tflag, rel, sim, _slot_classes(pool_idx, row_class, V), target, lam, mu, gamma,
                       k, F, forced)


def cal_f64(pool_idx, pool_score, table, V, row_class, target, k, lam, mu, gamma, similarity="cosine", normalize=True, forced=None):
    """The definition with real (float64) arithmetic over ``table`` (V, D); ``table`` may be ``None`` with ``mu == 0``."""
    pool_idx = np.asarray(pool_idx, dtype=np.int64)
    score32 = np.asarray(pool_score, dtype=F)
    pool_score = score32.astype(np.float64)
    N = len(pool_idx)
    lam, mu, gamma = float(F(lam)), float(F(mu)), float(F(gamma))
    target, tflag = clean_target(target, np.float64)
    with np.errstate(all="ignore"):
        sim = None
        if mu != 0:
            table = np.asarray(table, dtype=np.float64)
            row_ok = (pool_idx >= 0) & (pool_idx < V)
            rows = table[np.where(row_ok, pool_idx, 0)] * row_ok[:, None]
            G = rows @ rows.T
            live, flags = M.live_slots(pool_idx, pool_score, V, np.diagonal(G))
            if similarity == "cosine":
                d = np.diagonal(G)
                r = np.where(live & (d != 0), 1.0 / np.sqrt(np.where(live & (d > 0), d, 1.0)), 0.0)
                sim = G * (r[:, None] * r[None, :])
            else:
                sim = G
        else:
            live, flags = M.live_slots(pool_idx, pool_score, V, np.zeros(N))
        rel = _relevance(pool_score, live, normalize, np.float64)
        idx, _, obj, cal, flags, steps = _greedy(pool_idx, pool_score, live, flags | tflag, rel, sim,
                                                 _slot_classes(pool_idx, row_class, V), target, lam, mu, gamma, k, np.float64, forced)
    score = np.where(idx >= 0, 0, -np.inf).astype(F)
    for t, (c, _) in enumerate(steps):
        if c >= 0:
            score[t] = score32[c]
    return idx, score, obj, cal, flags, steps
