"""Calibrated greedy re-ranking of top-k pools (``nrl_calibrated_rerank``, ``ops.calibrated_rerank``, ``ops.class_targets``,
``*Cache.rerank_calibrated``, ``recommend_users(calibrate=...)``).

Expected values come from ``tests/cal_ref.py``.  The exact cases use table entries, scores and targets that are multiples of 1/8:
the Gram matrix is exact (``test_gpu_mmr`` says why), and everything behind it -- the square root, the divisions, the products,
the differences, the two chains of additions and the quotient of the calibration term -- is a single correctly rounded float32
operation on both sides, so the float32 restatement must reproduce rows, scores, objectives, terms and the status word bit for
bit.  The real-valued cases check the kernel's own prefix against the float64 objective under a tolerance worked out from D and
the three weights."""
import warnings

import numpy as np
import pytest
import torch

from tests import builders
from tests import cal_ref as R
from tests import catalogue_ref as C
from tests import mmr_ref as M

pytestmark = pytest.mark.gpu
F = np.float32


@pytest.fixture(autouse=True, params=["f32", "bf16x3"])
def engine(request):
    from newsreclib_amd import _lib
    prev = _lib.get_gemm_engine()
    _lib.set_gemm_engine(request.param)
    yield request.param
    _lib.set_gemm_engine(prev)


def _dev(x):
    return None if x is None else (torch.from_numpy(x) if isinstance(x, np.ndarray) else x).cuda()


def _rerank(idx, score, table, row_class, target, k, lam, mu, gamma, similarity="cosine", normalize=True):
    from newsreclib_amd import ops
    return ops.calibrated_rerank(_dev(idx), _dev(score), _dev(table), _dev(row_class), _dev(target), k, lam, mu, gamma, similarity,
                                 normalize)


def _flags_of(idx, score, row_class, target, V, S):
    """the status word of a whole batch on a finite-diagonal table, without the greedy steps"""
    row_ok = (idx >= 0) & (idx < V)
    fin = np.isfinite(score)
    live = row_ok & fin
    cls = row_class[np.where(row_ok, idx, 0)]
    want = 0
    want |= R.E_ROW if ((idx != -1) & ~row_ok).any() else 0
    want |= R.E_NAN if (row_ok & ~fin).any() else 0
    want |= R.E_CLASS if (live & ((cls < 0) | (cls >= S))).any() else 0
    want |= R.E_TARGET if not (np.isfinite(target) & (target >= 0)).all() else 0
    return want


# ---- 1. the exact sweep ---------------------------------------------------------------------------------------------------------------------
V_SWEEP = 200
_CACHE = {}
# (B, N, S, D): every B, N, S and D of the issue; N = 63 / 64 / 65 / 128 each with one table tile and with two; S = 64 with N = 128
_SHAPES = [(1, 1, 1, 4), (3, 2, 2, 300), (1, 63, 19, 4), (3, 63, 1, 300), (3, 64, 64, 300), (65, 64, 2, 4), (65, 65, 19, 4),
           (1, 65, 64, 300), (3, 128, 64, 300), (65, 128, 19, 4), (1, 128, 2, 300)]


def _sweep_case(B, N, S, D):
    """``test_gpu_mmr``'s pools (user 0: an empty slot in the middle and one at the tail, the rows V and -2, a NaN and a +inf
    score, a duplicated row, the zero row; user 1 all empty; user 2 two live slots) with classes and targets beside them: two table
    rows carry the classes S and -1 and user 0's pool holds both, user 0's target has a NaN, a negative and an infinite entry as far
    as S has room, user 1's target is all zero; eighth-grid scores and targets tie everywhere."""
    key = ("case", B, N, S, D)
    if key not in _CACHE:
        rng = np.random.default_rng(100000 * B + 100 * N + 10 * S + D)
        table = (rng.integers(-16, 17, (V_SWEEP, D)) / 8.0).astype(F)
        table[0] = 0.0
        idx = rng.integers(0, V_SWEEP - 2, (B, N))
        score = (rng.integers(-16, 17, (B, N)) / 8.0).astype(F)
        row_class = rng.integers(0, S, V_SWEEP).astype(np.int64)
        row_class[V_SWEEP - 2], row_class[V_SWEEP - 1] = S, -1
        target = (rng.integers(0, 33, (B, S)) / 8.0).astype(F)
        edges = [("mid", 1, -1), ("row", 2, V_SWEEP), ("row", 3, -2), ("nan", 4, np.nan), ("inf", 5, np.inf), ("dup", 6, None),
                 ("zero", 8, 0), ("cls", 9, V_SWEEP - 2), ("cls", 10, V_SWEEP - 1), ("tail", N - 1, -1)]
        for kind, slot, value in edges:
            if slot >= N or (kind != "tail" and slot == N - 1) or N < 2:
                continue
            if kind in ("mid", "tail", "row", "zero", "cls"):
                idx[0, slot] = value
            elif kind == "dup":
                idx[0, slot + 1 if slot + 1 < N - 1 else slot] = idx[0, slot]
            else:
                score[0, slot] = value
        for j, bad in enumerate((np.nan, -0.125, np.inf)):
            if j + 1 < S:
                target[0, j + 1] = bad
        if B >= 3:
            idx[1, :] = -1
            target[1, :] = 0.0
            idx[2, 2:] = -1
        idx = idx.astype(np.int64)
        _CACHE[key] = (table, idx, score, row_class, target, _flags_of(idx, score, row_class, target, V_SWEEP, S))
    return _CACHE[key]


def _expected(B, N, S, D, users, k, lam, mu, gamma, sim, norm):
    key = ("want", B, N, S, D, tuple(users), k, lam, mu, gamma, sim, norm)
    if key not in _CACHE:
        table, idx, score, row_class, target, _ = _sweep_case(B, N, S, D)
        outs = [R.cal_f32(idx[u], score[u], M.gram_f32(idx[u], table) if mu else None, V_SWEEP, row_class, target[u], k, lam, mu,
                          gamma, sim, norm) for u in users]
        _CACHE[key] = tuple(np.stack([o[j] for o in outs]) for j in range(4))
    return _CACHE[key]


def _settings(N):
    """(k, lambda, mu, gamma, similarity, normalize, with a table): k in {1, N}; mu = 0 without and with a table, and mu > 0"""
    return [(N, 0.5, 0.0, 0.5, "cosine", True, False), (N, 0.5, 0.0, 0.5, "cosine", True, True), (1, 1.0, 0.0, 1.0, "dot", False, False),
            (1, 1.0, 0.0, 1.0, "dot", False, True), (N, 0.5, 0.25, 0.5, "cosine", True, True), (1, 0.25, 0.5, 1.0, "dot", False, True),
            (N, 0.25, 0.5, 1.0, "dot", False, True), (1, 0.5, 0.25, 0.5, "cosine", True, True)]


def test_the_sweep_covers_the_shapes_of_the_issue():
    assert {s[0] for s in _SHAPES} == {1, 3, 65} and {s[1] for s in _SHAPES} == {1, 2, 63, 64, 65, 128}
    assert {s[2] for s in _SHAPES} == {1, 2, 19, 64} and {s[3] for s in _SHAPES} == {4, 300}
    for n in (63, 64, 65, 128):                              # each pool size around the tile edge with both D
        assert {s[3] for s in _SHAPES if s[1] == n} == {4, 300}
    seen = _settings(128)
    assert {s[0] for s in seen} == {1, 128}
    assert {(s[2] != 0, s[6]) for s in seen} == {(False, False), (False, True), (True, True)}
    assert {s[0] for s in seen if s[2] == 0 and not s[6]} == {1, 128} == {s[0] for s in seen if s[2] != 0}


@pytest.mark.parametrize("B,N,S,D", _SHAPES)
def test_exact_sweep_rows_scores_objective_term_and_status_bits(B, N, S, D):
    table, idx, score, row_class, target, want_flags = _sweep_case(B, N, S, D)
    if N >= 12 and S >= 4:
        assert want_flags == (R.E_ROW | R.E_NAN | R.E_CLASS | R.E_TARGET)
    for k, lam, mu, gamma, sim, norm, with_table in _settings(N):
        k = min(k, N)
        got = _rerank(idx, score, table if with_table else None, row_class, target, k, lam, mu, gamma, sim, norm)
        # the python restatement of a long list is slow: in a large batch the full-length lists are compared for the users at both
        # ends of it (those with the edges among them), every user for the shorter ones; the prefix test below ties the two
        users = list(range(B)) if B * k <= 400 else [0, 1, 2, 3, B - 2, B - 1]
        want = _expected(B, N, S, D, users, k, lam, mu, gamma, sim, norm)
        where = (k, lam, mu, gamma, sim, norm, with_table)
        assert int(got[4]) == want_flags, (where, int(got[4]))
        assert C.same(got[0][users], want[0]) and C.same(got[1][users], want[1]), where
        assert C.same(got[2][users], want[2]) and C.same(got[3][users], want[3]), where
        if B >= 3:                                           # the all-empty user and the user with two live slots
            assert bool((got[0][1] == -1).all()) and all(bool(torch.isneginf(g[1]).all()) for g in got[1:4])
            assert int((got[0][2] >= 0).sum()) == min(k, 2)
        if B * k > 400:                                      # every user: the list of k is a prefix-extension of the list of 5
            short = _rerank(idx, score, table if with_table else None, row_class, target, 5, lam, mu, gamma, sim, norm)
            assert torch.equal(short[0], got[0][:, :5]) and all(torch.equal(C.bits(s), C.bits(g[:, :5])) for s, g in zip(short[1:4], got[1:4]))
            all5 = _expected(B, N, S, D, list(range(B)), 5, lam, mu, gamma, sim, norm)
            assert all(C.same(s, w) for s, w in zip(short[:4], all5))


# ---- 2. the flags, alone and together ---------------------------------------------------------------------------------------------------
def _flag_case():
    rng = np.random.default_rng(7)
    V, N, S, D, B = 50, 12, 5, 8, 2
    table = (rng.integers(-8, 9, (V, D)) / 8.0).astype(F)
    idx = np.stack([rng.permutation(V - 1)[:N] for _ in range(B)]).astype(np.int64)      # (row V - 1 is kept for the bad class)
    score = (np.arange(N, 0, -1)[None, :] / 8.0 + np.zeros((B, 1))).astype(F)               # descending: slot 0 is the best
    row_class = rng.integers(0, S, V).astype(np.int64)
    row_class[V - 1] = S
    target = rng.integers(0, 4, (B, S)).astype(F)
    return table, idx, score, row_class, target, V, N, S


_BREAK = {
    "row": lambda idx, score, target, V: idx.__setitem__((0, 3), V),
    "score": lambda idx, score, target, V: score.__setitem__((1, 5), np.inf),
    # the bad class sits on a slot whose score alone (4 against at most 1.375) wins step 0: it must still be selected first
    "class": lambda idx, score, target, V: (idx.__setitem__((0, 0), V - 1), score.__setitem__((0, 0), 4.0)),
    "target": lambda idx, score, target, V: target.__setitem__((1, 2), -1.0),
}
_BIT = {"row": R.E_ROW, "score": R.E_NAN, "class": R.E_CLASS, "target": R.E_TARGET}


@pytest.mark.parametrize("which", [(), ("row",), ("score",), ("class",), ("target",), ("row", "score", "class", "target")])
@pytest.mark.parametrize("mu", [0.0, 0.25])
def test_each_flag_alone_and_all_together(which, mu):
    table, idx, score, row_class, target, V, N, S = _flag_case()
    idx, score, target = idx.copy(), score.copy(), target.copy()
    idx[:, 6] = -1                                           # dead slots in the middle of the pool, so the live slots run out before k
    idx[1, 8] = -1
    for name in which:
        _BREAK[name](idx, score, target, V)
    want_flags = sum(_BIT[name] for name in which)
    assert want_flags == _flags_of(idx, score, row_class, target, V, S)
    got = _rerank(idx, score, table, row_class, target, N, 0.5, mu, 0.5, "cosine", False)
    assert int(got[4]) == want_flags
    for u in range(idx.shape[0]):
        want = R.cal_f32(idx[u], score[u], M.gram_f32(idx[u], table) if mu else None, V, row_class, target[u], N, 0.5, mu, 0.5, "cosine",
                         False)
        assert want[4] == (want_flags & _flags_of(idx[u:u + 1], score[u:u + 1], row_class, target[u:u + 1], V, S))
        assert all(C.same(g[u], w) for g, w in zip(got[:4], want[:4])), (which, mu, u)
        live = int((np.isfinite(score[u]) & (idx[u] >= 0) & (idx[u] < V)).sum())
        assert live < N and int((got[0][u] >= 0).sum()) == live and bool((got[0][u, live:] == -1).all())
        assert all(bool(torch.isneginf(g[u, live:]).all()) for g in got[1:4])
    if "class" in which:                                     # still selectable: 0.5 * 4 + 0 beats 0.5 * 1.375 + 0.5 * 1
        assert int(got[0][0, 0]) == V - 1 and float(got[3][0, 0]) == 0.0 and float(got[2][0, 0]) == 2.0


# ---- 3. general inputs: the kernel's own prefix is greedy in float64 ------------------------------------------------------------------------
V_GEN, B_GEN, K_GEN, S_GEN, D_GEN = 1000, 40, 20, 19, 300


def _general():
    """pools of 128 from ``ops.topk_scores`` over a non-grid table, classes in [1, S) (``aspect_metrics`` scores a list 0 when its
    class ids sum to 0), ragged histories and their integer class counts as the target"""
    if "general" not in _CACHE:
        from newsreclib_amd import ops
        g = torch.Generator().manual_seed(0)
        table = torch.randn(V_GEN, D_GEN, generator=g)
        users = torch.randn(B_GEN, D_GEN, generator=g)
        row_class = torch.randint(1, S_GEN, (V_GEN,), generator=g)
        sizes = torch.randint(1, 30, (B_GEN,), generator=g)
        hist = torch.randint(0, V_GEN, (int(sizes.sum()),), generator=g)
        off = torch.cat([torch.zeros(1, dtype=torch.int64), sizes.cumsum(0)])
        idx, score, status = ops.topk_scores(users.cuda(), table.cuda(), 128)
        assert int(status) == 0
        target = ops.class_targets(hist.cuda(), off.cuda(), row_class.cuda(), S_GEN)
        counts = np.stack([np.bincount(row_class[hist[off[u]:off[u + 1]]].numpy(), minlength=S_GEN) for u in range(B_GEN)])
        assert np.array_equal(target.cpu().numpy(), counts.astype(F))
        _CACHE["general"] = (table, idx, score, row_class, target, hist, off)
    return _CACHE["general"]


@pytest.mark.parametrize("lam,mu,gamma", [(0.5, 0.25, 0.5), (0.3, 0.7, 1.0), (1.0, 0.0, 0.5), (0.0, 1.0, 1.0)])
def test_general_inputs_follow_the_float64_objective(lam, mu, gamma):
    table, idx, score, row_class, target, _, _ = _general()
    # MMR's bound times the objective's scale: rel in [0, 1], |cos| <= 1, cal in [0, 1]
    tol = (D_GEN + 16) * 2.0 ** -23 * max(1.0, lam + mu + gamma)
    got = _rerank(idx, score, table, row_class, target, K_GEN, lam, mu, gamma)
    assert int(got[4]) == 0 and bool((got[0] >= 0).all())
    pool, pool_score, rows = idx.cpu().numpy(), score.cpu().numpy(), got[0].cpu().numpy()
    obj, cal = got[2].cpu().numpy().astype(np.float64), got[3].cpu().numpy().astype(np.float64)
    rc, tg, tb = row_class.numpy(), target.cpu().numpy(), table.numpy()
    worst_gap = worst_err = worst_cal = 0.0
    for u in range(B_GEN):
        slots = [int(np.nonzero(pool[u] == r)[0][0]) for r in rows[u]]
        assert len(set(slots)) == K_GEN
        assert np.array_equal(got[1][u].cpu().numpy(), pool_score[u][slots])
        ref = R.cal_f64(pool[u], pool_score[u], tb, V_GEN, rc, tg[u], K_GEN, lam, mu, gamma, forced=slots)
        for t, (c, o) in enumerate(ref[5]):                  # every step, none exempt
            worst_gap, worst_err = max(worst_gap, float(np.nanmax(o) - o[c])), max(worst_err, abs(obj[u, t] - o[c]))
        worst_cal = max(worst_cal, float(np.abs(cal[u] - ref[3]).max()))
    print(f"lambda={lam} mu={mu} gamma={gamma}: largest float64 gap to the maximum {worst_gap:.3e}, largest |obj - objective| "
          f"{worst_err:.3e}, largest |cal - term| {worst_cal:.3e}, tol {tol:.3e}")
    assert worst_gap <= tol and worst_err <= tol and worst_cal <= tol


# ---- 4. the header's properties on the device -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lam", [0.3, 0.5])
def test_property_3_gamma_zero_is_mmr_rerank(lam):
    from newsreclib_amd import ops
    table, idx, score, row_class, target, _, _ = _general()
    table = table.cuda()
    for sim, norm in (("cosine", True), ("dot", False)):
        want = ops.mmr_rerank(idx, score, table, K_GEN, lam, sim, norm)
        got = ops.calibrated_rerank(idx, score, table, row_class.cuda(), target, K_GEN, lam, float(F(1) - F(lam)), 0.0, sim, norm)
        assert int(got[4]) == 0 == int(want[3])
        assert torch.equal(got[0], want[0]) and torch.equal(C.bits(got[1]), C.bits(want[1]))
        assert torch.equal(got[2], want[2])                  # (compares equal: a -0 there may be +0 here)


def test_property_4_lambda_one_alone_returns_the_pool_of_topk_scores():
    from newsreclib_amd import ops
    table, idx, score, row_class, target, _, _ = _general()
    for tbl in (None, table.cuda()):
        got = ops.calibrated_rerank(idx, score, tbl, row_class.cuda(), target, K_GEN, 1.0, 0.0, 0.0, "cosine", False)
        assert int(got[4]) == 0 and torch.equal(got[0], idx[:, :K_GEN]) and torch.equal(C.bits(got[1]), C.bits(score[:, :K_GEN]))
        assert torch.equal(got[2], score[:, :K_GEN])


@pytest.mark.parametrize("mu", [0.0, 0.25])
def test_property_5_the_last_term_is_personalization_at_k(mu):
    from newsreclib_amd.metrics import aspect_metrics
    table, idx, score, row_class, target, hist, off = _general()
    k = 10
    got = _rerank(idx, score, table, row_class, target, k, 0.5, mu, 0.5)
    assert int(got[4]) == 0 and bool((got[0] >= 0).all())
    rows, tg, rc = got[0].cpu(), target.cpu().numpy(), row_class.numpy()
    last = got[3][:, k - 1].cpu().numpy()
    for u in range(B_GEN):
        want = R.count_formula(rc[rows[u].numpy()], tg[u])
        assert last[u].tobytes() == F(want).tobytes(), u
    classes = row_class[rows]
    assert bool((classes > 0).all())
    # the lists as one impression each, scored in their own order
    order_scores = torch.arange(k, 0, -1).float().repeat(B_GEN)
    pers = aspect_metrics(order_scores, classes.reshape(-1), row_class[hist], torch.full((B_GEN,), k), off[1:] - off[:-1], S_GEN, (k,))
    assert abs(pers[f"categ_pers@{k}"] - float(last.astype(np.float64).mean())) <= 1e-6
    first = aspect_metrics(order_scores, row_class[idx[:, :k].cpu()].reshape(-1), row_class[hist], torch.full((B_GEN,), k),
                           off[1:] - off[:-1], S_GEN, (k,))
    print(f"mu={mu}: categ_pers@{k} of the pool's first {k}: {first[f'categ_pers@{k}']:.4f}; calibrated at gamma 0.5: "
          f"{pers[f'categ_pers@{k}']:.4f}")


def test_prefix_batch_composition_and_engine():
    from newsreclib_amd import _lib, ops
    table, idx, score, row_class, target, _, _ = _general()
    table, row_class = table.cuda(), row_class.cuda()
    for tbl, mu in ((table, 0.25), (None, 0.0)):
        full = ops.calibrated_rerank(idx, score, tbl, row_class, target, K_GEN, 0.5, mu, 0.5)
        part = ops.calibrated_rerank(idx, score, tbl, row_class, target, 5, 0.5, mu, 0.5)
        assert all(torch.equal(C.bits(p), C.bits(f[:, :5])) for p, f in zip(part[:4], full[:4]))
        # a user alone, and inside a batch of 130 at another place
        rep = lambda x: x.repeat(4, 1)[:130].contiguous()  # noqa: E731
        big = ops.calibrated_rerank(rep(idx), rep(score), tbl, row_class, rep(target), K_GEN, 0.5, mu, 0.5)
        alone = ops.calibrated_rerank(idx[7:8].contiguous(), score[7:8].contiguous(), tbl, row_class, target[7:8].contiguous(), K_GEN,
                                      0.5, mu, 0.5)
        for u in (7, 47, 87, 127):
            assert all(torch.equal(C.bits(a[0]), C.bits(b[u])) for a, b in zip(alone[:4], big[:4]))
        assert all(torch.equal(C.bits(b[:B_GEN]), C.bits(f)) for b, f in zip(big[:4], full[:4]))
        prev = _lib.get_gemm_engine()
        try:
            for name in ("f32", "bf16x3"):
                _lib.set_gemm_engine(name)
                again = ops.calibrated_rerank(idx, score, tbl, row_class, target, K_GEN, 0.5, mu, 0.5)
                assert all(torch.equal(C.bits(a), C.bits(f)) for a, f in zip(again[:4], full[:4])), name
        finally:
            _lib.set_gemm_engine(prev)
    # int32 classes are taken as they are, int64 converted: the same lists
    a = ops.calibrated_rerank(idx, score, None, row_class.int(), target, 5, 0.5, 0.0, 0.5)
    assert all(torch.equal(C.bits(x), C.bits(y)) for x, y in zip(a[:4], part[:4]))


def test_bad_arguments_are_refused_before_any_launch():
    from newsreclib_amd import ops
    idx, score = torch.zeros(2, 8, dtype=torch.int64).cuda(), torch.zeros(2, 8).cuda()
    table, cls, tgt = torch.zeros(9, 4).cuda(), torch.zeros(9, dtype=torch.int32).cuda(), torch.tensor([[1.0, 0.0, 0.0]] * 2).cuda()
    for call in (lambda: ops.calibrated_rerank(idx.int(), score, table, cls, tgt, 3, 0.5, 0.5, 0.5),
                 lambda: ops.calibrated_rerank(idx, score, table, cls, tgt[:1], 3, 0.5, 0.5, 0.5),
                 lambda: ops.calibrated_rerank(idx, score, table, cls, tgt, 9, 0.5, 0.5, 0.5),
                 lambda: ops.calibrated_rerank(idx, score, table, cls, tgt, 3, 0.5, 0.5, 1.5),
                 lambda: ops.calibrated_rerank(idx, score, None, cls, tgt, 3, 0.5, 0.5, 0.5)):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(RuntimeError, match=r"calibrated_rerank: with mu != 0, D a multiple of 4"):
        ops.calibrated_rerank(idx, score, torch.zeros(9, 6).cuda(), cls, tgt, 3, 0.5, 0.5, 0.5)
    torch.cuda.synchronize()                                 # nothing was launched: nothing can have gone wrong on the device
    # mu == 0: D is not looked at; all slots are row 0 of class 0, target (1, 0, 0): the term is 1/1, 1/2, 1/3
    out = ops.calibrated_rerank(idx, score, torch.zeros(9, 6).cuda(), cls, tgt, 3, 0.5, 0.0, 1.0)
    assert int(out[4]) == 0 and out[0].tolist() == [[0, 0, 0]] * 2
    assert out[3].tolist() == [[1.0, 0.5, float(F(1) / F(3))]] * 2 and torch.equal(out[2], out[3])
    # an empty table: every slot with a row is flagged and dead
    out = ops.calibrated_rerank(idx, score, None, torch.zeros(0, dtype=torch.int32).cuda(), tgt, 3, 0.5, 0.0, 0.5)
    assert int(out[4]) == R.E_ROW and bool((out[0] == -1).all()) and bool(torch.isneginf(out[3]).all())


def test_calibrated_rerank_and_class_targets_do_not_synchronise_with_the_host():
    from newsreclib_amd import ops
    table, idx, score, row_class, _, hist, off = _general()
    table, row_class, hist, off = table.cuda(), row_class.cuda(), hist.cuda(), off.cuda()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        if not C.sync_debug_honoured():
            pytest.skip("this torch build does not raise on synchronising calls under set_sync_debug_mode('error')")
        target = ops.class_targets(hist, off, row_class, S_GEN)
        quota = ops.class_targets(hist, off, row_class, S_GEN, k=10)
        out = ops.calibrated_rerank(idx, score, table, row_class, target, 10, 0.5, 0.25, 0.5)
        short = ops.calibrated_rerank(idx[:, :40].contiguous(), score[:, :40].contiguous(), None, row_class, quota, 10, 0.7, 0.0, 0.3,
                                      "dot", False)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert int(out[4]) == 0 and out[0].shape == (B_GEN, 10) and int(short[4]) == 0 and short[3].shape == (B_GEN, 10)
    assert float((quota.sum(1) - 10.0).abs().max()) < 1e-4


# ---- 5. modules -----------------------------------------------------------------------------------------------------------------------------
def _listed(recs, users, idx, score):
    for b, u in enumerate(users):
        name = f"U{u['user_id']}"
        assert list(recs[name]) == [f"N{int(i)}" for i in idx[b] if i >= 0], b
        assert list(recs[name].values()) == [float(s) for s, i in zip(score[b], idx[b]) if i >= 0], b


def test_recommend_users_calibrates_an_nrms_cache():
    from newsreclib_amd import ops
    from newsreclib_amd.evaluation import DeviceNewsTable, NewsVectorCache, recommend_users
    mod, attrs = builders.tiny("nrms", n_news=200)
    cache = NewsVectorCache(mod, DeviceNewsTable(attrs), chunk=64)
    V, B, k = 200, 6, 10
    lists, hist, hs, _ = builders.hist_batch(V)
    off = torch.cat([torch.zeros(1, dtype=torch.int64), hs.cumsum(0)]).cuda()
    users = [{"hist": lists[b], "user_id": 100 + b} for b in range(B)]
    plain = recommend_users(cache, users, k, batch_size=B)
    assert recommend_users(cache, users, k, batch_size=B, calibrate=None) == plain
    pool_idx, pool_score, status = cache.recommend(hist.cuda(), hs, 64)
    assert int(status) == 0
    categ = cache.table.attrs["category"]
    for how, scale in (("history", None), ("proportional", k)):
        for lam, mu in ((1.0, 0.0), (0.5, 0.25)):
            target = ops.class_targets(hist.cuda(), off, categ, ops.CAL_MAX_CLASSES, scale)
            want = ops.calibrated_rerank(pool_idx, pool_score, cache.vectors, categ, target, k, lam, mu, 0.5, "cosine", True)
            by_hand = cache.rerank_calibrated(pool_idx, pool_score, k, "category", target, lam, mu, 0.5)
            assert int(want[4]) == 0 and all(torch.equal(C.bits(a), C.bits(b)) for a, b in zip(by_hand[:4], want[:4]))
            with warnings.catch_warnings():
                warnings.filterwarnings("error", message="recommend_users")       # a clean batch says nothing
                recs = recommend_users(cache, users, k, batch_size=B, calibrate=dict(pool=64, aspect="category", gamma=0.5, lam=lam,
                                                                                    mu=mu, target=how))
            _listed(recs, users, want[0].cpu(), want[1].cpu())
    target = ops.class_targets(hist.cuda(), off, categ, ops.CAL_MAX_CLASSES)
    want = cache.rerank_calibrated(pool_idx, pool_score, k, "category", target, 1.0, 0.0, 0.5)
    assert not torch.equal(want[0], pool_idx[:, :k])         # (the term changed some list)
    # in two batches, each composed by hand (NRMS' seq-first user attention couples the users of a batch, so the pools are the
    # batch's own): every user's target is its own
    recs = recommend_users(cache, users, k, batch_size=4, calibrate=dict(pool=64, aspect="category", gamma=0.5))
    for lo, hi in ((0, 4), (4, B)):
        part_idx, part_score, _ = cache.recommend(torch.cat(lists[lo:hi]).cuda(), hs[lo:hi], 64)
        part = cache.rerank_calibrated(part_idx, part_score, k, "category", target[lo:hi].contiguous(), 1.0, 0.0, 0.5)
        _listed(recs, users[lo:hi], part[0].cpu(), part[1].cpu())
    # together with a class cap: the capped method produces the pool
    capped = recommend_users(cache, users, k, batch_size=B, cap=("category", 5), calibrate=dict(pool=64, aspect="category", gamma=0.5))
    cap_idx, cap_score, _ = cache.recommend_capped(hist.cuda(), hs, 64, "category", 5)
    cap_want = cache.rerank_calibrated(cap_idx, cap_score, k, "category", target, 1.0, 0.0, 0.5)
    _listed(capped, users, cap_want[0].cpu(), cap_want[1].cpu())
    with pytest.raises(ValueError, match="exclude each other"):
        recommend_users(cache, users, k, diversify=(64, 0.5), calibrate=dict(pool=64, aspect="category", gamma=0.5))
    # a flagged batch warns in the words of CAL_FLAGS: a class id beyond the classes the target holds
    attrs2 = dict(attrs, category=attrs["category"].clone())
    attrs2["category"][::3] = ops.CAL_MAX_CLASSES + 6
    flagged = NewsVectorCache(mod, DeviceNewsTable(attrs2), chunk=64)
    with pytest.warns(UserWarning, match="class id outside"):
        recs = recommend_users(flagged, users, k, batch_size=B, calibrate=dict(pool=64, aspect="category", gamma=0.5))
    assert all(len(recs[f"U{100 + b}"]) == k for b in range(B))


def test_recommend_users_calibrates_a_manner_cache(tmp_path):
    from newsreclib_amd import ops
    from newsreclib_amd.evaluation import MannerVectorCache, recommend_users
    cr, ac, asent = builders.manner_modules(tmp_path)
    table, imps = builders.manner_table_and_impressions()
    cache = MannerVectorCache(builders.manner_ensemble(cr, ac, asent), table)
    lists = [i["hist"] for i in imps]
    hs, hist = torch.tensor([len(x) for x in lists]), torch.cat(lists)
    off = torch.cat([torch.zeros(1, dtype=torch.int64), hs.cumsum(0)]).cuda()
    B, k, pool = len(imps), 5, 16
    idx, score, status = cache.recommend_ensemble(hist.cuda(), hs, pool)
    assert int(status) == 0 and len(cache.vectors) >= 2
    target = ops.class_targets(hist.cuda(), off, table.attrs["sentiment"], ops.CAL_MAX_CLASSES)
    for s in (0, 1):
        got = cache.rerank_calibrated(idx, score, k, "sentiment", target, 0.5, 0.25, 0.5, which=s)
        want = ops.calibrated_rerank(idx, score, cache.vectors[s], table.attrs["sentiment"], target, k, 0.5, 0.25, 0.5)
        assert int(got[4]) == 0 and all(torch.equal(C.bits(a), C.bits(b)) for a, b in zip(got[:4], want[:4]))
    first = cache.rerank_calibrated(idx, score, k, "sentiment", target, 0.5, 0.25, 0.5)
    users = [{"hist": lists[b], "user_id": 100 + b} for b in range(B)]
    recs = recommend_users(cache, users, k, batch_size=B + 3, calibrate=dict(pool=pool, aspect="sentiment", gamma=0.5, lam=0.5, mu=0.25))
    _listed(recs, users, first[0].cpu(), first[1].cpu())


def test_recommend_users_calibrates_an_npa_cache_without_vectors():
    from newsreclib_amd import ops
    from newsreclib_amd.evaluation import recommend_users
    mod, table = builders.tiny_npa()
    V, B, k = 50, 6, 5
    table.attrs["category"] = torch.randint(1, 7, (V,), generator=torch.Generator().manual_seed(9)).cuda()
    cache = mod.feature_cache(table)
    lists, hist, hs = builders.hist_batch(V, sizes=[4] * B)[:3]
    off = torch.cat([torch.zeros(1, dtype=torch.int64), hs.cumsum(0)]).cuda()
    uidx = torch.tensor([3, 1, 4, 1, 5, 8])
    idx, score, status = cache.recommend_pooled(hist.cuda(), hs, 20, user_idx=uidx)
    assert int(status) == 0
    target = ops.class_targets(hist.cuda(), off, table.attrs["category"], ops.CAL_MAX_CLASSES)
    want = ops.calibrated_rerank(idx, score, None, table.attrs["category"], target, k, 1.0, 0.0, 0.5)
    got = cache.rerank_calibrated(idx, score, k, "category", target, 1.0, 0.0, 0.5)
    assert int(want[4]) == 0 and all(torch.equal(C.bits(a), C.bits(b)) for a, b in zip(got[:4], want[:4]))
    users = [{"hist": lists[b], "user_id": 100 + b, "user_idx": uidx[b]} for b in range(B)]
    recs = recommend_users(cache, users, k, batch_size=B, calibrate=dict(pool=20, aspect="category", gamma=0.5))
    _listed(recs, users, want[0].cpu(), want[1].cpu())
    with pytest.raises(ValueError, match="mu == 0 only"):
        recommend_users(cache, users, k, batch_size=B, calibrate=dict(pool=20, aspect="category", gamma=0.5, mu=0.25))
    with pytest.raises(ValueError, match="mu == 0 only"):
        cache.rerank_calibrated(idx, score, k, "category", target, 0.5, 0.25, 0.5)
