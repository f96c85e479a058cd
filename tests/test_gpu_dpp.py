"""Greedy DPP re-ranking of top-k pools (``nrl_dpp_rerank``, ``ops.dpp_rerank``, ``*Cache.rerank_dpp``,
``recommend_users(dpp=...)``).

Expected values come from ``tests/dpp_ref.py``.  The exact cases use table entries, scores and qualities that are multiples of 1/8:
the Gram matrix is exact, so the float32 restatement of the recurrence, fed that matrix and those qualities, must reproduce rows,
scores, gains and status bit for bit -- every operation behind them is a single correctly rounded one on both sides.  With D = 4 a
pool has rank 4: the lists run into rounding-noise d2 values and the fill phase, which is where bit equality is hardest.  The
real-valued cases check the kernel's own prefix against the float64 definition under a tolerance worked out from D and from the
error the restatement itself shows against the definition."""
import warnings

import numpy as np
import pytest
import torch

from tests import builders
from tests import catalogue_ref as C
from tests import dpp_ref as R

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


def _rerank(idx, score, table, k, alpha=1.0, similarity="cosine", normalize=True, quality=None, eps=1e-4):
    from newsreclib_amd import ops
    return ops.dpp_rerank(_dev(idx), _dev(score), _dev(table), k, alpha, similarity, normalize, _dev(quality), eps)


# ---- 1. the exact sweep ---------------------------------------------------------------------------------------------------------------------
V_SWEEP = 200
_CACHE = {}
_SHAPES = [(1, 1, 4), (3, 2, 300), (1, 63, 4), (3, 64, 300), (3, 65, 4), (1, 127, 300), (130, 128, 4), (3, 128, 300), (130, 9, 300)]


def _sweep_case(B, N, D):
    """The pools of the MMR sweep, edge for edge -- user 0 carries an empty slot in the middle and one at the tail, the rows V and
    -2, a NaN and a +inf score, a duplicated row and the zero row; user 1 is all empty; user 2 has two live slots; the eighth-grid
    scores tie everywhere -- and an eighth-grid quality in [0, 2] per slot: user 0 has a zero, a negative, a NaN and a +inf entry
    where N has room, a bad entry in its empty middle slot (not read: no flag) and zeros are scattered over every user."""
    key = ("case", B, N, D)
    if key not in _CACHE:
        rng = np.random.default_rng(1000 * B + 10 * N + D)
        table = (rng.integers(-16, 17, (V_SWEEP, D)) / 8.0).astype(F)
        table[0] = 0.0
        idx = rng.integers(0, V_SWEEP, (B, N))
        score = (rng.integers(-16, 17, (B, N)) / 8.0).astype(F)
        quality = (rng.integers(0, 17, (B, N)) / 8.0).astype(F)
        edges = [("mid", 1, -1), ("row", 2, V_SWEEP), ("row", 3, -2), ("nan", 4, np.nan), ("inf", 5, np.inf), ("dup", 6, None),
                 ("zero", 8, 0), ("q", 9, 0.0), ("q", 10, -0.125), ("q", 11, np.nan), ("q", 12, np.inf), ("tail", N - 1, -1)]
        for kind, slot, value in edges:
            if slot >= N or (kind != "tail" and slot == N - 1) or N < 2:
                continue
            if kind in ("mid", "tail", "row", "zero"):
                idx[0, slot] = value
            elif kind == "dup":
                idx[0, slot + 1 if slot + 1 < N - 1 else slot] = idx[0, slot]
            elif kind == "q":
                quality[0, slot] = value
            else:
                score[0, slot] = value
        if N > 2:
            quality[0, 1] = np.nan                          # in an empty slot: never read
        if B >= 3:
            idx[1, :] = -1
            idx[2, 2:] = -1
        _CACHE[key] = (table, idx.astype(np.int64), score, quality)
    return _CACHE[key]


def _expected(B, N, D, sim, eps):
    """every user's list of min(N, 64), its flags without the fill flag, and the step its fill phase starts at: the lists for a
    smaller k are prefixes (tests/test_dpp_host.py shows that of the restatement)"""
    key = ("want", B, N, D, sim, eps)
    if key not in _CACHE:
        table, idx, score, quality = _sweep_case(B, N, D)
        k = min(N, 64)
        outs = [R.dpp_f32(idx[u], score[u], R.gram_f32(idx[u], table), V_SWEEP, k, quality[u], eps, sim) for u in range(B)]
        fill = [next((t for t, s in enumerate(o[4]) if not s[2]), k) for o in outs]
        _CACHE[key] = (tuple(np.stack([o[j] for o in outs]) for j in range(3)), [o[3] & ~R.E_RANK for o in outs], fill)
    return _CACHE[key]


def test_the_sweep_covers_the_shapes_and_the_edges_of_the_issue():
    assert {s[0] for s in _SHAPES} == {1, 3, 130} and {s[1] for s in _SHAPES} >= {1, 2, 63, 64, 65, 127, 128}
    assert {s[2] for s in _SHAPES} == {4, 300}
    table, idx, score, quality = _sweep_case(130, 128, 4)
    assert (idx[0] == -1).sum() >= 2 and V_SWEEP in idx[0] and -2 in idx[0] and np.isnan(score[0]).any() and np.isinf(score[0]).any()
    assert idx[0, 6] == idx[0, 7] and idx[0, 8] == 0 and not table[0].any() and (idx[1] == -1).all() and (idx[2, 2:] == -1).all()
    assert quality[0, 9] == 0 and quality[0, 10] < 0 and np.isnan(quality[0, 11]) and np.isinf(quality[0, 12])
    (_, _, gain), flags, fill = _expected(130, 128, 4, "cosine", 1e-4)
    assert flags[0] == R.E_ROW | R.E_NAN | R.E_QUALITY and not any(flags[1:])
    # D = 4: every pool runs out of rank after at most 4 steps, and what is left of d2 then is rounding noise, not zero
    assert fill[0] <= 4 and all(3 <= f <= 4 for f in fill[3:])
    # with eps = 0 a noise d2 above zero is still a gain: some lists go on past the rank, by gains around 2^-22 of L_ii
    (_, _, gain0), _, fill0 = _expected(130, 128, 4, "cosine", 0.0)
    late = [float(gain0[u, t]) for u in range(3, 130) for t in range(4, fill0[u])]
    assert len(late) >= 10 and 0 < min(late) and max(late) < 1e-5 * 4.0       # (L_ii = q_i^2 <= 4 under cosine)


@pytest.mark.parametrize("B,N,D", _SHAPES)
def test_exact_sweep_rows_scores_gains_and_status_bits(B, N, D):
    table, idx, score, quality = _sweep_case(B, N, D)
    for sim in ("cosine", "dot"):
        for eps in (0.0, 1e-4):
            (w_idx, w_score, w_gain), flags, fill = _expected(B, N, D, sim, eps)
            for k in sorted({1, min(5, N), min(N, 64)}):
                got_idx, got_score, got_gain, status = _rerank(idx, score, table, k, 1.0, sim, True, quality, eps)
                want_status = 0
                for u in range(B):
                    listed = int((w_idx[u, :k] >= 0).sum())
                    want_status |= flags[u] | (R.E_RANK if fill[u] < listed else 0)
                assert int(status) == want_status, (k, sim, eps, int(status), want_status)
                assert C.same(got_idx, np.ascontiguousarray(w_idx[:, :k])), (k, sim, eps)
                assert C.same(got_score, np.ascontiguousarray(w_score[:, :k])), (k, sim, eps)
                assert C.same(got_gain, np.ascontiguousarray(w_gain[:, :k])), (k, sim, eps)
                if B >= 3:                                   # the all-empty user and the user with two live slots
                    assert bool((got_idx[1] == -1).all()) and bool(torch.isneginf(got_score[1]).all())
                    assert bool(torch.isneginf(got_gain[1]).all()) and int((got_idx[2] >= 0).sum()) == min(k, 2)
    if N >= 13:
        assert flags[0] == R.E_ROW | R.E_NAN | R.E_QUALITY


def test_the_hand_worked_pools():
    table = np.zeros((4, 4), dtype=F)
    table[1], table[2], table[3] = [2, 0, 0, 0], [0, 0, 2, 0], [2, 0, 2, 0]
    ones = np.ones((1, 3), dtype=F)
    # rows [a, a, b], a orthogonal to b, cosine, q = 1: slots 0, 2, then the duplicate as a fill with gain +0
    idx, score = np.array([[1, 1, 2]], dtype=np.int64), np.array([[1.0, 3.0, 2.0]], dtype=F)
    for eps in (0.0, 1e-4):
        got = _rerank(idx, score, table, 3, quality=ones, eps=eps)
        assert got[0].tolist() == [[1, 2, 1]] and got[1].tolist() == [[1.0, 2.0, 3.0]] and got[2].tolist() == [[1.0, 1.0, 0.0]]
        assert int(got[3]) == R.E_RANK and not bool(torch.signbit(got[2][0, 2]))
    assert int(_rerank(idx, score, table, 2, quality=ones)[3]) == 0
    # rows [a, b, a + b], dot: the pool has rank 2, the third listed news is a fill
    idx = np.array([[1, 2, 3]], dtype=np.int64)
    got = _rerank(idx, score, table, 3, similarity="dot", quality=ones)
    want = R.dpp_f32(idx[0], score[0], R.gram_f32(idx[0], table), 4, 3, ones[0], 1e-4, "dot")
    assert got[0].tolist() == [[3, 1, 2]] and int(got[3]) == R.E_RANK and C.same(got[2][0], want[2]) and float(got[2][0, 2]) == 0.0
    # the zero row is only ever a fill, whatever its score
    idx, score = np.array([[0, 1, 2]], dtype=np.int64), np.array([[9.0, 1.0, 2.0]], dtype=F)
    got = _rerank(idx, score, table, 3, quality=ones)
    assert got[0].tolist() == [[1, 2, 0]] and got[2].tolist() == [[1.0, 1.0, 0.0]] and int(got[3]) == R.E_RANK


# ---- 2. general inputs: the kernel's own prefix is greedy in float64 ------------------------------------------------------------------------
V_GEN, B_GEN, K_GEN = 1000, 40, 20


def _general(D):
    key = ("general", D)
    if key not in _CACHE:
        from newsreclib_amd import ops
        g = torch.Generator().manual_seed(0)
        table = torch.randn(V_GEN, D, generator=g)
        users = torch.randn(B_GEN, D, generator=g)
        idx, score, status = ops.topk_scores(users.cuda(), table.cuda(), 128)
        assert int(status) == 0
        _CACHE[key] = (table, idx, score)
    return _CACHE[key]


def _recurrence_error(idx, score, table, k, alpha):
    """From the restatements alone, on the CPU: the worst error of the float32 recurrence's DPP-phase gains against the float64
    definition along the same list, relative to the user's largest L_ii, over the pools (idx, score) of ``table``."""
    r = 0.0
    for u in range(idx.shape[0]):
        L, live, flags, q = R.kernel_matrix_f64(idx[u], score[u], table, None, alpha)
        if not live.any():
            continue
        ok = (idx[u] >= 0) & (idx[u] < table.shape[0])
        rows = table[np.where(ok, idx[u], 0)].astype(np.float64) * ok[:, None]
        a = R.dpp_f32(idx[u], score[u], (rows @ rows.T).astype(F), table.shape[0], k, q.astype(F))
        slots = [s[0] for s in a[4] if s[2]]
        b = R.dpp_f64(idx[u], score[u], table, len(slots), None, alpha, forced=slots)
        if slots:
            r = max(r, float(np.abs(a[2][:len(slots)].astype(np.float64) - b[2]).max()) / float(np.diagonal(L)[live].max()))
    return r


def _reference(D, alpha):
    """From the restatements alone, on the CPU: r (``_recurrence_error``) and the number of float64 steps whose runner-up is
    within the tolerance that r gives."""
    key = ("ref", D, alpha)
    if key not in _CACHE:
        table, idx, score = _general(D)
        table, idx, score = table.numpy(), idx.cpu().numpy(), score.cpu().numpy()
        r = _recurrence_error(idx, score, table, K_GEN, alpha)
        per_user = []
        for u in range(B_GEN):
            L, live, flags, _ = R.kernel_matrix_f64(idx[u], score[u], table, None, alpha)
            assert flags == 0 and live.all()
            steps = R.dpp_f64(idx[u], score[u], table, K_GEN, None, alpha)[4]
            assert len(steps) == K_GEN and all(s[2] for s in steps)
            per_user.append((L, float(np.diagonal(L).max()), steps))
        ties = 0
        for L, lmax, steps in per_user:
            tol = ((D + 16) * 2.0 ** -23 + 4 * r) * lmax
            for c, gains, _ in steps:
                ties += bool(np.nanmax(np.delete(gains, c)) >= gains[c] - tol)
        _CACHE[key] = (r, ties, [(L, lmax) for L, lmax, _ in per_user])
    return _CACHE[key]


@pytest.mark.parametrize("alpha", [1.0, 3.0])
@pytest.mark.parametrize("D", [32, 300])
def test_general_inputs_follow_the_float64_definition(D, alpha):
    table, idx, score = _general(D)
    r, ties, per_user = _reference(D, alpha)
    # the condition on the inputs, on the reference alone: near-ties are rare, so the check below is in effect an equality check
    print(f"D={D} alpha={alpha}: r = {r:.3e}; {ties} of {B_GEN * K_GEN} reference steps have a runner-up within tol")
    assert ties < 0.02 * B_GEN * K_GEN
    got_idx, got_score, got_gain, status = _rerank(idx, score, table, K_GEN, alpha)
    assert int(status) == 0 and bool((got_idx >= 0).all())
    pool, pool_score, rows = idx.cpu().numpy(), score.cpu().numpy(), got_idx.cpu().numpy()
    gain = got_gain.cpu().numpy().astype(np.float64)
    worst_gap = worst_err = worst_det = 0.0                  # each relative to its own bound
    for u in range(B_GEN):
        L, lmax = per_user[u]
        tol = ((D + 16) * 2.0 ** -23 + 4 * r) * lmax         # MMR's Gram bound + the recurrence (x 4: expf, the MFMA's summation order)
        slots = [int(np.nonzero(pool[u] == x)[0][0]) for x in rows[u]]
        assert len(set(slots)) == K_GEN and np.array_equal(got_score[u].cpu().numpy(), pool_score[u][slots])
        steps = R.dpp_f64(pool[u], pool_score[u], table.numpy(), K_GEN, None, alpha, forced=slots)[4]
        for t, (c, g, _) in enumerate(steps):
            worst_gap, worst_err = max(worst_gap, float(np.nanmax(g) - g[c]) / tol), max(worst_err, abs(gain[u, t] - g[c]) / tol)
            sign, logdet = np.linalg.slogdet(L[np.ix_(slots[:t + 1], slots[:t + 1])])
            bound = (t + 1) * tol / gain[u, :t + 1].min()
            worst_det = max(worst_det, abs(np.log(gain[u, :t + 1]).sum() - logdet) / bound)
            assert sign > 0
    print(f"D={D} alpha={alpha}: as fractions of their bounds: largest float64 gap to the best gain {worst_gap:.3f}, largest "
          f"|out_gain - gain| {worst_err:.3f}, largest |sum log gain - logdet| {worst_det:.3f}; tol / max L_ii = "
          f"{(D + 16) * 2.0 ** -23 + 4 * r:.3e}")
    assert worst_gap <= 1.0 and worst_err <= 1.0 and worst_det <= 1.0


@pytest.mark.parametrize("alpha", [1.0, 3.0])
def test_a_given_quality_lists_the_rows_of_the_alpha_path(alpha):
    table, idx, score = _general(300)
    lo, hi = score.min(dim=1, keepdim=True).values, score.max(dim=1, keepdim=True).values
    quality = torch.exp(alpha * ((score - lo) / (hi - lo)))
    by_alpha = _rerank(idx, score, table, K_GEN, alpha)
    by_quality = _rerank(idx, score, table, K_GEN, 0.0, "cosine", False, quality)         # (alpha and normalize are not used)
    assert int(by_alpha[3]) == 0 and int(by_quality[3]) == 0
    assert torch.equal(by_alpha[0], by_quality[0]) and torch.equal(C.bits(by_alpha[1]), C.bits(by_quality[1]))
    assert torch.allclose(by_alpha[2], by_quality[2], rtol=1e-5, atol=0)
    # and the scores matter: alpha = 0 lists other rows
    assert not torch.equal(_rerank(idx, score, table, K_GEN, 0.0)[0], by_alpha[0])


# ---- 3. invariance and entry ----------------------------------------------------------------------------------------------------------------
def test_prefix_batch_composition_and_engine():
    from newsreclib_amd import _lib, ops
    table, idx, score = _general(300)
    table = table.cuda()
    full = ops.dpp_rerank(idx, score, table, K_GEN, 1.0)
    part = ops.dpp_rerank(idx, score, table, 5, 1.0)
    assert all(torch.equal(C.bits(p), C.bits(f[:, :5])) for p, f in zip(part[:3], full[:3]))
    long = ops.dpp_rerank(idx, score, table, 64, 1.0)       # the largest layout: two tiles and 64 Cholesky rows
    assert all(torch.equal(C.bits(f), C.bits(g[:, :K_GEN])) for f, g in zip(full[:3], long[:3])) and int(long[3]) == 0
    # a user alone, and inside a batch of 130 at another place
    big_idx, big_score = idx.repeat(4, 1)[:130].contiguous(), score.repeat(4, 1)[:130].contiguous()
    big = ops.dpp_rerank(big_idx, big_score, table, K_GEN, 1.0)
    alone = ops.dpp_rerank(idx[7:8].contiguous(), score[7:8].contiguous(), table, K_GEN, 1.0)
    for u in (7, 47, 87, 127):
        assert all(torch.equal(C.bits(a[0]), C.bits(b[u])) for a, b in zip(alone[:3], big[:3]))
    assert all(torch.equal(C.bits(b[:B_GEN]), C.bits(f)) for b, f in zip(big[:3], full[:3]))
    # the engine setting
    prev = _lib.get_gemm_engine()
    try:
        for name in ("f32", "bf16x3"):
            _lib.set_gemm_engine(name)
            again = ops.dpp_rerank(idx, score, table, K_GEN, 1.0)
            assert all(torch.equal(C.bits(a), C.bits(f)) for a, f in zip(again[:3], full[:3])), name
    finally:
        _lib.set_gemm_engine(prev)
    # the run
    again = ops.dpp_rerank(idx, score, table, K_GEN, 1.0)
    assert all(torch.equal(C.bits(a), C.bits(f)) for a, f in zip(again[:3], full[:3]))


def test_bad_arguments_are_refused_before_any_launch():
    from newsreclib_amd import ops
    idx, score = torch.zeros(2, 8, dtype=torch.int64).cuda(), torch.zeros(2, 8).cuda()
    table = torch.eye(12, 4).cuda()
    for call in (lambda: ops.dpp_rerank(idx.int(), score, table, 3), lambda: ops.dpp_rerank(idx, score[:, :7], table, 3),
                 lambda: ops.dpp_rerank(idx, score, table, 9), lambda: ops.dpp_rerank(idx, score, table, 3, alpha=-0.1),
                 lambda: ops.dpp_rerank(idx, score, table, 3, eps=1.0), lambda: ops.dpp_rerank(idx, score, table, 3, similarity="l2"),
                 lambda: ops.dpp_rerank(idx, score, table, 3, quality=score[:1])):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(NotImplementedError, match="at most 128"):
        ops.dpp_rerank(torch.zeros(1, 129, dtype=torch.int64).cuda(), torch.zeros(1, 129).cuda(), table, 3)
    with pytest.raises(NotImplementedError, match="at most 64"):
        ops.dpp_rerank(torch.zeros(1, 100, dtype=torch.int64).cuda(), torch.zeros(1, 100).cuda(), table, 65)
    with pytest.raises(RuntimeError, match=r"dpp_rerank: D a multiple of 4"):
        ops.dpp_rerank(idx, score, torch.zeros(9, 6).cuda(), 3)
    torch.cuda.synchronize()                                 # nothing was launched: nothing can have gone wrong on the device
    # eight slots of one row: one listed by gain, the duplicates as fills
    out = ops.dpp_rerank(idx, score, table, 3)
    assert int(out[3]) == R.E_RANK and out[0].tolist() == [[0, 0, 0]] * 2 and out[2].tolist() == [[1.0, 0.0, 0.0]] * 2
    # an empty table: every slot with a row is flagged and dead
    out = ops.dpp_rerank(idx, score, torch.zeros(0, 4).cuda(), 3)
    assert int(out[3]) == R.E_ROW and bool((out[0] == -1).all()) and bool(torch.isneginf(out[2]).all())
    # no users
    out = ops.dpp_rerank(idx[:0], score[:0], table, 3)
    assert out[0].shape == (0, 3) and int(out[3]) == 0


def test_dpp_rerank_does_not_synchronise_with_the_host():
    from newsreclib_amd import ops
    table, idx, score = _general(32)
    table = table.cuda()
    quality = torch.ones_like(score)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        if not C.sync_debug_honoured():
            pytest.skip("this torch build does not raise on synchronising calls under set_sync_debug_mode('error')")
        out = ops.dpp_rerank(idx, score, table, 10, 1.0)
        short = ops.dpp_rerank(idx[:, :40].contiguous(), score[:, :40].contiguous(), table, 10, 0.5, "dot", False,
                               quality[:, :40].contiguous(), 0.0)
        long = ops.dpp_rerank(idx, score, table, 64, 1.0)   # (more than 64 KB of LDS: the attribute call is no synchronisation)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert int(out[3]) == 0 and out[0].shape == (B_GEN, 10) and short[2].shape == (B_GEN, 10) and long[0].shape == (B_GEN, 64)


# ---- 4. modules -----------------------------------------------------------------------------------------------------------------------------
def _listed(recs, first_id, idx, score=None):
    for b in range(idx.shape[0]):
        assert list(recs[f"U{first_id + b}"]) == [f"N{int(i)}" for i in idx[b] if i >= 0]
        if score is not None:
            assert list(recs[f"U{first_id + b}"].values()) == [float(s) for s, i in zip(score[b], idx[b]) if i >= 0]


def _greedy_in_f64(pool, pool_score, got, vectors, alpha):
    """every DPP-phase step of every list is a maximiser of the float64 marginal gain over the pool, up to the tolerance of
    test_general_inputs_follow_the_float64_definition, r measured on these pools the same way"""
    D = vectors.shape[1]
    rows, gain = got[0].cpu().numpy(), got[2].cpu().numpy()
    r = _recurrence_error(pool, pool_score, vectors, rows.shape[1], alpha)
    for u in range(pool.shape[0]):
        L = R.kernel_matrix_f64(pool[u], pool_score[u], vectors, None, alpha)[0]
        tol = ((D + 16) * 2.0 ** -23 + 4 * r) * float(np.diagonal(L).max())
        slots = [int(np.nonzero(pool[u] == r)[0][0]) for r, g in zip(rows[u], gain[u]) if r >= 0 and g > 0]
        for c, g, _ in R.dpp_f64(pool[u], pool_score[u], vectors, len(slots), None, alpha, forced=slots)[4]:
            assert np.nanmax(g) - g[c] <= tol, (u, c)


def test_recommend_users_reranks_an_nrms_cache_by_dpp():
    from newsreclib_amd import ops
    from newsreclib_amd.evaluation import DeviceNewsTable, NewsVectorCache, NpaFeatureCache, recommend_users
    from newsreclib_amd.metrics import intra_list_similarity
    mod, attrs = builders.tiny("nrms", n_news=200)
    cache = NewsVectorCache(mod, DeviceNewsTable(attrs), chunk=64)
    V, B, k = 200, 6, 10
    lists, hist, hs, uidx = builders.hist_batch(V)
    users = [{"hist": lists[b], "user_id": 100 + b} for b in range(B)]
    plain = recommend_users(cache, users, k, batch_size=B)
    assert recommend_users(cache, users, k, batch_size=B, dpp=None) == plain
    pool_idx, pool_score, status = cache.recommend(hist.cuda(), hs, 64)
    assert int(status) == 0
    _listed(plain, 100, pool_idx[:, :k])
    with warnings.catch_warnings(record=True) as said:
        warnings.simplefilter("always")
        recs = recommend_users(cache, users, k, batch_size=B, dpp=dict(pool=64, alpha=2.0))
    assert not [w for w in said if "recommend_users" in str(w.message)]      # a full-rank pool: nothing to warn about
    by_hand = cache.rerank_dpp(pool_idx, pool_score, k, 2.0)
    want = ops.dpp_rerank(pool_idx, pool_score, cache.vectors, k, 2.0, "cosine", True, None, 1e-4)
    assert int(by_hand[3]) == 0 and all(torch.equal(C.bits(a), C.bits(b)) for a, b in zip(by_hand[:3], want[:3]))
    _listed(recs, 100, by_hand[0], by_hand[1])
    default = recommend_users(cache, users, k, batch_size=B, dpp=dict(pool=64))
    _listed(default, 100, cache.rerank_dpp(pool_idx, pool_score, k)[0])
    _greedy_in_f64(pool_idx.cpu().numpy(), pool_score.cpu().numpy(), by_hand, cache.vectors.cpu().numpy(), 2.0)
    before, after = intra_list_similarity(pool_idx[:, :k], cache.vectors), intra_list_similarity(by_hand[0], cache.vectors)
    print(f"intra-list similarity of the first {k}: {before:.4f}; after DPP over 64 at alpha 2: {after:.4f}")
    assert after <= before
    with pytest.raises(ValueError, match="at least k"):
        recommend_users(cache, users, k, dpp=dict(pool=k - 1))
    with pytest.raises(ValueError, match="excludes"):
        recommend_users(cache, users, k, diversify=(64, 0.5), dpp=dict(pool=64))
    # together with a class cap: the capped method produces the pool, whose empty slots stay out of the list
    capped = recommend_users(cache, users, k, batch_size=B, cap=("category", 5), dpp=dict(pool=64, alpha=2.0))
    cap_idx, cap_score, _ = cache.recommend_capped(hist.cuda(), hs, 64, "category", 5)
    _listed(capped, 100, cache.rerank_dpp(cap_idx, cap_score, k, 2.0)[0])
    assert not torch.equal(cap_idx, pool_idx)
    # a pool that runs out of rank is reported as a warning worded from DPP_FLAGS
    with pytest.warns(UserWarning, match="ran out of rank"):
        recommend_users(cache, users, k, batch_size=B, dpp=dict(pool=64, alpha=2.0, eps=0.999))
    with pytest.raises(NotImplementedError, match="depends on the user"):
        NpaFeatureCache.rerank_dpp(None, pool_idx, pool_score, k)


def test_manner_reranks_against_either_sub_model(tmp_path):
    from newsreclib_amd import ops
    from newsreclib_amd.evaluation import MannerVectorCache, recommend_users
    cr, ac, asent = builders.manner_modules(tmp_path)
    table, imps = builders.manner_table_and_impressions()
    cache = MannerVectorCache(builders.manner_ensemble(cr, ac, asent), table)
    lists = [i["hist"] for i in imps]
    hs, hist = torch.tensor([len(x) for x in lists]), torch.cat(lists)
    B, k, pool = len(imps), 5, 16
    idx, score, status = cache.recommend_ensemble(hist.cuda(), hs, pool)
    assert int(status) == 0 and len(cache.vectors) >= 2
    for s in (0, 1):
        got = cache.rerank_dpp(idx, score, k, 1.0, submodel=s)
        want = ops.dpp_rerank(idx, score, cache.vectors[s], k, 1.0)
        assert all(torch.equal(C.bits(a), C.bits(b)) for a, b in zip(got[:3], want[:3])) and int(got[3]) == int(want[3])
        assert int(got[3]) & ~R.E_RANK == 0
    first = cache.rerank_dpp(idx, score, k, 1.0)
    users = [{"hist": lists[b], "user_id": 100 + b} for b in range(B)]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        recs = recommend_users(cache, users, k, batch_size=B + 3, dpp=dict(pool=pool))
    _listed(recs, 100, first[0], first[1])


def test_a_miner_cache_is_reranked_like_any_other(tmp_path):
    from newsreclib_amd.evaluation import recommend_users
    mod, cfg, cache, hist, hs = builders.miner_cache("miner_tiny_no_bias", "max", tmp_path)
    V, B = cache.table.num_news, int(hs.numel())
    pool = min(12, V - int(hs.max()))
    k = min(5, pool)
    lists = list(torch.split(hist, hs.tolist()))
    idx, score, status = cache.recommend_interests(hist.cuda(), hs, pool)
    want = cache.rerank_dpp(idx, score, k, 1.0)
    assert int(status) == 0 and int(want[3]) & ~R.E_RANK == 0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        recs = recommend_users(cache, [{"hist": lists[b]} for b in range(B)], k, batch_size=B, dpp=dict(pool=pool, alpha=1.0))
    _listed(recs, 1, want[0], want[1])
    _greedy_in_f64(idx.cpu().numpy(), score.cpu().numpy(), want, cache.vectors.cpu().numpy(), 1.0)
