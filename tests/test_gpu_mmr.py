"""Greedy MMR re-ranking of top-k pools (``nrl_mmr_rerank``, ``ops.mmr_rerank``, ``*Cache.rerank_diverse``,
``recommend_users(diversify=...)``).

Expected values come from ``tests/mmr_ref.py``.  The exact cases use table entries and scores that are multiples of 1/8 in
[-2, 2]: every product is a multiple of 1/64 and every partial sum stays far below 2^24 / 64, so the Gram matrix is exact and the
float32 restatement, fed that matrix, must reproduce rows, scores and objectives bit for bit -- the square root, the divisions,
the products and the differences behind it are single correctly rounded operations on both sides.  The real-valued cases check
the kernel's own prefix against the float64 objective under a tolerance worked out from D."""
import numpy as np
import pytest
import torch

from tests import builders
from tests import catalogue_ref as C
from tests import mmr_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True, params=["f32", "bf16x3"])
def engine(request):
    from newsreclib_amd import _lib
    prev = _lib.get_gemm_engine()
    _lib.set_gemm_engine(request.param)
    yield request.param
    _lib.set_gemm_engine(prev)


def _rerank(idx, score, table, k, lam, similarity="cosine", normalize=True):
    from newsreclib_amd import ops
    as_dev = lambda x: (torch.from_numpy(x) if isinstance(x, np.ndarray) else x).cuda()  # noqa: E731
    return ops.mmr_rerank(as_dev(idx), as_dev(score), as_dev(table), k, lam, similarity, normalize)


# ---- 1. the exact sweep ---------------------------------------------------------------------------------------------------------------------
V_SWEEP = 200
_CACHE = {}


def _sweep_case(B, N, D):
    """Pools with every edge the header names, as far as N has room for them: user 0 carries an empty slot in the middle and one
    at the tail, the rows V and -2, a NaN and a +inf score, a duplicated row and the zero row; user 1 is all empty; user 2 has
    two live slots (fewer than k = 5 / N); the eighth-grid scores tie everywhere."""
    key = ("case", B, N, D)
    if key not in _CACHE:
        rng = np.random.default_rng(1000 * B + 10 * N + D)
        table = (rng.integers(-16, 17, (V_SWEEP, D)) / 8.0).astype(np.float32)
        table[0] = 0.0
        idx = rng.integers(0, V_SWEEP, (B, N))
        score = (rng.integers(-16, 17, (B, N)) / 8.0).astype(np.float32)
        want = 0
        edges = [("mid", 1, -1), ("row", 2, V_SWEEP), ("row", 3, -2), ("nan", 4, np.nan), ("inf", 5, np.inf), ("dup", 6, None),
                 ("zero", 8, 0), ("tail", N - 1, -1)]
        for kind, slot, value in edges:
            if slot >= N or (kind != "tail" and slot == N - 1) or N < 2:
                continue
            if kind in ("mid", "tail", "row", "zero"):
                idx[0, slot] = value
                want |= R.E_ROW if kind == "row" else 0
            elif kind == "dup":
                idx[0, slot + 1 if slot + 1 < N - 1 else slot] = idx[0, slot]
            else:
                score[0, slot] = value
                want |= R.E_NAN
        if B >= 3:
            idx[1, :] = -1
            idx[2, 2:] = -1
        _CACHE[key] = (table, idx.astype(np.int64), score, want)
    return _CACHE[key]


def _expected(B, N, D, users, k, lam, sim, norm):
    key = ("want", B, N, D, tuple(users), k, lam, sim, norm)
    if key not in _CACHE:
        table, idx, score, _ = _sweep_case(B, N, D)
        outs = [R.mmr_f32(idx[u], score[u], R.gram_f32(idx[u], table), V_SWEEP, k, lam, sim, norm) for u in users]
        _CACHE[key] = tuple(np.stack([o[j] for o in outs]) for j in range(3))
    return _CACHE[key]


def _settings(N):
    """(k, lambda, similarity, normalize): every value of each at least once, the three k against both similarities"""
    ks = sorted({1, min(5, N), N})
    out = [(N, 0.5, "cosine", True), (min(5, N), 0.0, "dot", False), (1, 1.0, "cosine", False), (N, 0.0, "cosine", False),
           (min(5, N), 0.5, "dot", True), (N, 1.0, "dot", False), (min(5, N), 0.5, "cosine", True), (1, 0.5, "dot", True)]
    assert {s[0] for s in out} == set(ks)
    return out


_SHAPES = [(1, 1, 4), (3, 2, 300), (1, 63, 4), (3, 64, 300), (3, 65, 4), (1, 127, 300), (130, 128, 4), (3, 128, 300), (130, 9, 300)]


def test_the_sweep_covers_the_shapes_of_the_issue():
    assert {s[0] for s in _SHAPES} == {1, 3, 130} and {s[1] for s in _SHAPES} >= {1, 2, 63, 64, 65, 127, 128}
    assert {s[2] for s in _SHAPES} == {4, 300}
    seen = {(lam, sim, norm) for _, lam, sim, norm in _settings(128)}
    assert {s[0] for s in seen} == {0.0, 0.5, 1.0} and {s[1] for s in seen} == {"cosine", "dot"} and {s[2] for s in seen} == {True, False}


@pytest.mark.parametrize("B,N,D", _SHAPES)
def test_exact_sweep_rows_scores_and_objective_bits(B, N, D):
    table, idx, score, want_flags = _sweep_case(B, N, D)
    assert N < 8 or want_flags == (R.E_ROW | R.E_NAN)
    for k, lam, sim, norm in _settings(N):
        got_idx, got_score, got_mmr, status = _rerank(idx, score, table, k, lam, sim, norm)
        # the python restatement of a long list is slow: in a large batch the full-length lists are compared for the users at both
        # ends of it (those with the edges among them), every user for the shorter ones; the prefix test below ties the two
        users = list(range(B)) if B * k <= 2000 else [0, 1, 2, 3, B - 2, B - 1]
        w_idx, w_score, w_mmr = _expected(B, N, D, users, k, lam, sim, norm)
        assert int(status) == want_flags, (k, lam, sim, norm, int(status))
        assert C.same(got_idx[users], w_idx), (k, lam, sim, norm)
        assert C.same(got_score[users], w_score) and C.same(got_mmr[users], w_mmr), (k, lam, sim, norm)
        if B >= 3:                                           # the all-empty user and the user with two live slots
            assert bool((got_idx[1] == -1).all()) and bool(torch.isneginf(got_score[1]).all()) and bool(torch.isneginf(got_mmr[1]).all())
            assert int((got_idx[2] >= 0).sum()) == min(k, 2)
        if B * k > 2000:                                     # every user: the list of k is a prefix-extension of the list of 5
            s_idx, s_score, s_mmr, _ = _rerank(idx, score, table, 5, lam, sim, norm)
            assert torch.equal(s_idx, got_idx[:, :5]) and torch.equal(C.bits(s_score), C.bits(got_score[:, :5]))
            assert torch.equal(C.bits(s_mmr), C.bits(got_mmr[:, :5]))
            all5 = _expected(B, N, D, list(range(B)), 5, lam, sim, norm)
            assert C.same(s_idx, all5[0]) and C.same(s_score, all5[1]) and C.same(s_mmr, all5[2])


def test_a_duplicated_row_has_cosine_one_and_the_zero_row_cosine_zero():
    table = np.zeros((4, 4), dtype=np.float32)
    table[1], table[2] = [2, 0, 0, 0], [0, 0, 2, 0]            # (squared norms 4: the cosine of a row with itself is exactly 1)
    idx = np.array([[1, 1, 2, 0]], dtype=np.int64)
    score = np.array([[2.0, 2.0, 1.0, 1.0]], dtype=np.float32)
    # lambda = 0.5, raw scores: slot 0 first (1.0); then slot 1 pays its cosine 1 with slot 0 (1.0 - 0.5 = 0.5) and ties with the
    # orthogonal slot 2 and the zero row (0.5 - 0): the lower slot wins
    got_idx, got_score, got_mmr, status = _rerank(idx, score, table, 4, 0.5, "cosine", False)
    assert int(status) == 0 and got_idx.tolist() == [[1, 1, 2, 0]] and got_mmr.tolist() == [[1.0, 0.5, 0.5, 0.5]]
    got_idx, _, got_mmr, _ = _rerank(idx, score, table, 4, 0.25, "cosine", False)
    assert got_idx.tolist() == [[1, 2, 0, 1]] and got_mmr.tolist() == [[0.5, 0.25, 0.25, -0.25]]


# ---- 2. the same chain as topk_scores ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [4, 300])
def test_the_gram_matrix_has_the_bits_of_topk_scores(D):
    from newsreclib_amd import ops
    g = torch.Generator().manual_seed(5)
    V, N, B = 128, 70, 3                                     # (V = the longest list topk_scores returns)
    table = torch.randn(V, D, generator=g).cuda()
    idx = torch.stack([torch.randperm(V, generator=g)[:N] for _ in range(B)]).cuda()
    score = torch.randn(B, N, generator=g).cuda()
    # lambda = 0, dot, raw scores: step 0 takes slot 0 (every objective is a zero), step 1 the slot of smallest dot product with
    # it, and its objective is that product negated
    got_idx, _, got_mmr, status = _rerank(idx, score, table, 2, 0.0, "dot", False)
    assert int(status) == 0 and torch.equal(got_idx[:, 0], idx[:, 0])
    all_idx, all_score, _ = ops.topk_scores(table[got_idx[:, 0]].contiguous(), table, V)
    for u in range(B):
        pos = (all_idx[u] == got_idx[u, 1]).nonzero()
        assert pos.numel() == 1
        assert torch.equal(C.bits(got_mmr[u, 1:2]), C.bits(-all_score[u, pos[0, 0]].reshape(1)))
        in_pool = torch.isin(all_idx[u], idx[u, 1:])
        assert float(all_score[u][in_pool].min()) == -float(got_mmr[u, 1])       # and it is the pool's smallest


# ---- 3. general inputs: the kernel's own prefix is greedy in float64 ------------------------------------------------------------------------
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


def _near_ties(D, lam, tol):
    key = ("ties", D, lam)
    if key not in _CACHE:
        table, idx, score = _general(D)
        idx, score, n = idx.cpu().numpy(), score.cpu().numpy(), 0
        for u in range(B_GEN):
            for c, obj in R.mmr_f64(idx[u], score[u], table.numpy(), K_GEN, lam)[4]:
                rest = np.delete(obj, c)
                n += bool(np.nanmax(rest) >= obj[c] - tol)
        _CACHE[key] = n
    return _CACHE[key]


@pytest.mark.parametrize("lam", [0.3, 0.5, 0.7])
@pytest.mark.parametrize("D", [4, 300])
def test_general_inputs_follow_the_float64_objective(D, lam):
    table, idx, score = _general(D)
    tol = (D + 16) * 2.0 ** -23                              # max(1, lam |rel|max + (1 - lam) |sim|max) = 1: rel in [0, 1], |cos| <= 1
    # the condition on the inputs, on the reference alone: near-ties are rare, so the check below is in effect an equality check
    ties = _near_ties(D, lam, tol)
    print(f"D={D} lambda={lam}: {ties} of {B_GEN * K_GEN} reference steps have a runner-up within tol = {tol:.3e}")
    assert ties < 0.02 * B_GEN * K_GEN
    got_idx, got_score, got_mmr, status = _rerank(idx, score, table, K_GEN, lam)
    assert int(status) == 0 and bool((got_idx >= 0).all())
    pool, pool_score, rows, mmr = idx.cpu().numpy(), score.cpu().numpy(), got_idx.cpu().numpy(), got_mmr.cpu().numpy().astype(np.float64)
    worst_gap = worst_err = 0.0
    for u in range(B_GEN):
        slots = [int(np.nonzero(pool[u] == r)[0][0]) for r in rows[u]]
        assert len(set(slots)) == K_GEN
        assert np.array_equal(got_score[u].cpu().numpy(), pool_score[u][slots])
        for t, (c, obj) in enumerate(R.mmr_f64(pool[u], pool_score[u], table.numpy(), K_GEN, lam, forced=slots)[4]):
            worst_gap, worst_err = max(worst_gap, float(np.nanmax(obj) - obj[c])), max(worst_err, abs(mmr[u, t] - obj[c]))
    print(f"D={D} lambda={lam}: largest float64 gap to the maximum {worst_gap:.3e}, largest |mmr - objective| {worst_err:.3e}")
    assert worst_gap <= tol and worst_err <= tol


# ---- 4. invariance and entry ----------------------------------------------------------------------------------------------------------------
def test_prefix_batch_composition_engine_and_lambda_one():
    from newsreclib_amd import _lib, ops
    table, idx, score = _general(300)
    table = table.cuda()
    full = ops.mmr_rerank(idx, score, table, K_GEN, 0.5)
    part = ops.mmr_rerank(idx, score, table, 5, 0.5)
    assert all(torch.equal(C.bits(p), C.bits(f[:, :5])) for p, f in zip(part[:3], full[:3]))
    # a user alone, and inside a batch of 130 at another place
    big_idx, big_score = idx.repeat(4, 1)[:130].contiguous(), score.repeat(4, 1)[:130].contiguous()
    big = ops.mmr_rerank(big_idx, big_score, table, K_GEN, 0.5)
    alone = ops.mmr_rerank(idx[7:8].contiguous(), score[7:8].contiguous(), table, K_GEN, 0.5)
    for u in (7, 47, 87, 127):
        assert all(torch.equal(C.bits(a[0]), C.bits(b[u])) for a, b in zip(alone[:3], big[:3]))
    assert all(torch.equal(C.bits(b[:B_GEN]), C.bits(f)) for b, f in zip(big[:3], full[:3]))
    # the engine setting
    prev = _lib.get_gemm_engine()
    try:
        for name in ("f32", "bf16x3"):
            _lib.set_gemm_engine(name)
            again = ops.mmr_rerank(idx, score, table, K_GEN, 0.5)
            assert all(torch.equal(C.bits(a), C.bits(f)) for a, f in zip(again[:3], full[:3])), name
    finally:
        _lib.set_gemm_engine(prev)
    # lambda = 1 without normalisation: the pool's first k entries, whatever the similarity
    for sim in ("cosine", "dot"):
        one = ops.mmr_rerank(idx, score, table, K_GEN, 1.0, sim, False)
        assert int(one[3]) == 0 and torch.equal(one[0], idx[:, :K_GEN]) and torch.equal(C.bits(one[1]), C.bits(score[:, :K_GEN]))
        assert torch.equal(C.bits(one[2]), C.bits(score[:, :K_GEN]))


def test_bad_arguments_are_refused_before_any_launch():
    from newsreclib_amd import ops
    idx, score = torch.zeros(2, 8, dtype=torch.int64).cuda(), torch.zeros(2, 8).cuda()
    table = torch.zeros(9, 4).cuda()
    for call in (lambda: ops.mmr_rerank(idx.int(), score, table, 3, 0.5), lambda: ops.mmr_rerank(idx, score[:, :7], table, 3, 0.5),
                 lambda: ops.mmr_rerank(idx, score, table, 9, 0.5), lambda: ops.mmr_rerank(idx, score, table, 3, -0.1),
                 lambda: ops.mmr_rerank(idx, score, table, 3, 0.5, similarity="l2")):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(NotImplementedError, match="at most 128"):
        ops.mmr_rerank(torch.zeros(1, 129, dtype=torch.int64).cuda(), torch.zeros(1, 129).cuda(), table, 3, 0.5)
    with pytest.raises(RuntimeError, match=r"mmr_rerank: D a multiple of 4"):
        ops.mmr_rerank(idx, score, torch.zeros(9, 6).cuda(), 3, 0.5)
    torch.cuda.synchronize()                                 # nothing was launched: nothing can have gone wrong on the device
    out = ops.mmr_rerank(idx, score, table, 3, 0.5)
    assert int(out[3]) == 0 and out[0].tolist() == [[0, 0, 0]] * 2
    # an empty table: every slot with a row is flagged and dead
    out = ops.mmr_rerank(idx, score, torch.zeros(0, 4).cuda(), 3, 0.5)
    assert int(out[3]) == R.E_ROW and bool((out[0] == -1).all())


def test_mmr_rerank_does_not_synchronise_with_the_host():
    from newsreclib_amd import ops
    table, idx, score = _general(4)
    table = table.cuda()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        if not C.sync_debug_honoured():
            pytest.skip("this torch build does not raise on synchronising calls under set_sync_debug_mode('error')")
        out = ops.mmr_rerank(idx, score, table, 10, 0.5)
        short = ops.mmr_rerank(idx[:, :40].contiguous(), score[:, :40].contiguous(), table, 10, 0.7, "dot", False)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert int(out[3]) == 0 and out[0].shape == (B_GEN, 10) and int(short[3]) == 0 and short[2].shape == (B_GEN, 10)


# ---- 5. modules -----------------------------------------------------------------------------------------------------------------------------
def _greedy_in_f64(pool, pool_score, rows, vectors, lam):
    """every list ``rows[u]`` is, step by step, a maximiser of the float64 objective over ``pool[u]`` up to the tolerance of D"""
    D = vectors.shape[1]
    tol = (D + 16) * 2.0 ** -23
    for u in range(pool.shape[0]):
        slots = [int(np.nonzero(pool[u] == r)[0][0]) for r in rows[u] if r >= 0]
        for c, obj in R.mmr_f64(pool[u], pool_score[u], vectors, len(slots), lam, forced=slots)[4]:
            assert np.nanmax(obj) - obj[c] <= tol, (u, c)


def test_recommend_users_diversifies_an_nrms_cache():
    from newsreclib_amd import ops
    from newsreclib_amd.evaluation import DeviceNewsTable, NewsVectorCache, NpaFeatureCache, recommend_users
    from newsreclib_amd.metrics import intra_list_similarity
    mod, attrs = builders.tiny("nrms", n_news=200)
    cache = NewsVectorCache(mod, DeviceNewsTable(attrs), chunk=64)
    V, B, k = 200, 6, 10
    lists, hist, hs, uidx = builders.hist_batch(V)
    users = [{"hist": lists[b], "user_id": 100 + b} for b in range(B)]
    plain = recommend_users(cache, users, k, batch_size=B)
    assert recommend_users(cache, users, k, batch_size=B, diversify=None) == plain
    pool_idx, pool_score, status = cache.recommend(hist.cuda(), hs, 64)
    assert int(status) == 0 and all(list(plain[f"U{100 + b}"]) == [f"N{int(i)}" for i in pool_idx[b, :k]] for b in range(B))
    recs = recommend_users(cache, users, k, batch_size=B, diversify=(64, 0.5))
    by_hand = cache.rerank_diverse(pool_idx, pool_score, k, 0.5)
    want = ops.mmr_rerank(pool_idx, pool_score, cache.vectors, k, 0.5, "cosine", True)
    assert int(by_hand[3]) == 0 and all(torch.equal(C.bits(a), C.bits(b)) for a, b in zip(by_hand[:3], want[:3]))
    for b in range(B):
        assert list(recs[f"U{100 + b}"]) == [f"N{int(i)}" for i in by_hand[0][b]]
        assert list(recs[f"U{100 + b}"].values()) == [float(s) for s in by_hand[1][b]]
    _greedy_in_f64(pool_idx.cpu().numpy(), pool_score.cpu().numpy(), by_hand[0].cpu().numpy(), cache.vectors.cpu().numpy(), 0.5)
    before, after = intra_list_similarity(pool_idx[:, :k], cache.vectors), intra_list_similarity(by_hand[0], cache.vectors)
    print(f"intra-list similarity of the first {k}: {before:.4f}; after MMR over 64 at lambda 0.5: {after:.4f}")
    assert after <= before
    with pytest.raises(ValueError, match="at least k"):
        recommend_users(cache, users, k, diversify=(k - 1, 0.5))
    # together with a class cap: the capped method produces the pool
    capped = recommend_users(cache, users, k, batch_size=B, cap=("category", 5), diversify=(64, 0.7))
    cap_idx, cap_score, _ = cache.recommend_capped(hist.cuda(), hs, 64, "category", 5)
    cap_want = cache.rerank_diverse(cap_idx, cap_score, k, 0.7)
    assert all(list(capped[f"U{100 + b}"]) == [f"N{int(i)}" for i in cap_want[0][b] if i >= 0] for b in range(B))
    assert not torch.equal(cap_idx, pool_idx) and bool((cap_idx == -1).any())      # (the cap changed the pool and left empty slots)
    with pytest.raises(NotImplementedError, match="depends on the user"):
        NpaFeatureCache.rerank_diverse(None, pool_idx, pool_score, k, 0.5)


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
        got = cache.rerank_diverse(idx, score, k, 0.5, submodel=s)
        want = ops.mmr_rerank(idx, score, cache.vectors[s], k, 0.5)
        assert int(got[3]) == 0 and all(torch.equal(C.bits(a), C.bits(b)) for a, b in zip(got[:3], want[:3]))
    first = cache.rerank_diverse(idx, score, k, 0.5)
    users = [{"hist": lists[b], "user_id": 100 + b} for b in range(B)]
    recs = recommend_users(cache, users, k, batch_size=B + 3, diversify=(pool, 0.5))
    assert all(list(recs[f"U{100 + b}"]) == [f"N{int(i)}" for i in first[0][b] if i >= 0] for b in range(B))


def test_a_miner_cache_is_diversified_like_any_other(tmp_path):
    from newsreclib_amd.evaluation import recommend_users
    mod, cfg, cache, hist, hs = builders.miner_cache("miner_tiny_no_bias", "max", tmp_path)
    V, B = cache.table.num_news, int(hs.numel())
    pool = min(12, V - int(hs.max()))
    k = min(5, pool)
    lists = list(torch.split(hist, hs.tolist()))
    idx, score, status = cache.recommend_interests(hist.cuda(), hs, pool)
    want = cache.rerank_diverse(idx, score, k, 0.5)
    assert int(status) == 0 and int(want[3]) == 0
    recs = recommend_users(cache, [{"hist": lists[b]} for b in range(B)], k, batch_size=B, diversify=(pool, 0.5))
    assert all(list(recs[f"U{b + 1}"]) == [f"N{int(i)}" for i in want[0][b] if i >= 0] for b in range(B))
    _greedy_in_f64(idx.cpu().numpy(), score.cpu().numpy(), want[0].cpu().numpy(), cache.vectors.cpu().numpy(), 0.5)
