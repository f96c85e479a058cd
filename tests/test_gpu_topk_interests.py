"""Multi-interest full-catalogue top-k (``nrl_topk_interest_scores`` / ``ops.topk_interest_scores`` /
``NewsVectorCache.recommend_interests``): a user is K interest vectors, a table row's score their max, mean or gate-weighted sum.

Expected values are computed on the CPU in float64: ``s[b, j, v] = E64[b, j] . T64[v]``, the aggregate over j
(``catalogue_rank_scorers_ref.interest_scores64``), under the population and the order of ``tests/catalogue_ref.py``.
Integer-valued vectors in [-4, 4] make every fp32 dot product exact (|s| <= 16 * 768), every sum over K <= 64 of them exact
(< 2^24) and the division by a power of two exact, so the max cases and the mean cases with K a power of two compare with
``torch.equal``.  Real-valued cases use derived worst cases (``interest_scores64``), not measurements: with
``bs_j = D 2^-23 sum_i |e_ji| |t_i|`` the error of one fp32 dot product of length D (``bl_j`` likewise from the gate),

  max       max_j bs_j                                     (the maximum of perturbed values moves by at most the largest perturbation)
  mean      max_j bs_j + K 2^-23 max_j |s_j|               (K - 1 additions and one division, each 2^-24 relative, rounded up)
  weighted  max_j bs_j + (max_j s_j - min_j s_j) (expm1(2 max_j bl_j) + (K + 8) 2^-23) + K 2^-23 max_j |s_j|
            (a convex combination moves by at most its spread times the relative change of the weights: logits off by bl_j change
            the weight ratios by up to exp(2 bl); expf, the subtraction and the two sums add (K + 8) 2^-23).

The fp32 CPU computation of the same formulas stays below 6 % of these on such inputs."""
import functools

import pytest
import torch

from tests import builders
from tests import catalogue_ref as C
from tests.catalogue_rank_scorers_ref import interest_scores64

pytestmark = pytest.mark.gpu

E_EXCLUDE, E_OFFSETS, E_NAN = 1, 2, 4
MODES = ("max", "mean", "weighted")


@pytest.fixture(autouse=True, params=["f32", "bf16x3"])
def engine(request):
    from newsreclib_amd import _lib
    prev = _lib.get_gemm_engine()
    _lib.set_gemm_engine(request.param)
    yield request.param
    _lib.set_gemm_engine(prev)


def _int_case(seed, B, K, V, D):
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(-4, 5, (B, K, D), generator=g).float(), torch.randint(-4, 5, (B, K, D), generator=g).float(),
            torch.randint(-4, 5, (V, D), generator=g).float())


def _real_case(seed, B, K, V, D):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, K, D, generator=g), torch.randn(B, K, D, generator=g), torch.randn(V, D, generator=g))


def _run(E, G, T, k, mode, excl=None, eligible=None, slices=0, off=None):
    from newsreclib_amd import ops
    ei = eo = None
    if excl is not None:
        ei, eo = C.ragged(excl)
        ei, eo = ei.cuda(), (off if off is not None else eo).cuda()
    idx, score, status = ops.topk_interest_scores(E.cuda(), T.cuda(), k, mode, G.cuda() if mode == "weighted" else None, ei, eo,
                                                  eligible.cuda() if eligible is not None else None, slices)
    return idx.cpu(), score.cpu(), int(status)


# ---- 1. exact, with ties ----------------------------------------------------------------------------------------------------------
# (K, B, V, D, k, slices): B in {1, Ut, Ut + 1, 130} with Ut = 64 // K users per workgroup, V around the 128-row table tile
_EXACT_MAX = [(1, 64, 1000, 300, 5, 0), (1, 65, 129, 4, 128, 2), (1, 130, 1000, 300, 128, 7),
              (2, 32, 127, 300, 64, 1), (2, 33, 128, 4, 65, 0), (2, 1, 1, 4, 1, 0),
              (3, 21, 1000, 768, 5, 7), (3, 22, 129, 300, 1, 2), (3, 130, 1000, 4, 64, 0), (3, 1, 1, 300, 5, 0),
              (32, 2, 1000, 300, 5, 0), (32, 3, 127, 768, 128, 1), (32, 130, 1000, 300, 65, 2), (32, 1, 128, 4, 1, 7),
              (33, 1, 1000, 300, 64, 2), (33, 2, 129, 4, 5, 0), (33, 130, 127, 300, 5, 1),
              (64, 1, 1000, 768, 128, 0), (64, 2, 128, 300, 65, 7), (64, 130, 1000, 4, 5, 2), (64, 1, 1, 4, 1, 1)]
_EXACT_MEAN = [(1, 65, 129, 300, 5, 0), (2, 33, 1000, 768, 65, 2), (4, 17, 127, 4, 128, 1), (32, 3, 1000, 300, 5, 7),
               (64, 2, 128, 300, 64, 0), (64, 130, 1000, 4, 10, 0)]


@functools.lru_cache(maxsize=None)
def _exact_expected(mode, K, B, V, D, k):
    E, G, T = _int_case(K * 1000 + B * 7 + V + D + k, B, K, V, D)
    return E, G, T, C.expected_topk(interest_scores64(E, T, mode, G)[0], k)


def _check_exact(mode, K, B, V, D, k, slices):
    E, G, T, (want_idx, want_score) = _exact_expected(mode, K, B, V, D, k)
    idx, score, status = _run(E, G, T, k, mode, slices=slices)
    assert status == 0
    assert torch.equal(idx, want_idx)
    assert torch.equal(score, want_score)


@pytest.mark.parametrize("K,B,V,D,k,slices", _EXACT_MAX)
def test_exact_max_with_ties(K, B, V, D, k, slices):
    _check_exact("max", K, B, V, D, k, slices)


@pytest.mark.parametrize("K,B,V,D,k,slices", _EXACT_MEAN)
def test_exact_mean_with_ties(K, B, V, D, k, slices):
    _check_exact("mean", K, B, V, D, k, slices)


# ---- 2. K = 1 is topk_scores -----------------------------------------------------------------------------------------------------
def test_one_interest_returns_the_bits_of_topk_scores():
    from newsreclib_amd import ops
    B, V, D, k = 37, 3000, 300, 10
    E, G, T = _real_case(41, B, 1, V, D)
    g = torch.Generator().manual_seed(4)
    excl = [torch.randint(0, V, (int(n),), generator=g).tolist() for n in torch.randint(0, 51, (B,), generator=g)]
    ei, eo = C.ragged(excl)
    E, G, T, ei, eo = E.cuda(), G.cuda(), T.cuda(), ei.cuda(), eo.cuda()
    want_idx, want_score, want_status = ops.topk_scores(E[:, 0], T, k, ei, eo)
    assert int(want_status) == 0
    for mode in MODES:
        idx, score, status = ops.topk_interest_scores(E, T, k, mode, G if mode == "weighted" else None, ei, eo)
        assert int(status) == 0, mode
        assert torch.equal(idx, want_idx), mode
        assert torch.equal(score.view(torch.int32), want_score.view(torch.int32)), mode


# ---- 3. real values against float64 -------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _real_expected(K, D):
    B, V = 9, 5000
    E, G, T = _real_case(K * 31 + D, B, K, V, D)
    g = torch.Generator().manual_seed(K + D)
    excl = tuple(tuple(torch.randint(0, V, (int(n),), generator=g).tolist()) for n in torch.randint(0, 51, (B,), generator=g))
    return E, G, T, excl, {mode: interest_scores64(E, T, mode, G) for mode in MODES}


def _check_real(agg, tol, idx, score, excl, k):
    C.check_floor(idx, score, agg, tol, C.population(agg, excl)[0], k)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("K,D", [(K, D) for K in (3, 32, 33) for D in (8, 256, 300)])
def test_real_values_against_float64(K, D, mode):
    k = 10
    E, G, T, excl, expected = _real_expected(K, D)
    idx, score, status = _run(E, G, T, k, mode, [list(x) for x in excl])
    assert status == 0
    _check_real(*expected[mode], idx, score, excl, k)


# ---- 4. exclusion, eligibility, status ------------------------------------------------------------------------------------------------
def test_exclusion_list_longer_than_the_cached_part_and_eligibility():
    """150 exclusion entries (64 are cached in LDS), several table tiles, an eligibility mask, two users per workgroup and more."""
    B, K, V, D, k = 5, 3, 700, 8, 20
    E, G, T = _int_case(5, B, K, V, D)
    agg = interest_scores64(E, T, "max", G)[0]
    g = torch.Generator().manual_seed(3)
    eligible = torch.ones(V, dtype=torch.uint8)
    eligible[[0, 7, 130, 699]] = 0
    excl = [torch.randperm(V, generator=g)[:150].tolist(), [], C.expected_topk(agg, 150)[0][2].tolist(), [3, 3, 9, 3], list(range(V))]
    idx, score, status = _run(E, G, T, k, "max", excl, eligible, slices=3)
    want_idx, want_score = C.expected_topk(agg, k, excl, eligible)
    assert status == 0 and torch.equal(idx, want_idx) and torch.equal(score, want_score)
    assert torch.equal(idx[4], torch.full((k,), -1)) and bool(torch.isinf(score[4]).all())
    # mean over K = 4 (exact): the same selection code after the other aggregate
    E, G, T = _int_case(6, B, 4, V, D)
    agg = interest_scores64(E, T, "mean", G)[0]
    idx, score, status = _run(E, G, T, k, "mean", excl, eligible.bool(), slices=0)
    want_idx, want_score = C.expected_topk(agg, k, excl, eligible)
    assert status == 0 and torch.equal(idx, want_idx) and torch.equal(score, want_score)


def test_status_bad_exclusion_index_is_ignored():
    B, K, V, D, k = 4, 3, 300, 12, 6
    E, G, T = _int_case(17, B, K, V, D)
    agg = interest_scores64(E, T, "max", G)[0]
    excl = [[1, 2], [5], [], [7, 7]]
    bad = [[-1, 1, 2], [5, V], [], [7, 7]]
    idx, score, status = _run(E, G, T, k, "max", bad)
    want_idx, want_score = C.expected_topk(agg, k, excl)
    assert status == E_EXCLUDE
    assert torch.equal(idx, want_idx) and torch.equal(score, want_score)


def test_status_decreasing_offsets_blank_that_user_alone():
    B, K, V, D, k = 4, 3, 300, 12, 6
    E, G, T = _int_case(18, B, K, V, D)
    agg = interest_scores64(E, T, "max", G)[0]
    flat = list(range(12))
    off = torch.tensor([0, 5, 3, 8, 12])                    # user 1 runs backwards
    idx, score, status = _run(E, G, T, k, "max", [flat], off=off)
    assert status == E_OFFSETS
    want_idx, want_score = C.expected_topk(agg, k, [flat[0:5], [], flat[3:8], flat[8:12]])
    for b in (0, 2, 3):
        assert torch.equal(idx[b], want_idx[b]) and torch.equal(score[b], want_score[b])
    assert torch.equal(idx[1], torch.full((k,), -1)) and bool((score[1] == float("-inf")).all())


@pytest.mark.parametrize("mode", MODES)
def test_status_nan_table_row_is_left_out_for_every_user(mode):
    B, K, V, D, k = 5, 3, 300, 12, 9
    E, G, T = _int_case(23, B, K, V, D)
    clean_idx, _, status = _run(E, G, T, k, mode, slices=2)
    assert status == 0
    nan_row = int(clean_idx[0, 0])                          # a row that would be returned
    Tn = T.clone()
    Tn[nan_row, 3] = float("nan")
    idx, score, status = _run(E, G, Tn, k, mode, slices=2)
    assert status == E_NAN
    assert not bool((idx == nan_row).any())
    elig = torch.ones(V, dtype=torch.uint8)
    elig[nan_row] = 0
    want_idx, want_score, status = _run(E, G, T, k, mode, eligible=elig, slices=2)      # every other position unchanged
    assert status == 0
    assert torch.equal(idx, want_idx) and torch.equal(score.view(torch.int32), want_score.view(torch.int32))
    if mode != "weighted":
        ref_idx, ref_score = C.expected_topk(interest_scores64(E, T, mode, G)[0], k, eligible=elig)
        assert torch.equal(idx, ref_idx)
        assert mode == "mean" or torch.equal(score, ref_score)


@pytest.mark.parametrize("mode,where", [("weighted", "gate"), ("weighted", "interests"), ("max", "interests"), ("mean", "interests")])
def test_status_nan_in_one_users_row_blanks_that_user_alone(mode, where):
    """A NaN in one gate (or interest) row makes every aggregate of that user NaN: E_NAN, that user all -1 / -inf, the others
    unchanged."""
    B, K, V, D, k = 5, 3, 300, 12, 9
    E, G, T = _int_case(29, B, K, V, D)
    clean_idx, clean_score, status = _run(E, G, T, k, mode)
    assert status == 0
    En, Gn = E.clone(), G.clone()
    (Gn if where == "gate" else En)[2, 1, 5] = float("nan")
    idx, score, status = _run(En, Gn, T, k, mode)
    assert status == E_NAN
    assert torch.equal(idx[2], torch.full((k,), -1)) and bool((score[2] == float("-inf")).all())
    others = [0, 1, 3, 4]
    assert torch.equal(idx[others], clean_idx[others])
    assert torch.equal(score[others].view(torch.int32), clean_score[others].view(torch.int32))


# ---- 5. invariance and determinism ---------------------------------------------------------------------------------------------------
def test_invariance_and_determinism():
    """Bit-equal rows whatever the slicing, the batch (all 70 users one at a time), the GEMM engine setting (both are set here,
    inside the one test, on top of the fixture's) and on a second run."""
    from newsreclib_amd import _lib, ops
    B, K, V, D, k = 70, 32, 1000, 256, 10
    E, G, T = (t.cuda() for t in _real_case(31, B, K, V, D))
    G = G * 0.05                                            # logits of a few units: several interests share the weight

    def same(out, name):
        assert int(out[2]) == 0, name
        assert torch.equal(out[0], base[0]) and torch.equal(out[1].view(torch.int32), base[1].view(torch.int32)), name

    base = ops.topk_interest_scores(E, T, k, "weighted", G)
    assert int(base[2]) == 0 and bool((base[0] >= 0).all())
    for slices in (1, 2, 7, 0):
        same(ops.topk_interest_scores(E, T, k, "weighted", G, slices=slices), slices)
    singles = [ops.topk_interest_scores(E[b:b + 1], T, k, "weighted", G[b:b + 1]) for b in range(B)]
    same((torch.cat([s[0] for s in singles]), torch.cat([s[1] for s in singles]), sum(s[2] for s in singles)), "one at a time")
    prev = _lib.get_gemm_engine()
    try:
        for name in ("f32", "bf16x3"):
            _lib.set_gemm_engine(name)
            same(ops.topk_interest_scores(E, T, k, "weighted", G), name)
    finally:
        _lib.set_gemm_engine(prev)


# ---- 6. memory -------------------------------------------------------------------------------------------------------------------------
def test_peak_memory_is_far_below_the_score_matrix():
    from newsreclib_amd import ops
    B, K, V, D, k = 64, 8, 20000, 64, 10
    E, G, T = (t.cuda() for t in _real_case(2, B, K, V, D))
    for mode in MODES:
        gate = G if mode == "weighted" else None
        ops.topk_interest_scores(E[:2], T[:256], k, mode, gate[:2] if gate is not None else None)      # kernels resident
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        live = torch.cuda.memory_allocated()
        out = ops.topk_interest_scores(E, T, k, mode, gate)
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - live
        print(f"{mode}: peak above the inputs: {peak} bytes; (B K, V) score matrix: {B * K * V * 4} bytes")
        assert peak < B * K * V * 4 / 8, mode
        assert int(out[2]) == 0 and bool((out[0] >= 0).all())
        del out


# ---- 7. no read-back ---------------------------------------------------------------------------------------------------------------------
def test_topk_interest_scores_does_not_synchronise_with_the_host():
    from newsreclib_amd import ops
    E, G, T = (t.cuda() for t in _int_case(3, 5, 3, 200, 12))
    ei, eo = C.ragged([[1, 2], [], [5], [7, 7], []])
    ei, eo, elig = ei.cuda(), eo.cuda(), torch.ones(200, dtype=torch.bool).cuda()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        if not C.sync_debug_honoured():
            pytest.skip("this torch build does not raise on synchronising calls under set_sync_debug_mode('error')")
        outs = [ops.topk_interest_scores(E, T, 4, mode, G, ei, eo, elig) for mode in MODES]
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert all(int(o[2]) == 0 and o[0].shape == (5, 4) for o in outs)


# ---- 8. wiring -----------------------------------------------------------------------------------------------------------------------------

_WIRING = [("miner_tiny_no_bias", "max"), ("miner_tiny_no_bias", "mean"), ("miner_tiny_no_bias", "weighted"),
           ("miner_tiny_late_fusion", None), ("miner_tiny_eval", None)]


@pytest.mark.parametrize("name,score_type", _WIRING)
def test_recommend_interests_against_the_cache_scores(name, score_type, tmp_path):
    from newsreclib_amd import ops
    from newsreclib_amd.evaluation import recommend_users
    mod, cfg, cache, hist, hs = builders.miner_cache(name, score_type, tmp_path)
    mod.train()
    V, B = cache.table.num_news, int(hs.numel())
    k = min(10, V - int(hs.max()))
    lists = list(torch.split(hist, hs.tolist()))
    idx, score, status = cache.recommend_interests(hist.cuda(), hs, k)
    assert mod.training                                          # the mode is restored
    assert int(status) == 0 and idx.shape == (B, k)
    idx, score = idx.cpu(), score.cpu()
    mode = mod.interest_score_mode
    assert mode == ("mean" if cfg["late_fusion"] else cfg["score_type"])
    # the candidate list is the whole table for every user; the category bias (a function of the batch's candidate lists) is
    # not part of recommend_interests, so the scores to agree with are those with it switched off
    had_bias = mod.hparams.use_categ_bias
    mod.hparams.use_categ_bias = False
    try:
        full = cache.scores(hist, hs, torch.arange(V).repeat(B), torch.full((B,), V)).double().cpu()      # (B, V)
    finally:
        mod.hparams.use_categ_bias = had_bias
    assert mod.training
    vec = cache.vectors
    with torch.no_grad():
        mod.eval()
        interests, gate = mod.user_interests(ops.embedding_gather(vec, hist.cuda().reshape(-1, 1)).reshape(-1, vec.shape[1]),
                                             cache._user_meta(hs, None))
        mod.train()
    assert interests.shape == (B, 1 if cfg["late_fusion"] else cfg["K"], vec.shape[1])
    assert (gate is not None) == (mode == "weighted")
    _, tol = interest_scores64(interests.cpu(), vec.cpu(), mode, gate.cpu() if gate is not None else None)
    for b in range(B):
        rows = idx[b]
        assert bool((rows >= 0).all()) and not (set(rows.tolist()) & set(lists[b].tolist()))
        err = (score[b].double() - full[b, rows]).abs()
        print(f"user {b}: max |score - cache.scores| = {float(err.max()):.3e}, tol >= {float(tol[b, rows].min()):.3e}")
        assert bool((err <= tol[b, rows]).all())
        assert bool((score[b][1:] <= score[b][:-1]).all())
        rest = torch.ones(V, dtype=torch.bool)
        rest[rows] = False
        rest[lists[b]] = False
        assert bool((full[b][rest] <= full[b, rows].min() + 2 * tol[b][rest]).all())
    # without the exclusion the history may appear: every row of the table is returned when k is its length
    idx2, _, _ = cache.recommend_interests(hist.cuda(), hs, V, exclude_history=False)
    assert all(set(idx2[b].tolist()) == set(range(V)) for b in range(B))
    # recommend_users takes this entry for a multi-interest module: the same rows in the same order for the same batch
    users = [{"hist": lists[b], "user_id": 100 + b} for b in range(B)]
    recs = recommend_users(cache, users, k, batch_size=B + 3)
    assert list(recs) == [f"U{100 + b}" for b in range(B)]
    assert all(list(recs[f"U{100 + b}"]) == [f"N{int(i)}" for i in idx[b]] for b in range(B))
    assert list(recs["U100"].values()) == [float(v) for v in score[0]]
    # and `recommend` itself still refuses the module
    with pytest.raises(NotImplementedError, match="dot product"):
        cache.recommend(hist.cuda(), hs, k)


def test_recommend_interests_does_not_synchronise_with_the_host(tmp_path):
    mod, cfg, cache, hist, hs = builders.miner_cache("miner_tiny_no_bias", "weighted", tmp_path)
    mod.eval()
    cache.build()
    hist = hist.cuda()                                           # the sizes stay on the host, as recommend_users builds them
    cache.recommend_interests(hist, hs, 5)                       # library loaded, kernels resident
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        if not C.sync_debug_honoured():
            pytest.skip("this torch build does not raise on synchronising calls under set_sync_debug_mode('error')")
        idx, score, status = cache.recommend_interests(hist, hs, 5)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert int(status) == 0 and idx.shape == (int(hs.numel()), 5)
