"""Full-catalogue top-k recommendation (``nrl_topk_scores`` / ``ops.topk_scores`` / ``NewsVectorCache.recommend``).

Expected values are computed on the CPU in float64: ``s = U64 @ T64.T`` under the population and the order of
``tests/catalogue_ref.py`` (score descending, equal scores by ascending row).  Integer-valued vectors in [-4, 4] make every fp32
dot product exact in any order (|s| <= 16 * 768 < 2^24), so those cases compare with ``torch.equal``.  Real-valued cases use
``catalogue_ref.dot_bound``, the worst-case error of an fp32 dot product of length D (derived, not measured)."""
import pytest
import torch

from tests import builders
from tests import catalogue_ref as C

pytestmark = pytest.mark.gpu

E_EXCLUDE, E_OFFSETS, E_NAN = 1, 2, 4


@pytest.fixture(autouse=True, params=["f32", "bf16x3"])
def engine(request):
    from newsreclib_amd import _lib
    prev = _lib.get_gemm_engine()
    _lib.set_gemm_engine(request.param)
    yield request.param
    _lib.set_gemm_engine(prev)


def _reference(U, T, k, excl=None, eligible=None):
    """idx (B, k) int64 and score (B, k) float32 of the exact cases; -1 / -inf where fewer than k rows qualify."""
    return C.expected_topk(U.double() @ T.double().T, k, excl, eligible)


def _run(U, T, k, excl=None, eligible=None, slices=0, off=None):
    from newsreclib_amd import ops
    ei = eo = None
    if excl is not None:
        ei, eo = C.ragged(excl)
        ei, eo = ei.cuda(), (off if off is not None else eo).cuda()
    idx, score, status = ops.topk_scores(U.cuda(), T.cuda(), k, ei, eo, eligible.cuda() if eligible is not None else None, slices)
    return idx.cpu(), score.cpu(), int(status)


# ---- 1. exact, with ties --------------------------------------------------------------------------------------------------------
_EXACT = [(130, 1000, 300, 128, 1), (130, 1000, 300, 128, 2), (130, 1000, 300, 128, 7), (130, 1000, 768, 5, 0),
          (1, 1, 4, 1, 0), (1, 1, 4, 5, 0), (3, 63, 4, 128, 0), (3, 64, 300, 5, 1), (3, 65, 300, 128, 2), (1, 65, 768, 1, 7),
          (3, 1000, 4, 1, 7), (130, 63, 4, 5, 2), (1, 1000, 300, 5, 0), (130, 64, 768, 1, 0), (3, 65, 4, 5, 0)]


@pytest.mark.parametrize("B,V,D,k,slices", _EXACT)
def test_exact_with_ties(B, V, D, k, slices):
    U, T = C.int_vectors(B * 7 + V + D + k, B, V, D)
    idx, score, status = _run(U, T, k, slices=slices)
    want_idx, want_score = _reference(U, T, k)
    assert status == 0
    assert torch.equal(idx, want_idx)
    assert torch.equal(score, want_score)


@pytest.mark.parametrize("slices", [0, 2])
def test_all_equal_scores_return_the_first_rows(slices):
    U, T = torch.ones(3, 8), torch.ones(300, 8) * 2
    idx, score, status = _run(U, T, 16, slices=slices)
    assert status == 0
    assert torch.equal(idx, torch.arange(16).expand(3, 16))
    assert torch.equal(score, torch.full((3, 16), 16.0))


# ---- 2. exclusion and eligibility --------------------------------------------------------------------------------------------------
def _excl_case():
    B, V, D, k = 5, 40, 12, 16
    U, T = C.int_vectors(91, B, V, D)
    eligible = torch.ones(V, dtype=torch.uint8)
    eligible[[0, 7, 8, 31]] = 0
    first = _reference(U, T, k, eligible=eligible)[0][:, 0]           # every user's would-be first place
    everything = [v for v in range(V) if eligible[v]]
    excl = [[], [3, 3, 9, 3, 9], [int(first[2]), 5], everything, [int(first[4])] * 3 + [39, 1]]
    return U, T, k, excl, eligible


@pytest.mark.parametrize("slices", [0, 1])
def test_exclusion_and_eligibility(slices):
    U, T, k, excl, eligible = _excl_case()
    idx, score, status = _run(U, T, k, excl, eligible, slices)
    want_idx, want_score = _reference(U, T, k, excl, eligible)
    assert status == 0
    assert torch.equal(idx, want_idx) and torch.equal(score, want_score)
    assert torch.equal(idx[3], torch.full((k,), -1)) and bool(torch.isinf(score[3]).all())
    for b in range(len(excl)):
        got = set(idx[b].tolist()) - {-1}
        assert not (got & set(excl[b])) and not (got & {0, 7, 8, 31})


def test_exclusion_list_longer_than_the_cached_part():
    """Lists beyond the 64 entries a workgroup caches are read from global memory: 150 entries, several table tiles."""
    B, V, D, k = 3, 700, 8, 20
    U, T = C.int_vectors(5, B, V, D)
    g = torch.Generator().manual_seed(3)
    excl = [torch.randperm(V, generator=g)[:150].tolist(), [], _reference(U, T, 150)[0][2].tolist()]
    idx, score, status = _run(U, T, k, excl, slices=3)
    want_idx, want_score = _reference(U, T, k, excl)
    assert status == 0 and torch.equal(idx, want_idx) and torch.equal(score, want_score)


# ---- 3. status word ----------------------------------------------------------------------------------------------------------------
def test_status_bad_exclusion_index_is_ignored():
    U, T, k, excl, eligible = _excl_case()
    bad = [list(x) for x in excl]
    bad[1] = [-1] + bad[1]
    bad[2] = bad[2] + [T.shape[0]]
    idx, score, status = _run(U, T, k, bad, eligible)
    want_idx, want_score = _reference(U, T, k, excl, eligible)
    assert status == E_EXCLUDE
    assert torch.equal(idx, want_idx) and torch.equal(score, want_score)


def test_status_decreasing_offsets_blank_that_user_alone():
    B, V, D, k = 4, 40, 12, 6
    U, T = C.int_vectors(17, B, V, D)
    flat = list(range(12))
    off = torch.tensor([0, 5, 3, 8, 12])                    # user 1 runs backwards
    from newsreclib_amd import ops
    idx, score, status = ops.topk_scores(U.cuda(), T.cuda(), k, torch.tensor(flat).cuda(), off.cuda())
    idx, score = idx.cpu(), score.cpu()
    assert int(status) == E_OFFSETS
    want_idx, want_score = _reference(U, T, k, [flat[0:5], [], flat[3:8], flat[8:12]])
    for b in (0, 2, 3):
        assert torch.equal(idx[b], want_idx[b]) and torch.equal(score[b], want_score[b])
    assert torch.equal(idx[1], torch.full((k,), -1)) and bool((score[1] == float("-inf")).all())


def test_status_offsets_beyond_the_list():
    B, V, D, k = 3, 40, 12, 6
    U, T = C.int_vectors(18, B, V, D)
    from newsreclib_amd import ops
    idx, score, status = ops.topk_scores(U.cuda(), T.cuda(), k, torch.arange(6).cuda(), torch.tensor([0, 2, 9, 6]).cuda())
    assert int(status) == E_OFFSETS
    want_idx, _ = _reference(U, T, k, [[0, 1], [], []])
    assert torch.equal(idx.cpu()[0], want_idx[0])
    assert torch.equal(idx.cpu()[1:], torch.full((2, k), -1))


def test_status_nan_row_is_left_out():
    B, V, D, k = 5, 300, 12, 9
    U, T = C.int_vectors(23, B, V, D)
    clean_idx, clean_score, status = _run(U, T, k, slices=2)
    assert status == 0
    nan_row = int(clean_idx[0, 0])                          # a row that would be returned
    Tn = T.clone()
    Tn[nan_row, 3] = float("nan")
    idx, score, status = _run(U, Tn, k, slices=2)
    assert status == E_NAN
    assert not bool((idx == nan_row).any())
    elig = torch.ones(V, dtype=torch.uint8)
    elig[nan_row] = 0
    want_idx, want_score = _reference(U, T, k, eligible=elig)          # every other position unchanged
    assert torch.equal(idx, want_idx) and torch.equal(score, want_score)


# ---- 4. real values against float64 -------------------------------------------------------------------------------------------------
def test_real_values_against_float64():
    B, V, D, k = 37, 5000, 300, 10
    g = torch.Generator().manual_seed(12)
    U, T = torch.randn(B, D, generator=g), torch.randn(V, D, generator=g)
    excl = [torch.randint(0, V, (int(n),), generator=g).tolist() for n in torch.randint(0, 51, (B,), generator=g)]
    idx, score, status = _run(U, T, k, excl)
    assert status == 0
    raw = U.double() @ T.double().T
    C.check_floor(idx, score, raw, C.dot_bound(U, T), C.population(raw, excl)[0], k)


# ---- 5. invariance and determinism ---------------------------------------------------------------------------------------------------
def test_invariance_and_determinism():
    """Bit-equal rows whatever the slicing, the batch (all 130 users one at a time), the GEMM engine setting (both are set here,
    inside the one test, on top of the fixture's) and on a second run."""
    from newsreclib_amd import _lib, ops
    B, V, D, k = 130, 1000, 300, 10
    g = torch.Generator().manual_seed(31)
    U, T = torch.randn(B, D, generator=g).cuda(), torch.randn(V, D, generator=g).cuda()
    base_idx, base_score, _ = ops.topk_scores(U, T, k)
    for slices in (1, 2, 7, 0):
        idx, score, status = ops.topk_scores(U, T, k, slices=slices)
        assert int(status) == 0
        assert torch.equal(idx, base_idx) and torch.equal(score.view(torch.int32), base_score.view(torch.int32)), slices
    singles = [ops.topk_scores(U[b:b + 1], T, k) for b in range(B)]
    assert all(int(s[2]) == 0 for s in singles)
    assert torch.equal(torch.cat([s[0] for s in singles]), base_idx)
    assert torch.equal(torch.cat([s[1] for s in singles]).view(torch.int32), base_score.view(torch.int32))
    prev = _lib.get_gemm_engine()
    try:
        for name in ("f32", "bf16x3"):
            _lib.set_gemm_engine(name)
            idx, score, _ = ops.topk_scores(U, T, k)
            assert torch.equal(idx, base_idx) and torch.equal(score.view(torch.int32), base_score.view(torch.int32)), name
    finally:
        _lib.set_gemm_engine(prev)


# ---- 6. memory -------------------------------------------------------------------------------------------------------------------------
def test_peak_memory_is_far_below_the_score_matrix():
    from newsreclib_amd import ops
    B, V, D, k = 256, 60000, 64, 10
    g = torch.Generator().manual_seed(2)
    U, T = torch.randn(B, D, generator=g).cuda(), torch.randn(V, D, generator=g).cuda()
    ops.topk_scores(U[:2], T[:256], k)                      # library loaded, kernels resident
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    live = torch.cuda.memory_allocated()
    out = ops.topk_scores(U, T, k)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - live
    print(f"peak above the inputs: {peak} bytes; score matrix: {B * V * 4} bytes")
    assert peak < B * V * 4 / 8
    assert int(out[2]) == 0 and bool((out[0] >= 0).all())


# ---- 7. no read-back ---------------------------------------------------------------------------------------------------------------------
def test_topk_scores_does_not_synchronise_with_the_host():
    from newsreclib_amd import ops
    U, T = C.int_vectors(3, 5, 200, 12)
    U, T = U.cuda(), T.cuda()
    ei, eo = C.ragged([[1, 2], [], [5], [7, 7], []])
    ei, eo, elig = ei.cuda(), eo.cuda(), torch.ones(200, dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        if not C.sync_debug_honoured():
            pytest.skip("this torch build does not raise on synchronising calls under set_sync_debug_mode('error')")
        idx, score, status = ops.topk_scores(U, T, 4, ei, eo, elig)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert int(status) == 0 and idx.shape == (5, 4)


# ---- 8. wiring -----------------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("model,late", [("nrms", False), ("nrms", True), ("lstur_ini", False), ("lstur_con", False), ("naml", False),
                                        ("tanr", False), ("cen", False), ("mins", False), ("sentirec", False),
                                        ("manner_cr", False), ("manner_cr", True)])
def test_user_vectors_is_the_first_half_of_score_news_vectors(model, late, tmp_path):
    """Ragged histories, and histories that are all of the longest length (NRMS / SentiRec / the CR-Module then take the
    reshape path of ``dense_rows(..., max_is_exact=True)``)."""
    from newsreclib_amd import ops
    from newsreclib_amd.dense_batch import dense_rows
    from newsreclib_amd.evaluation import DeviceNewsTable, NewsVectorCache
    mod, table = builders.tiny(model, late, tmp_path)
    assert type(mod).dot_product_scorer is True
    table = table if isinstance(table, DeviceNewsTable) else DeviceNewsTable(table)
    cache = NewsVectorCache(mod, table, chunk=32)
    vec = cache.build()
    V = table.num_news
    for full in (False, True):
        _, hist, hs, uidx = builders.hist_batch(V, full=full)
        cand, cs = torch.arange(V).repeat(6), torch.full((6,), V)
        meta = cache._meta(hs, cs, None, uidx, None)
        hv = ops.embedding_gather(vec, hist.cuda().reshape(-1, 1)).reshape(-1, vec.shape[1])
        cv = ops.embedding_gather(vec, cand.cuda().reshape(-1, 1)).reshape(-1, vec.shape[1])
        with torch.no_grad():
            want = mod.score_news_vectors(hv, cv, meta)
            user = mod.user_vectors(hv, meta)
            cand_agg = dense_rows(cv, meta["batch_cand"], 6, meta["max_cand"], meta["cand_offsets"])
            got = mod.click_predictor(user.unsqueeze(dim=1), cand_agg.permute(0, 2, 1))
        assert user.shape == (6, vec.shape[1])
        assert torch.equal(got, want), full


@pytest.mark.parametrize("model", ["nrms", "lstur_ini"])
def test_recommend_against_the_cache_scores(model):
    from newsreclib_amd.evaluation import DeviceNewsTable, NewsVectorCache, recommend_users
    mod, attrs = builders.tiny(model)
    mod.train()
    cache = NewsVectorCache(mod, DeviceNewsTable(attrs), chunk=32)
    V, B, k = 50, 6, 10
    lists, hist, hs, uidx = builders.hist_batch(V)
    idx, score, status = cache.recommend(hist.cuda(), hs, k, user_idx=uidx)
    assert mod.training                                          # the mode is restored
    assert int(status) == 0 and idx.shape == (B, k)
    full = cache.scores(hist, hs, torch.arange(V).repeat(B), torch.full((B,), V), uidx).double().cpu()      # (B, V)
    assert mod.training
    idx, score = idx.cpu(), score.cpu()
    # bound of the dot product: the user vectors are not exposed by `scores`, so it is evaluated from recommend's own operands
    vec = cache.vectors
    from newsreclib_amd import ops
    with torch.no_grad():
        mod.eval()
        user = mod.user_vectors(ops.embedding_gather(vec, hist.cuda().reshape(-1, 1)).reshape(-1, vec.shape[1]),
                                cache._user_meta(hs, uidx))
        mod.train()
    bound = C.dot_bound(user.cpu(), vec.cpu())
    for b in range(B):
        rows = idx[b]
        assert bool((rows >= 0).all()) and not (set(rows.tolist()) & set(lists[b].tolist()))
        assert bool(((score[b].double() - full[b, rows]).abs() <= bound[b, rows]).all())
        rest = torch.ones(V, dtype=torch.bool)
        rest[rows] = False
        rest[lists[b]] = False
        assert bool((full[b][rest] <= full[b, rows].min() + 2 * bound[b][rest]).all())
    # without the exclusion the history may appear: the best row overall is returned whether it was read or not
    idx2, _, _ = cache.recommend(hist.cuda(), hs, V, user_idx=uidx, exclude_history=False)
    assert all(set(idx2[b].tolist()) == set(range(V)) for b in range(B))
    users = [{"hist": lists[b], "user_idx": uidx[b], "user_id": 100 + b} for b in range(B)]
    for batch_size in (4, 8):                                    # two batches (the second partial), one batch
        recs = recommend_users(cache, users, k, batch_size=batch_size)
        assert list(recs) == [f"U{100 + b}" for b in range(B)]
        assert all(0 < len(v) <= k for v in recs.values())
    # (the same batch composition as `recommend` above: NRMS' seq-first user attention couples the users of a batch)
    assert all(list(recs[f"U{100 + b}"]) == [f"N{int(i)}" for i in idx[b]] for b in range(B))
    assert list(recs["U100"].values()) == [float(v) for v in score[0]]


def test_recommend_does_not_synchronise_with_the_host():
    from newsreclib_amd.evaluation import DeviceNewsTable, NewsVectorCache
    mod, attrs = builders.tiny("nrms")
    cache = NewsVectorCache(mod, DeviceNewsTable(attrs), chunk=32)
    cache.build()
    _, hist, hs, _ = builders.hist_batch(50)
    hist = hist.cuda()                                           # the sizes stay on the host, as evaluate_impressions builds them
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        if not C.sync_debug_honoured():
            pytest.skip("this torch build does not raise on synchronising calls under set_sync_debug_mode('error')")
        idx, score, status = cache.recommend(hist, hs, 5)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert int(status) == 0 and idx.shape == (6, 5)
