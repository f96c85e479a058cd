"""Class-capped full-catalogue top-k (``nrl_topk_scores_capped`` / ``nrl_topk_ensemble_scores_capped``, ``ops.topk_scores_capped``
/ ``ops.topk_ensemble_scores_capped``, ``NewsVectorCache.recommend_capped`` / ``MannerVectorCache.recommend_ensemble_capped``).

Expected values come from the greedy definition on the CPU (``tests/topk_capped_ref.py``): the float64 scores and the
population of ``tests/catalogue_ref.py``, walked in the family's order, a row taken iff fewer than m rows of its class have been.
Integer-valued vectors in [-4, 4] make every fp32 dot product exact, so the lists compare with ``torch.equal``.  The ensemble's
scores are real-valued: there the walk runs over the bit-equal scores the uncapped entry returns for the same call."""
import pytest
import torch

from tests import builders
from tests import catalogue_ref as C
from tests import topk_capped_ref as R

pytestmark = pytest.mark.gpu

E_NAN, E_STATS = 4, 8


@pytest.fixture(autouse=True, params=["f32", "bf16x3"])
def engine(request):
    from newsreclib_amd import _lib
    prev = _lib.get_gemm_engine()
    _lib.set_gemm_engine(request.param)
    yield request.param
    _lib.set_gemm_engine(prev)


def _classes(seed, V, n_cls):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, n_cls, (V,), generator=g).to(torch.int32) * 7 - 3          # (any int32 is a class, negatives too)


def _run(U, T, k, cls, m, excl=None, eligible=None, slices=0):
    from newsreclib_amd import ops
    ei = eo = None
    if excl is not None:
        ei, eo = C.ragged(excl)
        ei, eo = ei.cuda(), eo.cuda()
    idx, score, status = ops.topk_scores_capped(U.cuda(), T.cuda(), k, cls.cuda(), m, ei, eo,
                                                eligible.cuda() if eligible is not None else None, slices)
    return idx.cpu(), score.cpu(), int(status)


def _reference(U, T, cls, k, m, excl=None, eligible=None):
    s = U.double() @ T.double().T
    return R.reference(s, C.population(s, excl, eligible)[0], cls, k, m)


# ---- 1. exact, with ties: every B, V, D, k, m, class count and slicing of the issue appears ------------------------------------------
_EXACT = [(130, 1000, 300, 64, 2, 19, 7), (130, 1000, 4, 5, 1, 3, 0), (3, 1000, 300, 64, 64, 19, 2), (1, 1000, 300, 5, 2, 1, 1),
          (1, 1, 4, 1, 1, 1, 0), (3, 1, 4, 5, 2, 3, 0), (3, 63, 4, 64, 1, 19, 0), (130, 64, 300, 5, 5, 3, 1), (3, 65, 300, 64, 2, 3, 2),
          (1, 65, 4, 1, 1, 19, 7), (3, 129, 300, 5, 2, 19, 2), (130, 129, 4, 64, 2, 3, 7), (1, 129, 4, 64, 1, 1, 0),
          (3, 1000, 4, 1, 1, 3, 7), (130, 63, 4, 5, 1, 19, 2), (3, 64, 4, 64, 64, 1, 0)]


@pytest.mark.parametrize("B,V,D,k,m,n_cls,slices", _EXACT)
def test_exact_with_ties(B, V, D, k, m, n_cls, slices):
    U, T = C.int_vectors(B * 7 + V + D + k + m, B, V, D)
    cls = _classes(V + n_cls, V, n_cls)
    idx, score, status = _run(U, T, k, cls, m, slices=slices)
    want_idx, want_score = _reference(U, T, cls, k, m)
    assert status == 0
    assert torch.equal(idx, want_idx)
    assert torch.equal(score, want_score)


@pytest.mark.parametrize("slices", [0, 3])
def test_one_class_and_a_cap_of_one_return_one_row(slices):
    U, T = C.int_vectors(8, 5, 700, 12)
    cls = torch.full((700,), 11, dtype=torch.int32)
    idx, score, status = _run(U, T, 6, cls, 1, slices=slices)
    assert status == 0
    assert torch.equal(idx[:, 0], C.expected_topk(U.double() @ T.double().T, 1)[0][:, 0])
    assert torch.equal(idx[:, 1:], torch.full((5, 5), -1)) and bool((score[:, 1:] == float("-inf")).all())


# ---- 2. the two paths of the insertion -------------------------------------------------------------------------------------------------
def _ramp(V, descending):
    """One user; row v of class 5 (v % 3 != 0) scores v + 1 ascending along the table (or V - v descending), the rows of class 9
    (v % 3 == 0) score 0.  D = 4: u = (1, 0, 0, 0), row = (score, 0, 0, 0)."""
    U = torch.tensor([[1.0, 0.0, 0.0, 0.0]])
    v = torch.arange(V)
    s = torch.where(v % 3 != 0, (V - v if descending else v + 1), torch.zeros_like(v)).float()
    T = torch.zeros(V, 4)
    T[:, 0] = s
    return U, T, torch.where(v % 3 != 0, 5, 9).to(torch.int32)


@pytest.mark.parametrize("slices", [1, 3, 0])
@pytest.mark.parametrize("descending", [False, True], ids=["displacement", "rejection"])
def test_a_full_class_is_displaced_by_better_rows_and_rejects_worse_ones(descending, slices):
    """Ascending: every tile's rows of class 5 beat the list's, so each one evicts the class's worst entry (never the list's last,
    which is of class 9).  Descending: the first rows fill the class and every later one is dropped by its class."""
    V, k, m = 700, 8, 3                                     # six tiles; three slices of two
    U, T, cls = _ramp(V, descending)
    idx, score, status = _run(U, T, k, cls, m, slices=slices)
    want_idx, want_score = _reference(U, T, cls, k, m)
    assert status == 0 and torch.equal(idx, want_idx) and torch.equal(score, want_score)
    top5 = [1, 2, 4] if descending else [698, 697, 695]
    assert idx[0].tolist() == top5 + [0, 3, 6, -1, -1]      # three of class 5, then class 9's first three (ties: lowest rows)


@pytest.mark.parametrize("slices", [1, 2, 0])
def test_ties_across_tile_and_slice_borders_go_to_the_lower_row(slices):
    """Rows 126 ... 129 (the border of the first two tiles) and 254 ... 257 (with two slices of two tiles: the slice border) all
    score 7 in class 1; everything else scores less.  m = 3 keeps rows 126, 127, 128: one from beyond the tile border, none
    from beyond the slice border."""
    V = 512
    U = torch.tensor([[1.0, 0.0, 0.0, 0.0]] * 2)
    T = torch.zeros(V, 4)
    T[:, 0] = 1.0
    tie = [126, 127, 128, 129, 254, 255, 256, 257]
    T[tie, 0] = 7.0
    cls = torch.zeros(V, dtype=torch.int32)
    cls[tie] = 1
    idx, score, status = _run(U, T, 5, cls, 3, slices=slices)
    assert status == 0
    assert idx.tolist() == [[126, 127, 128, 0, 1]] * 2
    assert score.tolist() == [[7.0, 7.0, 7.0, 1.0, 1.0]] * 2
    # with the lower rows excluded for user 1 the tie moves across the slice border
    idx, _, _ = _run(U, T, 5, cls, 3, excl=[[], [126, 127, 128, 129, 254]], slices=slices)
    assert idx.tolist() == [[126, 127, 128, 0, 1], [255, 256, 257, 0, 1]]


# ---- 3. exclusion, eligibility, NaN: what is removed never counts toward a cap -----------------------------------------------------------
def _removal_case():
    B, V, D, k, m = 4, 300, 12, 10, 2
    U, T = C.int_vectors(77, B, V, D)
    cls = _classes(5, V, 4)
    base_idx, _ = _reference(U, T, cls, k, m)
    return B, V, k, m, U, T, cls, base_idx


def _next_of_class(U, T, cls, b, row, k, m, excl=None):
    """user b's capped list once `row` is gone, and the rows in it that were not there before (``excl``: lists in force
    before and after)"""
    s = U.double() @ T.double().T
    pop = C.population(s, excl)[0]
    before = set(R.reference(s, pop, cls, k, m)[0][b].tolist())
    pop[b, row] = False
    after = R.reference(s, pop, cls, k, m)[0][b].tolist()
    return after, [v for v in after if v not in before]


@pytest.mark.parametrize("slices", [0, 2])
def test_excluding_the_best_row_of_a_full_class_admits_the_next(slices):
    B, V, k, m, U, T, cls, base_idx = _removal_case()
    first = [int(base_idx[b, 0]) for b in range(B)]
    g = torch.Generator().manual_seed(1)
    long_list = [v for v in torch.randperm(V, generator=g)[:150].tolist() if v not in base_idx[3].tolist()]      # > 64 entries
    assert len(long_list) > 64
    others = [[], [], [], long_list]
    excl = [[first[0]], [], [first[2]] * 3, long_list + [first[3]]]
    idx, score, status = _run(U, T, k, cls, m, excl=excl, slices=slices)
    want_idx, want_score = _reference(U, T, cls, k, m, excl)
    assert status == 0 and torch.equal(idx, want_idx) and torch.equal(score, want_score)
    for b in (0, 2, 3):
        after, new = _next_of_class(U, T, cls, b, first[b], k, m, others)
        assert len(new) == 1 and int(cls[new[0]]) == int(cls[first[b]])          # the class's next row came in
        assert idx[b].tolist() == after and first[b] not in after
    assert torch.equal(idx[1], base_idx[1])


def test_an_ineligible_row_does_not_count_toward_the_cap():
    B, V, k, m, U, T, cls, base_idx = _removal_case()
    gone = int(base_idx[0, 0])
    elig = torch.ones(V, dtype=torch.uint8)
    elig[gone] = 0
    idx, score, status = _run(U, T, k, cls, m, eligible=elig, slices=2)
    want_idx, want_score = _reference(U, T, cls, k, m, eligible=elig)
    assert status == 0 and torch.equal(idx, want_idx) and torch.equal(score, want_score)
    _, new = _next_of_class(U, T, cls, 0, gone, k, m)
    assert len(new) == 1 and int(cls[new[0]]) == int(cls[gone]) and new[0] in idx[0].tolist()
    assert sum(int(cls[v]) == int(cls[gone]) for v in idx[0].tolist()) == m


def test_a_nan_row_is_flagged_left_out_and_does_not_count_toward_the_cap():
    B, V, k, m, U, T, cls, base_idx = _removal_case()
    gone = int(base_idx[0, 0])
    Tn = T.clone()
    Tn[gone, 3] = float("nan")
    idx, score, status = _run(U, Tn, k, cls, m, slices=2)
    elig = torch.ones(V, dtype=torch.uint8)
    elig[gone] = 0
    want_idx, want_score = _reference(U, T, cls, k, m, eligible=elig)      # every other position unchanged
    assert status == E_NAN
    assert torch.equal(idx, want_idx) and torch.equal(score, want_score)
    assert not bool((idx == gone).any())
    assert sum(int(cls[v]) == int(cls[gone]) for v in idx[0].tolist()) == m


# ---- 4. agreement with the uncapped entry ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,V,D,k,m,slices", [(130, 1000, 300, 64, 64, 0), (3, 1000, 300, 10, 10, 7), (65, 129, 768, 5, 2 ** 31 - 1, 2)])
def test_a_cap_of_k_or_more_returns_the_bits_of_topk_scores(B, V, D, k, m, slices):
    from newsreclib_amd import ops
    g = torch.Generator().manual_seed(B + V)
    U, T = torch.randn(B, D, generator=g).cuda(), torch.randn(V, D, generator=g).cuda()
    T[5] = T[9]                                              # (a tie between real values)
    cls = _classes(3, V, 3).cuda()
    excl_idx, excl_off = C.ragged([[5, 7]] + [[] for _ in range(B - 1)])
    got = ops.topk_scores_capped(U, T, k, cls, m, excl_idx.cuda(), excl_off.cuda(), slices=slices)
    want = ops.topk_scores(U, T, k, excl_idx.cuda(), excl_off.cuda(), slices=slices)
    assert int(got[2]) == int(want[2]) == 0
    assert torch.equal(got[0], want[0]) and torch.equal(C.bits(got[1]), C.bits(want[1]))


def test_every_returned_score_has_the_bits_of_the_uncapped_entry():
    from newsreclib_amd import ops
    B, V, D, k, m = 9, 128, 300, 8, 2
    g = torch.Generator().manual_seed(6)
    U, T = torch.randn(B, D, generator=g).cuda(), torch.randn(V, D, generator=g).cuda()
    cls = _classes(4, V, 5)
    idx, score, status = ops.topk_scores_capped(U, T, k, cls.cuda(), m)
    all_idx, all_score, _ = ops.topk_scores(U, T, V)
    assert int(status) == 0
    want_idx, want_score, decided = R.walk_listed(all_idx.cpu(), all_score.cpu(), cls, k, m)
    assert decided
    assert torch.equal(idx.cpu(), want_idx) and torch.equal(C.bits(score.cpu()), C.bits(want_score))


# ---- 5. invariance ---------------------------------------------------------------------------------------------------------------------------
def test_invariance_under_batch_slicing_and_engine():
    from newsreclib_amd import _lib, ops
    B, V, D, k, m = 130, 1000, 300, 10, 2
    g = torch.Generator().manual_seed(31)
    U, T = torch.randn(B, D, generator=g).cuda(), torch.randn(V, D, generator=g).cuda()
    cls = _classes(9, V, 19).cuda()
    base_idx, base_score, status = ops.topk_scores_capped(U, T, k, cls, m)
    assert int(status) == 0
    per = torch.stack([(cls[base_idx] == c).sum(1) for c in cls.unique()], 1)
    assert int(per.max()) <= m and bool((base_idx >= 0).all())
    for slices in (1, 2, 7, 0):
        idx, score, _ = ops.topk_scores_capped(U, T, k, cls, m, slices=slices)
        assert torch.equal(idx, base_idx) and torch.equal(C.bits(score), C.bits(base_score)), slices
    for b in (0, 63, 64, 129):                               # a user alone against the same user inside the batch of 130
        idx, score, _ = ops.topk_scores_capped(U[b:b + 1], T, k, cls, m)
        assert torch.equal(idx[0], base_idx[b]) and torch.equal(C.bits(score[0]), C.bits(base_score[b])), b
    prev = _lib.get_gemm_engine()
    try:
        for name in ("f32", "bf16x3"):
            _lib.set_gemm_engine(name)
            idx, score, _ = ops.topk_scores_capped(U, T, k, cls, m)
            assert torch.equal(idx, base_idx) and torch.equal(C.bits(score), C.bits(base_score)), name
    finally:
        _lib.set_gemm_engine(prev)
    # int64 classes are the same classes
    idx, score, _ = ops.topk_scores_capped(U, T, k, cls.long(), m)
    assert torch.equal(idx, base_idx) and torch.equal(C.bits(score), C.bits(base_score))


# ---- 6. argument checks, no read-back ---------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_before_any_launch():
    from newsreclib_amd import ops
    U, T = C.int_vectors(3, 5, 200, 12)
    U, T, cls = U.cuda(), T.cuda(), _classes(1, 200, 3).cuda()
    with pytest.raises(RuntimeError, match=r"k in \[1, 64\]"):
        ops.topk_scores_capped(U, T, 65, cls, 2)
    with pytest.raises(RuntimeError, match="max_per_class"):
        ops.topk_scores_capped(U, T, 5, cls, 0)
    with pytest.raises(ValueError, match="row_class"):
        ops.topk_scores_capped(U, T, 5, None, 2)
    with pytest.raises(ValueError, match="one entry per table row"):
        ops.topk_scores_capped(U, T, 5, cls[:199], 2)
    with pytest.raises(ValueError, match="one entry per table row"):
        ops.topk_ensemble_scores_capped([U], [T], [1.0], 5, cls[:199], 2)
    with pytest.raises(RuntimeError, match="max_per_class"):
        ops.topk_ensemble_scores_capped([U], [T], [1.0], 5, cls, 0)
    with pytest.raises(RuntimeError, match=r"k in \[1, 64\]"):
        ops.topk_ensemble_scores_capped([U], [T], [1.0], 65, cls, 2)
    torch.cuda.synchronize()                                 # nothing was launched: nothing can have gone wrong on the device
    idx, _, status = ops.topk_scores_capped(U, T, 5, cls, 2)
    assert int(status) == 0 and bool((idx >= 0).all())


def test_capped_entries_do_not_synchronise_with_the_host():
    from newsreclib_amd import ops
    U, T = C.int_vectors(3, 5, 200, 12)
    U, T = U.cuda(), T.cuda()
    ei, eo = C.ragged([[1, 2], [], [5], [7, 7], []])
    ei, eo, elig = ei.cuda(), eo.cuda(), torch.ones(200, dtype=torch.uint8).cuda()
    cls32, cls64 = _classes(1, 200, 3).cuda(), _classes(1, 200, 3).long().cuda()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        if not C.sync_debug_honoured():
            pytest.skip("this torch build does not raise on synchronising calls under set_sync_debug_mode('error')")
        idx, score, status = ops.topk_scores_capped(U, T, 4, cls32, 1, ei, eo, elig)
        idx64, _, _ = ops.topk_scores_capped(U, T, 4, cls64, 1, ei, eo, elig)
        ens = ops.topk_ensemble_scores_capped([U, U], [T, T], [1.0, 0.5], 4, cls64, 1, ei, eo, elig)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert int(status) == 0 and idx.shape == (5, 4) and torch.equal(idx, idx64)
    assert int(ens[2]) == 0 and ens[0].shape == (5, 4) and ens[3].shape == (5, 2, 2)


# ---- 7. the ensemble --------------------------------------------------------------------------------------------------------------------------
def _ensemble_case(seed, B, V, D, T=3):
    from tests.topk_ensemble_ref import real_case
    users, tables = real_case(seed, T, B, V, D)
    return [u.cuda() for u in users], [t.cuda() for t in tables], [1.0, 0.2, -0.25][:T]


@pytest.mark.parametrize("V,k,m,slices", [(128, 10, 2, 0), (65, 64, 1, 1), (100, 5, 5, 2)])
def test_ensemble_is_the_greedy_walk_over_the_uncapped_scores(V, k, m, slices):
    from newsreclib_amd import ops
    B, D = 70, 32
    users, tables, weights = _ensemble_case(V, B, V, D)
    users[0][4] = float("nan")                              # user 4 cannot be standardised
    cls = _classes(2, V, 3)
    excl_idx, excl_off = C.ragged([[1, 2, 3]] + [[] for _ in range(B - 1)])
    elig = torch.ones(V, dtype=torch.uint8)
    elig[0] = 0
    tail = (excl_idx.cuda(), excl_off.cuda(), elig.cuda())
    idx, score, status, stats = ops.topk_ensemble_scores_capped(users, tables, weights, k, cls.cuda(), m, *tail, slices=slices)
    all_idx, all_score, all_status, all_stats = ops.topk_ensemble_scores(users, tables, weights, V, *tail)
    assert int(status) == int(all_status) and int(status) & E_STATS
    assert torch.equal(C.bits(stats), C.bits(all_stats))
    want_idx, want_score, decided = R.walk_listed(all_idx.cpu(), all_score.cpu(), cls, k, m)
    assert decided
    assert torch.equal(idx.cpu(), want_idx) and torch.equal(C.bits(score.cpu()), C.bits(want_score))
    assert torch.equal(idx[4].cpu(), torch.full((k,), -1)) and bool((score[4] == float("-inf")).all())      # blank and flagged
    assert bool((idx[:4] >= 0)[:, :min(k, 3 * m)].all())


def test_ensemble_over_a_long_table_walks_the_uncapped_list():
    """V = 1000, 19 uniform classes, m = 2, k = 10: the uncapped list of 128 decides the walk -- a condition on the inputs (seed
    chosen so that the float64 ensemble of the same inputs needs at most 60 entries for every user), asserted, not assumed."""
    from newsreclib_amd import ops
    B, V, D, k, m = 66, 1000, 32, 10, 2
    users, tables, weights = _ensemble_case(1000, B, V, D)
    cls = _classes(19, V, 19)
    idx, score, status, stats = ops.topk_ensemble_scores_capped(users, tables, weights, k, cls.cuda(), m, slices=3)
    all_idx, all_score, _, all_stats = ops.topk_ensemble_scores(users, tables, weights, 128)
    assert int(status) == 0 and torch.equal(C.bits(stats), C.bits(all_stats))
    want_idx, want_score, decided = R.walk_listed(all_idx.cpu(), all_score.cpu(), cls, k, m)
    assert decided
    assert torch.equal(idx.cpu(), want_idx) and torch.equal(C.bits(score.cpu()), C.bits(want_score))


# ---- 8. cache level -----------------------------------------------------------------------------------------------------------------------------
def _per_class_max(idx, cls):
    worst = 0
    for row in idx.tolist():
        seen = {}
        for v in row:
            if v >= 0:
                seen[int(cls[v])] = seen.get(int(cls[v]), 0) + 1
        worst = max(worst, max(seen.values(), default=0))
    return worst


def test_recommend_capped_is_the_walk_over_recommend():
    from newsreclib_amd.evaluation import DeviceNewsTable, NewsVectorCache, recommend_users
    from newsreclib_amd.metrics import aspect_metrics, recommendation_aspect_metrics
    mod, attrs = builders.tiny("nrms")
    cache = NewsVectorCache(mod, DeviceNewsTable(attrs), chunk=32)
    V, B, k, m = 50, 6, 10, 2
    lists, hist, hs, uidx = builders.hist_batch(V)
    cls = cache.table.attrs["category"].cpu()
    mod.train()
    idx, score, status = cache.recommend_capped(hist.cuda(), hs, k, "category", m, user_idx=uidx)
    assert mod.training and int(status) == 0
    all_idx, all_score, _ = cache.recommend(hist.cuda(), hs, 128, user_idx=uidx)
    want_idx, want_score, decided = R.walk_listed(all_idx.cpu(), all_score.cpu(), cls, k, m)
    assert decided and torch.equal(idx.cpu(), want_idx) and torch.equal(C.bits(score.cpu()), C.bits(want_score))
    assert _per_class_max(idx.cpu(), cls) <= m
    kept = cache._row_class["category"]
    assert kept.dtype == torch.int32
    cache.recommend_capped(hist.cuda(), hs, k, "category", m, user_idx=uidx)
    assert cache._row_class["category"] is kept                  # converted once per aspect, kept on the cache
    with pytest.raises(ValueError, match="no such `title`"):
        cache.recommend_capped(hist.cuda(), hs, k, "title", m)
    # recommend_users: without a cap the dictionary of before, with one the capped lists
    users = [{"hist": lists[b], "user_idx": uidx[b], "user_id": 100 + b} for b in range(B)]
    plain_idx, plain_score, _ = cache.recommend(hist.cuda(), hs, k, user_idx=uidx)
    recs = recommend_users(cache, users, k, batch_size=8)
    assert recs == recommend_users(cache, users, k, batch_size=8, cap=None)
    assert all(list(recs[f"U{100 + b}"]) == [f"N{int(i)}" for i in plain_idx[b]] for b in range(B))
    capped = recommend_users(cache, users, k, batch_size=8, cap=("category", m))
    assert all(list(capped[f"U{100 + b}"]) == [f"N{int(i)}" for i in idx[b] if i >= 0] for b in range(B))
    assert list(capped["U100"].values()) == [float(v) for v in score[0] if v > float("-inf")]
    # what the cap bought, in the library's own metric: equal to aspect_metrics (torch) on the same lists
    n_cls = int(cls.max()) + 1
    hist_off = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(hs, 0)]).cuda()
    for got_idx, got_score in ((idx, score), (plain_idx, plain_score)):
        got = recommendation_aspect_metrics(got_idx, got_score, cls.cuda(), hist.cuda(), hist_off, n_cls, (5, 10), "categ")
        valid = got_idx >= 0
        want = aspect_metrics(got_score[valid], cls.cuda()[got_idx[valid]], cls.cuda()[hist.cuda()], valid.sum(1), hs.cuda(), n_cls,
                              (5, 10), prefix="categ")
        assert set(got) == set(want) == {"categ_div@5", "categ_pers@5", "categ_div@10", "categ_pers@10"}
        for key in want:
            print(f"{key}: {got[key]:.7f} against {want[key]:.7f}")
            assert abs(got[key] - want[key]) <= 2e-5, key


def test_recommend_users_refuses_a_cap_for_the_other_scorers():
    from types import SimpleNamespace
    from newsreclib_amd.evaluation import recommend_users
    for flag in ("multi_interest_scorer", "dnn_predictor_scorer", "personalized_pooling_scorer"):
        cache = SimpleNamespace(module=SimpleNamespace(**{flag: True}), table=None)
        with pytest.raises(NotImplementedError, match="does not exist yet"):
            recommend_users(cache, [{"hist": torch.tensor([1])}], 5, cap=("category", 2))


def test_recommend_ensemble_capped_is_the_walk_over_recommend_ensemble(tmp_path):
    from newsreclib_amd.evaluation import MannerVectorCache, recommend_users
    cr, ac, asent = builders.manner_modules(tmp_path)
    ens = builders.manner_ensemble(cr, ac, asent)
    table, imps = builders.manner_table_and_impressions()
    B, k, m = len(imps), 10, 2
    cache = MannerVectorCache(ens, table)
    lists = [i["hist"] for i in imps]
    hs, hist = torch.tensor([len(x) for x in lists]), torch.cat(lists)
    cls = table.attrs["category"].cpu()
    idx, score, status, stats = cache.recommend_ensemble_capped(hist.cuda(), hs, k, "category", m, return_stats=True)
    all_idx, all_score, _, all_stats = cache.recommend_ensemble(hist.cuda(), hs, 128, return_stats=True)
    assert int(status) == 0 and torch.equal(C.bits(stats), C.bits(all_stats))
    want_idx, want_score, decided = R.walk_listed(all_idx.cpu(), all_score.cpu(), cls, k, m)
    assert decided and torch.equal(idx.cpu(), want_idx) and torch.equal(C.bits(score.cpu()), C.bits(want_score))
    assert _per_class_max(idx.cpu(), cls) <= m and len(cache.recommend_ensemble_capped(hist.cuda(), hs, k, "category", m)) == 3
    users = [{"hist": lists[b], "user_id": 100 + b} for b in range(B)]
    capped = recommend_users(cache, users, k, batch_size=B + 3, cap=("category", m))
    assert all(list(capped[f"U{100 + b}"]) == [f"N{int(i)}" for i in idx[b] if i >= 0] for b in range(B))
    plain_idx, _, _ = cache.recommend_ensemble(hist.cuda(), hs, k)
    plain = recommend_users(cache, users, k, batch_size=B + 3)
    assert all(list(plain[f"U{100 + b}"]) == [f"N{int(i)}" for i in plain_idx[b]] for b in range(B))
