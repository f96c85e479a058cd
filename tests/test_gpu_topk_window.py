"""Per-user time windows on the full-catalogue top-k and rank (``nrl_topk_window_scores`` / ``nrl_catalogue_window_ranks``, their
``ops`` wrappers, ``NewsVectorCache.recommend`` / ``rank_clicks`` with ``window=``, ``recommend_users(window=)`` and
``evaluate_full_rank(until_request=True)``).

Expected values come from ``tests/topk_window_ref.py`` (CPU, float64), which ANDs the window into the population of
``tests/catalogue_ref.py``.  Integer-valued vectors in [-4, 4] make every fp32 dot product exact in any order, so every comparison
is ``catalogue_ref.same``: bit equality, ties included.  The real-valued cases have an exact oracle that needs no tolerance: the
plain entries called for one user at a time with that user's window folded into ``eligible``.  Sorted time columns (``row // 16``:
a tile's rows share 8 time values, so whole tiles fall outside a window and are skipped) and shuffled ones (no tile can be
skipped) run against the same reference."""
import pytest
import torch

from tests import builders
from tests import catalogue_ref as C
from tests import topk_window_ref as R

pytestmark = pytest.mark.gpu

E_EXCLUDE, E_OFFSETS, E_NAN, E_TARGETS, E_TARGET_ROW = 1, 2, 4, 16, 32
NEG_INF = float("-inf")
SHAPES = [(1, 1, 4), (3, 130, 20), (65, 129, 4), (70, 700, 36), (5, 128, 1024)]
_REF = {}                                                  # float64 expectations, computed once for both engines


@pytest.fixture(autouse=True, params=["f32", "bf16x3"])
def engine(request):
    from newsreclib_amd import _lib
    prev = _lib.get_gemm_engine()
    _lib.set_gemm_engine(request.param)
    yield request.param
    _lib.set_gemm_engine(prev)


def _cuda(t):
    return t.cuda() if t is not None else None


def _topk(U, T, k, row_time, lo, hi, excl=None, eligible=None, slices=0, excl_off=None):
    from newsreclib_amd import ops
    ei = eo = None
    if excl is not None:
        ei, eo = C.ragged(excl)
        ei, eo = ei.cuda(), (excl_off if excl_off is not None else eo).cuda()
    idx, score, status = ops.topk_window_scores(U.cuda(), T.cuda(), k, row_time.cuda(), lo.cuda(), hi.cuda(), ei, eo, _cuda(eligible),
                                                slices)
    return idx.cpu(), score.cpu(), int(status)


def _ranks(U, T, targets, row_time, lo, hi, excl=None, eligible=None, slices=0, excl_off=None):
    from newsreclib_amd import ops
    ti, to = C.ragged(targets)
    ei = eo = None
    if excl is not None:
        ei, eo = C.ragged(excl)
        ei, eo = ei.cuda(), (excl_off if excl_off is not None else eo).cuda()
    rank, score, ranked, status = ops.catalogue_window_ranks(U.cuda(), T.cuda(), ti.cuda(), to.cuda(), row_time.cuda(), lo.cuda(),
                                                             hi.cuda(), ei, eo, _cuda(eligible), slices)
    return rank.cpu(), score.cpu(), ranked.cpu(), int(status)


def _times(V, shuffled, seed=0):
    t = (torch.arange(V) // 16).to(torch.int32)
    return t[torch.randperm(V, generator=torch.Generator().manual_seed(1000 + seed))] if shuffled else t


def _case(B, V, D, shuffled, shift=0):
    """Integer vectors, targets (0 to 4 a user), exclusion lists (0 to 9, duplicates allowed), a mixed mask, the time column and
    the window mix from kind ``shift`` on."""
    seed = B * 7 + V + D
    U, T = C.int_vectors(seed, B, V, D)
    g = torch.Generator().manual_seed(seed + 1)
    targets = [torch.randint(0, V, (int(n),), generator=g).tolist() for n in torch.randint(0, 5, (B,), generator=g)]
    targets[0] = targets[0] or [0]
    excl = [torch.randint(0, V, (int(n),), generator=g).tolist() for n in torch.randint(0, 10, (B,), generator=g)]
    eligible = (torch.rand(V, generator=g) > 0.15).to(torch.uint8)
    row_time = _times(V, shuffled, seed)
    lo, hi = R.window_mix(B, row_time, shift)
    return U, T, targets, excl, eligible, row_time, lo, hi


def _want(key, make):
    if key not in _REF:
        _REF[key] = make()
    return _REF[key]


# ---- 1. exact, with ties, against the reference -------------------------------------------------------------------------------------
@pytest.mark.parametrize("shuffled", [False, True], ids=["sorted", "shuffled"])
@pytest.mark.parametrize("B,V,D", SHAPES)
def test_exact_with_ties(B, V, D, shuffled):
    for shift in ((0, 3, 6) if B < 9 else (0,)):                 # (few users: every kind of window still gets its turn)
        U, T, targets, excl, eligible, row_time, lo, hi = _case(B, V, D, shuffled, shift)
        s = U.double() @ T.double().T
        for masks in ((None, None), (excl, eligible)):
            for k in (1, 10):
                want = _want(("topk", B, V, D, shuffled, shift, masks[0] is None, k),
                             lambda: R.expected_topk(s, k, row_time, lo, hi, *masks))
                idx, score, status = _topk(U, T, k, row_time, lo, hi, *masks)
                assert status == 0 and C.same((idx, score), want), (shift, k, masks[0] is None)
            want = _want(("rank", B, V, D, shuffled, shift, masks[0] is None), lambda: R.expected_ranks(s, targets, row_time, lo, hi, *masks))
            rank, score, ranked, status = _ranks(U, T, targets, row_time, lo, hi, *masks)
            assert status == 0 and C.same((rank, score, ranked), want), (shift, masks[0] is None)
            assert C.same(ranked, R.population(s, row_time, lo, hi, *masks)[0].sum(1).to(torch.int32))


@pytest.mark.parametrize("shuffled", [False, True], ids=["sorted", "shuffled"])
def test_exact_k_128(shuffled):
    U, T, targets, excl, eligible, row_time, lo, hi = _case(70, 700, 36, shuffled)
    s = U.double() @ T.double().T
    want = _want(("topk128", shuffled), lambda: R.expected_topk(s, 128, row_time, lo, hi, excl, eligible))
    idx, score, status = _topk(U, T, 128, row_time, lo, hi, excl, eligible)
    assert status == 0 and C.same((idx, score), want)
    assert bool((idx[6] == -1).all()) and bool((score[6] == NEG_INF).all())      # user 6: the empty window


# ---- 2. every slice count -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shuffled", [False, True], ids=["sorted", "shuffled"])
def test_slice_counts(shuffled):
    """(70, 700, 36) has 6 table tiles: every slice count gives the reference, for both entries."""
    U, T, targets, excl, eligible, row_time, lo, hi = _case(70, 700, 36, shuffled)
    s = U.double() @ T.double().T
    want_k = _want(("topk", 70, 700, 36, shuffled, 0, False, 10), lambda: R.expected_topk(s, 10, row_time, lo, hi, excl, eligible))
    want_r = _want(("rank", 70, 700, 36, shuffled, 0, False), lambda: R.expected_ranks(s, targets, row_time, lo, hi, excl, eligible))
    for slices in (0, 1, 2, 3, 4, 6):
        idx, score, status = _topk(U, T, 10, row_time, lo, hi, excl, eligible, slices)
        assert status == 0 and C.same((idx, score), want_k), slices
        rank, score, ranked, status = _ranks(U, T, targets, row_time, lo, hi, excl, eligible, slices)
        assert status == 0 and C.same((rank, score, ranked), want_r), slices


# ---- 3. equivalence with the existing entries, on real-valued vectors ------------------------------------------------------------------
@pytest.mark.parametrize("B", [5, 66])
def test_each_row_equals_the_plain_entry_under_the_users_own_mask(B):
    """Row b of a batched windowed call has the idx, the score bits, the population and the ranks of ``ops.topk_scores`` /
    ``ops.catalogue_ranks`` called for user b alone with ``eligible & window_mask[b]``: an exact oracle that is not the code under
    test (the score of a (user, row) pair does not depend on B)."""
    from newsreclib_amd import ops
    V, D, k = 700, 36, 10
    g = torch.Generator().manual_seed(50 + B)
    U, T = torch.randn(B, D, generator=g).cuda(), torch.randn(V, D, generator=g).cuda()
    targets = [torch.randint(0, V, (int(n),), generator=g).tolist() for n in torch.randint(0, 4, (B,), generator=g)]
    excl = [torch.randint(0, V, (int(n),), generator=g).tolist() for n in torch.randint(0, 10, (B,), generator=g)]
    eligible = (torch.rand(V, generator=g) > 0.15).to(torch.uint8)
    row_time = _times(V, False)
    lo, hi = R.window_mix(B, row_time)
    mask = R.window_mask(row_time, lo, hi)
    (ti, to), (ei, eo) = C.ragged(targets), C.ragged(excl)
    args = (row_time.cuda(), lo.cuda(), hi.cuda(), ei.cuda(), eo.cuda(), eligible.cuda())
    idx, score, status = ops.topk_window_scores(U, T, k, *args)
    rank, rscore, ranked, rstatus = ops.catalogue_window_ranks(U, T, ti.cuda(), to.cuda(), *args)
    assert int(status) == 0 and int(rstatus) == 0
    singles_k, singles_r = [], []
    for b in range(B):
        e1, t1 = torch.tensor(excl[b], dtype=torch.int64).cuda(), torch.tensor(targets[b], dtype=torch.int64).cuda()
        eo1, to1 = torch.tensor([0, len(excl[b])]).cuda(), torch.tensor([0, len(targets[b])]).cuda()
        elig_b = (eligible.bool() & mask[b]).to(torch.uint8).cuda()
        singles_k.append(ops.topk_scores(U[b:b + 1], T, k, e1, eo1, elig_b))
        singles_r.append(ops.catalogue_ranks(U[b:b + 1], T, t1, to1, e1, eo1, elig_b))
    assert all(int(x[-1]) == 0 for x in singles_k + singles_r)
    assert C.same((idx, score), tuple(torch.cat([x[i] for x in singles_k]) for i in range(2)))
    assert C.same((rank, rscore, ranked), tuple(torch.cat([x[i] for x in singles_r]) for i in range(3)))


# ---- 4. the skip path ---------------------------------------------------------------------------------------------------------------
def test_all_windows_empty():
    U, T, targets, excl, eligible, row_time, _, _ = _case(70, 700, 36, False)
    lo, hi = torch.full((70,), 5, dtype=torch.int32), torch.full((70,), 4, dtype=torch.int32)
    idx, score, status = _topk(U, T, 10, row_time, lo, hi, excl, eligible)
    assert status == 0 and bool((idx == -1).all()) and bool((score == NEG_INF).all())
    rank, score, ranked, status = _ranks(U, T, targets, row_time, lo, hi, excl, eligible)
    assert status == 0 and bool((rank == 0).all()) and bool((score == NEG_INF).all()) and bool((ranked == 0).all())
    assert ranked.shape == (70,) and rank.numel() == sum(len(t) for t in targets)


@pytest.mark.parametrize("who", [3, 60], ids=["first_wave", "last_wave"])
def test_one_window_among_empty_ones(who):
    """65 users: one non-empty window among the 64 of the first user tile (in the first and in the last wave's share of it), an
    empty one in the second tile.  The survivor's window covers one table tile out of six."""
    B, V, D = 65, 700, 36
    U, T, targets, excl, eligible, row_time, _, _ = _case(B, V, D, False)
    lo, hi = torch.full((B,), 5, dtype=torch.int32), torch.full((B,), 4, dtype=torch.int32)
    lo[who], hi[who] = 16, 23                                    # rows 256 ... 383: the third tile
    targets[who] = [300, 10, 383, 384]
    s = U.double() @ T.double().T
    idx, score, status = _topk(U, T, 10, row_time, lo, hi, excl, eligible)
    assert status == 0 and C.same((idx, score), R.expected_topk(s, 10, row_time, lo, hi, excl, eligible))
    assert bool((idx[who] >= 256).all()) and bool((idx[who] < 384).all()) and int((idx >= 0).any(1).sum()) == 1
    rank, score, ranked, status = _ranks(U, T, targets, row_time, lo, hi, excl, eligible)
    assert status == 0 and C.same((rank, score, ranked), R.expected_ranks(s, targets, row_time, lo, hi, excl, eligible))
    assert int((ranked > 0).sum()) == 1 and 0 < int(ranked[who]) <= 128


# ---- 5. rank-specific ---------------------------------------------------------------------------------------------------------------
def test_targets_windows_and_the_topk_list_agree():
    B, V, D, k = 6, 300, 12, 16
    U, T = C.int_vectors(41, B, V, D)
    row_time = _times(V, False)
    lo = torch.tensor([R.INT32_MIN, 2, 8, 0, 5, 3], dtype=torch.int32)
    hi = torch.tensor([R.INT32_MAX, 2, 12, 7, 4, 18], dtype=torch.int32)
    excl = [[], [33], [150, 150, 3], [], [], [60]]
    eligible = torch.ones(V, dtype=torch.uint8)
    eligible[[7, 200]] = 0
    s = U.double() @ T.double().T
    idx, top_score, status = _topk(U, T, k, row_time, lo, hi, excl, eligible)
    assert status == 0
    # per user: its best and its last listed row, a row outside its window, one inside, an excluded and an ineligible one
    targets = [[int(idx[b, 0]), int(idx[b, k - 1])] + extra for b, extra in
               enumerate([[7, 299], [31, 48, 33, 40], [127, 128, 150, 208, 209], [128, 5], [70, 80], [47, 48, 60, 200, 303]])]
    targets[4] = [70, 80]                                        # (an empty window lists nothing)
    rank, score, ranked, status = _ranks(U, T, targets, row_time, lo, hi, excl, eligible)
    assert status == E_TARGET_ROW                                # user 5's row 303 is outside the table; nothing else is flagged
    want = R.expected_ranks(s, targets, row_time, lo, hi, excl, eligible)
    assert C.same((rank, score, ranked), want)
    assert C.same(ranked, R.population(s, row_time, lo, hi, excl, eligible)[0].sum(1).to(torch.int32))
    mask = R.window_mask(row_time, lo, hi)
    at = 0
    for b in range(B):
        for t in targets[b]:
            r = int(rank[at])
            if 0 <= t < V and not bool(mask[b, t]):              # outside the owner's window: rank 0, -inf
                assert r == 0 and float(score[at]) == NEG_INF, (b, t)
            assert (1 <= r <= k) == (t >= 0 and bool((idx[b] == t).any())), (b, t, r)
            if 1 <= r <= k:
                assert int(idx[b, r - 1]) == t and C.same(score[at], top_score[b, r - 1]), (b, t)
            at += 1
    assert rank[:2].tolist() == [1, k] and int(ranked[4]) == 0 and ranked.tolist()[1] == 15


# ---- 6. NaN -------------------------------------------------------------------------------------------------------------------------
def test_nan_rows_count_only_inside_a_window():
    B, V, D, k = 4, 300, 12, 10
    U, T = C.int_vectors(23, B, V, D)
    T[200, 3] = float("nan")                                     # row 200 (time 12) scores NaN for every user
    row_time = _times(V, False)
    targets = [[200, 5], [200], [180, 200], []]
    lo = torch.tensor([0, 13, 5, 3], dtype=torch.int32)
    hi = torch.tensor([11, 18, 4, 3], dtype=torch.int32)
    s = U.double() @ T.double().T
    assert not R.population(s, row_time, lo, hi)[1]
    idx, score, status = _topk(U, T, k, row_time, lo, hi)
    assert status == 0 and C.same((idx, score), R.expected_topk(s, k, row_time, lo, hi))
    rank, rscore, ranked, status = _ranks(U, T, targets, row_time, lo, hi)
    assert status == 0 and C.same((rank, rscore, ranked), R.expected_ranks(s, targets, row_time, lo, hi))
    lo[2], hi[2] = 11, 12                                        # rows 176 ... 207 for user 2 alone
    assert R.population(s, row_time, lo, hi)[1]
    idx, score, status = _topk(U, T, 32, row_time, lo, hi)
    assert status == E_NAN and C.same((idx, score), R.expected_topk(s, 32, row_time, lo, hi))
    assert sorted(idx[2][idx[2] >= 0].tolist()) == [v for v in range(176, 208) if v != 200]
    rank, rscore, ranked, status = _ranks(U, T, targets, row_time, lo, hi)
    assert status == E_NAN and C.same((rank, rscore, ranked), R.expected_ranks(s, targets, row_time, lo, hi))
    assert ranked.tolist() == [192, 92, 31, 16] and int(rank[4]) == 0 and int(rank[3]) > 0


# ---- 7. status passthrough ----------------------------------------------------------------------------------------------------------
def test_bad_exclusion_indices_and_offsets_behave_as_in_the_plain_entries():
    B, V, D, k = 3, 300, 12, 10
    U, T = C.int_vectors(29, B, V, D)
    row_time = _times(V, False)
    lo, hi = torch.tensor([2, 0, 4], dtype=torch.int32), torch.tensor([9, 18, 15], dtype=torch.int32)
    targets = [[40, 10], [5], [100, 250]]
    s = U.double() @ T.double().T
    excl = [[40, V + 3, -2], [], [100, 101]]
    idx, score, status = _topk(U, T, k, row_time, lo, hi, excl)
    assert status == E_EXCLUDE and C.same((idx, score), R.expected_topk(s, k, row_time, lo, hi, excl))
    rank, rscore, ranked, status = _ranks(U, T, targets, row_time, lo, hi, excl)
    assert status == E_EXCLUDE and C.same((rank, rscore, ranked), R.expected_ranks(s, targets, row_time, lo, hi, excl))
    # user 1's offsets run backwards: flat [64, 65, 66, 67], offsets [0, 3, 2, 4] -> user 0 [64, 65, 66], user 2 [66, 67]
    flat, off = [[64, 65, 66, 67], [], []], torch.tensor([0, 3, 2, 4])
    sound = [[64, 65, 66], [], [66, 67]]
    want_k, want_r = R.expected_topk(s, k, row_time, lo, hi, sound), R.expected_ranks(s, targets, row_time, lo, hi, sound)
    idx, score, status = _topk(U, T, k, row_time, lo, hi, flat, excl_off=off)
    assert status == E_OFFSETS and bool((idx[1] == -1).all()) and bool((score[1] == NEG_INF).all())
    assert C.same((idx[[0, 2]], score[[0, 2]]), (want_k[0][[0, 2]], want_k[1][[0, 2]]))
    rank, rscore, ranked, status = _ranks(U, T, targets, row_time, lo, hi, flat, excl_off=off)
    assert status == E_OFFSETS and int(rank[2]) == 0 and float(rscore[2]) == NEG_INF and int(ranked[1]) == 0
    keep = torch.tensor([0, 1, 3, 4])
    assert C.same((rank[keep], rscore[keep], ranked[[0, 2]]), (want_r[0][keep], want_r[1][keep], want_r[2][[0, 2]]))


# ---- 8. empty sizes -----------------------------------------------------------------------------------------------------------------
def test_no_rows_and_no_users():
    from newsreclib_amd import ops
    U, T = C.int_vectors(3, 4, 8, 12)
    lo, hi = torch.zeros(4, dtype=torch.int32), torch.ones(4, dtype=torch.int32)
    none = torch.zeros(0, dtype=torch.int32)
    idx, score, status = _topk(U, T[:0], 3, none, lo, hi)
    assert status == 0 and idx.shape == (4, 3) and bool((idx == -1).all()) and bool((score == NEG_INF).all())
    rank, score, ranked, status = _ranks(U, T[:0], [[], [], [], []], none, lo, hi)
    assert status == 0 and rank.numel() == 0 and ranked.tolist() == [0, 0, 0, 0]
    rt = torch.zeros(8, dtype=torch.int32)
    idx, score, status = _topk(U[:0], T, 3, rt, none, none)
    assert status == 0 and idx.shape == (0, 3) and score.shape == (0, 3)
    rank, score, ranked, status = ops.catalogue_window_ranks(U[:0].cuda(), T.cuda(), torch.zeros(0, dtype=torch.int64).cuda(),
                                                             torch.zeros(1, dtype=torch.int64).cuda(), rt.cuda(), none.cuda(), none.cuda())
    assert int(status) == 0 and rank.numel() == 0 and ranked.numel() == 0


# ---- 9. no read-back ----------------------------------------------------------------------------------------------------------------
def test_the_windowed_entries_do_not_synchronise_with_the_host():
    from newsreclib_amd import ops
    U, T = C.int_vectors(3, 5, 200, 12)
    U, T = U.cuda(), T.cuda()
    (ti, to), (ei, eo) = C.ragged([[1, 2], [], [5], [7, 7], [199]]), C.ragged([[1], [], [5, 6], [], []])
    ti, to, ei, eo, elig = ti.cuda(), to.cuda(), ei.cuda(), eo.cuda(), torch.ones(200, dtype=torch.uint8).cuda()
    rt = _times(200, False).cuda()
    lo, hi = torch.tensor([0, 3, 0, 0, 5], dtype=torch.int32).cuda(), torch.tensor([12, 2, 0, 12, 12], dtype=torch.int32).cuda()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        if not C.sync_debug_honoured():
            pytest.skip("this torch build does not raise on synchronising calls under set_sync_debug_mode('error')")
        idx, score, status = ops.topk_window_scores(U, T, 4, rt, lo, hi, ei, eo, elig)
        rank, rscore, ranked, rstatus = ops.catalogue_window_ranks(U, T, ti, to, rt, lo, hi, ei, eo, elig)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert int(status) == 0 and int(rstatus) == 0 and idx.shape == (5, 4) and rank.shape == (6,) and ranked.tolist()[1] == 0


# ---- 10. cache level ----------------------------------------------------------------------------------------------------------------
def _cache_case(with_time=True):
    from newsreclib_amd.evaluation import DeviceNewsTable, NewsVectorCache
    mod, attrs = builders.tiny("nrms")
    if with_time:
        attrs = dict(attrs, time=torch.arange(50) // 4)          # int64, as a frame's column arrives
    cache = NewsVectorCache(mod, DeviceNewsTable(attrs), chunk=32)
    lists, hist, hs, uidx = builders.hist_batch(50)
    return mod, cache, lists, hist, hs, uidx


def _users_by_hand(mod, cache, hist, hs, uidx):
    from newsreclib_amd import ops
    vec = cache.vectors if cache.vectors is not None else cache.build()
    with torch.no_grad():
        was = mod.training
        mod.eval()
        user = mod.user_vectors(ops.embedding_gather(vec, hist.cuda().reshape(-1, 1)).reshape(-1, vec.shape[1]), cache._user_meta(hs, uidx))
        mod.train(was)
    return user, vec, cache._user_meta(hs, uidx)["hist_offsets"]


def test_cache_recommend_and_rank_clicks_with_a_window():
    from newsreclib_amd import ops
    mod, cache, lists, hist, hs, uidx = _cache_case()
    V, B, k = 50, 6, 8
    eligible = torch.ones(V, dtype=torch.uint8)
    eligible[0] = 0
    lo = torch.tensor([R.INT32_MIN, 3, 6, 0, 9, 2], dtype=torch.int32)
    hi = torch.tensor([R.INT32_MAX, 8, 5, 4, 12, 2], dtype=torch.int32)
    clicks = [torch.tensor([1 + 7 * b, 49 - b]) for b in range(B)]
    click_idx, cs = torch.cat(clicks), torch.tensor([2] * B)
    user, vec, hist_off = _users_by_hand(mod, cache, hist, hs, uidx)
    rt32 = (torch.arange(V) // 4).to(torch.int32).cuda()
    want_k = ops.topk_window_scores(user, vec, k, rt32, lo.cuda(), hi.cuda(), hist.cuda(), hist_off, eligible.cuda())
    want_r = ops.catalogue_window_ranks(user, vec, click_idx.cuda(), (torch.arange(B + 1) * 2).cuda(), rt32, lo.cuda(), hi.cuda(),
                                        hist.cuda(), hist_off, eligible.cuda())
    # the times from the table's column (host bounds, device bounds) and as an explicit third member
    for window in ((lo, hi), (lo.cuda(), hi.cuda()), (lo, hi, rt32), (lo, hi, rt32.cpu())):
        got = cache.recommend(hist.cuda(), hs, k, user_idx=uidx, eligible=eligible, window=window)
        assert int(got[2]) == 0 and C.same(got[:2], want_k[:2])
        got = cache.rank_clicks(hist.cuda(), hs, click_idx.cuda(), cs, user_idx=uidx, eligible=eligible, window=window)
        assert int(got[3]) == 0 and C.same(got[:3], want_r[:3])
    assert cache._row_time is not None and cache._row_time.dtype == torch.int32
    assert bool((want_k[0][2] == -1).all()) and int(want_r[2][2]) == 0           # user 2: the empty window
    # window=None is the call without the argument
    plain = cache.recommend(hist.cuda(), hs, k, user_idx=uidx, eligible=eligible)
    assert C.same(cache.recommend(hist.cuda(), hs, k, user_idx=uidx, eligible=eligible, window=None)[:2], plain[:2])
    assert C.same(plain[:2], ops.topk_scores(user, vec, k, hist.cuda(), hist_off, eligible.cuda())[:2])
    plain = cache.rank_clicks(hist.cuda(), hs, click_idx.cuda(), cs, user_idx=uidx, eligible=eligible)
    assert C.same(cache.rank_clicks(hist.cuda(), hs, click_idx.cuda(), cs, user_idx=uidx, eligible=eligible, window=None)[:3], plain[:3])


def test_cache_refusals():
    from newsreclib_amd import evaluation as E
    mod, cache, lists, hist, hs, uidx = _cache_case(with_time=False)
    lo, hi = torch.zeros(6, dtype=torch.int32), torch.ones(6, dtype=torch.int32)
    with pytest.raises(ValueError, match="integer news attribute `time`"):
        cache.recommend(hist.cuda(), hs, 4, user_idx=uidx, window=(lo, hi))
    with pytest.raises(ValueError, match="integer news attribute `time`"):
        cache.rank_clicks(hist.cuda(), hs, torch.ones(6, dtype=torch.int64).cuda(), torch.ones(6, dtype=torch.int64), user_idx=uidx,
                          window=(lo, hi))
    with pytest.raises(TypeError, match="int32"):
        cache.recommend(hist.cuda(), hs, 4, user_idx=uidx, window=(lo.long(), hi, torch.zeros(50, dtype=torch.int32)))
    with pytest.raises(ValueError, match=r"window = \(win_lo, win_hi\)"):
        cache.recommend(hist.cuda(), hs, 4, user_idx=uidx, window=(lo,))
    users = [{"hist": lists[b], "clicks": torch.tensor([3]), "user_idx": uidx[b], "time": 5} for b in range(6)]
    with pytest.raises(ValueError, match="integer news attribute `time`"):
        E.recommend_users(cache, users, 4, window=(2, 0))
    mod, cache, lists, hist, hs, uidx = _cache_case()
    with pytest.raises(NotImplementedError, match="class-capped"):
        E.recommend_users(cache, users, 4, window=(2, 0), cap=("category", 1))
    with pytest.raises(ValueError, match='no "time"'):
        E.recommend_users(cache, [{k: v for k, v in u.items() if k != "time"} for u in users], 4, window=(2, 0))
    with pytest.raises(ValueError, match='no "time"'):
        E.evaluate_full_rank(cache, [{k: v for k, v in u.items() if k != "time"} for u in users], until_request=True)
    from newsreclib_amd.dkn_module import DKNModule
    from newsreclib_amd.miner_module import MINERModule
    from newsreclib_amd.npa_module import NPAModule
    for cls in (MINERModule, DKNModule, NPAModule):
        other = E.NewsVectorCache(object.__new__(cls), cache.table)
        with pytest.raises(NotImplementedError, match="tkw_scores_kernel"):
            E.recommend_users(other, users, 4, window=(2, 0))
        with pytest.raises(NotImplementedError, match="tkw_scores_kernel"):
            E.evaluate_full_rank(other, users, until_request=True)
    with pytest.raises(NotImplementedError, match="MannerVectorCache"):
        E.recommend_users(object.__new__(E.MannerVectorCache), users, 4, window=(2, 0))
    with pytest.raises(NotImplementedError, match="tkec_count_kernel"):
        E.evaluate_full_rank(object.__new__(E.MannerVectorCache), users, until_request=True, ensemble=True)


def test_recommend_users_and_evaluate_full_rank_against_per_user_plain_calls():
    """NRMS' seq-first user attention couples the users of a batch, so the plain call keeps the batch and folds one user's window
    into ``eligible``: row b of that call is what the windowed call must give user b."""
    import warnings

    from newsreclib_amd.evaluation import evaluate_full_rank, format_recommendations, recommend_users
    from newsreclib_amd.metrics import full_rank_metrics
    mod, cache, lists, hist, hs, uidx = _cache_case()
    V, B, k = 50, 6, 5
    eligible = torch.ones(V, dtype=torch.uint8)
    eligible[0] = 0
    times = [12, 3, 7, 11, 0, 9]
    clicks = [torch.tensor([2 + 6 * b, 48 - 3 * b, 20]) for b in range(B)]
    users = [{"hist": lists[b], "clicks": clicks[b], "user_idx": uidx[b], "time": times[b]} for b in range(B)]
    row_time = torch.arange(V) // 4
    click_idx, cs = torch.cat(clicks), torch.tensor([3] * B)

    def plain(lo, hi):
        rows_idx, rows_score, ranks, ranked = [], [], [], []
        for b in range(B):
            elig_b = eligible.bool() & (row_time >= lo[b]) & (row_time <= hi[b])
            i, s, st = cache.recommend(hist.cuda(), hs, k, user_idx=uidx, eligible=elig_b)
            r, _, n, rst = cache.rank_clicks(hist.cuda(), hs, click_idx.cuda(), cs, user_idx=uidx, eligible=elig_b)
            assert int(st) == 0 and int(rst) == 0
            rows_idx.append(i[b:b + 1].cpu()), rows_score.append(s[b:b + 1].cpu())
            ranks.append(r[3 * b:3 * b + 3].cpu()), ranked.append(n[b:b + 1].cpu())
        return torch.cat(rows_idx), torch.cat(rows_score), torch.cat(ranks), torch.cat(ranked)

    with warnings.catch_warnings():
        warnings.simplefilter("error")
        got = recommend_users(cache, users, k, batch_size=8, eligible=eligible, window=(3, 1))
        idx, score, _, _ = plain([t - 3 for t in times], [t + 1 for t in times])
        assert got == format_recommendations(list(range(1, B + 1)), idx, score)
        assert got["U5"] and all(1 <= int(n[1:]) < 8 for n in got["U5"])                    # time 0: rows 1 ... 7 (0 is padding)
        full = evaluate_full_rank(cache, users, (5, 10), batch_size=8, eligible=eligible, until_request=True)
        _, _, ranks, ranked = plain([R.INT32_MIN] * B, times)
        assert full == full_rank_metrics(ranks, cs, ranked, (5, 10))
        # the pool of a re-ranker comes from the windowed call: every listed news is inside its user's window
        div = recommend_users(cache, users, 3, batch_size=8, eligible=eligible, window=(3, 1), diversify=(5, 0.5))
    for b in range(B):
        listed = [int(n[1:]) for n in div[f"U{b + 1}"]]
        assert len(listed) == min(3, int((idx[b] >= 0).sum())) and set(listed) <= set(idx[b].tolist()), b


def test_every_reranker_takes_its_pool_from_the_windowed_call():
    """``diversify`` / ``dpp`` / ``calibrate`` under ``window``: the list is the re-ranker's own answer on the pool
    ``cache.recommend(pool, window=...)`` returns for the batch, so no listed news is outside its user's window."""
    import warnings

    from newsreclib_amd import ops
    from newsreclib_amd.evaluation import format_recommendations, recommend_users, user_windows
    mod, cache, lists, hist, hs, uidx = _cache_case()
    V, B, k, pool = 50, 6, 3, 6
    eligible = torch.ones(V, dtype=torch.uint8)
    eligible[0] = 0
    users = [{"hist": lists[b], "user_idx": uidx[b], "time": t} for b, t in enumerate([12, 3, 7, 11, 0, 9])]
    lo, hi = user_windows(users, 3, 1)
    mask = R.window_mask(torch.arange(V) // 4, lo, hi)
    pool_idx, pool_score, status = cache.recommend(hist.cuda(), hs, pool, user_idx=uidx, eligible=eligible, window=(lo, hi))
    assert int(status) == 0 and all(bool(mask[b, r]) for b in range(B) for r in pool_idx[b].tolist() if r >= 0)
    assert int((pool_idx >= 0).sum()) > B * k                    # (the pools are larger than the lists: there is something to pick)
    off = torch.cat([torch.zeros(1, dtype=torch.int64), hs.cumsum(0)]).cuda()
    target = ops.class_targets(hist.cuda(), off, cache.table.attrs["category"], ops.CAL_MAX_CLASSES)
    by_hand = {"diversify": cache.rerank_diverse(pool_idx, pool_score, k, 0.5),
               "dpp": cache.rerank_dpp(pool_idx, pool_score, k, 1.0, eps=1e-4),
               "calibrate": cache.rerank_calibrated(pool_idx, pool_score, k, "category", target, 1.0, 0.0, 0.5)}
    asked = {"diversify": (pool, 0.5), "dpp": dict(pool=pool), "calibrate": dict(pool=pool, aspect="category", gamma=0.5)}
    for how, want in by_hand.items():
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")                      # (a re-ranker's own flags on these tiny pools are not the subject)
            got = recommend_users(cache, users, k, batch_size=8, eligible=eligible, window=(3, 1), **{how: asked[how]})
        assert got == format_recommendations(list(range(1, B + 1)), want[0].cpu(), want[1].cpu()), how
        for b in range(B):
            assert all(bool(mask[b, int(n[1:])]) for n in got[f"U{b + 1}"]), (how, b)
