"""Full-catalogue rank of held-out clicks (``nrl_catalogue_ranks`` / ``ops.catalogue_ranks`` / ``NewsVectorCache.rank_clicks`` /
``evaluate_full_rank``).

Expected values come from ``tests/catalogue_ref.py`` (CPU, float64) over ``s = U64 @ T64.T``.  Integer-valued vectors in
[-4, 4] make every fp32 dot product exact in any order (|s| <= 16 * 1024 < 2^24), so those cases compare with ``torch.equal``,
ties included.  The real-valued case uses ``catalogue_ref.dot_bound``, the worst-case error of an fp32 dot product of length D
(derived): a row can change sides of a target only if their float64 scores are closer than the sum of their two bounds."""
import pytest
import torch

from tests import builders
from tests import catalogue_ref as C

pytestmark = pytest.mark.gpu

E_EXCLUDE, E_OFFSETS, E_NAN, E_TARGETS, E_TARGET_ROW = 1, 2, 4, 16, 32
NEG_INF = float("-inf")
_F32 = {}                                                  # results recorded under the f32 engine, compared under bf16x3


@pytest.fixture(autouse=True, params=["f32", "bf16x3"])
def engine(request):
    from newsreclib_amd import _lib
    prev = _lib.get_gemm_engine()
    _lib.set_gemm_engine(request.param)
    yield request.param
    _lib.set_gemm_engine(prev)


def _reference(U, T, targets, excl=None, eligible=None):
    return C.expected_ranks(U.double() @ T.double().T, targets, excl, eligible)


def _run(U, T, targets, excl=None, eligible=None, slices=0, tgt_off=None, excl_off=None):
    from newsreclib_amd import ops
    ti, to = C.ragged(targets)
    ei = eo = None
    if excl is not None:
        ei, eo = C.ragged(excl)
        ei, eo = ei.cuda(), (excl_off if excl_off is not None else eo).cuda()
    rank, score, ranked, status = ops.catalogue_ranks(U.cuda(), T.cuda(), ti.cuda(), (tgt_off if tgt_off is not None else to).cuda(),
                                                      ei, eo, eligible.cuda() if eligible is not None else None, slices)
    return rank.cpu(), score.cpu(), ranked.cpu(), int(status)


def _random_case(seed, B, V, D):
    """Targets (0 to 4 a user, a duplicate now and then), exclusion lists (0 to 9, duplicates allowed) and a mixed mask."""
    U, T = C.int_vectors(seed, B, V, D)
    g = torch.Generator().manual_seed(seed + 1)
    targets = [torch.randint(0, V, (int(n),), generator=g).tolist() for n in torch.randint(0, 5, (B,), generator=g)]
    targets[0] = targets[0] or [0]
    excl = [torch.randint(0, V, (int(n),), generator=g).tolist() for n in torch.randint(0, 10, (B,), generator=g)]
    eligible = (torch.rand(V, generator=g) > 0.15).to(torch.uint8)
    return U, T, targets, excl, eligible


# ---- 1. exact, with ties --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,V,D", [(1, 1, 4), (3, 130, 20), (65, 129, 4), (70, 700, 36), (5, 128, 1024)])
def test_exact_with_ties(B, V, D):
    U, T, targets, excl, eligible = _random_case(B * 7 + V + D, B, V, D)
    rank, score, ranked, status = _run(U, T, targets)
    assert status == 0 and C.same((rank, score, ranked), _reference(U, T, targets))
    assert bool((ranked == V).all())
    rank, score, ranked, status = _run(U, T, targets, excl, eligible)
    assert status == 0 and C.same((rank, score, ranked), _reference(U, T, targets, excl, eligible))


def test_slice_counts():
    """(70, 700, 36) has 6 table tiles: every slice count gives the reference."""
    U, T, targets, excl, eligible = _random_case(77, 70, 700, 36)
    want = _reference(U, T, targets, excl, eligible)
    for slices in (0, 1, 2, 3, 4, 6):
        rank, score, ranked, status = _run(U, T, targets, excl, eligible, slices)
        assert status == 0 and C.same((rank, score, ranked), want), slices


# ---- 2. target lists --------------------------------------------------------------------------------------------------------------
def _target_case():
    B, V, D = 6, 300, 12
    U, T = C.int_vectors(41, B, V, D)
    g = torch.Generator().manual_seed(42)
    eligible = torch.ones(V, dtype=torch.uint8)
    eligible[[7, 200]] = 0
    excl = [[], [5, 9], [150, 150, 3], [], [], [1]]
    targets = [[], torch.randperm(V, generator=g)[:32].tolist(), [17, 150, 17, 7, -1, V, 3, 299], [4], [0, 299], [200, 1, 2]]
    return U, T, targets, excl, eligible


def test_target_lists():
    """No targets, exactly 32, the same row twice, a target on the own exclusion list, an ineligible one, -1 and V."""
    U, T, targets, excl, eligible = _target_case()
    rank, score, ranked, status = _run(U, T, targets, excl, eligible, slices=2)
    want = _reference(U, T, targets, excl, eligible)
    assert status == E_TARGET_ROW and C.same((rank, score, ranked), want)
    r2 = rank[32:40].tolist()                                    # user 2: [17, 150, 17, 7, -1, V, 3, 299]
    assert r2[0] == r2[2] > 0 and r2[1] == r2[3] == r2[4] == r2[5] == r2[6] == 0 and r2[7] > 0
    assert bool((score[32:40][torch.tensor(r2) == 0] == NEG_INF).all())
    assert rank[-3:].tolist()[:2] == [0, 0] and int(rank[-1]) > 0 # user 5: ineligible, excluded, fine


def test_more_than_32_targets_blank_that_user_alone():
    U, T, targets, excl, eligible = _target_case()
    clean = [[t for t in tl if 0 <= t < T.shape[0]] for tl in targets]
    want = _reference(U, T, clean, excl, eligible)
    over = [list(tl) for tl in clean]
    over[3] = list(range(33))
    rank, score, ranked, status = _run(U, T, over, excl, eligible)
    assert status == E_TARGETS and torch.equal(ranked, want[2])
    n_before = sum(len(tl) for tl in over[:3])
    assert bool((rank[n_before:n_before + 33] == 0).all()) and bool((score[n_before:n_before + 33] == NEG_INF).all())
    keep = torch.ones(rank.numel(), dtype=torch.bool)
    keep[n_before:n_before + 33] = False
    drop = torch.ones(want[0].numel(), dtype=torch.bool)
    drop[n_before:n_before + 1] = False                          # (user 3 had one target in the clean case)
    assert torch.equal(rank[keep], want[0][drop]) and torch.equal(score[keep], want[1][drop])


def test_decreasing_target_offsets_blank_that_user_alone():
    B, V, D = 4, 40, 12
    U, T = C.int_vectors(17, B, V, D)
    flat = [3, 9, 9, 0, 21, 39, 5, 6, 7]
    off = torch.tensor([0, 4, 9, 7, 7])                          # user 2 runs backwards; user 3 is empty
    from newsreclib_amd import ops
    rank, score, ranked, status = ops.catalogue_ranks(U.cuda(), T.cuda(), torch.tensor(flat).cuda(), off.cuda())
    assert int(status) == E_TARGETS
    want = _reference(U, T, [flat[0:4], flat[4:9], [], []])
    assert C.same((rank.cpu(), score.cpu(), ranked.cpu()), want)
    # an offset beyond the list is rejected the same way
    rank, score, ranked, status = ops.catalogue_ranks(U.cuda(), T.cuda(), torch.tensor(flat).cuda(), torch.tensor([0, 4, 12, 9, 9]).cuda())
    assert int(status) == E_TARGETS
    want = _reference(U, T, [flat[0:4], [], [], []])
    assert torch.equal(rank.cpu()[:4], want[0]) and bool((rank.cpu()[4:] == 0).all()) and torch.equal(ranked.cpu(), want[2])


def test_no_targets_still_counts_the_population():
    U, T, _, excl, eligible = _target_case()
    rank, score, ranked, status = _run(U, T, [[] for _ in range(6)], excl, eligible)
    assert status == 0 and rank.numel() == 0 and score.numel() == 0
    assert torch.equal(ranked, _reference(U, T, [[]] * 6, excl, eligible)[2])
    assert ranked.tolist() == [298, 296, 296, 298, 298, 297]


# ---- 3. masks -------------------------------------------------------------------------------------------------------------------------
def _mask_case():
    B, V, D = 5, 700, 8
    U, T = C.int_vectors(5, B, V, D)
    g = torch.Generator().manual_seed(3)
    long = torch.randperm(V, generator=g)[:70].tolist()          # beyond the 64 entries a workgroup caches
    excl = [[], [3, 3, 9, 3, 9, 650], long, [699, 0, 128, 127], long[:64] + long[:6]]
    targets = [[0, 699], [3, 9, 4, 650], long[60:70] + [1, 2], [127, 128, 129], [long[5], long[69], 300]]
    return U, T, targets, excl


@pytest.mark.parametrize("slices", [0, 1, 3])
def test_exclusion_lists(slices):
    """Empty, with duplicates (a duplicate removes its row once), 70 entries (beyond the cached 64), at tile edges."""
    U, T, targets, excl = _mask_case()
    rank, score, ranked, status = _run(U, T, targets, excl, slices=slices)
    assert status == 0 and C.same((rank, score, ranked), _reference(U, T, targets, excl))
    assert ranked.tolist() == [700, 697, 630, 696, 636]


def test_status_bad_exclusion_index_is_ignored():
    U, T, targets, excl = _mask_case()
    bad = [list(x) for x in excl]
    bad[1] = [-1] + bad[1]
    bad[3] = bad[3] + [T.shape[0]]
    rank, score, ranked, status = _run(U, T, targets, bad)
    assert status == E_EXCLUDE and C.same((rank, score, ranked), _reference(U, T, targets, excl))


def test_status_bad_exclusion_offsets_blank_that_user_alone():
    B, V, D = 4, 40, 12
    U, T = C.int_vectors(19, B, V, D)
    excl_flat, targets = list(range(12)), [[20, 1], [30], [31, 4], [32]]
    off = torch.tensor([0, 5, 3, 8, 12])                         # user 1 runs backwards
    from newsreclib_amd import ops
    ti, to = C.ragged(targets)
    rank, score, ranked, status = ops.catalogue_ranks(U.cuda(), T.cuda(), ti.cuda(), to.cuda(), torch.tensor(excl_flat).cuda(), off.cuda())
    rank, score, ranked = rank.cpu(), score.cpu(), ranked.cpu()
    assert int(status) == E_OFFSETS
    want = _reference(U, T, targets, [excl_flat[0:5], [], excl_flat[3:8], excl_flat[8:12]])
    keep = torch.tensor([True, True, False, True, True, True])
    assert torch.equal(rank[keep], want[0][keep]) and torch.equal(score[keep], want[1][keep])
    assert int(rank[2]) == 0 and float(score[2]) == NEG_INF and int(ranked[1]) == 0
    assert torch.equal(ranked[[0, 2, 3]], want[2][[0, 2, 3]])


def test_eligibility():
    U, T, targets, excl = _mask_case()
    V = T.shape[0]
    g = torch.Generator().manual_seed(8)
    mixed = (torch.rand(V, generator=g) > 0.5).to(torch.uint8)
    for eligible in (None, mixed, mixed.bool()):
        rank, score, ranked, status = _run(U, T, targets, excl, eligible)
        assert status == 0 and C.same((rank, score, ranked), _reference(U, T, targets, excl, eligible))
    rank, score, ranked, status = _run(U, T, targets, excl, torch.zeros(V, dtype=torch.uint8))
    assert status == 0 and not bool(rank.any()) and not bool(ranked.any()) and bool((score == NEG_INF).all())


def test_empty_table():
    U = C.int_vectors(1, 3, 1, 8)[0]
    rank, score, ranked, status = _run(U, torch.zeros(0, 8), [[0], [], [1, -1]])
    assert status == E_TARGET_ROW                                # every index is outside an empty table
    assert rank.tolist() == [0, 0, 0] and bool((score == NEG_INF).all()) and ranked.tolist() == [0, 0, 0]


def test_nan_row_is_left_out():
    B, V, D = 5, 300, 12
    U, T = C.int_vectors(23, B, V, D)
    nan_row = 140
    targets = [[nan_row, 3], [5], [141, 139], [], [nan_row]]
    Tn = T.clone()
    Tn[nan_row, 3] = float("nan")
    rank, score, ranked, status = _run(U, Tn, targets, slices=2)
    assert status == E_NAN
    elig = torch.ones(V, dtype=torch.uint8)
    elig[nan_row] = 0
    assert C.same((rank, score, ranked), _reference(U, T, targets, eligible=elig))      # as if the row were not there
    assert C.same((rank, score, ranked), _reference(U, Tn, targets))                   # (the reference drops NaN itself)
    assert int(rank[0]) == 0 and int(rank[-1]) == 0 and bool((ranked == V - 1).all())
    # a NaN row nobody may be recommended is not reported
    assert _run(U, Tn, targets, eligible=elig)[3] == 0


# ---- 4. consistency with topk_scores on real values ----------------------------------------------------------------------------------
_REAL_SEED = 36


def _real_case():
    B, V, D = 70, 1000, 300
    g = torch.Generator().manual_seed(_REAL_SEED)
    U, T = torch.randn(B, D, generator=g), torch.randn(V, D, generator=g)
    extra = torch.randint(0, V, (B, 3), generator=g)
    return U, T, extra


def test_consistency_with_topk_scores_on_real_values(engine):
    """rank <= 128 exactly when the target is slot rank - 1 of the top-k list, with the list's score bits; against float64 the
    rank is off by at most the number of rows whose score is closer to the target's than the two error bounds together -- and
    with these seeded inputs that number stays below 3 for every target (checked on the CPU when the test was written: it makes
    the allowance a condition of the test, not a loophole)."""
    from newsreclib_amd import ops
    B, V, D, k = 70, 1000, 300, 128
    U, T, extra = _real_case()
    idx, top_score, st = ops.topk_scores(U.cuda(), T.cuda(), k)
    idx, top_score = idx.cpu(), top_score.cpu()
    assert int(st) == 0
    targets = [extra[b].tolist() + [int(idx[b, 0]), int(idx[b, 63]), int(idx[b, 127])] for b in range(B)]
    rank, score, ranked, status = _run(U, T, targets)
    assert status == 0 and bool((ranked == V).all()) and bool((rank >= 1).all())
    rank2, score2 = rank.reshape(B, 6), score.reshape(B, 6)
    assert rank2[:, 3:].tolist() == [[1, 64, 128]] * B
    s64, bound = U.double() @ T.double().T, C.dot_bound(U, T)
    ref = C.expected_ranks(s64, targets)[0].reshape(B, 6)
    worst_allow = worst_off = 0
    for b in range(B):
        for j, t in enumerate(targets[b]):
            r = int(rank2[b, j])
            inside = r <= k
            assert inside == bool((idx[b] == t).any())
            if inside:
                assert int(idx[b, r - 1]) == t
                assert torch.equal(score2[b, j].view(torch.int32), top_score[b, r - 1].view(torch.int32))
            assert abs(float(score2[b, j]) - float(s64[b, t])) <= float(bound[b, t])
            close = (s64[b] - s64[b, t]).abs() <= bound[b] + bound[b, t]
            allow = int(close.sum()) - 1                         # (the target itself is always close)
            worst_allow, worst_off = max(worst_allow, allow), max(worst_off, abs(r - int(ref[b, j])))
            assert allow < 3
            assert abs(r - int(ref[b, j])) <= allow, (b, t, r, int(ref[b, j]), allow)
    print(f"largest allowance {worst_allow}, largest |rank - float64 rank| {worst_off}")
    key = "real"
    if engine == "f32":
        _F32[key] = (rank, score, ranked)
    elif key in _F32:
        assert C.same((rank, score.view(torch.int32), ranked), (_F32[key][0], _F32[key][1].view(torch.int32), _F32[key][2]))


# ---- 5. invariance ----------------------------------------------------------------------------------------------------------------------
def test_invariance(engine):
    """Bit-equal ranks, scores and populations for the whole batch against each user alone, across slice counts and across the two
    GEMM engine settings (the f32 result is recorded in the first parametrisation and compared in the second)."""
    from newsreclib_amd import _lib, ops
    B, V, D = 70, 1000, 300
    g = torch.Generator().manual_seed(31)
    U, T = torch.randn(B, D, generator=g).cuda(), torch.randn(V, D, generator=g).cuda()
    sizes = torch.randint(0, 5, (B,), generator=g)
    targets = [torch.randint(0, V, (int(n),), generator=g).tolist() for n in sizes]
    excl = [torch.randint(0, V, (int(n),), generator=g).tolist() for n in torch.randint(0, 30, (B,), generator=g)]
    (ti, to), (ei, eo) = C.ragged(targets), C.ragged(excl)
    ti, to, ei, eo = ti.cuda(), to.cuda(), ei.cuda(), eo.cuda()

    def bits(out):
        return out[0], out[1].view(torch.int32), out[2]

    base = ops.catalogue_ranks(U, T, ti, to, ei, eo)
    assert int(base[3]) == 0
    for slices in (1, 2, 7):
        out = ops.catalogue_ranks(U, T, ti, to, ei, eo, slices=slices)
        assert int(out[3]) == 0 and C.same(bits(out), bits(base)), slices
    singles = []
    for b in range(B):
        t1, e1 = torch.tensor(targets[b], dtype=torch.int64).cuda(), torch.tensor(excl[b], dtype=torch.int64).cuda()
        singles.append(ops.catalogue_ranks(U[b:b + 1], T, t1, torch.tensor([0, len(targets[b])]).cuda(), e1,
                                           torch.tensor([0, len(excl[b])]).cuda()))
    assert all(int(s[3]) == 0 for s in singles)
    assert C.same(bits(tuple(torch.cat([s[i] for s in singles]) for i in range(3))), bits(base))
    if engine == "f32":
        _F32["invariance"] = tuple(x.cpu() for x in bits(base))
    else:
        if "invariance" not in _F32:                             # (this parametrisation selected alone)
            _lib.set_gemm_engine("f32")
            _F32["invariance"] = tuple(x.cpu() for x in bits(ops.catalogue_ranks(U, T, ti, to, ei, eo)))
            _lib.set_gemm_engine(engine)
        assert C.same(tuple(x.cpu() for x in bits(base)), _F32["invariance"])


# ---- 6. no read-back, memory ---------------------------------------------------------------------------------------------------------------
def test_catalogue_ranks_does_not_synchronise_with_the_host():
    from newsreclib_amd import ops
    U, T = C.int_vectors(3, 5, 200, 12)
    U, T = U.cuda(), T.cuda()
    (ti, to), (ei, eo) = C.ragged([[1, 2], [], [5], [7, 7], [199]]), C.ragged([[1], [], [5, 6], [], []])
    ti, to, ei, eo, elig = ti.cuda(), to.cuda(), ei.cuda(), eo.cuda(), torch.ones(200, dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        if not C.sync_debug_honoured():
            pytest.skip("this torch build does not raise on synchronising calls under set_sync_debug_mode('error')")
        rank, score, ranked, status = ops.catalogue_ranks(U, T, ti, to, ei, eo, elig)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert int(status) == 0 and rank.shape == (6,) and ranked.shape == (5,)


def test_peak_memory_is_far_below_the_score_matrix():
    from newsreclib_amd import ops
    B, V, D = 256, 60000, 64
    g = torch.Generator().manual_seed(2)
    U, T = torch.randn(B, D, generator=g).cuda(), torch.randn(V, D, generator=g).cuda()
    ti = torch.randint(0, V, (B * 3,), generator=g).cuda()
    to = (torch.arange(B + 1) * 3).cuda()
    ops.catalogue_ranks(U[:2], T[:256], ti[:6] % 256, to[:3])     # library loaded, kernels resident
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    live = torch.cuda.memory_allocated()
    out = ops.catalogue_ranks(U, T, ti, to)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - live
    print(f"peak above the inputs: {peak} bytes; score matrix: {B * V * 4} bytes")
    assert peak < B * V * 4 / 8
    assert int(out[3]) == 0 and bool((out[0] >= 1).all()) and bool((out[2] == V).all())


# ---- 7. cache level ---------------------------------------------------------------------------------------------------------------------------
def _cache_case():
    from newsreclib_amd.evaluation import DeviceNewsTable, NewsVectorCache
    mod, attrs = builders.tiny("nrms")
    cache = NewsVectorCache(mod, DeviceNewsTable(attrs), chunk=32)
    lists, hist, hs, uidx = builders.hist_batch(50)
    return mod, cache, lists, hist, hs, uidx


def test_rank_clicks_against_ops_and_recommend():
    from newsreclib_amd import ops
    mod, cache, lists, hist, hs, uidx = _cache_case()
    V, B, k = 50, 6, 16
    mod.train()
    eligible = torch.ones(V, dtype=torch.uint8)
    eligible[0] = 0                                              # the padding row
    idx, top_score, st = cache.recommend(hist.cuda(), hs, k, user_idx=uidx, eligible=eligible)
    idx, top_score = idx.cpu(), top_score.cpu()
    g = torch.Generator().manual_seed(6)
    clicks = [[int(idx[b, 0]), int(idx[b, 15])] + torch.randint(0, V, (b,), generator=g).tolist() + [int(lists[b][0])] for b in range(B)]
    click_idx, cs = torch.tensor([c for cl in clicks for c in cl]), torch.tensor([len(cl) for cl in clicks])
    rank, score, ranked, status = cache.rank_clicks(hist.cuda(), hs, click_idx.cuda(), cs, user_idx=uidx, eligible=eligible)
    assert mod.training                                          # the mode is restored
    assert int(status) == 0 and rank.shape == (int(cs.sum()),) and ranked.shape == (B,)
    # the same call by hand: the module's user vectors, the cached table
    vec = cache.vectors
    with torch.no_grad():
        mod.eval()
        user = mod.user_vectors(ops.embedding_gather(vec, hist.cuda().reshape(-1, 1)).reshape(-1, vec.shape[1]),
                                cache._user_meta(hs, uidx))
        mod.train()
    off = torch.cat([torch.zeros(1, dtype=torch.int64), cs.cumsum(0)])
    want = ops.catalogue_ranks(user, vec, click_idx.cuda(), off.cuda(), hist.cuda(), cache._user_meta(hs, uidx)["hist_offsets"],
                               eligible.cuda())
    assert int(want[3]) == 0 and torch.equal(rank, want[0]) and torch.equal(score.view(torch.int32), want[1].view(torch.int32))
    assert torch.equal(ranked, want[2])
    rank, score, ranked = rank.cpu(), score.cpu(), ranked.cpu()
    assert ranked.tolist() == [V - 1 - int(n) for n in hs]       # everything but the padding row and the history
    at = 0
    for b in range(B):
        for c in clicks[b]:
            r = int(rank[at])
            assert (1 <= r <= k) == bool((idx[b] == c).any()), (b, c, r)
            if 1 <= r <= k:
                assert int(idx[b, r - 1]) == c
                assert torch.equal(score[at].view(torch.int32), top_score[b, r - 1].view(torch.int32))
            if c in lists[b].tolist() or c == 0:
                assert r == 0 and float(score[at]) == NEG_INF
            at += 1
        assert int(rank[at - len(clicks[b])]) == 1 and int(rank[at - len(clicks[b]) + 1]) == 16
    # without the exclusion a click from the history ranks like any other row
    rank2, _, ranked2, _ = cache.rank_clicks(hist.cuda(), hs, click_idx.cuda(), cs, user_idx=uidx, exclude_history=False)
    assert bool((ranked2 == V).all()) and bool((rank2 >= 1).all())


def test_rank_clicks_refusals():
    from newsreclib_amd import evaluation as E
    from newsreclib_amd.dkn_module import DKNModule
    from newsreclib_amd.miner_module import MINERModule
    from newsreclib_amd.npa_module import NPAModule
    mod, cache, lists, hist, hs, uidx = _cache_case()
    many = torch.zeros(6, dtype=torch.int64)
    many[2] = 33
    with pytest.raises(ValueError, match="at most 32 clicks"):
        cache.rank_clicks(hist.cuda(), hs, torch.ones(33, dtype=torch.int64).cuda(), many, user_idx=uidx)
    args = (hist.cuda(), hs, torch.ones(6, dtype=torch.int64).cuda(), torch.ones(6, dtype=torch.int64))
    for cls in (MINERModule, DKNModule, NPAModule):
        with pytest.raises(NotImplementedError, match="only the dot-product families are served"):
            E.NewsVectorCache(object.__new__(cls), None).rank_clicks(*args)
    with pytest.raises(NotImplementedError, match="only the dot-product families are served"):
        E.NpaFeatureCache(object.__new__(NPAModule), None).rank_clicks(*args)
    with pytest.raises(NotImplementedError, match="only the dot-product families are served"):
        object.__new__(E.MannerVectorCache).rank_clicks(*args)


def test_evaluate_full_rank():
    """Two batches give ``full_rank_metrics`` of the two ``rank_clicks`` calls (NRMS' seq-first user attention couples the users of
    a batch, so the split is part of the input), one batch that of the one call; a status flag is passed on as ONE warning."""
    import warnings

    from newsreclib_amd.evaluation import evaluate_full_rank
    from newsreclib_amd.metrics import full_rank_metrics
    mod, cache, lists, hist, hs, uidx = _cache_case()
    V, B = 50, 6
    g = torch.Generator().manual_seed(13)
    clicks = [torch.randint(1, V, (int(n),), generator=g) for n in (2, 1, 0, 3, 5, 1)]
    users = [{"hist": lists[b], "clicks": clicks[b], "user_idx": uidx[b]} for b in range(B)]
    eligible = torch.ones(V, dtype=torch.uint8)
    eligible[0] = 0

    def by_hand(parts):
        outs = []
        for lo, hi in parts:
            h, c = torch.cat([lists[b] for b in range(lo, hi)]), torch.cat([clicks[b] for b in range(lo, hi)])
            outs.append(cache.rank_clicks(h.cuda(), hs[lo:hi], c.cuda(), torch.tensor([len(clicks[b]) for b in range(lo, hi)]),
                                          user_idx=uidx[lo:hi], eligible=eligible))
        assert all(int(o[3]) == 0 for o in outs)
        return full_rank_metrics(torch.cat([o[0] for o in outs]).cpu(), torch.tensor([len(c) for c in clicks]),
                                 torch.cat([o[2] for o in outs]).cpu(), (5, 10))

    with warnings.catch_warnings():
        warnings.simplefilter("error")                           # no flag, no warning
        two = evaluate_full_rank(cache, users, (5, 10), batch_size=4, eligible=eligible)
        one = evaluate_full_rank(cache, users, (5, 10), batch_size=8, eligible=eligible)
    assert two == by_hand([(0, 4), (4, 6)]) and one == by_hand([(0, 6)])
    assert set(one) == {"mrr", "auc_user", "ndcg@5", "ndcg@10", "recall@5", "recall@10", "hit@5", "hit@10"}
    assert 0.0 < one["mrr"] <= 1.0 and 0.0 < one["auc_user"] <= 1.0
    users[1] = dict(users[1], clicks=torch.tensor([V]))          # outside the table: flag 32 in the first batch only
    with pytest.warns(UserWarning, match=r"evaluate_full_rank: a target index is outside \[0, V\)") as rec:
        evaluate_full_rank(cache, users, (5, 10), batch_size=4, eligible=eligible)
    assert len(rec) == 1
