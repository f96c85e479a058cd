"""Class-biased full-catalogue top-k and rank (``nrl_topk_bias_scores`` / ``nrl_topk_bias_scores_capped`` /
``nrl_catalogue_bias_ranks``, their ``ops`` wrappers, ``NewsVectorCache.recommend_biased`` / ``rank_clicks_biased``).

Expected values come from the float64 scores of ``tests/topk_bias_ref.py`` under the contract of ``tests/catalogue_ref.py``.
The exact cases use entries that are multiples of 1/8 in [-2, 2] (vectors) and [-4, 4] (bias): every product is a multiple of
1/64, every partial sum stays below 2^11 and so has at most 17 significant bits, and the one add of the bias is exact too --
fp32 and float64 must agree in rows AND score bits.  The real-valued cases compare against ``ops.topk_scores`` of the same call plus ONE torch fp32 add."""
import functools

import numpy as np
import pytest
import torch

from tests import builders
from tests import catalogue_ref as C
from tests import topk_bias_ref as R
from tests import topk_capped_ref

pytestmark = pytest.mark.gpu

E_EXCLUDE, E_NAN, E_TARGET_ROW, E_CLASS = 1, 4, 32, 64
NEG_INF = float("-inf")


@pytest.fixture(autouse=True, params=["f32", "bf16x3"])
def engine(request):
    from newsreclib_amd import _lib
    prev = _lib.get_gemm_engine()
    _lib.set_gemm_engine(request.param)
    yield request.param
    _lib.set_gemm_engine(prev)


def _eighths(rng, shape, top):
    return (rng.integers(-8 * top, 8 * top + 1, shape) / 8.0).astype(np.float32)


def _masks(excl, eligible):
    ei = eo = None
    if excl is not None:
        ei, eo = C.ragged(excl)
        ei, eo = ei.cuda(), eo.cuda()
    return ei, eo, torch.from_numpy(eligible).cuda() if eligible is not None else None


def _topk(U, T, bias, cls, k, excl=None, eligible=None, slices=0, cap=None):
    from newsreclib_amd import ops
    args = [torch.from_numpy(x).cuda() for x in (U, T, bias, cls)]
    tail = (*_masks(excl, eligible), slices)
    if cap is None:
        idx, score, status = ops.topk_bias_scores(*args, k, *tail)
    else:
        idx, score, status = ops.topk_bias_scores_capped(*args, k, torch.from_numpy(cap[0]).cuda(), cap[1], *tail)
    return idx, score, int(status)


def _ranks(U, T, bias, cls, targets, excl=None, eligible=None, slices=0):
    from newsreclib_amd import ops
    args = [torch.from_numpy(x).cuda() for x in (U, T, bias, cls)]
    ti, to = C.ragged(targets)
    rank, score, ranked, status = ops.catalogue_bias_ranks(*args, ti.cuda(), to.cuda(), *_masks(excl, eligible), slices)
    return rank, score, ranked, int(status)


# ---- 1. the edge sweep: every B, V, D, S, k and slicing of the issue appears; exclusion (one list longer than 64) and eligibility ----
_SWEEP = [(130, 1000, 300, 19, 128, 7), (130, 1000, 4, 64, 5, 0), (3, 1000, 300, 4, 128, 2), (1, 1000, 300, 1, 5, 1),
          (1, 1, 4, 1, 1, 0), (3, 1, 4, 4, 5, 7), (3, 63, 4, 19, 128, 0), (65, 64, 300, 4, 5, 1), (3, 65, 300, 64, 128, 2),
          (1, 65, 4, 19, 1, 7), (65, 127, 300, 1, 5, 2), (3, 128, 4, 64, 128, 1), (130, 129, 4, 4, 1, 7), (3, 129, 300, 19, 5, 2),
          (65, 1000, 4, 64, 1, 0), (1, 127, 4, 4, 128, 2), (130, 128, 300, 19, 1, 0), (65, 63, 4, 1, 1, 1)]
assert {c[0] for c in _SWEEP} == {1, 3, 65, 130} and {c[1] for c in _SWEEP} == {1, 63, 64, 65, 127, 128, 129, 1000}
assert {c[2] for c in _SWEEP} == {4, 300} and {c[3] for c in _SWEEP} == {1, 4, 19, 64}
assert {c[4] for c in _SWEEP} == {1, 5, 128} and {c[5] for c in _SWEEP} == {0, 1, 2, 7}


@functools.lru_cache(maxsize=None)
def _sweep_case(B, V, D, S, k):
    """inputs and the float64 expectations, computed once for both engines"""
    rng = np.random.default_rng(B * 7 + V * 3 + D + S * 11 + k)
    U, T, bias = _eighths(rng, (B, D), 2), _eighths(rng, (V, D), 2), _eighths(rng, (B, S), 4)
    cls = rng.integers(0, S, V).astype(np.int32)
    cap_cls = (rng.integers(0, 5, V) * 1000003 - 7).astype(np.int32)          # another array than the bias's, any int32
    excl = [rng.integers(0, V, int(rng.integers(0, 9))).tolist() for _ in range(B)]
    excl[0] = rng.permutation(V)[:min(V - 1, 90)].tolist() if V > 1 else []  # longer than the 64 cached entries where V allows
    eligible = (rng.random(V) > 0.1).astype(np.uint8)
    targets = [rng.integers(0, V, int(rng.integers(0, 4))).tolist() for _ in range(B)]
    targets[0] = targets[0] + excl[0][:1]                                      # a target in the history
    s, flags = R.scores(U, T, bias, cls)
    pop, nan = C.population(s, excl, eligible)
    assert flags == 0 and not nan
    kc, m = min(k, 64), 2
    return (U, T, bias, cls, cap_cls, excl, eligible, targets), C.topk(s, pop, k), C.ranks(s, pop, targets), \
        topk_capped_ref.reference(s, pop, torch.from_numpy(cap_cls), kc, m), C.topk(s, pop, kc)


@pytest.mark.parametrize("B,V,D,S,k,slices", _SWEEP)
def test_edge_sweep_rows_and_score_bits(B, V, D, S, k, slices):
    (U, T, bias, cls, cap_cls, excl, eligible, targets), want, want_rank, want_cap, want_kc = _sweep_case(B, V, D, S, k)
    idx, score, status = _topk(U, T, bias, cls, k, excl, eligible, slices)
    assert status == 0 and C.same(idx, want[0]) and C.same(score, want[1])
    if excl[0]:
        assert len(excl[0]) > 64 or V <= 65
    # the rank entry: ranks, score bits and populations
    rank, tscore, ranked, status = _ranks(U, T, bias, cls, targets, excl, eligible, slices)
    assert status == 0 and C.same(rank, want_rank[0]) and C.same(tscore, want_rank[1]) and C.same(ranked, want_rank[2])
    # the capped entry, its classes another array than the bias's: the greedy definition; m >= k: the uncapped new entry
    kc = min(k, 64)
    idx, score, status = _topk(U, T, bias, cls, kc, excl, eligible, slices, cap=(cap_cls, 2))
    assert status == 0 and C.same(idx, want_cap[0]) and C.same(score, want_cap[1])
    idx, score, status = _topk(U, T, bias, cls, kc, excl, eligible, slices, cap=(cap_cls, kc))
    assert status == 0 and C.same(idx, want_kc[0]) and C.same(score, want_kc[1])


# ---- 2. ties made by the bias --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("slices", [1, 2, 0])
def test_ties_made_by_the_bias_go_to_the_lower_row(slices):
    """Different dot products, equal sums: rows 127 / 128 (the border of the first two tiles) and 255 / 256 (with two slices of
    two tiles: the slice border) all score 5; every other row scores 0 + 0."""
    V, S = 512, 5
    U = np.array([[1.0, 0.0, 0.0, 0.0]] * 2, dtype=np.float32)
    T = np.zeros((V, 4), dtype=np.float32)
    cls = np.full(V, 4, dtype=np.int32)
    bias = np.array([[2.0, 4.0, 0.5, 0.0, 0.0]] * 2, dtype=np.float32)
    for row, dot, c in ((127, 3.0, 0), (128, 1.0, 1), (255, 4.5, 2), (256, 5.0, 3)):
        T[row, 0], cls[row] = dot, c
    idx, score, status = _topk(U, T, bias, cls, 6, slices=slices)
    assert status == 0
    assert idx.tolist() == [[127, 128, 255, 256, 0, 1]] * 2 and score.tolist() == [[5.0, 5.0, 5.0, 5.0, 0.0, 0.0]] * 2
    idx, _, _ = _topk(U, T, bias, cls, 3, excl=[[], [127, 255]], slices=slices)
    assert idx.tolist() == [[127, 128, 255], [128, 256, 0]]
    rank, tscore, ranked, status = _ranks(U, T, bias, cls, [[256, 128], [127]], slices=slices)
    assert status == 0 and rank.tolist() == [4, 2, 1] and tscore.tolist() == [5.0, 5.0, 5.0] and ranked.tolist() == [V, V]


# ---- 3. what a bias does --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _effect_case():
    rng = np.random.default_rng(77)
    B, V, D, S = 5, 1000, 12, 19
    U, T, bias = _eighths(rng, (B, D), 2), _eighths(rng, (V, D), 2), _eighths(rng, (B, S), 1)
    cls = rng.integers(0, S - 1, V).astype(np.int32)
    cls[V - 1] = S - 1                                      # the last row of the last tile is alone in class S - 1
    return U, T, bias, cls


def _expect(U, T, bias, cls, k, **kw):
    s, flags = R.scores(U, T, bias, cls)
    pop, nan = C.population(s, **kw)
    return C.topk(s, pop, k), flags | (E_NAN if nan else 0), s, pop


@pytest.mark.parametrize("slices", [0, 3])
def test_a_class_bias_lifts_a_row_of_the_last_tile_to_the_top(slices):
    U, T, bias, cls = _effect_case()
    bias = bias.copy()
    bias[:, 18] = 512.0
    idx, score, status = _topk(U, T, bias, cls, 5, slices=slices)
    want, flags, _, _ = _expect(U, T, bias, cls, 5)
    assert status == flags == 0 and C.same(idx, want[0]) and C.same(score, want[1])
    assert idx[:, 0].tolist() == [999] * 5 and bool((score[:, 0] > 400).all())


def test_a_large_negative_bias_empties_a_class_from_every_list():
    U, T, bias, cls = _effect_case()
    bias = bias.copy()
    bias[:, 3] = -1e30
    idx, score, status = _topk(U, T, bias, cls, 128, slices=2)
    want, flags, _, _ = _expect(U, T, bias, cls, 128)
    assert status == flags == 0 and C.same(idx, want[0]) and C.same(score, want[1])
    assert int((cls == 3).sum()) > 10 and not bool((torch.from_numpy(cls)[idx.cpu()] == 3).any())


def test_a_nan_bias_drops_that_class_for_that_user_only():
    U, T, bias, cls = _effect_case()
    bias = bias.copy()
    bias[2, 3] = np.nan
    idx, score, status = _topk(U, T, bias, cls, 128, slices=2)
    want, flags, s, pop = _expect(U, T, bias, cls, 128)
    assert status == flags == E_NAN and C.same(idx, want[0]) and C.same(score, want[1])
    per_user = (torch.from_numpy(cls)[idx.cpu()] == 3).sum(1).tolist()
    assert per_user[2] == 0 and all(n > 0 for b, n in enumerate(per_user) if b != 2)
    # the rank entry drops the same rows from the population and gives a target among them rank 0
    gone = int(np.nonzero(cls == 3)[0][0])
    targets = [[gone], [], [gone, 5], [], []]
    rank, tscore, ranked, status = _ranks(U, T, bias, cls, targets, slices=2)
    want_rank = C.ranks(s, pop, targets)
    assert status == E_NAN and C.same(rank, want_rank[0]) and C.same(tscore, want_rank[1]) and C.same(ranked, want_rank[2])
    assert rank.tolist()[1] == 0 and rank.tolist()[0] > 0 and ranked.tolist()[2] == 1000 - int((cls == 3).sum())


@pytest.mark.parametrize("slices", [0, 2])
def test_class_ids_outside_the_bias_are_scored_with_zero_and_flagged(slices):
    U, T, bias, cls = _effect_case()
    cls = cls.copy()
    cls[[0, 130, 998]] = -1
    cls[[5, 700]] = 19
    cls[64] = -2 ** 31
    idx, score, status = _topk(U, T, bias, cls, 128, slices=slices)
    want, flags, s, pop = _expect(U, T, bias, cls, 128)
    assert status == flags == E_CLASS and C.same(idx, want[0]) and C.same(score, want[1])
    targets = [[0, 5], [700], [], [64], [998, 1]]
    rank, tscore, ranked, status = _ranks(U, T, bias, cls, targets, slices=slices)
    want_rank = C.ranks(s, pop, targets)
    assert status == E_CLASS and C.same(rank, want_rank[0]) and C.same(tscore, want_rank[1]) and C.same(ranked, want_rank[2])
    plain = (U.astype(np.float64) @ T.astype(np.float64).T)[0, 0]
    assert float(tscore[0]) == plain                        # bias 0: the dot product itself


# ---- 4. identities ---------------------------------------------------------------------------------------------------------------------------
def _real(seed, B, V, D, S):
    g = torch.Generator().manual_seed(seed)
    U, T, bias = torch.randn(B, D, generator=g).cuda(), torch.randn(V, D, generator=g).cuda(), torch.randn(B, S, generator=g).cuda()
    return U, T, bias, torch.randint(0, S, (V,), generator=g).to(torch.int32).cuda()


@pytest.mark.parametrize("B,V,D,S,k,slices", [(130, 1000, 300, 19, 128, 0), (3, 129, 768, 64, 5, 2), (65, 64, 4, 1, 64, 1)])
def test_a_zero_bias_returns_topk_scores(B, V, D, S, k, slices):
    from newsreclib_amd import ops
    U, T, bias, cls = _real(B + V, B, V, D, S)
    T[5] = T[9]                                              # (a tie between real values)
    ei, eo = C.ragged([[5, 7]] + [[] for _ in range(B - 1)])
    got = ops.topk_bias_scores(U, T, torch.zeros_like(bias), cls, k, ei.cuda(), eo.cuda(), slices=slices)
    want = ops.topk_scores(U, T, k, ei.cuda(), eo.cuda(), slices=slices)
    assert int(got[2]) == int(want[2]) == 0 and torch.equal(got[0], want[0]) and bool((got[1] == want[1]).all())
    tgt = torch.arange(B, dtype=torch.int64).cuda() % V
    off = torch.arange(B + 1, dtype=torch.int64).cuda()
    got = ops.catalogue_bias_ranks(U, T, torch.zeros_like(bias), cls, tgt, off, ei.cuda(), eo.cuda(), slices=slices)
    want = ops.catalogue_ranks(U, T, tgt, off, ei.cuda(), eo.cuda(), slices=slices)
    assert all(torch.equal(a, b) for a, b in zip(got, want))


@pytest.mark.parametrize("B,V,D,S", [(9, 128, 300, 19), (70, 65, 768, 64), (3, 127, 4, 4)])
def test_every_score_is_the_dot_product_of_topk_scores_plus_one_fp32_add(B, V, D, S):
    from newsreclib_amd import ops
    U, T, bias, cls = _real(V + S, B, V, D, S)
    all_idx, all_score, _ = ops.topk_scores(U, T, V)
    dots = torch.empty(B, V, device="cuda").scatter_(1, all_idx, all_score)
    total = dots + bias[:, cls.long()]                       # ONE fp32 add per element
    want_score, want_idx = torch.sort(total, dim=1, descending=True, stable=True)
    idx, score, status = ops.topk_bias_scores(U, T, bias, cls, V)
    assert int(status) == 0 and torch.equal(idx, want_idx) and torch.equal(C.bits(score), C.bits(want_score + 0.0))
    tgt = torch.arange(V, dtype=torch.int64).cuda().repeat(B)[:32 * B].reshape(B, 32)
    rank, tscore, ranked, status = ops.catalogue_bias_ranks(U, T, bias, cls, tgt.reshape(-1), torch.arange(B + 1).cuda() * 32)
    assert int(status) == 0 and bool((ranked == V).all())
    assert torch.equal(C.bits(tscore.reshape(B, 32)), C.bits(total.gather(1, tgt) + 0.0))
    assert torch.equal(idx.gather(1, rank.reshape(B, 32).long() - 1), tgt)


def test_invariance_under_batch_slicing_and_engine():
    from newsreclib_amd import _lib, ops
    B, V, D, S, k = 130, 1000, 300, 19, 10
    U, T, bias, cls = _real(31, B, V, D, S)
    tgt, off = (torch.arange(2 * B, dtype=torch.int64).cuda() * 7) % V, torch.arange(B + 1, dtype=torch.int64).cuda() * 2
    base = ops.topk_bias_scores(U, T, bias, cls, k)
    base_rank = ops.catalogue_bias_ranks(U, T, bias, cls, tgt, off)
    assert int(base[2]) == 0 and int(base_rank[3]) == 0

    def same(got, got_rank, sel=slice(None), tsel=slice(None)):
        return torch.equal(got[0], base[0][sel]) and torch.equal(C.bits(got[1]), C.bits(base[1][sel])) and \
            torch.equal(got_rank[0], base_rank[0][tsel]) and torch.equal(C.bits(got_rank[1]), C.bits(base_rank[1][tsel])) and \
            torch.equal(got_rank[2], base_rank[2][sel])

    for slices in (1, 2, 7):
        assert same(ops.topk_bias_scores(U, T, bias, cls, k, slices=slices),
                    ops.catalogue_bias_ranks(U, T, bias, cls, tgt, off, slices=slices)), slices
    for b in (0, 63, 64, 129):                               # a user alone against the same user inside the batch of 130
        assert same(ops.topk_bias_scores(U[b:b + 1], T, bias[b:b + 1], cls, k),
                    ops.catalogue_bias_ranks(U[b:b + 1], T, bias[b:b + 1], cls, tgt[2 * b:2 * b + 2], off[:2]),
                    slice(b, b + 1), slice(2 * b, 2 * b + 2)), b
    prev = _lib.get_gemm_engine()
    try:
        for name in ("f32", "bf16x3"):
            _lib.set_gemm_engine(name)
            assert same(ops.topk_bias_scores(U, T, bias, cls, k), ops.catalogue_bias_ranks(U, T, bias, cls, tgt, off)), name
    finally:
        _lib.set_gemm_engine(prev)
    assert same(ops.topk_bias_scores(U, T, bias, cls.long(), k), base_rank)      # int64 classes are the same classes
    # a score's bits do not depend on k either
    wide = ops.topk_bias_scores(U, T, bias, cls, 128)
    assert torch.equal(wide[0][:, :k], base[0]) and torch.equal(C.bits(wide[1][:, :k]), C.bits(base[1]))


# ---- 5. the rank entry against the list ------------------------------------------------------------------------------------------------------
def test_a_rank_of_at_most_k_is_the_slot_of_the_list():
    from newsreclib_amd import ops
    B, V, D, S, k = 70, 700, 300, 19, 16
    U, T, bias, cls = _real(5, B, V, D, S)
    hist = [[(b * 13 + j) % V for j in range(b % 5)] for b in range(B)]
    ei, eo = C.ragged(hist)
    elig = torch.ones(V, dtype=torch.uint8)
    elig[0] = 0
    tail = (ei.cuda(), eo.cuda(), elig.cuda())
    idx, score, status = ops.topk_bias_scores(U, T, bias, cls, k, *tail)
    assert int(status) == 0
    idx_c, score_c = idx.cpu(), score.cpu()
    g = torch.Generator().manual_seed(8)
    clicks = [[int(idx_c[b, 0]), int(idx_c[b, k - 1])] + torch.randint(0, V, (3,), generator=g).tolist() + hist[b][:1] + [0, V, -1]
              for b in range(B)]
    ti, to = C.ragged(clicks)
    rank, tscore, ranked, status = ops.catalogue_bias_ranks(U, T, bias, cls, ti.cuda(), to.cuda(), *tail)
    assert int(status) == E_TARGET_ROW                       # the targets V and -1, as for catalogue_ranks
    rank, tscore, ranked = rank.cpu(), tscore.cpu(), ranked.cpu()
    assert ranked.tolist() == [V - 1 - len(set(h)) for h in hist]
    at = 0
    for b in range(B):
        assert int(rank[at]) == 1 and int(rank[at + 1]) == k
        for c in clicks[b]:
            r = int(rank[at])
            assert (1 <= r <= k) == bool((idx_c[b] == c).any()), (b, c, r)
            if 1 <= r <= k:
                assert int(idx_c[b, r - 1]) == c and torch.equal(C.bits(tscore[at]), C.bits(score_c[b, r - 1]))
            if c in hist[b] or c == 0 or not 0 <= c < V:
                assert r == 0 and float(tscore[at]) == NEG_INF
            at += 1


# ---- 6. the capped entry -----------------------------------------------------------------------------------------------------------------------
def test_a_cap_of_k_or_more_returns_the_bits_of_the_uncapped_entry_and_a_smaller_one_walks_its_list():
    from newsreclib_amd import ops
    B, V, D, S, k = 66, 128, 300, 4, 8
    U, T, bias, cls = _real(12, B, V, D, S)
    cap_cls = (torch.arange(V) % 5).to(torch.int32).cuda()   # the cap goes by another array than the bias
    for m in (k, 2 ** 31 - 1):
        got, want = ops.topk_bias_scores_capped(U, T, bias, cls, k, cap_cls, m), ops.topk_bias_scores(U, T, bias, cls, k)
        assert int(got[2]) == 0 and torch.equal(got[0], want[0]) and torch.equal(C.bits(got[1]), C.bits(want[1]))
    idx, score, status = ops.topk_bias_scores_capped(U, T, bias, cls, k, cap_cls.long(), 1, slices=1)
    all_idx, all_score, _ = ops.topk_bias_scores(U, T, bias, cls, V)
    want_idx, want_score, _ = topk_capped_ref.walk_listed(all_idx.cpu(), all_score.cpu(), cap_cls.cpu(), k, 1)
    assert int(status) == 0 and bool((all_idx >= 0).all())   # (the list of V rows is every user's whole population)
    assert torch.equal(idx.cpu(), want_idx) and torch.equal(C.bits(score.cpu()), C.bits(want_score))
    assert bool((idx[:, 5:] == -1).all()) and bool((idx[:, :5] >= 0).all())      # five classes, one row each


# ---- 7. refusals, no read-back ---------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_before_any_launch():
    from newsreclib_amd import ops
    U, T, bias, cls = _real(3, 5, 200, 12, 4)
    tgt, off = torch.zeros(5, dtype=torch.int64).cuda(), torch.arange(6, dtype=torch.int64).cuda()
    for call in (lambda b, c: ops.topk_bias_scores(U, T, b, c, 5), lambda b, c: ops.topk_bias_scores_capped(U, T, b, c, 5, cls, 2),
                 lambda b, c: ops.catalogue_bias_ranks(U, T, b, c, tgt, off)):
        with pytest.raises(ValueError, match=r"bias \(B, S\)"):
            call(bias[:, :0], cls)                           # S = 0
        with pytest.raises(NotImplementedError, match="at most 64 classes"):
            call(torch.zeros(5, 65).cuda(), cls)             # S = 65
        with pytest.raises(ValueError, match="are required"):
            call(None, cls)
        with pytest.raises(ValueError, match=r"bias \(B, S\)"):
            call(bias[:4], cls)
        with pytest.raises(ValueError, match="one entry per table row"):
            call(bias, cls[:199])
    with pytest.raises(RuntimeError, match=r"topk_bias_scores_capped: k in \[1, 64\]"):
        ops.topk_bias_scores_capped(U, T, bias, cls, 65, cls, 2)
    with pytest.raises(RuntimeError, match="max_per_class"):
        ops.topk_bias_scores_capped(U, T, bias, cls, 5, cls, 0)
    with pytest.raises(RuntimeError, match=r"topk_bias_scores: k in \[1, 128\]"):
        ops.topk_bias_scores(U, T, bias, cls, 129)
    torch.cuda.synchronize()                                 # nothing was launched: nothing can have gone wrong on the device
    idx, _, status = ops.topk_bias_scores_capped(U, T, bias, cls, 5, cls, 2)
    assert int(status) == 0 and bool((idx >= 0).all())


def test_biased_entries_do_not_synchronise_with_the_host():
    from newsreclib_amd import ops
    U, T, bias, cls = _real(3, 5, 200, 12, 4)
    ei, eo = C.ragged([[1, 2], [], [5], [7, 7], []])
    ei, eo, elig = ei.cuda(), eo.cuda(), torch.ones(200, dtype=torch.uint8).cuda()
    tgt, off, cls64 = torch.arange(5, dtype=torch.int64).cuda(), torch.arange(6, dtype=torch.int64).cuda(), cls.long()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        if not C.sync_debug_honoured():
            pytest.skip("this torch build does not raise on synchronising calls under set_sync_debug_mode('error')")
        idx, score, status = ops.topk_bias_scores(U, T, bias, cls, 4, ei, eo, elig)
        idx64, _, _ = ops.topk_bias_scores(U, T, bias, cls64, 4, ei, eo, elig)
        capped = ops.topk_bias_scores_capped(U, T, bias, cls64, 4, cls, 1, ei, eo, elig)
        ranks = ops.catalogue_bias_ranks(U, T, bias, cls64, tgt, off, ei, eo, elig)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert int(status) == 0 and idx.shape == (5, 4) and torch.equal(idx, idx64)
    assert int(capped[2]) == 0 and capped[0].shape == (5, 4) and int(ranks[3]) == 0 and ranks[0].shape == (5,)


# ---- 8. SentiDebias end to end, and a dot-product module with the caller's bias ------------------------------------------------------------
def _sentidebias_case(late_fusion):
    from newsreclib_amd.evaluation import DeviceNewsTable, NewsVectorCache
    from tests import sentidebias_oracle as SO
    from tests.sentidebias_helpers import build_module
    rng = np.random.default_rng(17)
    vocab, n_news, B = 300, 203, 7
    mod = build_module(SO.make_params(vocab, 4, 1, late_fusion), p_drop=0.2, late_fusion=late_fusion).eval()
    lens = rng.integers(3, 31, n_news)
    ids = rng.integers(1, vocab, (n_news, 30))
    ids[np.arange(30)[None, :] >= lens[:, None]] = 0
    ids[0] = 0
    table = DeviceNewsTable({"title": torch.from_numpy(ids), "category": torch.from_numpy(rng.integers(1, 19, n_news)),
                             "sentiment": torch.from_numpy(rng.integers(0, SO.N_SENT, n_news))})
    lists = [torch.from_numpy(rng.choice(np.arange(1, n_news), int(n), replace=False)) for n in rng.integers(1, 13, B)]
    eligible = torch.ones(n_news, dtype=torch.uint8)
    eligible[0] = 0                                          # the padding row
    return mod, table, NewsVectorCache(mod, table, chunk=64), lists, eligible


@pytest.mark.parametrize("late_fusion", [False, True], ids=["early", "late"])
def test_sentidebias_is_ranked_by_its_bias_free_and_by_its_combined_score(late_fusion):
    from newsreclib_amd import ops
    from newsreclib_amd.evaluation import evaluate_full_rank, recommend_users
    mod, table, cache, lists, eligible = _sentidebias_case(late_fusion)
    B, V, k = len(lists), table.num_news, 10
    hist, hs = torch.cat(lists).cuda(), torch.tensor([len(x) for x in lists])
    # combined=False: ops.topk_scores over Generator.user_vectors' bias-free vectors
    idx, score, status = cache.recommend_biased(hist, hs, k, eligible=eligible)
    meta = cache._user_meta(hs, None)
    hv = ops.embedding_gather(cache.vectors, hist.reshape(-1, 1)).reshape(-1, cache.vectors.shape[1])
    with torch.no_grad():
        free, none = mod.generator.user_vectors(hv, meta, None)
    want = ops.topk_scores(free, cache.vectors, k, hist, meta["hist_offsets"], eligible.cuda())
    assert none is None and int(status) == int(want[2]) == 0
    assert torch.equal(idx, want[0]) and torch.equal(C.bits(score), C.bits(want[1]))
    # combined=True: every returned (user, row) against the module's own forward over those rows as the candidate lists
    cidx, cscore, status = cache.recommend_biased(hist, hs, k, eligible=eligible, combined=True)
    assert int(status) == 0 and bool((cidx >= 0).all())
    batch = table.build_batch(hist, hs, cidx.reshape(-1), torch.full((B,), k), torch.zeros(B * k))
    with torch.no_grad():
        combined, bias_free, *_ = mod(batch)
    bound = 1e-4 * max(1.0, float(combined.abs().max()))
    err = float((cscore - combined).abs().max())
    print(f"late_fusion={late_fusion}: combined score against forward: max |diff| {err:.3e}, bound {bound:.3e}")
    assert err <= bound
    assert float((combined - bias_free).abs().max()) > 10 * bound        # (the sentiment term is there to be seen)
    # rank_clicks_biased is consistent with recommend_biased, under either score
    for comb, (lidx, lscore) in ((False, (idx, score)), (True, (cidx, cscore))):
        clicks = torch.stack([lidx[:, 0], lidx[:, k - 1], torch.tensor([lists[b][0] for b in range(B)]).cuda()], 1).reshape(-1)
        rank, tscore, ranked, status = cache.rank_clicks_biased(hist, hs, clicks, torch.full((B,), 3), eligible=eligible, combined=comb)
        assert int(status) == 0 and rank.reshape(B, 3).tolist() == [[1, k, 0]] * B
        assert ranked.tolist() == [V - 1 - int(n) for n in hs]
        assert torch.equal(C.bits(tscore.reshape(B, 3)[:, :2]), C.bits(lscore[:, [0, k - 1]]))
    # recommend_users and evaluate_full_rank pick the biased methods; the dictionary and the metric keys are the usual ones
    users = [{"hist": lists[b], "clicks": idx[b, :2].cpu(), "user_id": 100 + b} for b in range(B)]
    recs = recommend_users(cache, users, k, batch_size=4, eligible=eligible)
    capped = recommend_users(cache, users, k, batch_size=B, eligible=eligible, cap=("category", 1))
    logs = evaluate_full_rank(cache, users, (5, 10), batch_size=B, eligible=eligible)
    assert list(recs) == [f"U{100 + b}" for b in range(B)] == list(capped)
    by_hand = torch.cat([cache.recommend_biased(torch.cat(lists[lo:lo + 4]).cuda(), hs[lo:lo + 4], k, eligible=eligible)[0]
                         for lo in (0, 4)])
    assert all(list(recs[f"U{100 + b}"]) == [f"N{int(i)}" for i in by_hand[b]] for b in range(B))
    categ = table.attrs["category"].cpu()
    for b in range(B):
        rows = [int(n[1:]) for n in capped[f"U{100 + b}"]]
        assert len(rows) == k and len({int(categ[r]) for r in rows}) == k       # at most one news of a category
    assert set(logs) == {"mrr", "auc_user", "ndcg@5", "ndcg@10", "recall@5", "recall@10", "hit@5", "hit@10"}
    assert logs["hit@5"] == 1.0                              # (the clicks are each user's two best news)
    # the dot-product methods keep refusing
    with pytest.raises(NotImplementedError, match="dot_product_scorer"):
        cache.recommend(hist, hs, k)
    with pytest.raises(NotImplementedError, match="dot_product_scorer"):
        cache.rank_clicks(hist, hs, clicks, torch.full((B,), 3))


def test_a_dot_product_module_with_the_callers_bias():
    from newsreclib_amd import ops
    from newsreclib_amd.evaluation import DeviceNewsTable, NewsVectorCache
    mod, attrs = builders.tiny("nrms")
    cache = NewsVectorCache(mod, DeviceNewsTable(attrs), chunk=32)
    V, B, k = 50, 6, 10
    lists, hist, hs, uidx = builders.hist_batch(V)
    categ = cache.table.attrs["category"]
    S = int(categ.max()) + 1
    bias = torch.randn(B, S, generator=torch.Generator().manual_seed(2)).cuda() * 3
    mod.train()
    idx, score, status = cache.recommend_biased(hist.cuda(), hs, k, user_idx=uidx, aspect="category", bias=bias)
    assert mod.training and int(status) == 0
    # the reference's rows: float64 over recommend's user vectors and the cached table
    meta = cache._user_meta(hs, uidx)
    with torch.no_grad():
        mod.eval()
        user = mod.user_vectors(ops.embedding_gather(cache.vectors, hist.cuda().reshape(-1, 1)).reshape(-1, cache.vectors.shape[1]), meta)
        mod.train()
    s, flags = R.scores(user.cpu().numpy(), cache.vectors.cpu().numpy(), bias.cpu().numpy(), categ.cpu().numpy())
    pop, _ = C.population(s, [x.tolist() for x in lists])
    want_idx, want_score = C.topk(s, pop, k)
    # (a user without a near-tie among its first k + 1 float64 scores: fp32 cannot reorder them)
    clear = torch.sort(C.masked(s, pop), dim=1, descending=True)[0][:, :k + 1].diff(dim=1).abs().min(1)[0] > 1e-4
    assert flags == 0 and clear.sum() >= B - 1
    assert torch.equal(idx.cpu()[clear], want_idx[clear])
    assert float((score.cpu()[clear] - want_score[clear]).abs().max()) <= 1e-4
    # the same call by hand, the capped one, the rank
    want = ops.topk_bias_scores(user, cache.vectors, bias, categ, k, hist.cuda(), meta["hist_offsets"])
    assert torch.equal(idx, want[0]) and torch.equal(C.bits(score), C.bits(want[1]))
    cidx, _, status = cache.recommend_biased(hist.cuda(), hs, k, user_idx=uidx, aspect="category", bias=bias, cap=("category", 2))
    assert int(status) == 0 and int(torch.stack([(categ[cidx.clamp(min=0)] == c).sum(1) for c in range(S)]).max()) <= 2
    rank, tscore, _, status = cache.rank_clicks_biased(hist.cuda(), hs, idx[:, 3].contiguous(), torch.ones(B, dtype=torch.int64),
                                                       user_idx=uidx, aspect="category", bias=bias)
    assert int(status) == 0 and rank.tolist() == [4] * B and torch.equal(C.bits(tscore), C.bits(score[:, 3]))
