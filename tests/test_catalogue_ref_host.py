"""``tests/catalogue_ref.py`` pinned by hand-worked cases small enough to check by eye (V <= 6, B <= 3, the expected lists written
out), one seeded case of ``rank <= k`` against the list, and the containment of ``rank_intervals``: with ``|e| <= bound``
elementwise the rank under ``s + e`` lies in ``[lo, hi]`` by the inequality itself, so not one target may fall outside."""
import torch

from tests import catalogue_ref as C

NAN, INF = float("nan"), float("inf")


def _signs(x):
    return torch.signbit(x).tolist()


def test_all_equal_scores_return_the_first_rows():
    s = torch.full((2, 5), 3.0, dtype=torch.float64)
    idx, score = C.topk(s, C.allowed(2, 5), 3)
    assert idx.tolist() == [[0, 1, 2]] * 2 and score.tolist() == [[3.0] * 3] * 2
    assert idx.dtype == torch.int64 and score.dtype == torch.float32


def test_minus_zero_ties_with_plus_zero_by_row_and_comes_back_as_plus_zero():
    s = torch.tensor([[0.0, -0.0, 1.0, -0.0, 0.0, -1.0]], dtype=torch.float64)
    pop, nan = C.population(s)
    idx, score = C.topk(s, pop, 6)
    assert not nan and idx.tolist() == [[2, 0, 1, 3, 4, 5]]
    assert score.tolist() == [[1.0, 0.0, 0.0, 0.0, 0.0, -1.0]] and not any(_signs(score[0, :5]))
    rank, tscore, ranked = C.ranks(s, pop, [[3, 0, 1]])
    assert rank.tolist() == [4, 2, 3] and _signs(tscore) == [False] * 3 and ranked.tolist() == [6]


def test_a_nan_is_dropped_and_reported_only_from_an_allowed_position():
    s = torch.tensor([[5.0, NAN, 4.0, 6.0], [NAN, 1.0, 2.0, 3.0]], dtype=torch.float64)
    pop, nan = C.population(s)
    assert nan and pop.tolist() == [[True, False, True, True], [False, True, True, True]]
    assert C.topk(s, pop, 4)[0].tolist() == [[3, 0, 2, -1], [3, 2, 1, -1]]
    assert C.masked(s, pop).tolist() == [[5.0, -INF, 4.0, 6.0], [-INF, 1.0, 2.0, 3.0]] and bool(torch.isnan(s[0, 1]))
    # the same NaNs under an exclusion entry and an ineligible row: nobody is told
    pop, nan = C.population(s, excl=[[1], []], eligible=torch.tensor([0, 1, 1, 1], dtype=torch.uint8))
    assert not nan and pop.tolist() == [[False, False, True, True], [False, True, True, True]]


def test_exclusion_entries_outside_the_table_are_ignored_and_duplicates_are_harmless():
    V = 5
    assert C.allowed(2, V, [[-1, V, 2], [V + 7, -V]]).tolist() == [[True, True, False, True, True], [True] * 5]
    assert C.allowed(1, V, [[3, 3, 0, 3]]).tolist() == [[False, True, True, False, True]]
    assert C.allowed(1, V, [[4]], torch.tensor([True, False, True, True, True])).tolist() == [[True, False, True, True, False]]
    idx, off = C.ragged([[3, 3], [], [0]])
    assert idx.tolist() == [3, 3, 0] and off.tolist() == [0, 2, 2, 3] and idx.dtype == off.dtype == torch.int64


def test_k_larger_than_the_population_k_zero_and_an_empty_table():
    s = torch.tensor([[1.0, 3.0, 2.0, 3.0]], dtype=torch.float64)
    idx, score = C.expected_topk(s, 6, excl=[[2]], eligible=torch.tensor([1, 1, 1, 0], dtype=torch.uint8))
    assert idx.tolist() == [[1, 0, -1, -1, -1, -1]] and score.tolist() == [[3.0, 1.0] + [-INF] * 4]
    assert C.expected_topk(s, 0)[0].shape == (1, 0)
    empty = torch.zeros(3, 0, dtype=torch.float64)
    assert C.allowed(3, 0, [[0], [], [-1]]).shape == (3, 0)
    idx, score = C.expected_topk(empty, 2, [[0], [], [-1]])
    assert idx.tolist() == [[-1, -1]] * 3 and score.tolist() == [[-INF, -INF]] * 3
    rank, tscore, ranked = C.expected_ranks(empty, [[0], [], [1, -1]])
    assert rank.tolist() == [0, 0, 0] and tscore.tolist() == [-INF] * 3 and ranked.tolist() == [0, 0, 0]


def test_targets_excluded_ineligible_outside_duplicated_and_best():
    s = torch.tensor([[2.0, 9.0, 2.0, 7.0, 2.0, 1.0]], dtype=torch.float64)
    eligible = torch.tensor([1, 1, 1, 1, 1, 0], dtype=torch.uint8)
    #          excluded  ineligible  outside  duplicated  best  a tie by row
    targets = [[3,       5,          -1, 6,   2, 2,       1,    4, 0]]
    rank, tscore, ranked = C.expected_ranks(s, targets, [[3, 3]], eligible)
    assert rank.tolist() == [0, 0, 0, 0, 3, 3, 1, 4, 2] and rank.dtype == ranked.dtype == torch.int32
    assert tscore.tolist() == [-INF, -INF, -INF, -INF, 2.0, 2.0, 9.0, 2.0, 2.0] and tscore.dtype == torch.float32
    assert ranked.tolist() == [4]                               # rows 0, 1, 2 and 4


def test_a_rank_of_at_most_k_is_the_slot_of_the_list():
    g = torch.Generator().manual_seed(7)
    B, V, k = 3, 40, 8
    s = torch.randint(-3, 4, (B, V), generator=g).double()       # seven values over forty rows: ties everywhere
    excl = [torch.randint(0, V, (5,), generator=g).tolist() for _ in range(B)]
    eligible = (torch.rand(V, generator=g) > 0.2).to(torch.uint8)
    pop, _ = C.population(s, excl, eligible)
    idx, score = C.topk(s, pop, k)
    rank, tscore, ranked = C.ranks(s, pop, [list(range(V))] * B)
    rank, tscore = rank.reshape(B, V), tscore.reshape(B, V)
    assert ranked.tolist() == pop.sum(1).tolist() and len(torch.unique(s)) <= 7
    for b in range(B):
        for t in range(V):
            r = int(rank[b, t])
            assert (r == 0) == (not bool(pop[b, t]))
            assert (1 <= r <= k) == (t in idx[b].tolist())
            if 1 <= r <= k:
                assert int(idx[b, r - 1]) == t and torch.equal(C.bits(score[b, r - 1]), C.bits(tscore[b, t]))


def test_rank_intervals_contain_every_rank_within_the_bound():
    g = torch.Generator().manual_seed(11)
    B, V = 4, 50
    s = torch.randn(B, V, generator=g, dtype=torch.float64)
    bound = 0.05 * torch.rand(B, V, generator=g, dtype=torch.float64)
    excl = [torch.randint(0, V, (4,), generator=g).tolist() for _ in range(B)]
    pop, _ = C.population(s, excl)
    targets = [torch.randint(0, V, (6,), generator=g).tolist() + [excl[b][0], V] for b in range(B)]
    intervals = C.rank_intervals(s, bound, pop, targets)
    flat = [(b, t) for b, tl in enumerate(targets) for t in tl]
    assert len(intervals) == len(flat) and sum(iv is not None and iv[0] < iv[1] for iv in intervals) >= 5      # (not vacuous)

    def inside(scores):
        rank = C.ranks(scores, pop, targets)[0].tolist()
        for (b, t), r, iv in zip(flat, rank, intervals):
            if iv is None:
                assert r == 0 and (t == V or not bool(pop[b, t]))
            else:
                assert iv[0] <= r <= iv[1], (b, t, r, iv)

    inside(s)
    for _ in range(20):
        inside(s + (2 * torch.rand(B, V, generator=g, dtype=torch.float64) - 1) * bound)
    inside(s + bound)
    inside(s - bound)


def test_check_floor_and_the_small_helpers():
    s = torch.tensor([[4.0, 1.0, 3.0, 2.0]], dtype=torch.float64)
    bound = torch.full((1, 4), 0.25, dtype=torch.float64)
    pop = C.allowed(1, 4, [[0]])
    C.check_floor(torch.tensor([[2, 3]]), torch.tensor([[3.1, 1.9]]), s, bound, pop, 2)
    for idx, score in (([[0, 2]], [[4.0, 3.0]]),               # a row outside the population
                       ([[2, 1]], [[3.0, 1.0]]),               # row 3 is left out and beats the floor by more than 2 bounds
                       ([[3, 2]], [[2.0, 3.0]]),               # ascending
                       ([[2, 3]], [[3.3, 2.0]])):              # a score off by more than its bound
        try:
            C.check_floor(torch.tensor(idx), torch.tensor(score), s, bound, pop, 2)
        except AssertionError:
            continue
        raise AssertionError((idx, score))
    assert C.dot_bound(torch.tensor([[1.0, -2.0]]), torch.tensor([[3.0, 4.0], [0.0, -1.0]])).tolist() == [[22 * 2.0 ** -23, 4 * 2.0 ** -23]]
    assert C.same((torch.tensor([1]), torch.tensor([0.0])), (torch.tensor([1]), torch.tensor([0.0])))
    assert not C.same(torch.tensor([0.0]), torch.tensor([-0.0])) and not C.same(torch.tensor([1, 2]), torch.tensor([1, 3]))
    U, T = C.int_vectors(3, 2, 5, 4)
    assert U.shape == (2, 4) and T.shape == (5, 4) and float(U.abs().max()) <= 4 and torch.equal(U, U.round())
