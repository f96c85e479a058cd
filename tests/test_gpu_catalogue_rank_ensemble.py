"""Full-catalogue rank of held-out clicks under MANNeR's ensemble of standardised scores (``nrl_catalogue_ensemble_ranks`` /
``ops.catalogue_ensemble_ranks`` / ``MannerVectorCache.rank_clicks_ensemble`` / ``evaluate_full_rank(ensemble=True)``).

Three references (tests/catalogue_rank_ensemble_ref.py):

* exact, at any D: every table's (B, V) raw fp32 score matrix is rebuilt bit for bit with ``ops.topk_scores`` (k = 128 over
  eligibility windows of 128 rows: raw scores have no statistics, so a window does not change them), the ensemble score is formed
  on the CPU in fp32 from the returned statistics, one rounded operation at a time in ascending t, and the ranks are counted in
  the order of the entry.  Every rank, population and score bit must be equal;
* ``ops.topk_ensemble_scores``: ``rank = r <= k`` exactly when slot ``r - 1`` of that call is the click, with equal score bits and
  equal statistics bits;
* float64 at D <= 64 under the derived tolerance of ``topk_ensemble_ref.ensemble64``: each rank inside its interval (the
  host tier checks on the reference alone that the intervals are sharp on these inputs)."""
import functools
import warnings

import pytest
import torch

from tests import builders
from tests import catalogue_rank_ensemble_ref as ER
from tests import catalogue_ref as C
from tests import topk_ensemble_ref as R

pytestmark = pytest.mark.gpu

E_EXCLUDE, E_OFFSETS, E_NAN, E_STATS, E_TARGETS, E_TARGET_ROW = 1, 2, 4, 8, 16, 32
NEG_INF = float("-inf")
WEIGHTS = ER.WEIGHTS


@pytest.fixture(autouse=True, params=["f32", "bf16x3"])
def engine(request):
    from newsreclib_amd import _lib
    prev = _lib.get_gemm_engine()
    _lib.set_gemm_engine(request.param)
    yield request.param
    _lib.set_gemm_engine(prev)


def _int_case(seed, T, B, V, D):
    g = torch.Generator().manual_seed(seed)
    return ([torch.randint(-4, 5, (B, D), generator=g).float() for _ in range(T)],
            [torch.randint(-4, 5, (V, D), generator=g).float() for _ in range(T)])


def _run(users, tables, weights, targets, excl=None, eligible=None, slices=0, tgt_off=None, excl_off=None):
    from newsreclib_amd import ops
    ti, to = C.ragged([list(x) for x in targets])
    ei = eo = None
    if excl is not None:
        ei, eo = C.ragged([list(x) for x in excl])
        ei, eo = ei.cuda(), (excl_off if excl_off is not None else eo).cuda()
    rank, score, ranked, status, stats = ops.catalogue_ensemble_ranks(
        [u.cuda() for u in users], [t.cuda() for t in tables], list(weights), ti.cuda(), (tgt_off if tgt_off is not None else to).cuda(),
        ei, eo, eligible.cuda() if eligible is not None else None, slices)
    return rank.cpu(), score.cpu(), ranked.cpu(), int(status), stats.cpu()


def _topk(users, tables, weights, k, excl=None, eligible=None, slices=0):
    from newsreclib_amd import ops
    ei = eo = None
    if excl is not None:
        ei, eo = (t.cuda() for t in C.ragged([list(x) for x in excl]))
    idx, score, status, stats = ops.topk_ensemble_scores([u.cuda() for u in users], [t.cuda() for t in tables], list(weights), k, ei, eo,
                                                         eligible.cuda() if eligible is not None else None, slices)
    return idx.cpu(), score.cpu(), int(status), stats.cpu()


def _same_slots(a, b, slots):
    return torch.equal(a[0][slots], b[0][slots]) and torch.equal(C.bits(a[1][slots]), C.bits(b[1][slots]))


def _same_users(a, b, users):
    return torch.equal(a[2][users], b[2][users]) and torch.equal(C.bits(a[4][users]), C.bits(b[4][users]))


def _slots(targets, users):
    """the flat slots of the given users' targets"""
    off = [0]
    for tl in targets:
        off.append(off[-1] + len(tl))
    return torch.tensor([j for b in users for j in range(off[b], off[b + 1])], dtype=torch.int64)


def _raw_scores(U, T):
    """(B, V) fp32 on the CPU: the library's own raw score bits, NaN where the score is NaN."""
    from newsreclib_amd import ops
    B, V = U.shape[0], T.shape[0]
    U, T = U.cuda(), T.cuda()
    out = torch.full((B, V), float("nan"))
    users = torch.arange(B)[:, None].expand(B, 128)
    for lo in range(0, V, 128):
        window = torch.zeros(V, dtype=torch.uint8)
        window[lo:lo + 128] = 1
        idx, score, _ = ops.topk_scores(U, T, 128, eligible=window.cuda())
        idx, score = idx.cpu(), score.cpu()
        ok = idx >= 0
        out[users[ok], idx[ok]] = score[ok]
    return out


# ---- 1. exact ranks from the library's own bits ------------------------------------------------------------------------------------
EXACT = [(1, 1, 2, 4, 0), (2, 64, 2, 4, 2), (3, 65, 2, 4, 7), (1, 130, 2, 4, 0),
         (3, 1, 129, 4, 2), (1, 64, 129, 300, 7), (2, 65, 129, 4, 0), (3, 130, 129, 4, 2),
         (2, 1, 1000, 768, 7), (3, 64, 1000, 4, 0), (1, 65, 1000, 4, 2), (3, 130, 1000, 300, 7), (3, 65, 1000, 768, 0)]


@functools.lru_cache(maxsize=None)
def _exact_case(T, B, V, D):
    """Inputs and the raw score matrices of one shape (shared by both engine settings: the raw bits do not depend on it).  From
    V = 129 on: exclusion lists of 0 to 29 rows, a mask that clears rows 0, 77 and V - 1, and row 100 a copy of row 3 in every
    table (equal ensemble scores: the tie goes to the lower row).  At V = 2 both rows are everybody's population."""
    users, tables = R.real_case(B * 7 + V + D + T, T, B, V, D)
    excl = eligible = None
    if V >= 129:
        g = torch.Generator().manual_seed(V + B)
        excl = [torch.randint(0, V, (int(n),), generator=g).tolist() for n in torch.randint(0, 30, (B,), generator=g)]
        excl[0] = excl[0] or [9]
        eligible = torch.ones(V, dtype=torch.uint8)
        eligible[[0, 77, V - 1]] = 0
        for t in tables:
            t[100] = t[3]
    clicks = ER.click_lists(B + V + D, B, V, excl, eligible)
    if V >= 129 and B > 1:
        clicks[1] = ([3, 100] + clicks[1])[:32]
    return users, tables, excl, eligible, clicks, [_raw_scores(u, t) for u, t in zip(users, tables)]


@pytest.mark.parametrize("T,B,V,D,slices", EXACT)
def test_exact_ranks_from_the_librarys_own_bits(T, B, V, D, slices):
    users, tables, excl, eligible, clicks, raw = _exact_case(T, B, V, D)
    assert len(clicks[0]) == 32 and (B == 1 or sum(len(c) for c in clicks) > 64)
    rank, score, ranked, status, stats = _run(users, tables, WEIGHTS[:T], clicks, excl, eligible, slices)
    assert status == E_TARGET_ROW                              # user 0 clicks -1 and V
    assert bool(ER.sd_ok(stats[:, :, 1]).all())
    want = ER.ranks_from_bits(raw, stats, WEIGHTS[:T], clicks, excl, eligible)
    assert torch.equal(ranked, want[2])
    assert torch.equal(rank, want[0])
    assert torch.equal(C.bits(score), C.bits(want[1]))
    r0 = rank[:32].tolist()                                   # user 0: a duplicate, -1, V, an excluded row, an ineligible row
    assert r0[0] == r0[1] and r0[2] == r0[3] == 0
    if V >= 129:
        assert r0[4] == r0[5] == 0 and bool((score[2:6] == NEG_INF).all())
        if B > 1:                                             # rows 3 and 100 are copies: equal bits, adjacent ranks
            a, b = int(rank[32]), int(rank[33])
            if a and b:
                assert b == a + 1 and torch.equal(C.bits(score[32]), C.bits(score[33]))


# ---- 2. agreement with the top-k ---------------------------------------------------------------------------------------------------
def _agrees_with_topk(rank, score, clicks, idx, top_score, k):
    at = 0
    for b, cl in enumerate(clicks):
        for c in cl:
            r = int(rank[at])
            assert (1 <= r <= k) == bool((idx[b] == c).any()), (b, c, r, k)
            if 1 <= r <= k:
                assert int(idx[b, r - 1]) == c and torch.equal(C.bits(score[at]), C.bits(top_score[b, r - 1])), (b, c, r, k)
            at += 1


@pytest.mark.parametrize("T,B,V,D", [(3, 65, 1000, 64), (2, 5, 300, 768)])
def test_agreement_with_the_topk(T, B, V, D):
    users, tables = R.real_case(B + V + D, T, B, V, D)
    g = torch.Generator().manual_seed(V)
    excl = [torch.randint(0, V, (int(n),), generator=g).tolist() for n in torch.randint(1, 30, (B,), generator=g)]
    eligible = torch.ones(V, dtype=torch.uint8)
    eligible[[0, V - 1]] = 0
    tops = {k: _topk(users, tables, WEIGHTS[:T], k, excl, eligible) for k in (1, 10, 128)}
    idx = tops[128][0]
    clicks = [[int(idx[b, 0]), int(idx[b, 9]), int(idx[b, 127]), int(idx[b, 10])] + torch.randint(0, V, (b % 5,), generator=g).tolist() +
              [excl[b][0], 0] for b in range(B)]
    rank, score, ranked, status, stats = _run(users, tables, WEIGHTS[:T], clicks, excl, eligible, slices=3)
    assert status == 0
    at = 0
    for b in range(B):
        assert rank[at:at + 4].tolist() == [1, 10, 128, 11]
        at += len(clicks[b])
        assert int(rank[at - 1]) == int(rank[at - 2]) == 0     # the excluded row and the ineligible row
    for k, (idx_k, score_k, status_k, stats_k) in tops.items():
        assert status_k == 0 and torch.equal(C.bits(stats_k), C.bits(stats)), k
        _agrees_with_topk(rank, score, clicks, idx_k, score_k, k)


def test_copies_of_one_row_rank_one_two_three_with_equal_bits():
    B, V, D = 9, 1000, 16
    users, tables = R.real_case(3, 3, B, V, D)
    for U, T in zip(users, tables):                         # every user's last coordinate is 1 and only the copies use it
        U[:, -1] = 1.0
        T[:, -1] = 0.0
        T[[5, 130, 700]] = 0.0
        T[[5, 130, 700], -1] = 1000.0
    clicks = [[700, 5, 130]] * B
    rank, score, ranked, status, _ = _run(users, tables, WEIGHTS, clicks, slices=3)
    assert status == 0 and bool((ranked == V).all())
    assert rank.reshape(B, 3).tolist() == [[3, 1, 2]] * B
    s = score.reshape(B, 3)
    assert torch.equal(C.bits(s[:, 0]), C.bits(s[:, 1])) and torch.equal(C.bits(s[:, 0]), C.bits(s[:, 2]))


# ---- 3. float64, small D -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,V,D", ER.INTERVAL_SHAPES)
def test_ranks_inside_the_float64_intervals(B, V, D):
    users, tables, excl, clicks, pop, intervals = ER.interval_case(B, V, D)
    rank, score, ranked, status, _ = _run(users, tables, WEIGHTS, clicks, excl)
    assert status == 0 and torch.equal(ranked, pop.sum(1).to(torch.int32))
    for j, iv in enumerate(intervals):
        r = int(rank[j])
        print(f"target {j}: rank {r}, float64 interval {iv}")
        assert (r == 0 and float(score[j]) == NEG_INF) if iv is None else iv[0] <= r <= iv[1], (j, r, iv)


# ---- 4. status -----------------------------------------------------------------------------------------------------------------------
_STATUS_SHAPE = (5, 300, 12)
_STATUS_CLICKS = [[4, 123, 17], [250], [123, 8, 299, 123], [], [0, 1]]


def _status_case(seed, T=2):
    B, V, D = _STATUS_SHAPE
    return _int_case(seed, T, B, V, D)


def _blank(out, targets, b):
    s = _slots(targets, [b])
    return bool((out[0][s] == 0).all()) and bool((out[1][s] == NEG_INF).all()) and int(out[2][b]) == 0


def test_status_a_population_of_one_row_refuses_that_user_alone():
    B, V, D = _STATUS_SHAPE
    users, tables = _status_case(41)
    clean = _run(users, tables, WEIGHTS[:2], _STATUS_CLICKS, [[1, 2], [], [], [7, 7], [5]])
    assert clean[3] == 0 and bool((clean[0] > 0).all())
    out = _run(users, tables, WEIGHTS[:2], _STATUS_CLICKS, [[1, 2], [], [v for v in range(V) if v != 123], [7, 7], [5]])
    assert out[3] == E_STATS
    assert _blank(out, _STATUS_CLICKS, 2) and bool(torch.isnan(out[4][2, :, 1]).all())
    others = [0, 1, 3, 4]
    assert _same_users(out, clean, others) and _same_slots(out, clean, _slots(_STATUS_CLICKS, others))


def test_status_a_constant_table_refuses_every_user():
    B, V, D = _STATUS_SHAPE
    users, tables = _status_case(42)
    tables[1] = tables[1][:1].expand(V, D).contiguous()     # integer values: every sum is exact and sd is exactly 0
    out = _run(users, tables, WEIGHTS[:2], _STATUS_CLICKS)
    assert out[3] == E_STATS
    assert all(_blank(out, _STATUS_CLICKS, b) for b in range(B))
    assert bool((out[4][:, 1, 1] == 0).all()) and bool((out[4][:, 0, 1] > 0).all())


def test_status_nan_table_row_is_left_out_of_every_population():
    B, V, D = _STATUS_SHAPE
    users, tables = _status_case(43)
    nan_row = 123                                           # users 0 and 2 click it
    elig = torch.ones(V, dtype=torch.uint8)
    elig[nan_row] = 0
    want = _run(users, tables, WEIGHTS[:2], _STATUS_CLICKS, eligible=elig, slices=2)
    assert want[3] == 0 and bool((want[2] == V - 1).all())
    tn = [t.clone() for t in tables]
    for t in tn:
        t[nan_row, 3] = float("nan")
    out = _run(users, tn, WEIGHTS[:2], _STATUS_CLICKS, slices=2)
    assert out[3] == E_NAN
    everyone = list(range(B))
    assert _same_users(out, want, everyone) and _same_slots(out, want, _slots(_STATUS_CLICKS, everyone))
    assert out[0].tolist()[1] == 0 and out[0].tolist()[4] == out[0].tolist()[7] == 0 and float(out[1][1]) == NEG_INF
    # NaN in one table alone: the row leaves that table's statistics and, its ensemble score being NaN, every population
    out = _run(users, [tables[0], tn[1]], WEIGHTS[:2], _STATUS_CLICKS, slices=2)
    assert out[3] == E_NAN and bool((out[2] == V - 1).all()) and out[0].tolist()[1] == 0
    assert torch.equal(C.bits(out[4][:, 1]), C.bits(want[4][:, 1]))


def test_status_nan_in_one_users_vector_refuses_that_user_alone():
    users, tables = _status_case(44)
    clean = _run(users, tables, WEIGHTS[:2], _STATUS_CLICKS)
    assert clean[3] == 0
    un = [users[0], users[1].clone()]
    un[1][2, 5] = float("nan")
    out = _run(un, tables, WEIGHTS[:2], _STATUS_CLICKS)
    assert out[3] == E_NAN | E_STATS
    assert _blank(out, _STATUS_CLICKS, 2)
    others = [0, 1, 3, 4]
    assert _same_users(out, clean, others) and _same_slots(out, clean, _slots(_STATUS_CLICKS, others))


def test_status_decreasing_exclusion_offsets_refuse_that_user_alone():
    users, tables = _status_case(45)
    flat = list(range(30, 42))
    off = torch.tensor([0, 5, 3, 8, 12, 12])                # user 1 runs backwards
    out = _run(users, tables, WEIGHTS[:2], _STATUS_CLICKS, [flat], excl_off=off)
    assert out[3] == E_OFFSETS
    assert _blank(out, _STATUS_CLICKS, 1)
    want = _run(users, tables, WEIGHTS[:2], _STATUS_CLICKS, [flat[0:5], [], flat[3:8], flat[8:12], []])
    others = [0, 2, 3, 4]
    assert want[3] == 0 and torch.equal(out[2][others], want[2][others])
    assert _same_slots(out, want, _slots(_STATUS_CLICKS, others))
    assert torch.equal(C.bits(out[4][others]), C.bits(want[4][others]))


def test_status_decreasing_target_offsets_refuse_that_user_alone():
    users, tables = _status_case(46)
    flat = [3, 9, 9, 0, 21, 39, 5, 6, 7]
    off = torch.tensor([0, 4, 9, 7, 7, 9])                  # user 2 runs backwards; user 3 is empty; user 4 owns slots 7 and 8
    out = _run(users, tables, WEIGHTS[:2], [flat], tgt_off=off)
    assert out[3] == E_TARGETS
    want = _run(users, tables, WEIGHTS[:2], [flat[0:4], flat[4:7], [], [], flat[7:9]])
    assert want[3] == 0
    # slots 4 .. 8 were claimed by users 1 and 4 (the later user owns 7 and 8); user 1 keeps 4, 5, 6
    assert torch.equal(out[0], want[0]) and torch.equal(C.bits(out[1]), C.bits(want[1]))
    assert torch.equal(out[2], want[2]) and torch.equal(C.bits(out[4]), C.bits(want[4]))


def test_status_33_clicks_through_the_c_entry_refuse_that_user_alone():
    users, tables = _status_case(47)
    clicks = [list(c) for c in _STATUS_CLICKS]
    clean = _run(users, tables, WEIGHTS[:2], clicks)
    clicks[3] = list(range(33))
    out = _run(users, tables, WEIGHTS[:2], clicks)
    assert out[3] == E_TARGETS
    s3 = _slots(clicks, [3])
    assert bool((out[0][s3] == 0).all()) and bool((out[1][s3] == NEG_INF).all())
    assert torch.equal(out[2], clean[2]) and torch.equal(C.bits(out[4]), C.bits(clean[4]))      # the population is still counted
    others = [0, 1, 2, 4]
    a, b = _slots(clicks, others), _slots(_STATUS_CLICKS, others)
    assert torch.equal(out[0][a], clean[0][b]) and torch.equal(C.bits(out[1][a]), C.bits(clean[1][b]))


def test_no_table_and_no_targets():
    """V == 0: ranks 0, populations 0 and the statistics flag; n_targets == 0 still fills the populations and the statistics."""
    users, tables = _status_case(48)
    out = _run(users, [t[:0] for t in tables], WEIGHTS[:2], _STATUS_CLICKS)
    assert out[3] == E_STATS | E_TARGET_ROW and not bool(out[0].any()) and not bool(out[2].any())
    assert bool((out[1] == NEG_INF).all()) and bool(torch.isnan(out[4]).all())
    empty = _run(users, tables, WEIGHTS[:2], [[]] * 5)
    clean = _run(users, tables, WEIGHTS[:2], _STATUS_CLICKS)
    assert empty[3] == 0 and empty[0].numel() == 0 and torch.equal(empty[2], clean[2]) and torch.equal(C.bits(empty[4]), C.bits(clean[4]))


# ---- 5. invariance and determinism ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [1000, 8200])
def test_invariance_and_determinism(V):
    """Bit-equal ranks, scores, populations and statistics whatever the slicing, the batch (every one of the 130 users alone), the
    GEMM engine setting (both are set here, inside the one test, on top of the fixture's) and on a second run."""
    from newsreclib_amd import _lib, ops
    B, D = 130, 256
    users, tables = R.real_case(V + 1, 3, B, V, D)
    users, tables = [u.cuda() for u in users], [t.cuda() for t in tables]
    g = torch.Generator().manual_seed(V)
    excl = [torch.randint(0, V, (int(n),), generator=g).tolist() for n in torch.randint(0, 80, (B,), generator=g)]
    clicks = [torch.randint(0, V, (int(n),), generator=g).tolist() for n in torch.randint(0, 6, (B,), generator=g)]
    clicks[0], clicks[64] = [1, 2, 3], [V - 2, 7]
    ei, eo = (t.cuda() for t in C.ragged(excl))
    ti, to = (t.cuda() for t in C.ragged(clicks))
    elig = torch.ones(V, dtype=torch.uint8)
    elig[[0, 500, V - 1]] = 0
    elig = elig.cuda()

    def run(slices=0):
        return ops.catalogue_ensemble_ranks(users, tables, list(WEIGHTS), ti, to, ei, eo, elig, slices)

    def same(out, name):
        assert int(out[3]) == 0, name
        assert torch.equal(out[0], base[0]) and torch.equal(C.bits(out[1]), C.bits(base[1])), name
        assert torch.equal(out[2], base[2]) and torch.equal(C.bits(out[4]), C.bits(base[4])), name

    base = run()
    assert int(base[3]) == 0 and bool((base[2] > V - 90).all())
    for slices in (1, 2, 7, 0):
        same(run(slices), slices)
    singles = []
    for b in range(B):
        (xi, xo), (ci, co) = C.ragged([excl[b]]), C.ragged([clicks[b]])
        singles.append(ops.catalogue_ensemble_ranks([u[b:b + 1] for u in users], tables, list(WEIGHTS), ci.cuda(), co.cuda(), xi.cuda(),
                                                    xo.cuda(), elig))
    same(tuple(torch.cat([s[i] for s in singles]) if i != 3 else sum(s[3] for s in singles) for i in range(5)), "one at a time")
    prev = _lib.get_gemm_engine()
    try:
        for name in ("f32", "bf16x3"):
            _lib.set_gemm_engine(name)
            same(run(), name)
    finally:
        _lib.set_gemm_engine(prev)


# ---- 6. cache and driver ---------------------------------------------------------------------------------------------------------------
def test_rank_clicks_ensemble_against_recommend_ensemble(tmp_path):
    from newsreclib_amd.evaluation import MannerVectorCache, evaluate_full_rank
    from newsreclib_amd.metrics import full_rank_metrics
    cr, ac, asent = builders.manner_modules(tmp_path)
    ens = builders.manner_ensemble(cr, ac, asent)
    table, imps = builders.manner_table_and_impressions()
    V, B, k = table.num_news, len(imps), 10
    cache = MannerVectorCache(ens, table)
    lists = [i["hist"] for i in imps]
    hs = torch.tensor([len(x) for x in lists])
    hist = torch.cat(lists)
    eligible = torch.ones(V, dtype=torch.uint8)
    eligible[0] = 0
    idx, top_score, st, top_stats = cache.recommend_ensemble(hist.cuda(), hs, k, eligible=eligible, return_stats=True)
    idx, top_score = idx.cpu(), top_score.cpu()
    assert int(st) == 0
    g = torch.Generator().manual_seed(6)
    clicks = [[int(idx[b, 0]), int(idx[b, 3])] + torch.randint(0, V, (b % 4,), generator=g).tolist() + [int(lists[b][0])] for b in range(B)]
    click_idx, cs = torch.tensor([c for cl in clicks for c in cl]), torch.tensor([len(cl) for cl in clicks])
    ens.train()
    rank, score, ranked, status, stats = cache.rank_clicks_ensemble(hist.cuda(), hs, click_idx.cuda(), cs, eligible=eligible,
                                                                    return_stats=True)
    assert ens.training                                          # the mode is restored
    ens.eval()
    assert int(status) == 0 and rank.shape == (int(cs.sum()),) and ranked.shape == (B,) and stats.shape == (B, 3, 2)
    assert len(cache.rank_clicks_ensemble(hist.cuda(), hs, click_idx.cuda(), cs, eligible=eligible)) == 4
    assert torch.equal(C.bits(stats.cpu()), C.bits(top_stats.cpu()))
    rank, score, ranked = rank.cpu(), score.cpu(), ranked.cpu()
    assert ranked.tolist() == [V - len(set(lists[b].tolist()) | {0}) for b in range(B)]    # all but the padding row and the history
    _agrees_with_topk(rank, score, clicks, idx, top_score, k)
    at = 0
    for b in range(B):
        assert int(rank[at]) == 1 and int(rank[at + 1]) == 4
        at += len(clicks[b])
        assert int(rank[at - 1]) == 0 and float(score[at - 1]) == NEG_INF                 # the click from the history
    # without the exclusion a click from the history ranks like any other row
    rank2, _, ranked2, _ = cache.rank_clicks_ensemble(hist.cuda(), hs, click_idx.cuda(), cs, exclude_history=False)
    assert bool((ranked2 == V).all()) and bool((rank2 >= 1).all())

    # evaluate_full_rank(ensemble=True) over two batches: full_rank_metrics of the two calls by hand, and no warning
    g = torch.Generator().manual_seed(13)
    held = [torch.randint(1, V, (int(n),), generator=g) for n in torch.randint(0, 5, (B,), generator=g)]
    held[0] = torch.tensor([1, 2])
    users = [{"hist": lists[b], "clicks": held[b]} for b in range(B)]
    parts, outs = [(0, 5), (5, B)], []
    for lo, hi in parts:
        h, c = torch.cat([lists[b] for b in range(lo, hi)]), torch.cat([held[b] for b in range(lo, hi)])
        outs.append(cache.rank_clicks_ensemble(h.cuda(), hs[lo:hi], c.cuda(), torch.tensor([len(held[b]) for b in range(lo, hi)]),
                                               eligible=eligible))
    assert all(int(o[3]) == 0 for o in outs)
    want = full_rank_metrics(torch.cat([o[0] for o in outs]).cpu(), torch.tensor([len(c) for c in held]),
                             torch.cat([o[2] for o in outs]).cpu(), (5, 10))
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        got = evaluate_full_rank(cache, users, (5, 10), batch_size=5, eligible=eligible, ensemble=True)
    assert got == want and set(got) == {"mrr", "auc_user", "ndcg@5", "ndcg@10", "recall@5", "recall@10", "hit@5", "hit@10"}
    # a status flag comes through as ONE warning, worded for ranks: a user without history has a NaN vector and is refused
    users[1] = dict(users[1], hist=torch.zeros(0, dtype=torch.int64))
    with pytest.warns(UserWarning, match=r"evaluate_full_rank: .*standardised.*ranks and population are 0") as rec:
        evaluate_full_rank(cache, users, (5, 10), batch_size=5, eligible=eligible, ensemble=True)
    assert len(rec) == 1
    # the default path still refuses MANNeR's cache
    with pytest.raises(NotImplementedError, match="only the dot-product families are served"):
        evaluate_full_rank(cache, users, (5, 10), batch_size=5, eligible=eligible)


# ---- 7. memory, no read-back -------------------------------------------------------------------------------------------------------------
def test_peak_memory_is_far_below_one_score_matrix():
    from newsreclib_amd import ops
    B, V, D, T = 256, 16384, 32, 3
    users, tables = R.real_case(2, T, B, V, D)
    users, tables = [u.cuda() for u in users], [t.cuda() for t in tables]
    g = torch.Generator().manual_seed(5)
    clicks = [torch.randint(0, V, (int(n),), generator=g).tolist() for n in torch.randint(1, 6, (B,), generator=g)]
    ti, to = (t.cuda() for t in C.ragged(clicks))
    ops.catalogue_ensemble_ranks([u[:2] for u in users], [t[:256] for t in tables], list(WEIGHTS), ti[:1] * 0, to[:3] * 0)   # kernels resident
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    live = torch.cuda.memory_allocated()
    out = ops.catalogue_ensemble_ranks(users, tables, list(WEIGHTS), ti, to)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - live
    print(f"peak above the inputs: {peak} bytes; one (B, V) fp32 score matrix: {B * V * 4} bytes")
    assert peak < B * V * 4 / 8
    assert int(out[3]) == 0 and bool((out[0] >= 1).all()) and bool((out[2] == V).all())


def test_catalogue_ensemble_ranks_does_not_synchronise_with_the_host():
    from newsreclib_amd import ops
    users, tables = _int_case(3, 3, 5, 200, 12)
    users, tables = [u.cuda() for u in users], [t.cuda() for t in tables]
    ei, eo = C.ragged([[1, 2], [], [5], [7, 7], []])
    ti, to = C.ragged([[3], [4, 4], [], [199], [0, 1, 2]])
    ei, eo, ti, to, elig = ei.cuda(), eo.cuda(), ti.cuda(), to.cuda(), torch.ones(200, dtype=torch.bool).cuda()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        if not C.sync_debug_honoured():
            pytest.skip("this torch build does not raise on synchronising calls under set_sync_debug_mode('error')")
        out = ops.catalogue_ensemble_ranks(users, tables, list(WEIGHTS), ti, to, ei, eo, elig)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert int(out[3]) == 0 and out[0].shape == (7,) and out[2].shape == (5,) and out[4].shape == (5, 3, 2)
