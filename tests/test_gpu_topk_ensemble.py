"""Z-scored ensemble full-catalogue top-k (``nrl_topk_ensemble_scores`` / ``ops.topk_ensemble_scores`` /
``MannerVectorCache.recommend_ensemble``): T <= 3 sub-models, a table row's score is ``sum_t w_t (s_t - mu_t) / sd_t`` with the
mean and the unbiased standard deviation taken over the user's population (eligible, not excluded).

Expected values are computed on the CPU in float64 (tests/topk_ensemble_ref.py).  The statistics are compared under the derived
worst case of that module's docstring (``dmu``, ``dsd``: from ``bs = D 2^-23 sum_i |u_i| |t_i|`` per dot product, the rounding of the
wave sum and of at most ``tiles_per_chunk + chunks`` pairwise updates -- not a measured number; tests/test_topk_ensemble_host.py
checks on the CPU that fp32 in the prescribed order stays inside it and that it is below 1 % of sd).  A returned score is compared
under

  tol[v] = sum_t |w_t| ((bs_t[v] + dmu_t) / sd_t + |z_t[v]| dsd_t / sd_t) + 8 * 2^-23 * sum_t |w_t z_t[v]|

(the raw score and the mean move the numerator, sd the quotient; the subtraction, the division, the product and the sum over t are
a few roundings of the terms).  Integer-valued vectors in [-4, 4] make the raw scores exact and full of ties: there the rows are
those of ``ops.topk_scores`` and every score is ``(s - mu) / sd`` in fp32 from the returned statistics, bit for bit."""
import functools
import warnings

import pytest
import torch

from tests import builders
from tests import catalogue_ref as C
from tests import topk_ensemble_ref as R

pytestmark = pytest.mark.gpu

E_EXCLUDE, E_OFFSETS, E_NAN, E_STATS = 1, 2, 4, 8
WEIGHTS = (1.0, 0.2, -0.25)


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


def _run(users, tables, weights, k, excl=None, eligible=None, slices=0, off=None):
    from newsreclib_amd import ops
    ei = eo = None
    if excl is not None:
        ei, eo = C.ragged([list(x) for x in excl])
        ei, eo = ei.cuda(), (off if off is not None else eo).cuda()
    idx, score, status, stats = ops.topk_ensemble_scores([u.cuda() for u in users], [t.cuda() for t in tables], list(weights), k, ei,
                                                         eo, eligible.cuda() if eligible is not None else None, slices)
    return idx.cpu(), score.cpu(), int(status), stats.cpu()


def _blank(idx, score, b):
    return bool((idx[b] == -1).all()) and bool((score[b] == float("-inf")).all())


# ---- 1. statistics against float64 -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _stats_expected(V, D):
    users, tables, eligible, excl = R.stats_case(V, D)
    pop = C.allowed(R.STATS_B, V, excl, eligible)
    per_t = R.stats64(users, tables, pop)
    return users, tables, eligible, excl, [(n, mean, sd) + R.stat_bounds(s, bs, n, sd, pop, V) for s, bs, n, mean, sd in per_t]


@pytest.mark.parametrize("V", R.STATS_V)
@pytest.mark.parametrize("D", R.STATS_D)
def test_statistics_against_float64(V, D):
    """T in (1, 2, 3) x B in (1, 64, 65) at every (V, D): the first B users of the first T sub-models of one case (a user's
    statistics do not depend on the others).  Masked rows 0 and V - 1, an empty exclusion list, one with duplicates, one of 150
    entries and one with indices outside V (flagged, ignored); a user left with fewer than two rows is flagged and gets NaN."""
    users, tables, eligible, excl, expected = _stats_expected(V, D)
    for T in (1, 2, 3):
        for B in (1, 64, 65):
            idx, score, status, stats = _run([u[:B] for u in users[:T]], tables[:T], WEIGHTS[:T], 1, excl[:B], eligible)
            few = expected[0][0][:B] < 2
            want = (E_EXCLUDE if B > 3 else 0) | (E_STATS if bool(few.any()) else 0)
            assert status == want, (T, B, status, want)
            assert stats.shape == (B, T, 2)
            for t in range(T):
                n, mean, sd, dmu, dsd = (x[:B] for x in expected[t])
                ok = ~few
                assert bool(torch.isnan(stats[:, t, 1][few]).all()) and bool(torch.isnan(stats[:, t, 0][n == 0]).all())
                em, es = (stats[:, t, 0].double() - mean).abs()[ok], (stats[:, t, 1].double() - sd).abs()[ok]
                if em.numel():
                    print(f"T = {T}, B = {B}, t = {t}: |mean - float64| <= {float(em.max()):.3e} (dmu >= {float(dmu[ok].min()):.3e}), "
                          f"|sd - float64| <= {float(es.max()):.3e} (dsd >= {float(dsd[ok].min()):.3e})")
                assert bool((em <= dmu[ok]).all()) and bool((es <= dsd[ok]).all())
            for b in range(B):
                assert _blank(idx, score, b) == bool(few[b]), b


# ---- 2. exact ranking, T = 1 -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,V,D,k,slices", [(64, 1000, 300, 5, 0), (65, 129, 4, 128, 2), (130, 1000, 768, 65, 7), (1, 2, 4, 1, 0)])
def test_exact_ranking_of_one_table(B, V, D, k, slices):
    from newsreclib_amd import ops
    (U,), (T,) = _int_case(B * 7 + V + D + k, 1, B, V, D)
    excl = eligible = None
    if V >= 129:                                            # (at V = 2 both rows are the population)
        g = torch.Generator().manual_seed(V + k)
        excl = [torch.randint(0, V, (int(n),), generator=g).tolist() for n in torch.randint(0, 30, (B,), generator=g)]
        eligible = torch.ones(V, dtype=torch.uint8)
        eligible[[0, 77, V - 1]] = 0
    s = (U.double() @ T.double().T).float()                 # exact
    assert bool((s.max(1)[0] > s.min(1)[0]).all())          # (no user's scores are all equal: every sd is positive)
    ei, eo = C.ragged(excl) if excl is not None else (None, None)
    cuda = lambda t: t.cuda() if t is not None else None  # noqa: E731
    for sign in (1.0, -1.0):
        want_idx, _, want_status = ops.topk_scores((sign * U).cuda(), T.cuda(), k, cuda(ei), cuda(eo), cuda(eligible))
        idx, score, status, stats = _run([U], [T], [sign], k, excl, eligible, slices)
        assert status == 0 and int(want_status) == 0
        assert torch.equal(idx, want_idx.cpu()), sign
        z64 = sign * s.double()                             # (z is strictly increasing in sign * s)
        assert torch.equal(idx, C.topk(z64, C.population(z64, excl, eligible)[0], k)[0]), sign
        mu, sd = stats[:, 0, 0:1], stats[:, 0, 1:2]
        z = sign * ((s - mu) / sd)                          # fp32, every operation rounded on its own, as the kernel
        want_score = torch.where(idx >= 0, z.gather(1, idx.clamp(min=0)), torch.full_like(z[:, :1], float("-inf")).expand_as(idx))
        assert torch.equal(score, want_score), sign


# ---- 3. ties across three tables -----------------------------------------------------------------------------------------------------------
def test_copies_of_one_row_lead_in_ascending_row_order_with_equal_bits():
    B, V, D, k = 9, 1000, 16, 5
    users, tables = R.real_case(3, 3, B, V, D)
    for U, T in zip(users, tables):                         # every user's last coordinate is 1 and only the copies use it
        U[:, -1] = 1.0
        T[:, -1] = 0.0
        T[[5, 130, 700]] = 0.0
        T[[5, 130, 700], -1] = 1000.0
    idx, score, status, _ = _run(users, tables, WEIGHTS, k, slices=3)
    assert status == 0
    assert torch.equal(idx[:, :3], torch.tensor([5, 130, 700]).expand(B, 3))
    assert torch.equal(C.bits(score[:, 0]), C.bits(score[:, 1])) and torch.equal(C.bits(score[:, 0]), C.bits(score[:, 2]))
    assert bool((score[:, 3] < score[:, 2]).all())


# ---- 4. real values against float64 ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _real_expected(D):
    B, V = 9, 5000
    users, tables = R.real_case(31 + D, 3, B, V, D)
    g = torch.Generator().manual_seed(D)
    excl = tuple(tuple(torch.randint(0, V, (int(n),), generator=g).tolist()) for n in torch.randint(0, 51, (B,), generator=g))
    pop = C.allowed(B, V, excl)
    return users, tables, excl, pop, R.ensemble64(users, tables, WEIGHTS, pop)


@pytest.mark.parametrize("D", [8, 256, 768])
def test_real_values_against_float64(D):
    k = 10
    users, tables, excl, pop, (agg, tol) = _real_expected(D)
    idx, score, status, _ = _run(users, tables, WEIGHTS, k, excl)
    assert status == 0
    C.check_floor(idx, score, agg, tol, pop, k)


# ---- 5. agreement with the impression scorer ---------------------------------------------------------------------------------------------
def _history_means(tables, hist, hs):
    """users[t] (B, D) on the device the way ``recommend_ensemble`` forms them: gather, dense rows, the history-mean kernel."""
    from newsreclib_amd import ops
    from newsreclib_amd.dense_batch import dense_rows
    B = int(hs.numel())
    off = torch.cat([torch.zeros(1, dtype=torch.int64), hs.cumsum(0)]).cuda()
    batch = torch.repeat_interleave(torch.arange(B), hs).cuda()
    out = []
    for vec in tables:
        hv = ops.embedding_gather(vec, hist.cuda().reshape(-1, 1)).reshape(-1, vec.shape[1])
        out.append(ops.HistMeanFn.apply(dense_rows(hv, batch, B, int(hs.max()), off), off))
    return out


def _check_against_impression_scorer(tables, weights, lists, idx, score, scorer):
    """``scorer(cand_idx, cand_sizes) -> (B, max_cand)`` is the impression scorer over the same tables and histories; the candidate
    list of user b is its whole population.  Both sides carry the derived error, so the bound is twice ``tol``."""
    B, V = len(lists), tables[0].shape[0]
    hs = torch.tensor([len(x) for x in lists])
    pop = C.allowed(B, V, [x.tolist() for x in lists])
    cand = [torch.nonzero(pop[b]).reshape(-1) for b in range(B)]
    cs = torch.tensor([len(c) for c in cand])
    out = scorer(torch.cat(cand), cs).double().cpu()
    full = torch.zeros(B, V, dtype=torch.float64)
    for b in range(B):
        full[b, cand[b]] = out[b, :len(cand[b])]
    users = [u.cpu() for u in _history_means(tables, torch.cat(lists), hs)]
    _, tol = R.ensemble64(users, [t.cpu() for t in tables], weights, pop)
    C.check_floor(idx.cpu(), score.cpu(), full, 2 * tol, pop, idx.shape[1])


def test_agreement_with_the_impression_scorer():
    from newsreclib_amd import ops
    from newsreclib_amd.ops_manner import manner_scores
    B, V, D, k = 5, 1500, 64, 10
    _, tables = R.real_case(5, 3, B, V, D)
    tables = [t.cuda() for t in tables]
    g = torch.Generator().manual_seed(6)
    lists = [torch.randint(0, V, (int(n),), generator=g) for n in torch.randint(1, 7, (B,), generator=g)]
    hs = torch.tensor([len(x) for x in lists])
    hist = torch.cat(lists).cuda()
    hoff = torch.cat([torch.zeros(1, dtype=torch.int64), hs.cumsum(0)]).cuda()
    users = _history_means(tables, hist, hs)
    idx, score, status, _ = ops.topk_ensemble_scores(users, tables, list(WEIGHTS), k, hist, hoff)
    assert int(status) == 0

    def scorer(cand_idx, cs):
        coff = torch.cat([torch.zeros(1, dtype=torch.int64), cs.cumsum(0)]).cuda()
        return manner_scores(tables, list(WEIGHTS), hist, hoff, cand_idx.cuda(), coff, int(cs.max()))

    _check_against_impression_scorer(tables, WEIGHTS, lists, idx, score, scorer)


# ---- 6. status ---------------------------------------------------------------------------------------------------------------------------
_STATUS_SHAPE = (5, 300, 12)


def _status_case(seed, T=2):
    B, V, D = _STATUS_SHAPE
    return _int_case(seed, T, B, V, D)


def _same_users(a, b, users):
    return torch.equal(a[0][users], b[0][users]) and torch.equal(C.bits(a[1][users]), C.bits(b[1][users])) and \
        torch.equal(C.bits(a[3][users]), C.bits(b[3][users]))


def test_status_a_population_of_one_row_blanks_that_user_alone():
    B, V, D = _STATUS_SHAPE
    users, tables = _status_case(41)
    k = 7
    clean = _run(users, tables, WEIGHTS[:2], k, [[1, 2], [], [], [7, 7], [5]])
    assert clean[2] == 0
    out = _run(users, tables, WEIGHTS[:2], k, [[1, 2], [], [v for v in range(V) if v != 123], [7, 7], [5]])
    assert out[2] == E_STATS
    assert _blank(out[0], out[1], 2) and bool(torch.isnan(out[3][2, :, 1]).all())
    assert _same_users(out, clean, [0, 1, 3, 4])


def test_status_a_constant_table_blanks_every_user():
    B, V, D = _STATUS_SHAPE
    users, tables = _status_case(42)
    tables[1] = tables[1][:1].expand(V, D).contiguous()     # integer values: every sum is exact and sd is exactly 0
    idx, score, status, stats = _run(users, tables, WEIGHTS[:2], 4)
    assert status == E_STATS
    assert all(_blank(idx, score, b) for b in range(B))
    assert bool((stats[:, 1, 1] == 0).all()) and bool((stats[:, 0, 1] > 0).all())


def test_status_nan_table_row_is_left_out_for_every_user():
    B, V, D = _STATUS_SHAPE
    users, tables = _status_case(43)
    k = 9
    clean = _run(users, tables, WEIGHTS[:2], k, slices=2)
    assert clean[2] == 0
    nan_row = int(clean[0][0, 0])                           # a row that would be returned
    elig = torch.ones(V, dtype=torch.uint8)
    elig[nan_row] = 0
    want = _run(users, tables, WEIGHTS[:2], k, eligible=elig, slices=2)
    assert want[2] == 0
    # the row is NaN in every table: it leaves every table's statistics, and every other position is that of the run without it
    tn = [t.clone() for t in tables]
    for t in tn:
        t[nan_row, 3] = float("nan")
    out = _run(users, tn, WEIGHTS[:2], k, slices=2)
    assert out[2] == E_NAN
    assert not bool((out[0] == nan_row).any())
    assert _same_users(out, want, list(range(B)))
    # NaN in one table alone: it leaves that table's statistics only (the other table's still count the row)
    tn = [tables[0], tn[1]]
    out = _run(users, tn, WEIGHTS[:2], k, slices=2)
    assert out[2] == E_NAN
    assert not bool((out[0] == nan_row).any())
    assert torch.equal(C.bits(out[3][:, 0]), C.bits(clean[3][:, 0])) and torch.equal(C.bits(out[3][:, 1]), C.bits(want[3][:, 1]))


def test_status_nan_in_one_users_vector_blanks_that_user_alone():
    B, V, D = _STATUS_SHAPE
    users, tables = _status_case(44)
    k = 9
    clean = _run(users, tables, WEIGHTS[:2], k)
    assert clean[2] == 0
    un = [users[0], users[1].clone()]
    un[1][2, 5] = float("nan")
    out = _run(un, tables, WEIGHTS[:2], k)
    assert out[2] == E_NAN | E_STATS
    assert _blank(out[0], out[1], 2)
    assert _same_users(out, clean, [0, 1, 3, 4])


def test_status_decreasing_offsets_blank_that_user_alone():
    B, V, D = _STATUS_SHAPE
    users, tables = _status_case(45)
    k = 6
    flat = list(range(12))
    off = torch.tensor([0, 5, 3, 8, 12, 12])                # user 1 runs backwards
    out = _run(users, tables, WEIGHTS[:2], k, [flat], off=off)
    assert out[2] == E_OFFSETS
    assert _blank(out[0], out[1], 1)
    want = _run(users, tables, WEIGHTS[:2], k, [flat[0:5], [], flat[3:8], flat[8:12], []])
    assert want[2] == 0 and _same_users(out, want, [0, 2, 3, 4])


# ---- 7. invariance and determinism -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [1000, 8200])
def test_invariance_and_determinism(V):
    """Bit-equal rows, scores and statistics whatever the slicing, the batch (all 70 users one at a time), the GEMM engine setting
    (both are set here, inside the one test, on top of the fixture's) and on a second run."""
    from newsreclib_amd import _lib, ops
    B, D, k = 70, 256, 10
    users, tables = R.real_case(V + 1, 3, B, V, D)
    users, tables = [u.cuda() for u in users], [t.cuda() for t in tables]
    g = torch.Generator().manual_seed(V)
    excl = [torch.randint(0, V, (int(n),), generator=g).tolist() for n in torch.randint(0, 80, (B,), generator=g)]
    ragged = [tuple(t.cuda() for t in C.ragged([x])) for x in excl]
    ei, eo = (t.cuda() for t in C.ragged(excl))
    elig = torch.ones(V, dtype=torch.uint8)
    elig[[0, 500, V - 1]] = 0
    elig = elig.cuda()

    def run(slices=0):
        return ops.topk_ensemble_scores(users, tables, list(WEIGHTS), k, ei, eo, elig, slices)

    def same(out, name):
        assert int(out[2]) == 0, name
        assert torch.equal(out[0], base[0]) and torch.equal(C.bits(out[1]), C.bits(base[1])), name
        assert torch.equal(C.bits(out[3]), C.bits(base[3])), name

    base = run()
    assert int(base[2]) == 0 and bool((base[0] >= 0).all())
    for slices in (1, 2, 7, 0):
        same(run(slices), slices)
    singles = [ops.topk_ensemble_scores([u[b:b + 1] for u in users], tables, list(WEIGHTS), k, ragged[b][0], ragged[b][1], elig)
               for b in range(B)]
    same(tuple(torch.cat([s[i] for s in singles]) if i != 2 else sum(s[2] for s in singles) for i in range(4)), "one at a time")
    prev = _lib.get_gemm_engine()
    try:
        for name in ("f32", "bf16x3"):
            _lib.set_gemm_engine(name)
            same(run(), name)
    finally:
        _lib.set_gemm_engine(prev)


# ---- 8. memory -----------------------------------------------------------------------------------------------------------------------------
def test_peak_memory_is_far_below_the_score_matrices():
    from newsreclib_amd import ops
    B, V, D, T, k = 64, 20000, 64, 3, 10
    users, tables = R.real_case(2, T, B, V, D)
    users, tables = [u.cuda() for u in users], [t.cuda() for t in tables]
    ops.topk_ensemble_scores([u[:2] for u in users], [t[:256] for t in tables], list(WEIGHTS), k)      # kernels resident
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    live = torch.cuda.memory_allocated()
    out = ops.topk_ensemble_scores(users, tables, list(WEIGHTS), k)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - live
    print(f"peak above the inputs: {peak} bytes; the T (B, V) score matrices: {T * B * V * 4} bytes")
    assert peak < T * B * V * 4 / 8
    assert int(out[2]) == 0 and bool((out[0] >= 0).all())


# ---- 9. no read-back -------------------------------------------------------------------------------------------------------------------------
def test_topk_ensemble_scores_does_not_synchronise_with_the_host():
    from newsreclib_amd import ops
    users, tables = _int_case(3, 3, 5, 200, 12)
    users, tables = [u.cuda() for u in users], [t.cuda() for t in tables]
    ei, eo = C.ragged([[1, 2], [], [5], [7, 7], []])
    ei, eo, elig = ei.cuda(), eo.cuda(), torch.ones(200, dtype=torch.bool).cuda()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        if not C.sync_debug_honoured():
            pytest.skip("this torch build does not raise on synchronising calls under set_sync_debug_mode('error')")
        out = ops.topk_ensemble_scores(users, tables, list(WEIGHTS), 4, ei, eo, elig)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert int(out[2]) == 0 and out[0].shape == (5, 4) and out[3].shape == (5, 3, 2)


# ---- 10. wiring ------------------------------------------------------------------------------------------------------------------------------
def test_recommend_ensemble_against_the_cache_scores(tmp_path):
    from newsreclib_amd.evaluation import MannerVectorCache, recommend_users
    cr, ac, asent = builders.manner_modules(tmp_path)
    ens = builders.manner_ensemble(cr, ac, asent)
    table, imps = builders.manner_table_and_impressions()
    V, B, k = table.num_news, len(imps), 10
    cache = MannerVectorCache(ens, table)
    lists = [i["hist"] for i in imps]
    hs = torch.tensor([len(x) for x in lists])
    hist = torch.cat(lists)
    ens.train()
    idx, score, status, stats = cache.recommend_ensemble(hist.cuda(), hs, k, return_stats=True)
    assert ens.training                                          # the mode is restored
    ens.eval()
    assert int(status) == 0 and idx.shape == (B, k) and stats.shape == (B, 3, 2)
    assert len(cache.recommend_ensemble(hist.cuda(), hs, k)) == 3
    _check_against_impression_scorer(cache.vectors, cache.weights, lists, idx, score,
                                     lambda cand_idx, cs: cache.scores(hist, hs, cand_idx, cs))
    # without the exclusion the history may appear: every row of the table is returned when k is its length
    idx2, _, status2 = cache.recommend_ensemble(hist.cuda(), hs, V, exclude_history=False)
    assert int(status2) == 0 and all(set(idx2[b].tolist()) == set(range(V)) for b in range(B))
    # recommend_users takes this entry: the same rows in the same order for the same batch, and no warning
    users = [{"hist": lists[b], "user_id": 100 + b} for b in range(B)]
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        recs = recommend_users(cache, users, k, batch_size=B + 3)
    assert not [w for w in caught if "recommend_users" in str(w.message)]
    assert list(recs) == [f"U{100 + b}" for b in range(B)]
    assert all(list(recs[f"U{100 + b}"]) == [f"N{int(i)}" for i in idx[b]] for b in range(B))
    assert list(recs["U100"].values()) == [float(v) for v in score[0]]
    # a user without history has a NaN vector: refused through the flags, which recommend_users passes on as a warning
    with pytest.warns(UserWarning, match="standardised"):
        recs = recommend_users(cache, users + [{"hist": torch.zeros(0, dtype=torch.int64), "user_id": 7}], k, batch_size=B + 3)
    assert recs["U7"] == {} and list(recs["U100"]) == [f"N{int(i)}" for i in idx[0]]
    # the weight-0 ensemble is the CR-Module alone (T = 1)
    only = MannerVectorCache(builders.manner_ensemble(cr, None, None, cw=0, sw=0), table)
    idx1, score1, status1, stats1 = only.recommend_ensemble(hist.cuda(), hs, k, return_stats=True)
    assert int(status1) == 0 and stats1.shape == (B, 1, 2) and only.weights == [1.0]
    _check_against_impression_scorer(only.vectors, only.weights, lists, idx1, score1,
                                     lambda cand_idx, cs: only.scores(hist, hs, cand_idx, cs))
    # and `recommend` itself still refuses
    with pytest.raises(NotImplementedError, match="z-scores"):
        cache.recommend(hist.cuda(), hs, k)
