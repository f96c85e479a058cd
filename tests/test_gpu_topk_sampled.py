"""Gumbel top-k on the GPU (``nrl_topk_sampled_scores`` / ``nrl_gumbel_noise``, their ``ops`` wrappers, ``NewsVectorCache.recommend``
with ``sample=``, ``recommend_users(sample=)`` and ``sample_recommendations``).

The noise is checked on its own first: ``u`` bit for bit against the restatement in ``tests/topk_sampled_ref.py``, ``g`` against
float64 within a measured tolerance.  With the device's own ``g32`` given, the sampled call has an exact oracle wherever the scores
are exact in fp32 (integer vectors in [-4, 4], ``inv_temp`` a power of two): ``catalogue_ref.topk`` over
``fl32(fl32(s * inv_temp) + g32)``, compared with ``catalogue_ref.same`` -- bit equality, ties included.  Real-valued cases use the
floor form with a derived bound, and the raw scores have an exact oracle of their own: the plain entry."""
import math

import numpy as np
import pytest
import torch

from tests import builders
from tests import catalogue_ref as C
from tests import topk_sampled_ref as R

pytestmark = pytest.mark.gpu

E_EXCLUDE, E_OFFSETS, E_NAN = 1, 2, 4
NEG_INF = float("-inf")
SHAPES = [(1, 1, 4), (3, 130, 20), (63, 127, 4), (64, 128, 4), (65, 129, 4), (130, 1000, 300), (5, 128, 1024)]
INV_TEMPS = (1.0, 0.5, 0.25, 0.0)                          # powers of two (and 0): s * inv_temp is exact
# |g - g64| <= TOL * max(1, |g64|).  MEASURED is the largest such ratio found on an MI355X over the pairs of
# test_noise_against_the_restatement (2^20 random pairs, the ends of the range of m, the m nearest u = 1 / e): 1.0141e-07 = 2^-23.23,
# at u = 0.06575, g = -1.0013.  TOL is four times it (the margin covers inputs the sample did not hit): 4.0564e-07 = 2^-21.23.
# CEILING is a condition, not a measurement: see test_the_tolerance_stays_under_its_ceiling.
MEASURED = 1.0141e-07
TOL = 4 * MEASURED
CEILING = 2.0 ** -20
_REF = {}                                                  # expectations and results shared between the two engine settings


@pytest.fixture(autouse=True, params=["f32", "bf16x3"])
def engine(request):
    from newsreclib_amd import _lib
    prev = _lib.get_gemm_engine()
    _lib.set_gemm_engine(request.param)
    yield request.param
    _lib.set_gemm_engine(prev)


def _cuda(t):
    return t.cuda() if t is not None else None


def _keys(B, seed=0):
    """One int64 key per user: small ones, negative ones and ones above 2^32."""
    g = torch.Generator().manual_seed(900 + seed)
    keys = torch.randint(-2 ** 62, 2 ** 62, (B,), generator=g)
    keys[::3] = torch.arange(B)[::3] + 1
    return keys


def _noise(keys, V, seed):
    """(u, g) fp32 (B, V) on the host: the device's noise of every (user, row) pair"""
    from newsreclib_amd import ops
    B = keys.numel()
    u, g = ops.gumbel_noise(keys.cuda().repeat_interleave(V), torch.arange(V).cuda().repeat(B), seed)
    return u.cpu().reshape(B, V), g.cpu().reshape(B, V)


def _sampled(U, T, k, keys, seed, inv_temp, excl=None, eligible=None, slices=0, excl_off=None):
    from newsreclib_amd import ops
    ei = eo = None
    if excl is not None:
        ei, eo = C.ragged(excl)
        ei, eo = ei.cuda(), (excl_off if excl_off is not None else eo).cuda()
    idx, key, score, status = ops.topk_sampled_scores(U.cuda(), T.cuda(), k, keys.cuda(), seed, inv_temp, ei, eo, _cuda(eligible), slices)
    return idx.cpu(), key.cpu(), score.cpu(), int(status)


def _case(B, V, D):
    """Integer vectors, exclusion lists (0 to 9 rows, duplicates allowed), a mixed mask, keys."""
    seed = B * 7 + V + D
    U, T = C.int_vectors(seed, B, V, D)
    g = torch.Generator().manual_seed(seed + 1)
    excl = [torch.randint(0, V, (int(n),), generator=g).tolist() for n in torch.randint(0, 10, (B,), generator=g)]
    excl[-1] = (excl[-1] + [0, 0])[:9]                           # a duplicate for certain
    eligible = (torch.rand(V, generator=g) > 0.15).to(torch.uint8)
    return U, T, excl, eligible, _keys(B, seed)


def _want(key, make):
    if key not in _REF:
        _REF[key] = make()
    return _REF[key]


# ---- 1. the noise -------------------------------------------------------------------------------------------------------------------
# (seed, key, row) whose m is 0, 1, 2^23 - 2, 2^23 - 1 and 3085996 (u nearest 1 / e: -log(u) is nearest 1 and g nearest 0), found by
# a search over keys and rows below 2^14 with the restatement on the host
EDGES = {0: (7, 910, 4279), 1: (7, 184, 448), 2 ** 23 - 2: (7, 916, 14722), 2 ** 23 - 1: (7, 179, 16069), 3085996: (7, 283, 1685)}


def _ratio(g, u):
    g64 = R.gumbel64(u.numpy())
    return np.abs(g.double().numpy() - g64) / np.maximum(1.0, np.abs(g64)), g64


def test_noise_against_the_restatement():
    from newsreclib_amd import ops
    assert TOL == 4 * MEASURED
    assert round((2 ** 24 / math.e - 1) / 2) == 3085996
    n, seed = 1 << 20, 2 ** 40 + 12345
    gen = torch.Generator().manual_seed(77)
    keys = torch.randint(-2 ** 63, 2 ** 63 - 1, (n,), generator=gen)
    keys[: n // 2] = torch.randint(0, 100000, (n // 2,), generator=gen)         # user ids as they come, and all 64 bits
    rows = torch.randint(0, 2 ** 31, (n,), generator=gen)
    rows[: n // 4] = torch.arange(n // 4)
    u, g = ops.gumbel_noise(keys.cuda(), rows.cuda(), seed)
    u, g = u.cpu(), g.cpu()
    assert C.same(u, R.uniform(seed, keys.numpy(), rows.numpy()))
    assert bool(torch.isfinite(g).all())
    ratio, g64 = _ratio(g, u)
    worst, at = float(ratio.max()), int(ratio.argmax())
    print(f"worst of the 2^20 pairs: u = {float(u[at]):.9g}, -log(u) = {-math.log(float(u[at])):.9g}, g = {float(g[at]):.9g}, "
          f"float64 {float(g64[at]):.17g}, ratio {worst:.4e}")
    for m, (s, key, row) in EDGES.items():
        assert int(R.mantissa(s, [key], [row])[0]) == m
        ue, ge = ops.gumbel_noise(torch.tensor([key]).cuda(), torch.tensor([row]).cuda(), s)
        ue, ge = ue.cpu(), ge.cpu()
        assert C.same(ue, R.uniform(s, [key], [row])) and float(ue) == (2 * m + 1) * 2.0 ** -24
        assert math.isfinite(float(ge))
        r, ge64 = _ratio(ge, ue)
        print(f"m = {m}: u = {float(ue):.9g}, g = {float(ge):.9g}, float64 {float(ge64[0]):.17g}, ratio {float(r[0]):.3e}")
        worst = max(worst, float(r[0]))
    print(f"largest |g - g64| / max(1, |g64|) = {worst:.4e} (2^{math.log2(worst):.2f}); MEASURED = {MEASURED:.4e}, TOL = {TOL:.4e}; "
          f"mean u = {float(u.double().mean()):.5f}, mean g = {float(g.double().mean()):.5f}, g in [{float(g.min()):.4f}, {float(g.max()):.4f}]")
    assert worst <= TOL
    assert abs(float(u.double().mean()) - 0.5) < 2e-3 and abs(float(g.double().mean()) - 0.5772) < 5e-3
    # one output alone, and no pairs
    only_g = ops.gumbel_noise(keys[:100].cuda(), rows[:100].cuda(), seed)[1]
    assert C.same(only_g, g[:100])
    none = torch.zeros(0, dtype=torch.int64).cuda()
    assert ops.gumbel_noise(none, none, 3)[0].shape == (0,)


def test_the_tolerance_stays_under_its_ceiling():
    """TOL may not exceed 2^-20 = 9.5367e-07: a larger value means the wrong log is in use.  Two logs each within half an ulp give
    about 2^-23 max(1, |g|) (an error of e1 ulp of -log(u) and e2 ulp of g arrives as (e1 + e2) 2^-23 at g just above 1), which is
    what is measured.  The library's ``logf`` (up to 2 ulp) measured 2.5812e-07 = 2^-21.89 here, four times which is above the
    ceiling: that is why the kernels evaluate each log in float64 and round it to fp32."""
    print(f"MEASURED = {MEASURED:.4e} (2^{math.log2(MEASURED):.2f}), TOL = {TOL:.4e} (2^{math.log2(TOL):.2f}), ceiling {CEILING:.4e}")
    assert TOL <= CEILING


# ---- 2. bit equality on exact scores ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,V,D", SHAPES)
def test_exact_with_ties(B, V, D):
    U, T, excl, eligible, keys = _case(B, V, D)
    s = U.double() @ T.double().T
    seed = 1000 + B
    u32, g32 = _want(("noise", B, V, D), lambda: _noise(keys, V, seed))
    assert C.same(u32, R.uniform(seed, keys.numpy()[:, None], np.arange(V)[None, :]))
    for inv_temp in INV_TEMPS:
        for masks in ((None, None), (excl, eligible)):
            for k in (1, 10, 128):
                want = _want(("topk", B, V, D, inv_temp, masks[0] is None, k), lambda: R.expected(s, g32, inv_temp, k, *masks))
                idx, key, score, status = _sampled(U, T, k, keys, seed, inv_temp, *masks)
                assert status == 0 and C.same((idx, key, score), want), (inv_temp, k, masks[0] is None)
    # k above the population: the tail is -1 / -inf / -inf
    idx, key, score, _ = _sampled(U, T, 128, keys, seed, 1.0, excl, eligible)
    pop = C.population(s, excl, eligible)[0].sum(1)
    assert bool(((idx >= 0).sum(1) == pop.clamp(max=128)).all())
    assert bool((key[idx < 0] == NEG_INF).all()) and bool((score[idx < 0] == NEG_INF).all())


def test_slice_counts():
    """(130, 1000, 300) has 8 table tiles and 3 user tiles: every slice count gives the reference."""
    B, V, D = 130, 1000, 300
    U, T, excl, eligible, keys = _case(B, V, D)
    s = U.double() @ T.double().T
    seed = 1000 + B
    g32 = _want(("noise", B, V, D), lambda: _noise(keys, V, seed))[1]
    for k, inv_temp in ((10, 0.5), (128, 1.0)):
        want = _want(("topk", B, V, D, inv_temp, False, k), lambda: R.expected(s, g32, inv_temp, k, excl, eligible))
        for slices in (0, 1, 2, 7, 8, 100):
            idx, key, score, status = _sampled(U, T, k, keys, seed, inv_temp, excl, eligible, slices)
            assert status == 0 and C.same((idx, key, score), want), (k, slices)


def test_bad_exclusion_indices_and_offsets_raise_the_plain_entrys_flags():
    B, V, D, k = 3, 300, 12, 10
    U, T = C.int_vectors(29, B, V, D)
    keys, seed = _keys(B), 5
    s = U.double() @ T.double().T
    g32 = _noise(keys, V, seed)[1]
    excl = [[40, V + 3, -2, 40], [], [100, 101]]
    idx, key, score, status = _sampled(U, T, k, keys, seed, 0.5, excl)
    assert status == E_EXCLUDE and C.same((idx, key, score), R.expected(s, g32, 0.5, k, excl))
    # user 1's offsets run backwards: flat [64, 65, 66, 67], offsets [0, 3, 2, 4] -> user 0 [64, 65, 66], user 2 [66, 67]
    flat, off = [[64, 65, 66, 67], [], []], torch.tensor([0, 3, 2, 4])
    want = R.expected(s, g32, 0.5, k, [[64, 65, 66], [], [66, 67]])
    idx, key, score, status = _sampled(U, T, k, keys, seed, 0.5, flat, excl_off=off)
    assert status == E_OFFSETS and bool((idx[1] == -1).all()) and bool((key[1] == NEG_INF).all()) and bool((score[1] == NEG_INF).all())
    assert C.same((idx[[0, 2]], key[[0, 2]], score[[0, 2]]), tuple(w[[0, 2]] for w in want))


def test_a_nan_score_is_dropped_and_flagged():
    B, V, D, k = 4, 300, 12, 16
    U, T = C.int_vectors(23, B, V, D)
    keys, seed = _keys(B), 9
    g32 = _noise(keys, V, seed)[1]
    T[200, 3] = float("nan")                                     # row 200 scores NaN for every user
    s = U.double() @ T.double().T
    eligible = torch.ones(V, dtype=torch.uint8)
    eligible[200] = 0
    idx, key, score, status = _sampled(U, T, k, keys, seed, 1.0, None, eligible)
    assert status == 0 and C.same((idx, key, score), R.expected(s, g32, 1.0, k, None, eligible))
    idx, key, score, status = _sampled(U, T, k, keys, seed, 1.0)
    assert status == E_NAN and not bool((idx == 200).any()) and C.same((idx, key, score), R.expected(s, g32, 1.0, k))
    idx, key, score, status = _sampled(U, T, 128, keys, seed, 0.0)
    assert status == E_NAN and not bool((idx == 200).any())      # NaN * 0 is NaN: dropped under inv_temp = 0 as well


def test_no_rows_and_no_users():
    U, T = C.int_vectors(3, 4, 8, 12)
    keys = _keys(4)
    idx, key, score, status = _sampled(U, T[:0], 3, keys, 1, 1.0)
    assert status == 0 and idx.shape == (4, 3) and bool((idx == -1).all())
    assert bool((key == NEG_INF).all()) and bool((score == NEG_INF).all())
    idx, key, score, status = _sampled(U[:0], T, 3, keys[:0], 1, 1.0)
    assert status == 0 and idx.shape == (0, 3) and key.shape == (0, 3) and score.shape == (0, 3)


# ---- 3. the raw scores ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,V,D,k", [(70, 700, 36, 10), (70, 128, 36, 128), (5, 100, 1024, 7)])
def test_raw_scores_are_the_plain_entrys_bits_and_the_key_is_two_roundings(B, V, D, k):
    """Real-valued vectors.  ``score`` of every returned slot has the bits ``ops.topk_scores(k = min(V, 128))`` reports for that
    (user, row) -- looked up where the row is in that list; with V <= 128 it always is -- and ``key`` is
    ``fl(fl(score * inv_temp) + g32)`` computed on the CPU from the returned score."""
    from newsreclib_amd import ops
    g = torch.Generator().manual_seed(40 + V)
    U, T = torch.randn(B, D, generator=g), torch.randn(V, D, generator=g)
    keys, seed, inv_temp = _keys(B, V), 2 ** 63 + 11, 0.7
    g32 = _noise(keys, V, seed)[1]
    pidx, pscore, pstatus = ops.topk_scores(U.cuda(), T.cuda(), min(V, 128))
    pidx, pscore = pidx.cpu(), pscore.cpu()
    plain = torch.full((B, V), float("nan"))
    plain.scatter_(1, pidx, pscore)                              # (every slot of the plain list is a row: nothing is masked)
    idx, key, score, status = _sampled(U, T, k, keys, seed, inv_temp)
    assert status == 0 and int(pstatus) == 0 and bool((idx >= 0).all())
    want = plain.gather(1, idx)
    known = ~torch.isnan(want)
    assert bool(known.all()) if V <= 128 else int(known.sum()) > B
    assert C.same(score[known], want[known])
    z = (score * torch.tensor(inv_temp, dtype=torch.float32)) + g32.gather(1, idx) + 0.0
    assert C.same(key, z)


# ---- 4. the order on real-valued scores -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("inv_temp", [1.0, 0.3])
def test_real_valued_order_within_the_derived_bound(inv_temp):
    """``check_floor`` with raw = s64 * inv_temp + g32 and bound = dot_bound * inv_temp + 2^-23 (|s64 * inv_temp| + |raw|): the
    product's worst case, then the two roundings (half an ulp each would do; a whole one is claimed)."""
    B, V, D, k = 70, 700, 36, 10
    g = torch.Generator().manual_seed(61)
    U, T = torch.randn(B, D, generator=g), torch.randn(V, D, generator=g)
    excl = [torch.randint(0, V, (int(n),), generator=g).tolist() for n in torch.randint(0, 10, (B,), generator=g)]
    eligible = (torch.rand(V, generator=g) > 0.15).to(torch.uint8)
    keys, seed = _keys(B, 4), 31337
    g32 = _want(("noise-real",), lambda: _noise(keys, V, seed))[1]
    s64 = U.double() @ T.double().T
    raw = s64 * float(np.float32(inv_temp)) + g32.double()
    bound = C.dot_bound(U, T) * inv_temp + 2.0 ** -23 * ((s64 * inv_temp).abs() + raw.abs())
    idx, key, score, status = _sampled(U, T, k, keys, seed, inv_temp, excl, eligible)
    assert status == 0
    C.check_floor(idx, key, raw, bound, C.population(raw, excl, eligible)[0], k)


# ---- 5. independence ------------------------------------------------------------------------------------------------------------------
def test_a_users_lists_do_not_depend_on_the_batch_the_slicing_the_engine_or_the_run(engine):
    B, V, D, k = 70, 700, 36, 10
    g = torch.Generator().manual_seed(71)
    U, T = torch.randn(B, D, generator=g), torch.randn(V, D, generator=g)
    excl = [torch.randint(0, V, (int(n),), generator=g).tolist() for n in torch.randint(0, 10, (B,), generator=g)]
    eligible = (torch.rand(V, generator=g) > 0.15).to(torch.uint8)
    keys, seed, inv_temp = _keys(B, 5), 424242, 0.8

    def run(users, slices=0):
        users = list(users)
        got = _sampled(U[users], T, k, keys[users], seed, inv_temp, [excl[b] for b in users], eligible, slices)
        assert got[3] == 0
        return got[:3]

    base = run(range(B))
    assert C.same(base, _want(("independence",), lambda: base))                   # the other engine setting gave these bits
    assert C.same(run(range(B)), base)                                           # two calls in a row
    rev = run(reversed(range(B)))
    assert C.same(tuple(t.flip(0) for t in rev), base)
    first, rest = run([0]), run(range(1, B))
    assert C.same(tuple(torch.cat([a, b]) for a, b in zip(first, rest)), base)
    for b in (1, 33, 63, 64, 69):                                                # alone: one user, one workgroup per slice
        assert C.same(run([b]), tuple(t[b:b + 1] for t in base)), b
    for slices in (1, 7):
        assert C.same(run(range(B), slices), base), slices


def test_another_seed_or_another_key_is_another_draw():
    """On exact scores the expectation under the other seed / key is exact as well: the device returns it, and it is not the first
    draw's."""
    B, V, D, k = 5, 200, 8, 10
    U, T = C.int_vectors(83, B, V, D)
    s = U.double() @ T.double().T
    keys = _keys(B, 6)
    other_keys = keys.clone()
    other_keys[2] += 1
    wants = []
    for ks, seed in ((keys, 1), (keys, 2), (other_keys, 1), (keys, 1 + 2 ** 32)):
        g32 = _noise(ks, V, seed)[1]
        want = R.expected(s, g32, 1.0, k)
        idx, key, score, status = _sampled(U, T, k, ks, seed, 1.0)
        assert status == 0 and C.same((idx, key, score), want)
        wants.append(want[0])
    assert not torch.equal(wants[0], wants[1]) and not torch.equal(wants[0], wants[3])          # the seed, either half of it
    assert not torch.equal(wants[0][2], wants[2][2])                                            # the key: that user's list
    assert torch.equal(wants[0][[0, 1, 3, 4]], wants[2][[0, 1, 3, 4]])                          # ... and nobody else's


# ---- 6. the distribution --------------------------------------------------------------------------------------------------------------
def test_the_draws_follow_plackett_luce(engine):
    """4096 users with the same scores and keys 1000 ... 5095, one call per (seed, inv_temp): Pearson's chi-square of the first-slot
    counts against softmax(s * inv_temp) and of the second-slot counts against the Plackett-Luce marginal, each below the upper
    1e-6 quantile of chi-square with 7 degrees of freedom (40.52: derived, not tuned; the float64 restatement gives 3.2 - 16.3 and
    1.8 - 12.8 over these ten cases).  inv_temp = 0: the first slot against the uniform distribution."""
    if engine != "f32":
        return                                                   # (the unit does not read the engine setting: once is enough)
    B = 4096
    s = [2, 1, 0, -1, 0.5, 1.5, -0.5, 0]
    U = torch.zeros(B, 4)
    U[:, 0] = 1
    T = torch.zeros(8, 4)
    T[:, 0] = torch.tensor(s)
    keys = torch.arange(1000, 1000 + B)
    for inv_temp in (1.0, 0.5, 0.0):
        p1, p2 = R.pl_marginals(s, inv_temp)
        for seed in (1, 2, 3, 12345, 2 ** 40 + 7):
            idx, key, score, status = _sampled(U, T, 2, keys, seed, inv_temp)
            assert status == 0 and bool((idx >= 0).all()) and bool((idx[:, 0] != idx[:, 1]).all())
            assert C.same(score, T[:, 0][idx])
            c1 = R.chi2(np.bincount(idx[:, 0].numpy(), minlength=8), p1)
            c2 = R.chi2(np.bincount(idx[:, 1].numpy(), minlength=8), p2)
            print(f"inv_temp {inv_temp}, seed {seed}: chi-square first slot {c1:.2f}, second slot {c2:.2f}")
            assert c1 < R.CHI2_7_1E6, (inv_temp, seed, c1)
            if inv_temp > 0:
                assert c2 < R.CHI2_7_1E6, (inv_temp, seed, c2)


# ---- 7. no read-back ------------------------------------------------------------------------------------------------------------------
def test_the_sampled_entries_do_not_synchronise_with_the_host():
    from newsreclib_amd import ops
    U, T = C.int_vectors(3, 5, 200, 12)
    U, T = U.cuda(), T.cuda()
    ei, eo = C.ragged([[1], [], [5, 6], [], []])
    ei, eo, elig, keys = ei.cuda(), eo.cuda(), torch.ones(200, dtype=torch.uint8).cuda(), _keys(5).cuda()
    rows = torch.arange(5).cuda()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        if not C.sync_debug_honoured():
            pytest.skip("this torch build does not raise on synchronising calls under set_sync_debug_mode('error')")
        idx, key, score, status = ops.topk_sampled_scores(U, T, 4, keys, 3, 0.5, ei, eo, elig)
        u, g = ops.gumbel_noise(keys, rows, 3)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert int(status) == 0 and idx.shape == (5, 4) and key.shape == (5, 4) and score.shape == (5, 4) and u.shape == (5,)


# ---- 8. through the cache -------------------------------------------------------------------------------------------------------------
def _cache_case(late_fusion=False):
    from newsreclib_amd.evaluation import DeviceNewsTable, NewsVectorCache
    mod, attrs = builders.tiny("nrms", late_fusion=late_fusion)
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


def test_cache_recommend_with_a_sample():
    from newsreclib_amd import ops
    mod, cache, lists, hist, hs, uidx = _cache_case()
    V, B, k = 50, 6, 8
    eligible = torch.ones(V, dtype=torch.uint8)
    eligible[0] = 0
    keys = torch.tensor([7, 1, 2 ** 40, -3, 5, 6])
    user, vec, hist_off = _users_by_hand(mod, cache, hist, hs, uidx)
    want = ops.topk_sampled_scores(user, vec, k, keys.cuda(), 99, 0.5, hist.cuda(), hist_off, eligible.cuda())
    for key_tensor in (keys, keys.cuda()):                       # host keys (through pinned memory) and device keys
        got = cache.recommend(hist.cuda(), hs, k, user_idx=uidx, eligible=eligible, sample=(0.5, 99, key_tensor))
        assert len(got) == 3 and int(got[2]) == 0 and C.same(got[:2], (want[0], want[2]))
    # the listed scores are the raw scores: the plain call's for the same (user, row)
    plain = cache.recommend(hist.cuda(), hs, V, user_idx=uidx, eligible=eligible)
    table = torch.full((B, V), float("nan"))
    rows = plain[0].cpu()
    table.scatter_(1, rows.clamp(min=0), torch.where(rows >= 0, plain[1].cpu(), torch.full((), float("nan"))))
    idx, score = got[0].cpu(), got[1].cpu()
    assert bool((idx >= 0).all()) and C.same(score, table.gather(1, idx))
    # sample=None is the call without the argument
    assert C.same(cache.recommend(hist.cuda(), hs, k, user_idx=uidx, eligible=eligible, sample=None)[:2],
                  cache.recommend(hist.cuda(), hs, k, user_idx=uidx, eligible=eligible)[:2])
    assert C.same(cache.recommend(hist.cuda(), hs, k, user_idx=uidx, eligible=eligible)[:2],
                  ops.topk_scores(user, vec, k, hist.cuda(), hist_off, eligible.cuda())[:2])


def test_recommend_users_does_not_depend_on_the_batch_size_and_sample_recommendations_stacks_its_draws():
    """A late-fusion NRMS module (the user vector is the mean of the user's own history vectors: no user sees another user of the
    batch, unlike NRMS' seq-first user attention) under batch sizes 2 and 512: the same dictionary.  ``sample_recommendations``'
    draw j is ``recommend_users`` under ``seed + j``."""
    import warnings

    from newsreclib_amd.evaluation import recommend_users, sample_recommendations
    mod, cache, lists, hist, hs, uidx = _cache_case(late_fusion=True)
    k = 5
    eligible = torch.ones(50, dtype=torch.uint8)
    eligible[0] = 0
    ids = [11, 3, 2 ** 35, 8, 1, 20]
    users = [{"hist": lists[b], "user_idx": uidx[b], "user_id": ids[b]} for b in range(6)]
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        small = recommend_users(cache, users, k, batch_size=2, eligible=eligible, sample=(2.0, 17))
        large = recommend_users(cache, users, k, batch_size=512, eligible=eligible, sample=(2.0, 17))
        assert small == large and [list(small[u]) for u in small] == [list(large[u]) for u in large]
        assert sorted(small) == sorted("U" + str(i) for i in ids) and all(len(v) == k for v in small.values())
        moved = recommend_users(cache, users[::-1], k, batch_size=4, eligible=eligible, sample=(2.0, 17))
        assert moved == small
        assert recommend_users(cache, users, k, eligible=eligible, sample=None) == recommend_users(cache, users, k, eligible=eligible)
        draws = sample_recommendations(cache, users, k, 3, 2.0, 16, batch_size=4, eligible=eligible)
        assert draws.shape == (6, 3, k) and draws.dtype == torch.int64 and not draws.is_cuda
        for j in range(3):
            listed = recommend_users(cache, users, k, batch_size=512, eligible=eligible, sample=(2.0, 16 + j))
            for b, uid in enumerate(ids):
                assert ["N" + str(r) for r in draws[b, j].tolist()] == list(listed["U" + str(uid)]), (b, j)
        assert torch.equal(draws[:, 1], torch.tensor([[int(n[1:]) for n in small["U" + str(uid)]] for uid in ids]))
    # a user without an id is keyed by its position + 1
    anon = [{k_: v for k_, v in u.items() if k_ != "user_id"} for u in users]
    named = [dict(u, user_id=b + 1) for b, u in enumerate(anon)]
    assert recommend_users(cache, anon, k, batch_size=4, sample=(1.0, 3)) == recommend_users(cache, named, k, batch_size=3, sample=(1.0, 3))


def test_cache_refusals():
    from newsreclib_amd import evaluation as E
    mod, cache, lists, hist, hs, uidx = _cache_case()
    keys = torch.arange(6)
    lo = torch.zeros(6, dtype=torch.int32)
    with pytest.raises(NotImplementedError, match="tks_scores_kernel"):
        cache.recommend(hist.cuda(), hs, 4, user_idx=uidx, sample=(1.0, 1, keys), window=(lo, lo))
    with pytest.raises(TypeError, match="int64"):
        cache.recommend(hist.cuda(), hs, 4, user_idx=uidx, sample=(1.0, 1, keys.int()))
    with pytest.raises(ValueError, match="one entry per user"):
        cache.recommend(hist.cuda(), hs, 4, user_idx=uidx, sample=(1.0, 1, keys[:5]))
    users = [{"hist": lists[b], "user_idx": uidx[b], "time": 5} for b in range(6)]
    with pytest.raises(NotImplementedError, match="TkSelectCapped"):
        E.recommend_users(cache, users, 4, sample=(1.0, 1), cap=("category", 1))
    with pytest.raises(NotImplementedError, match="tkw_walk"):
        E.recommend_users(cache, users, 4, sample=(1.0, 1), window=(2, 0))
    for other in (dict(diversify=(5, 0.5)), dict(calibrate=dict(pool=5, aspect="category", gamma=0.5)), dict(dpp=dict(pool=5))):
        with pytest.raises(ValueError, match="`sample` excludes"):
            E.recommend_users(cache, users, 4, sample=(1.0, 1), **other)
    with pytest.raises(ValueError, match="temperature must be finite and > 0"):
        E.recommend_users(cache, users, 4, sample=(0.0, 1))
    from newsreclib_amd.dkn_module import DKNModule
    from newsreclib_amd.miner_module import MINERModule
    from newsreclib_amd.npa_module import NPAModule
    from newsreclib_amd.senti_debias_module import SentiDebiasModule
    for cls in (MINERModule, DKNModule, NPAModule, SentiDebiasModule):
        other = E.NewsVectorCache(object.__new__(cls), cache.table)
        with pytest.raises(NotImplementedError, match="tks_scores_kernel"):
            E.recommend_users(other, users, 4, sample=(1.0, 1))
        with pytest.raises(NotImplementedError, match="tks_scores_kernel"):
            E.sample_recommendations(other, users, 4, 2, 1.0, 1)
    with pytest.raises(NotImplementedError, match="MannerVectorCache"):
        E.recommend_users(object.__new__(E.MannerVectorCache), users, 4, sample=(1.0, 1))
