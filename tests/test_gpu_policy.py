"""The log-partition and the list propensities of the sampled policy on the GPU (``nrl_catalogue_logz`` / ``nrl_list_logprob``, their
``ops`` wrappers, ``NewsVectorCache.policy_stats`` / ``list_log_probs``, ``sample_recommendations(log_probs=True)`` and
``policy_report``).

The inputs are ``catalogue_ref.int_vectors`` -- every score is exact in fp32 -- under ``inv_temp`` in {1, 2^-4, 2^-8, 0}, so the scaled
score ``t`` is exact as well and the float64 restatement in ``tests/policy_ref.py`` sees the device's policy.  What is an integer or
one score's bits is compared bit for bit; ``logsum`` and ``entropy`` against float64 within a measured tolerance that is held under a
derived ceiling; the list log-probabilities within a tolerance derived from that one."""
import math

import numpy as np
import pytest
import torch

from tests import builders
from tests import catalogue_ref as C
from tests import policy_ref as P
from tests import topk_sampled_ref as R

pytestmark = pytest.mark.gpu

E_EXCLUDE, E_OFFSETS, E_NAN, E_LIST, E_INF = 1, 2, 4, 128, 256
NEG_INF = float("-inf")
SHAPES = [(1, 1, 4), (3, 130, 20), (63, 127, 4), (64, 128, 4), (65, 129, 4), (65, 8320, 20), (5, 128, 1024)]
INV_TEMPS = (1.0, 2.0 ** -4, 2.0 ** -8, 0.0)                # powers of two (and 0): s * inv_temp is exact
STAT_CHUNKS, TILE = 64, 128
# |device - float64| <= TOL.  MEASURED is the largest error found on an MI355X over test_logsum_and_entropy_against_float64 (all
# SHAPES, all INV_TEMPS, with and without masks) with the fast exponential the kernel uses: logsum 5.0973e-07 = 2^-20.90 and entropy
# 4.7395e-07 = 2^-21.01, both at (65, 8320, 20), inv_temp 2^-8, where the values are 8.5 - 9.0 and half an ulp of the fp32 output
# alone is 2^-21 = 4.7684e-07.  The library's expf in the same kernel measured 4.7804e-07 and 4.7972e-07: the output's own rounding
# dominates both variants, so the cheaper one stays.  TOL is four times MEASURED (the margin covers inputs the sample did not hit).
# The ceilings are a condition, not a measurement: see test_the_tolerances_stay_under_their_ceilings.
MEASURED = {"logsum": 5.0973e-07, "entropy": 4.7395e-07}
TOL = {k: 4 * v for k, v in MEASURED.items()}
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


def _want(key, make):
    if key not in _REF:
        _REF[key] = make()
    return _REF[key]


def _logz(U, T, inv_temp, excl=None, eligible=None, drop=None, excl_off=None):
    """-> (max, logsum, entropy, pop, dropped) on the host, the status word"""
    from newsreclib_amd import ops
    ei = eo = None
    if excl is not None:
        ei, eo = C.ragged(excl)
        ei, eo = ei.cuda(), (excl_off if excl_off is not None else eo).cuda()
    out = ops.catalogue_logz(U.cuda(), T.cuda(), inv_temp, ei, eo, _cuda(eligible), _cuda(drop))
    return tuple(t.cpu() for t in out[:5]), int(out[5])


def _logp(U, T, lists, inv_temp, excl=None, eligible=None):
    """-> (logp, total, score) on the host, the status word"""
    from newsreclib_amd import ops
    ei = eo = None
    if excl is not None:
        ei, eo = C.ragged(excl)
        ei, eo = ei.cuda(), eo.cuda()
    out = ops.list_logprob(U.cuda(), T.cuda(), lists.cuda(), inv_temp, ei, eo, _cuda(eligible))
    return tuple(t.cpu() for t in out[:3]), int(out[3])


def _case(B, V, D):
    """Integer vectors, exclusion lists (0 to 9 rows, duplicates allowed), a mixed mask."""
    seed = B * 7 + V + D
    U, T = C.int_vectors(seed, B, V, D)
    g = torch.Generator().manual_seed(seed + 1)
    excl = [torch.randint(0, V, (int(n),), generator=g).tolist() for n in torch.randint(0, 10, (B,), generator=g)]
    excl[-1] = (excl[-1] + [0, 0])[:9]                           # a duplicate for certain
    eligible = (torch.rand(V, generator=g) > 0.15).to(torch.uint8)
    if V == 1:
        excl, eligible = [[]], torch.ones(1, dtype=torch.uint8)   # (one row, and it is there)
    return U, T, excl, eligible


def _stats(s, pop, inv_temp):
    """the float64 statistics of every user -> (max float32 (B), logsum, entropy float64 (B), n int32 (B))"""
    rows = [P.stats(s[b].numpy(), inv_temp, pop[b].numpy()) for b in range(s.shape[0])]
    return (torch.tensor([r[0] for r in rows], dtype=torch.float64).float() + 0.0, torch.tensor([r[1] for r in rows], dtype=torch.float64),
            torch.tensor([r[2] for r in rows], dtype=torch.float64), torch.tensor([r[3] for r in rows], dtype=torch.int32))


def _err(got, want):
    """max |got - want| over the finite expectations; where the expectation is -inf the device must say -inf"""
    fin = torch.isfinite(want)
    assert torch.equal(got[~fin].double(), want[~fin])
    return float((got[fin].double() - want[fin]).abs().max()) if bool(fin.any()) else 0.0


def _chunks(V):
    nvt = -(-V // TILE)
    tpc = -(-nvt // STAT_CHUNKS)
    return tpc, -(-nvt // tpc)


# ---- 1. the exact parts ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,V,D", SHAPES)
def test_population_and_maximum_are_exact(B, V, D):
    from newsreclib_amd import ops
    U, T, excl, eligible = _case(B, V, D)
    s = U.double() @ T.double().T
    for masks in ((None, None), (excl, eligible)):
        pop = C.population(s, *masks)[0]
        for inv_temp in INV_TEMPS:
            want = _want(("stats", B, V, D, inv_temp, masks[0] is None), lambda: _stats(s, pop, inv_temp))
            (mx, ls, ent, n, dropped), status = _logz(U, T, inv_temp, *masks)
            assert status == 0 and C.same(n, want[3]) and C.same(mx, want[0]), (inv_temp, masks[0] is None)
            assert not bool(dropped.any())
            assert bool((ls[n > 0] >= 0).all()) and bool((ls[n > 0].double() <= torch.log(n[n > 0].double()) + TOL["logsum"]).all())
        ei, eo = (t.cuda() for t in C.ragged(masks[0])) if masks[0] is not None else (None, None)
        top = ops.topk_scores(U.cuda(), T.cuda(), 1, ei, eo, _cuda(masks[1]))[1].cpu()[:, 0]
        assert C.same(_logz(U, T, 1.0, *masks)[0][0], top)              # the best row's score, bit for bit


def test_masks_flags_and_edge_populations():
    """Six users over 300 rows: 65 exclusions (beyond the cached 64), everything excluded, all but one row excluded, an exclusion
    index outside the table, and two plain ones; then bad offsets, a NaN row, a +inf and a -inf row."""
    B, V, D = 6, 300, 12
    U, T = C.int_vectors(41, B, V, D)
    U[:, 5] = 1.0                                                # (no zero there: an infinite table entry gives +-inf, not NaN)
    s = U.double() @ T.double().T
    g = torch.Generator().manual_seed(5)
    excl = [torch.randperm(V, generator=g)[:65].tolist(), list(range(V)), [v for v in range(V) if v != 77], [3, V + 2, -1, 3], [], [9]]
    pop = C.population(s, excl)[0]
    assert pop.sum(1).tolist() == [V - 65, 0, 1, V - 1, V, V - 1]
    for inv_temp in (1.0, 2.0 ** -4):
        want = _stats(s, pop, inv_temp)
        (mx, ls, ent, n, _), status = _logz(U, T, inv_temp, excl)
        assert status == E_EXCLUDE and C.same(n, want[3]) and C.same(mx, want[0])
        assert _err(ls, want[1]) <= TOL["logsum"] and _err(ent, want[2]) <= TOL["entropy"]
        # the empty population, and the single row: logsum is +0 exactly, the entropy 0
        assert mx[1] == NEG_INF and ls[1] == NEG_INF and C.same(ent[1:2], torch.zeros(1)) and int(n[1]) == 0
        assert C.same(ls[2:3], torch.zeros(1)) and C.same(ent[2:3], torch.zeros(1)) and float(mx[2]) == float(s[2, 77]) * inv_temp
    # user 1's offsets run backwards: flat [64, 65, 66, 67], offsets [0, 3, 2, 4, 4, 4, 4] -> user 0 [64, 65, 66], user 2 [66, 67]
    flat, off = [[64, 65, 66, 67]] + [[]] * 5, torch.tensor([0, 3, 2, 4, 4, 4, 4])
    seen = [[64, 65, 66], [], [66, 67], [], [], []]
    want = _stats(s, C.population(s, seen)[0], 1.0)
    (mx, ls, ent, n, _), status = _logz(U, T, 1.0, flat, excl_off=off)
    assert status == E_OFFSETS and mx[1] == NEG_INF and ls[1] == NEG_INF and float(ent[1]) == 0 and int(n[1]) == 0
    keep = [0, 2, 3, 4, 5]
    assert C.same(n[keep], want[3][keep]) and C.same(mx[keep], want[0][keep]) and _err(ls[keep], want[1][keep]) <= TOL["logsum"]
    # a NaN row: flagged, left out; masked: no flag
    Tn = T.clone()
    Tn[200, 3] = float("nan")
    sn = U.double() @ Tn.double().T
    popn = C.population(sn)[0]
    want = _stats(sn, popn, 1.0)
    (mx, ls, ent, n, _), status = _logz(U, Tn, 1.0)
    assert status == E_NAN and bool((n == V - 1).all()) and C.same(mx, want[0]) and _err(ls, want[1]) <= TOL["logsum"]
    eligible = torch.ones(V, dtype=torch.uint8)
    eligible[200] = 0
    assert _logz(U, Tn, 1.0, None, eligible)[1] == 0
    assert _logz(U, Tn, 0.0)[1] == E_NAN                         # NaN * 0 is NaN
    # a +inf and a -inf row: flagged with the new bit, left out, the population two smaller
    Ti = T.clone()
    Ti[10, 5], Ti[20, 5] = float("inf"), float("-inf")
    si = U.double() @ Ti.double().T
    assert bool((si[:, 10] == float("inf")).all()) and bool((si[:, 20] == NEG_INF).all())
    popi = torch.isfinite(si)
    for inv_temp in (1.0, 2.0 ** -4):
        want = _stats(torch.where(popi, si, torch.zeros_like(si)), popi, inv_temp)
        (mx, ls, ent, n, _), status = _logz(U, Ti, inv_temp)
        assert status == E_INF and bool((n == V - 2).all()) and C.same(mx, want[0])
        assert _err(ls, want[1]) <= TOL["logsum"] and _err(ent, want[2]) <= TOL["entropy"]
    assert _logz(U, Ti, 0.0)[1] == E_NAN                         # inf * 0 is NaN: the older flag


def test_no_rows_and_no_users():
    U, T = C.int_vectors(3, 4, 8, 12)
    (mx, ls, ent, n, dropped), status = _logz(U, T[:0], 1.0)
    assert status == 0 and bool((mx == NEG_INF).all()) and bool((ls == NEG_INF).all()) and not bool(ent.any()) and not bool(n.any())
    (mx, ls, ent, n, dropped), status = _logz(U[:0], T, 1.0)
    assert status == 0 and mx.shape == (0,) and n.shape == (0,)
    (logp, total, score), status = _logp(U[:0], T, torch.zeros(0, 3, dtype=torch.int64), 1.0)
    assert status == 0 and logp.shape == (0, 3) and total.shape == (0,) and score.shape == (0, 3)


# ---- 2. logsum and entropy against float64 --------------------------------------------------------------------------------------------
def test_logsum_and_entropy_against_float64():
    worst = {"logsum": (0.0, None), "entropy": (0.0, None)}
    for B, V, D in SHAPES:
        U, T, excl, eligible = _case(B, V, D)
        s = U.double() @ T.double().T
        for masks in ((None, None), (excl, eligible)):
            pop = C.population(s, *masks)[0]
            for inv_temp in INV_TEMPS:
                want = _want(("stats", B, V, D, inv_temp, masks[0] is None), lambda: _stats(s, pop, inv_temp))
                (mx, ls, ent, n, _), status = _logz(U, T, inv_temp, *masks)
                assert status == 0
                for name, got, ref in (("logsum", ls, want[1]), ("entropy", ent, want[2])):
                    e = _err(got, ref)
                    if e > worst[name][0]:
                        worst[name] = (e, (B, V, D, inv_temp, masks[0] is None))
                if inv_temp == 0.0:                              # the uniform policy: both are log(pop)
                    some = n > 0
                    logn = torch.log(n[some].double())
                    assert float((ls[some].double() - logn).abs().max()) <= TOL["logsum"]
                    assert float((ent[some].double() - logn).abs().max()) <= TOL["entropy"]
    for name, (e, at) in worst.items():
        print(f"largest |{name} - float64| = {e:.4e} (2^{math.log2(e) if e else float('-inf'):.2f}) at (B, V, D, inv_temp, unmasked) = {at}; "
              f"MEASURED = {MEASURED[name]:.4e}, TOL = {TOL[name]:.4e}")
    for name, (e, at) in worst.items():
        assert e <= TOL[name], (name, e, at)


def test_the_tolerances_stay_under_their_ceilings():
    """``TOL <= CEILING(V)`` for every V of SHAPES: ``8 (tiles_per_chunk + 6 + chunks) 2^-24`` for logsum -- eight roundings of at most
    one ulp per fold along the longest chain (the lane's chain over the tiles of a chunk, six butterfly levels, the chain over the
    chunks) -- and that times ``max(1, log n)`` for the entropy.  A tolerance above it would mean that something accumulates in
    a lower precision; it says nothing about the choice of exp."""
    assert TOL == {k: 4 * v for k, v in MEASURED.items()}
    for B, V, D in SHAPES:
        tpc, chunks = _chunks(V)
        ceiling = 8 * (tpc + 6 + chunks) * 2.0 ** -24
        print(f"V = {V}: {tpc} tiles per chunk, {chunks} chunks, ceiling {ceiling:.4e} (entropy {ceiling * max(1.0, math.log(V)):.4e}); "
              f"TOL {TOL['logsum']:.4e} / {TOL['entropy']:.4e}")
        assert TOL["logsum"] <= ceiling
        assert TOL["entropy"] <= ceiling * max(1.0, math.log(V))
    assert _chunks(8320) == (2, 33) and _chunks(65536) == (8, 64) and _chunks(1) == (1, 1)


# ---- 3. invariance --------------------------------------------------------------------------------------------------------------------
def test_a_users_outputs_do_not_depend_on_the_batch_the_mask_form_or_the_engine(engine):
    """(65, 8320, 20): 33 chunks of two tiles.  One user alone and at positions 0, 63 and 64 of a batch of 65; ``eligible=None``
    against all ones; the other engine setting."""
    B, V, D = 65, 8320, 20
    g = torch.Generator().manual_seed(17)
    U, T = torch.randn(B, D, generator=g), torch.randn(V, D, generator=g)
    excl = [torch.randint(0, V, (int(n),), generator=g).tolist() for n in torch.randint(0, 10, (B,), generator=g)]
    drop = torch.randint(0, V, (B, 5), generator=g)
    for b in (0, 63, 64):
        U[b], excl[b], drop[b] = U[7], excl[7], drop[7]
    ones = torch.ones(V, dtype=torch.uint8)
    for inv_temp in (1.0, 0.3):
        alone, status = _logz(U[7:8], T, inv_temp, [excl[7]], None, drop[7:8])
        assert status == 0 and int(alone[3]) > 0 and int(alone[4]) > 0
        assert C.same(alone, _want(("alone", inv_temp), lambda: alone))                  # the other engine setting gave these bits
        for eligible in (None, ones):
            batch, status = _logz(U, T, inv_temp, excl, eligible, drop)
            assert status == 0
            for b in (0, 7, 63, 64):
                assert C.same(tuple(t[b:b + 1] for t in batch), alone), (inv_temp, b, eligible is None)
        assert C.same(_logz(U[7:8], T, inv_temp, [excl[7]], ones, drop[7:8])[0], alone)


# ---- 4. list log-probabilities --------------------------------------------------------------------------------------------------------
def _lists(pop, k, seed):
    """per user the first k rows of a random order of its population, -1 behind them"""
    g = torch.Generator().manual_seed(seed)
    out = torch.full((pop.shape[0], k), -1, dtype=torch.int64)
    for b in range(pop.shape[0]):
        rows = pop[b].nonzero()[:, 0]
        rows = rows[torch.randperm(rows.numel(), generator=g)][:k]
        out[b, :rows.numel()] = rows
    return out


def _pl(s, pop, lists, inv_temp):
    rows = [P.pl_logprobs(s[b].numpy(), inv_temp, pop[b].numpy(), lists[b].tolist()) for b in range(s.shape[0])]
    return torch.tensor(np.stack([r[0] for r in rows])), torch.tensor([r[1] for r in rows], dtype=torch.float64)


def _check_logp(logp, total, lists, want, k):
    tol = TOL["logsum"] + 2.0 ** -23 * want[0].abs().clamp(min=1.0)
    err = (logp.double() - want[0]).abs()
    assert bool((err <= tol).all()), float((err - tol).max())
    cnt = (lists >= 0).sum(1)
    assert bool(((total.double() - want[1]).abs() <= cnt * TOL["logsum"] + 2.0 ** -23 * want[1].abs().clamp(min=1.0)).all())
    return float(err.max())


@pytest.mark.parametrize("B,V,D", SHAPES)
def test_list_log_probabilities_against_float64(B, V, D):
    U, T, excl, eligible = _case(B, V, D)
    s = U.double() @ T.double().T
    pop = C.population(s, excl, eligible)[0]
    worst = 0.0
    for k in (1, 2, 10, 128):
        if V < k:
            continue
        lists = _lists(pop, k, 100 + k)
        for inv_temp in INV_TEMPS:
            want = _want(("pl", B, V, D, k, inv_temp), lambda: _pl(s, pop, lists, inv_temp))
            (logp, total, score), status = _logp(U, T, lists, inv_temp, excl, eligible)
            assert status == 0, (k, inv_temp)
            worst = max(worst, _check_logp(logp, total, lists, want, k))
            empty = lists < 0
            # the score of every pair is the plain entry's (exact here); an empty slot is +0 / -inf
            assert C.same(score, torch.where(empty, torch.full((), NEG_INF), s.float().gather(1, lists.clamp(min=0)) + 0.0))
            assert C.same(logp[empty], torch.zeros(int(empty.sum())))
            # a list that exhausts the population: its last row is certain
            full = (lists >= 0).sum(1) == pop.sum(1)
            last = (lists >= 0).sum(1) - 1
            for b in full.nonzero()[:, 0].tolist():
                if last[b] >= 0:
                    assert C.same(logp[b, last[b]].reshape(1), torch.zeros(1)), (b, k)
    print(f"({B}, {V}, {D}): largest |logp - float64| = {worst:.4e}")


def test_the_peaked_case_keeps_its_second_slot():
    """One row 40 above every other at inv_temp = 1: after it is drawn the subtractive form has nothing left to divide by, in
    float64 too; the tail form gives the second slot its log-probability."""
    V = 130
    U = torch.zeros(2, 4)
    U[:, 0] = 1
    T = torch.zeros(V, 4)
    T[:, 0] = torch.randint(-3, 4, (V,), generator=torch.Generator().manual_seed(9)).float()
    T[50, 0], T[51, 0] = 43.0, 3.0
    s = U.double() @ T.double().T
    assert float(s[0, 50]) - float(s[0][torch.arange(V) != 50].max()) == 40.0
    pop = torch.ones(2, V, dtype=torch.bool)
    lists = torch.tensor([[50, 3], [50, 120]])
    want = _pl(s, pop, lists, 1.0)
    (logp, total, score), status = _logp(U, T, lists, 1.0)
    assert status == 0 and bool(torch.isfinite(logp).all()) and float(logp[0, 1]) < -1
    _check_logp(logp, total, lists, want, 2)
    bad = P.pl_logprobs_subtractive(s[0].numpy(), 1.0, pop[0].numpy(), [50, 3])[0]
    assert not abs(bad[1] - float(want[0][0, 1])) <= 1e-3        # (-inf, NaN or noise)


def test_invalid_lists_are_nan_for_that_user_alone():
    B, V, D, k = 12, 200, 8, 3
    U, T = C.int_vectors(57, B, V, D)
    s = U.double() @ T.double().T
    excl = [[5, 6]] * B
    eligible = torch.ones(V, dtype=torch.uint8)
    eligible[9] = 0
    pop = C.population(s, excl, eligible)[0]
    lists = torch.tensor([[1, 2, 3]] * B)
    invalid = {1: [1, -1, 3], 3: [4, 4, 7], 5: [1, V, 2], 6: [1, 2, -7], 8: [5, 1, 2], 10: [1, 9, 2]}
    for b, rows in invalid.items():
        lists[b] = torch.tensor(rows)
    lists[11] = torch.tensor([8, -1, -1])                        # trailing empty slots are fine
    (logp, total, score), status = _logp(U, T, lists, 1.0, excl, eligible)
    assert status == E_LIST
    ok = [b for b in range(B) if b not in invalid]
    assert bool(torch.isnan(logp[list(invalid)]).all()) and bool(torch.isnan(total[list(invalid)]).all())
    assert bool(torch.isfinite(logp[ok]).all()) and bool(torch.isfinite(total[ok]).all())
    want = _pl(s[ok], pop[ok], lists[ok], 1.0)
    _check_logp(logp[ok], total[ok], lists[ok], want, k)
    assert C.same(logp[11, 1:], torch.zeros(2)) and bool((score[11, 1:] == NEG_INF).all())
    # each alone raises the flag as well, and a valid batch does not
    for b in invalid:
        got, status = _logp(U[b:b + 1], T, lists[b:b + 1], 1.0, excl[b:b + 1], eligible)
        assert status == E_LIST and bool(torch.isnan(got[0]).all()), b
    assert _logp(U[ok], T, lists[ok], 1.0, [excl[b] for b in ok], eligible)[1] == 0


# ---- 5. with the sampler --------------------------------------------------------------------------------------------------------------
def test_the_samplers_lists_are_lists_of_the_policy():
    from newsreclib_amd import ops
    B, V, D, k, inv_temp = 70, 700, 36, 10, 0.7
    g = torch.Generator().manual_seed(61)
    U, T = torch.randn(B, D, generator=g), torch.randn(V, D, generator=g)
    excl = [torch.randint(0, V, (int(n),), generator=g).tolist() for n in torch.randint(0, 10, (B,), generator=g)]
    eligible = (torch.rand(V, generator=g) > 0.15).to(torch.uint8)
    ei, eo = (t.cuda() for t in C.ragged(excl))
    idx, _, raw, status = ops.topk_sampled_scores(U.cuda(), T.cuda(), k, torch.arange(1, B + 1).cuda(), 31337, inv_temp, ei, eo, eligible.cuda())
    assert int(status) == 0 and bool((idx >= 0).all())
    dropped = ops.catalogue_logz(U.cuda(), T.cuda(), inv_temp, ei, eo, eligible.cuda(), idx)[4]
    assert bool((dropped == k).all())
    logp, total, score, status = ops.list_logprob(U.cuda(), T.cuda(), idx, inv_temp, ei, eo, eligible.cuda())
    assert int(status) == 0 and C.same(score, raw.cpu()) and bool(torch.isfinite(logp).all()) and bool((logp <= 0).all())
    # against float64 over the device's own scores would need the (B, V) matrix on the host in fp32 bits; the float64 scores are
    # within dot_bound of them, and a log-probability moves by at most twice the largest score error times inv_temp
    s = U.double() @ T.double().T
    pop = C.population(s, excl, eligible)[0]
    want = _pl(s, pop, idx.cpu(), float(np.float32(inv_temp)))
    bound = 2 * float(np.float32(inv_temp)) * (C.dot_bound(U, T).max(1)[0] + 2.0 ** -24 * s.abs().max(1)[0])
    err = (logp.cpu().double() - want[0]).abs()
    assert bool((err <= bound[:, None] + TOL["logsum"] + 2.0 ** -23 * want[0].abs().clamp(min=1.0)).all())


def test_the_draws_follow_the_reported_probabilities(engine):
    """4096 users with the same eight scores and distinct keys, one call, k = 2: the first-slot counts against exp(out_logp) of the
    first slot, taken per row, and the second-slot counts against the Plackett-Luce marginal of those probabilities, each below
    the upper 1e-6 quantile of chi-square with 7 degrees of freedom.  The smallest first-slot probability is 0.0192: 78 expected
    draws."""
    if engine != "f32":
        return                                                   # (the unit does not read the engine setting: once is enough)
    from newsreclib_amd import ops
    B = 4096
    s = [2, 1, 0, -1, 0.5, 1.5, -0.5, 0]
    U = torch.zeros(B, 4)
    U[:, 0] = 1
    T = torch.zeros(8, 4)
    T[:, 0] = torch.tensor(s)
    assert R.pl_marginals(s, 1.0)[0].min() * B >= 20
    idx, _, _, status = ops.topk_sampled_scores(U.cuda(), T.cuda(), 2, torch.arange(1000, 1000 + B).cuda(), 12345, 1.0)
    logp, total, score, lstatus = ops.list_logprob(U.cuda(), T.cuda(), idx, 1.0)
    assert int(status) == 0 and int(lstatus) == 0
    idx, logp = idx.cpu(), logp.cpu().double()
    p1 = np.zeros(8)
    for r in range(8):
        at = (idx[:, 0] == r).nonzero()[:, 0]
        assert at.numel() > 0
        p1[r] = math.exp(float(logp[at[0], 0]))
        # one number per row, whoever drew it and whatever it drew next: the tail differs, so within the slot's tolerance, twice
        assert float((logp[at, 0] - logp[at[0], 0]).abs().max()) <= 2 * (TOL["logsum"] + 2.0 ** -23 * max(1.0, abs(float(logp[at[0], 0]))))
    assert abs(p1.sum() - 1.0) <= 8 * (TOL["logsum"] + 2.0 ** -22)
    assert np.abs(p1 - R.pl_marginals(s, 1.0)[0]).max() <= TOL["logsum"] + 2.0 ** -22
    _, p2 = R.pl_marginals(np.log(p1), 1.0)
    c1 = R.chi2(np.bincount(idx[:, 0].numpy(), minlength=8), p1 / p1.sum())
    c2 = R.chi2(np.bincount(idx[:, 1].numpy(), minlength=8), p2)
    print(f"chi-square first slot {c1:.2f}, second slot {c2:.2f}")
    assert c1 < R.CHI2_7_1E6 and c2 < R.CHI2_7_1E6
    # the second slot's conditional probability is p_j / (1 - p_i)
    cond = torch.tensor(p1)[idx[:, 1]] / (1 - torch.tensor(p1)[idx[:, 0]])
    assert float((torch.exp(logp[:, 1]) - cond).abs().max()) <= 4 * (TOL["logsum"] + 2.0 ** -22)


def test_the_policy_entries_do_not_synchronise_with_the_host():
    from newsreclib_amd import ops
    U, T = C.int_vectors(3, 5, 200, 12)
    U, T = U.cuda(), T.cuda()
    ei, eo = C.ragged([[1], [], [5, 6], [], []])
    ei, eo, elig = ei.cuda(), eo.cuda(), torch.ones(200, dtype=torch.uint8).cuda()
    lists = torch.tensor([[7, 8]] * 5).cuda()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        if not C.sync_debug_honoured():
            return                                               # (this torch build does not raise on synchronising calls)
        stats = ops.catalogue_logz(U, T, 0.5, ei, eo, elig, lists)
        got = ops.list_logprob(U, T, lists, 0.5, ei, eo, elig)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert int(stats[5]) == 0 and int(got[3]) == 0 and got[0].shape == (5, 2) and bool((stats[4] == 2).all())


# ---- 6. through the cache -------------------------------------------------------------------------------------------------------------
def _cache_case():
    from newsreclib_amd.evaluation import DeviceNewsTable, NewsVectorCache
    mod, attrs = builders.tiny("nrms", late_fusion=True)
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


def test_the_cache_methods_are_the_ops_on_the_same_vectors():
    from newsreclib_amd import ops
    mod, cache, lists, hist, hs, uidx = _cache_case()
    V, k = 50, 4
    eligible = torch.ones(V, dtype=torch.uint8)
    eligible[0] = 0
    user, vec, hist_off = _users_by_hand(mod, cache, hist, hs, uidx)
    want = ops.catalogue_logz(user, vec, 0.5, hist.cuda(), hist_off, eligible.cuda())
    got = cache.policy_stats(hist.cuda(), hs, 0.5, user_idx=uidx, eligible=eligible)
    assert sorted(got) == ["entropy", "log_sum", "log_z", "max", "population", "status"] and int(got["status"]) == 0
    assert C.same((got["max"], got["log_sum"], got["entropy"], got["population"]), want[:4])
    assert C.same(got["log_z"], want[0].cpu() + want[1].cpu())
    assert bool((got["population"].cpu() == V - 1 - hs.int()).all())
    drawn = cache.recommend(hist.cuda(), hs, k, user_idx=uidx, eligible=eligible, sample=(0.5, 99, torch.arange(1, 7)))
    want = ops.list_logprob(user, vec, drawn[0], 0.5, hist.cuda(), hist_off, eligible.cuda())
    for given in (drawn[0], drawn[0].cpu()):                     # device lists, and host lists through pinned memory
        got = cache.list_log_probs(hist.cuda(), hs, given, 0.5, user_idx=uidx, eligible=eligible)
        assert int(got[3]) == 0 and C.same(got[:3], want[:3]) and C.same(got[2], drawn[1])
    # a list with a news of the history could not have been drawn
    bad = drawn[0].clone()
    bad[2, 1] = int(lists[2][0])
    got = cache.list_log_probs(hist.cuda(), hs, bad, 0.5, user_idx=uidx, eligible=eligible)
    assert int(got[3]) == E_LIST and bool(torch.isnan(got[1][2])) and bool(torch.isfinite(got[1].cpu()[[0, 1, 3, 4, 5]]).all())
    # without the history excluded the population is everything eligible
    assert bool((cache.policy_stats(hist.cuda(), hs, 0.5, user_idx=uidx, exclude_history=False, eligible=eligible)["population"] == V - 1).all())


def test_sample_recommendations_with_log_probs_and_the_policy_report():
    import warnings

    from newsreclib_amd.evaluation import policy_report, sample_recommendations
    mod, cache, lists, hist, hs, uidx = _cache_case()
    k = 5
    eligible = torch.ones(50, dtype=torch.uint8)
    eligible[0] = 0
    ids = [11, 3, 2 ** 35, 8, 1, 20]
    users = [{"hist": lists[b], "user_idx": uidx[b], "user_id": ids[b]} for b in range(6)]
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        plain = sample_recommendations(cache, users, k, 3, 2.0, 16, batch_size=4, eligible=eligible)
        small = sample_recommendations(cache, users, k, 3, 2.0, 16, batch_size=2, eligible=eligible, log_probs=True)
        large = sample_recommendations(cache, users, k, 3, 2.0, 16, batch_size=512, eligible=eligible, log_probs=True)
        assert isinstance(plain, torch.Tensor) and torch.equal(small[0], plain) and torch.equal(large[0], plain)
        assert small[1].shape == (6, 3, k) and small[1].dtype == torch.float32 and not small[1].is_cuda
        assert C.same(small[1], large[1]) and bool(torch.isfinite(small[1]).all()) and bool((small[1] < 0).all())
        for j in range(3):
            got = cache.list_log_probs(hist.cuda(), hs, plain[:, j].contiguous(), 0.5, user_idx=uidx, eligible=eligible)
            assert int(got[3]) == 0 and C.same(got[0], small[1][:, j])
        temps = [0.5, 2.0]
        report = policy_report(cache, users, temps, batch_size=4, eligible=eligible)
        assert sorted(report) == temps
        for t in temps:
            st = cache.policy_stats(hist.cuda(), hs, 1.0 / t, user_idx=uidx, eligible=eligible)
            ent, ls = st["entropy"].cpu().double(), st["log_sum"].cpu().double()
            for name, want in (("entropy", ent.mean()), ("perplexity", torch.exp(ent).mean()), ("top1", torch.exp(-ls).mean())):
                assert abs(report[t][name] - float(want)) <= 1e-12 * max(1.0, abs(float(want))), (t, name)
        assert report[0.5]["entropy"] < report[2.0]["entropy"] and report[0.5]["top1"] > report[2.0]["top1"]
        assert 1.0 <= report[2.0]["perplexity"] <= 49.0


def test_cache_refusals():
    from newsreclib_amd import evaluation as E
    mod, cache, lists, hist, hs, uidx = _cache_case()
    lo = torch.zeros(6, dtype=torch.int32)
    good = torch.ones(6, 2, dtype=torch.int64)
    with pytest.raises(NotImplementedError, match="tkz_sum_kernel"):
        cache.policy_stats(hist.cuda(), hs, 1.0, user_idx=uidx, window=(lo, lo))
    with pytest.raises(NotImplementedError, match="tkz_sum_kernel"):
        cache.list_log_probs(hist.cuda(), hs, good, 1.0, user_idx=uidx, window=(lo, lo))
    with pytest.raises(TypeError, match="int64"):
        cache.list_log_probs(hist.cuda(), hs, good.int(), 1.0, user_idx=uidx)
    with pytest.raises(ValueError, match="one list per user"):
        cache.list_log_probs(hist.cuda(), hs, good[:5], 1.0, user_idx=uidx)
    with pytest.raises(ValueError, match="`inv_temp`"):
        cache.policy_stats(hist.cuda(), hs, -1.0, user_idx=uidx)
    users = [{"hist": lists[b], "user_idx": uidx[b]} for b in range(6)]
    from newsreclib_amd.dkn_module import DKNModule
    from newsreclib_amd.miner_module import MINERModule
    from newsreclib_amd.npa_module import NPAModule
    from newsreclib_amd.senti_debias_module import SentiDebiasModule
    for cls in (MINERModule, DKNModule, NPAModule, SentiDebiasModule):
        other = E.NewsVectorCache(object.__new__(cls), cache.table)
        for call in (lambda: other.policy_stats(hist.cuda(), hs, 1.0), lambda: other.list_log_probs(hist.cuda(), hs, good, 1.0),
                     lambda: E.policy_report(other, users, [1.0])):
            with pytest.raises(NotImplementedError, match="tkz_sum_kernel"):
                call()
    for cls in (E.MannerVectorCache, E.NpaFeatureCache):
        with pytest.raises(NotImplementedError, match="tkz_sum_kernel"):
            object.__new__(cls).policy_stats(hist.cuda(), hs, 1.0)
        with pytest.raises(NotImplementedError, match="tkz_sum_kernel"):
            E.policy_report(object.__new__(cls), users, [1.0])
