"""Full-catalogue top-k by NPA's personalized-pooling score (``nrl_topk_pooled_scores``, ``ops.topk_pooled_scores``,
``NpaFeatureCache.recommend_pooled``).

Expected values are computed on the CPU in float64 (tests/topk_npa_ref.py).  The exact family of that module makes the softmax
weights exactly 1 / n on a peak set of n tokens and the score an integer sum over a power of two, so those cases compare with
``torch.equal`` and have many ties.  Real-valued cases use the derived bound of that module and its floor form: the gap between a
user's k-th and (k + 1)-th score can be below the bound, so row sets are never compared with float64."""
import functools

import pytest
import torch

from tests import builders
from tests import catalogue_ref as C
from tests import topk_npa_ref as R

pytestmark = pytest.mark.gpu

E_EXCLUDE, E_OFFSETS, E_NAN = 1, 2, 4


@pytest.fixture(autouse=True, params=["f32", "bf16x3"])
def engine(request):
    from newsreclib_amd import _lib
    prev = _lib.get_gemm_engine()
    _lib.set_gemm_engine(request.param)
    yield request.param
    _lib.set_gemm_engine(prev)


@functools.lru_cache(maxsize=None)
def _on_gpu(seed, B, V, L, F):
    """The exact case and its features on the device (uploaded once per case)."""
    q, user, feat, s = R.exact_case(seed, B, V, L, F)
    return q, user, feat, s, feat.cuda()


def _run(q, user, feat, k, excl=None, eligible=None, slices=0, off=None):
    from newsreclib_amd import ops
    ei = eo = None
    if excl is not None:
        ei, eo = C.ragged(excl)
        ei, eo = ei.cuda(), (off if off is not None else eo).cuda()
    idx, score, status = ops.topk_pooled_scores(q.cuda(), user.cuda(), feat.cuda(), k, ei, eo,
                                                eligible.cuda() if eligible is not None else None, slices)
    return idx.cpu(), score.cpu(), int(status)


# ---- 1. exact, with ties --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 10, 128])
@pytest.mark.parametrize("L,F", [(1, 4), (2, 8), (8, 16), (30, 24), (33, 36)])
def test_exact_with_ties(L, F, k):
    """Three user tiles (the last of 2 users), eight table tiles (the last of 104 rows), every slicing; one token, F below one
    k-tile, F no multiple of 16, L no multiple of anything."""
    q, user, _, s, feat = _on_gpu(200 + L, 130, 1000, L, F)
    want_idx, want_score = C.expected_topk(s, k)
    for slices in (0, 1, 2, 7):
        idx, score, status = _run(q, user, feat, k, slices=slices)
        assert status == 0, slices
        assert torch.equal(idx, want_idx), slices
        assert torch.equal(score, want_score), slices


# ---- 2. ordering and size edges ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("slices", [0, 2])
def test_all_equal_scores_return_the_first_rows(slices):
    q, user, feat = torch.ones(3, 8), torch.ones(3, 8), torch.ones(300, 3, 8)       # equal logits: weights 1 / 3, score 8
    idx, score, status = _run(q, user, feat, 16, slices=slices)
    assert status == 0
    assert torch.equal(idx, torch.arange(16).expand(3, 16))
    assert torch.equal(score, torch.full((3, 16), 8.0))


def test_fewer_rows_than_k_and_an_empty_table():
    q, user, feat, s = R.exact_case(7, 3, 5, 8, 16)
    idx, score, status = _run(q, user, feat, 8)
    want_idx, want_score = C.expected_topk(s, 8)
    assert status == 0 and torch.equal(idx, want_idx) and torch.equal(score, want_score)
    assert bool((idx[:, 5:] == -1).all()) and bool((score[:, 5:] == float("-inf")).all()) and bool((idx[:, :5] >= 0).all())
    idx, score, status = _run(q, user, feat[:0], 8)
    assert status == 0 and bool((idx == -1).all()) and bool((score == float("-inf")).all())


# ---- 3. exclusion, eligibility and status -----------------------------------------------------------------------------------------
def _excl_case():
    B, V, L, F, k = 5, 40, 8, 16, 16
    q, user, feat, s = R.exact_case(91, B, V, L, F)
    eligible = torch.ones(V, dtype=torch.uint8)
    eligible[[0, 7, 8, 31]] = 0
    first = C.expected_topk(s, k, None, eligible)[0][:, 0]           # every user's would-be first place
    everything = [v for v in range(V) if eligible[v]]
    excl = [[], [3, 3, 9, 3, 9], [int(first[2]), 5], everything, [int(first[4])] * 3 + [39, 1]]
    return (q, user, feat), s, k, excl, eligible


@pytest.mark.parametrize("slices", [0, 1])
def test_exclusion_and_eligibility(slices):
    ops_in, s, k, excl, eligible = _excl_case()
    idx, score, status = _run(*ops_in, k, excl, eligible, slices)
    want_idx, want_score = C.expected_topk(s, k, excl, eligible)
    assert status == 0
    assert torch.equal(idx, want_idx) and torch.equal(score, want_score)
    assert torch.equal(idx[3], torch.full((k,), -1)) and bool(torch.isinf(score[3]).all())
    for b in range(len(excl)):
        got = set(idx[b].tolist()) - {-1}
        assert not (got & set(excl[b])) and not (got & {0, 7, 8, 31})


def test_exclusion_list_longer_than_the_cached_part():
    """Lists beyond the 64 entries a workgroup caches are read from global memory: 150 entries and duplicates, several tiles."""
    B, V, L, F, k = 3, 700, 4, 8, 20
    q, user, feat, s = R.exact_case(5, B, V, L, F)
    g = torch.Generator().manual_seed(3)
    best = C.expected_topk(s, 150)[0][2].tolist()
    excl = [torch.randperm(V, generator=g)[:150].tolist(), [], best + best[:40]]
    idx, score, status = _run(q, user, feat, k, excl, slices=3)
    want_idx, want_score = C.expected_topk(s, k, excl)
    assert status == 0 and torch.equal(idx, want_idx) and torch.equal(score, want_score)


def test_status_bad_exclusion_index_is_ignored():
    ops_in, s, k, excl, eligible = _excl_case()
    bad = [list(x) for x in excl]
    bad[1] = [-1] + bad[1]
    bad[2] = bad[2] + [s.shape[1]]
    idx, score, status = _run(*ops_in, k, bad, eligible)
    want_idx, want_score = C.expected_topk(s, k, excl, eligible)
    assert status == E_EXCLUDE
    assert torch.equal(idx, want_idx) and torch.equal(score, want_score)


def test_status_decreasing_offsets_blank_that_user_alone():
    q, user, feat, s = R.exact_case(17, 4, 40, 8, 16)
    k, flat = 6, list(range(12))
    off = torch.tensor([0, 5, 3, 8, 12])                    # user 1 runs backwards
    idx, score, status = _run(q, user, feat, k, [flat], off=off)
    assert status == E_OFFSETS
    want_idx, want_score = C.expected_topk(s, k, [flat[0:5], [], flat[3:8], flat[8:12]])
    for b in (0, 2, 3):
        assert torch.equal(idx[b], want_idx[b]) and torch.equal(score[b], want_score[b])
    assert torch.equal(idx[1], torch.full((k,), -1)) and bool((score[1] == float("-inf")).all())


def test_status_offsets_beyond_the_list():
    q, user, feat, s = R.exact_case(18, 3, 40, 8, 16)
    k = 6
    idx, score, status = _run(q, user, feat, k, [list(range(6))], off=torch.tensor([0, 2, 9, 6]))
    assert status == E_OFFSETS
    want_idx, _ = C.expected_topk(s, k, [[0, 1], [], []])
    assert torch.equal(idx[0], want_idx[0])
    assert torch.equal(idx[1:], torch.full((2, k), -1))


@pytest.mark.parametrize("where", ["peak token", "other token"])
def test_status_nan_row_is_left_out(where):
    """A NaN in one element of a feature map reaches every user's score of that row through p = exp(a - m') (fmaxf alone would
    drop a NaN logit; on a token whose weight is otherwise exactly 0 as well): flagged, and the row is left out."""
    B, V, L, F, k = 5, 300, 8, 16, 9
    q, user, feat, s = R.exact_case(23, B, V, L, F)
    clean_idx, clean_score, status = _run(q, user, feat, k, slices=2)
    assert status == 0 and torch.equal(clean_idx, C.expected_topk(s, k)[0])
    in_peak = (feat[:, :, 0] > 0) | (feat[:, :, 1] > 0)     # (V, L)
    wanted = in_peak if where == "peak token" else ~in_peak
    nan_row = next(int(r) for r in clean_idx[0] if bool(wanted[int(r)].any()))      # a row that would be returned
    token = int(torch.nonzero(wanted[nan_row])[0])
    fn = feat.clone()
    fn[nan_row, token, F - 1] = float("nan")                # a column where q is 0: 0 * NaN is still NaN
    idx, score, status = _run(q, user, fn, k, slices=2)
    assert status == E_NAN
    assert not bool((idx == nan_row).any())
    elig = torch.ones(V, dtype=torch.uint8)
    elig[nan_row] = 0
    want_idx, want_score = C.expected_topk(s, k, None, elig)          # every other position unchanged
    assert torch.equal(idx, want_idx) and torch.equal(score, want_score)
    # not eligible: nobody is told
    idx, score, status = _run(q, user, fn, k, eligible=elig, slices=2)
    assert status == 0 and torch.equal(idx, want_idx) and torch.equal(score, want_score)


# ---- 4. real values against float64 -----------------------------------------------------------------------------------------------
def test_real_values_against_float64():
    c, k = R.real_case(), R.REAL["k"]
    idx, score, status = _run(c["q"], c["user"], c["feat"], k, c["excl"])
    assert status == 0
    rows = idx.clamp(min=0)
    ratio = ((score.double() - c["raw"].gather(1, rows)).abs() / c["bound"].gather(1, rows)).max(dim=1)[0]
    print("max |score - float64| / bound per user: " + " ".join(f"{float(x):.1e}" for x in ratio))
    C.check_floor(idx, score, c["raw"], c["bound"], C.population(c["raw"], c["excl"])[0], k)


# ---- 5. agreement with the existing scorer ------------------------------------------------------------------------------------------


def _cached_side_bound(cache, user, q_cand):
    """The fp32 bound of ``cache.scores`` for (user, news): the pooled vector by npa_cached_pool (its logits and its online softmax
    as in tests/topk_npa_ref.py, per component of c instead of per s_t) and then one dot product of length F with ``user``:
    sum_f |user_f| (sum_t w_t |c_tf|) (2 e_a + (K + L + 2) EPS) + F EPS sum_f |user_f| |pooled_f|."""
    feat = cache.features.double().cpu()                    # (V, L, F)
    V, L, F = feat.shape
    a = feat @ q_cand.double().T                            # (V, L, B)
    w = torch.softmax(a, dim=1)
    e_a = F * R.EPS * (feat.abs() @ q_cand.double().abs().T).max(dim=1)[0]          # (V, B)
    k_term = 2 * (L * (R.U_EXP + 2) + 208)
    pooled_abs = torch.einsum("vlb,vlf->vbf", w, feat.abs())                        # (V, B, F)
    S = torch.einsum("vbf,bf->vb", pooled_abs, user.double().abs())
    return (S * (2 * e_a + (k_term + L + 2) * R.EPS) + F * R.EPS * S).T             # (B, V)


@pytest.mark.parametrize("late_fusion", [False, True])
def test_recommend_pooled_against_the_cache_scores(late_fusion):
    """The fused ranking against ``cache.scores`` (nrl_npa_cached_scores: pooled vectors, then dot products) with the whole small
    table as every user's candidate list."""
    mod, table = builders.tiny_npa(late_fusion)
    mod.train()
    cache = mod.feature_cache(table, chunk=32)
    V, B, k = 50, 6, 10
    lists, hist, hs = builders.hist_batch(V)[:3]
    uidx = torch.tensor([3, 1, 4, 1, 5, 8])
    with pytest.raises(NotImplementedError, match="depend on the user"):
        cache.recommend(hist.cuda(), hs, k)
    idx, score, status = cache.recommend_pooled(hist.cuda(), hs, k, user_idx=uidx)
    assert mod.training                                          # the mode is restored
    assert int(status) == 0 and idx.shape == (B, k)
    full = cache.scores(hist, hs, torch.arange(V).repeat(B), torch.full((B,), V), uidx).double().cpu()      # (B, V)
    idx, score = idx.cpu(), score.cpu()
    # both sides' bounds from the fp32 user vectors and queries the cache itself uses
    from newsreclib_amd.ops_npa import npa_cached_scores
    with torch.no_grad():
        text_q, q_news = mod.user_queries(uidx.cuda())
    off = torch.cat([torch.zeros(1, dtype=torch.int64), hs.cumsum(0)]).cuda()
    _, user = npa_cached_scores(cache.features, hist.cuda(), off, torch.empty(0, dtype=torch.int64, device="cuda"),
                                torch.zeros(B + 1, dtype=torch.int64, device="cuda"), text_q[:B], text_q[B:], q_news, int(hs.max()), 1,
                                return_user_vectors=True)
    user, q_cand = user.cpu(), text_q[B:].detach().cpu()
    s_f, b_f = R.scores64(q_cand, user, cache.features.cpu())
    bound = b_f + _cached_side_bound(cache, user, q_cand)
    assert bool(((full - s_f).abs() <= bound).all())             # the same function, pooled vector formed or not
    for b in range(B):
        rows = idx[b]
        assert bool((rows >= 0).all()) and not (set(rows.tolist()) & set(lists[b].tolist()))
        assert bool(((score[b].double() - s_f[b, rows]).abs() <= b_f[b, rows]).all())
        assert bool(((score[b].double() - full[b, rows]).abs() <= bound[b, rows]).all())
        assert bool((score[b][1:] <= score[b][:-1]).all())
        rest = torch.ones(V, dtype=torch.bool)
        rest[rows] = False
        rest[lists[b]] = False
        assert bool((full[b][rest] <= full[b, rows].min() + 2 * bound[b][rest]).all())
    # without the exclusion the history may appear
    idx2, _, _ = cache.recommend_pooled(hist.cuda(), hs, V, user_idx=uidx, exclude_history=False)
    assert all(set(idx2[b].tolist()) == set(range(V)) for b in range(B))
    mod.eval()


def test_recommend_users_routes_an_npa_cache_to_recommend_pooled():
    """Users of equal history length, so the batch's longest history (the ``max_hist`` quirk) cannot differ between batchings:
    identical dictionaries for two batches (the second partial) and for one."""
    from newsreclib_amd.evaluation import recommend_users
    mod, table = builders.tiny_npa()
    cache = mod.feature_cache(table)
    V, B, k = 50, 6, 10
    lists, hist, hs = builders.hist_batch(V, sizes=[4] * B)[:3]
    uidx = torch.tensor([3, 1, 4, 1, 5, 8])
    idx, score, status = cache.recommend_pooled(hist.cuda(), hs, k, user_idx=uidx)
    assert int(status) == 0
    idx, score = idx.cpu(), score.cpu()
    users = [{"hist": lists[b], "user_id": 100 + b, "user_idx": uidx[b]} for b in range(B)]
    for batch_size in (4, 8):
        recs = recommend_users(cache, users, k, batch_size=batch_size)
        assert list(recs) == [f"U{100 + b}" for b in range(B)]
        assert all(list(recs[f"U{100 + b}"]) == [f"N{int(i)}" for i in idx[b]] for b in range(B))
        assert all(list(recs[f"U{100 + b}"].values()) == [float(v) for v in score[b]] for b in range(B))


# ---- 6. invariance and determinism ---------------------------------------------------------------------------------------------------
def test_invariance_and_determinism():
    """Bit-equal rows and scores whatever the slicing, the batch (all 130 users one at a time), the GEMM engine setting (both are
    set here, inside the one test, on top of the fixture's) and on a second run."""
    from newsreclib_amd import _lib, ops
    B, V, L, F, k = 130, 1000, 30, 100, 10
    g = torch.Generator().manual_seed(31)
    feat = torch.relu(torch.randn(V, L, F, generator=g)).cuda()
    q = torch.tanh(0.25 * torch.randn(B, F, generator=g)).cuda()
    user = (torch.randn(B, F, generator=g) / F ** 0.5).cuda()
    bits = lambda t: t.view(torch.int32)  # noqa: E731
    base_idx, base_score, status = ops.topk_pooled_scores(q, user, feat, k)
    assert int(status) == 0 and bool((base_idx >= 0).all())
    for slices in (1, 2, 7, 0):
        idx, score, status = ops.topk_pooled_scores(q, user, feat, k, slices=slices)
        assert int(status) == 0
        assert torch.equal(idx, base_idx) and torch.equal(bits(score), bits(base_score)), slices
    singles = [ops.topk_pooled_scores(q[b:b + 1], user[b:b + 1], feat, k) for b in range(B)]
    assert torch.equal(torch.cat([s[0] for s in singles]), base_idx)
    assert torch.equal(bits(torch.cat([s[1] for s in singles])), bits(base_score))
    assert int(torch.cat([s[2] for s in singles]).max()) == 0
    prev = _lib.get_gemm_engine()
    try:
        for name in ("f32", "bf16x3"):
            _lib.set_gemm_engine(name)
            idx, score, _ = ops.topk_pooled_scores(q, user, feat, k)
            assert torch.equal(idx, base_idx) and torch.equal(bits(score), bits(base_score)), name
    finally:
        _lib.set_gemm_engine(prev)


# ---- 7. memory -------------------------------------------------------------------------------------------------------------------------
def test_peak_memory_is_far_below_one_logit_tensor():
    from newsreclib_amd import ops
    B, V, L, F, k = 512, 8192, 30, 64, 10
    g = torch.Generator(device="cuda").manual_seed(2)
    feat = torch.relu(torch.randn(V, L, F, generator=g, device="cuda"))
    q = torch.tanh(0.25 * torch.randn(B, F, generator=g, device="cuda"))
    user = torch.randn(B, F, generator=g, device="cuda") / F ** 0.5
    ops.topk_pooled_scores(q[:2], user[:2], feat[:256], k)       # library loaded, kernels resident
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    live = torch.cuda.memory_allocated()
    out = ops.topk_pooled_scores(q, user, feat, k)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - live
    print(f"peak above the inputs: {peak} bytes; one (B, V, L) fp32 tensor: {B * V * L * 4} bytes")
    assert peak < B * V * L * 4 / 100
    assert int(out[2]) == 0 and bool((out[0] >= 0).all())


# ---- 8. no read-back ---------------------------------------------------------------------------------------------------------------------
def test_topk_pooled_scores_does_not_synchronise_with_the_host():
    from newsreclib_amd import ops
    q, user, feat, _ = R.exact_case(3, 5, 200, 8, 16)
    q, user, feat = q.cuda(), user.cuda(), feat.cuda()
    ei, eo = C.ragged([[1, 2], [], [5], [7, 7], []])
    ei, eo, elig = ei.cuda(), eo.cuda(), torch.ones(200, dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        if not C.sync_debug_honoured():
            pytest.skip("this torch build does not raise on synchronising calls under set_sync_debug_mode('error')")
        idx, score, status = ops.topk_pooled_scores(q, user, feat, 4, ei, eo, elig)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert int(status) == 0 and idx.shape == (5, 4)


def test_recommend_pooled_does_not_synchronise_with_the_host():
    mod, table = builders.tiny_npa()
    cache = mod.feature_cache(table)
    cache.build()
    _, hist, hs = builders.hist_batch(50)[:3]
    hist, uidx = hist.cuda(), torch.tensor([3, 1, 4, 1, 5, 8]).cuda()      # the sizes stay on the host
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        if not C.sync_debug_honoured():
            pytest.skip("this torch build does not raise on synchronising calls under set_sync_debug_mode('error')")
        idx, score, status = cache.recommend_pooled(hist, hs, 5, user_idx=uidx)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert int(status) == 0 and idx.shape == (6, 5)
