"""Several Gumbel top-k draws per walk and the class exposure of lists on the GPU (``nrl_topk_sampled_draws`` /
``nrl_list_class_exposure``, their ``ops`` wrappers, ``NewsVectorCache.recommend_draws``, ``sample_recommendations`` through it and
``exposure_report``).

The contract of the draws entry is an equality: draw ``r`` is ``ops.topk_sampled_scores`` under ``(seed + r) mod 2^64``, bit for bit
in the rows, the keys and the raw scores, and the status word is the OR of those calls' words.  The single entry has its own oracle
(``tests/test_gpu_topk_sampled.py``); one case here is also held against the restatement (``tests/topk_draws_ref.py``) directly.
The exposure is held against the float64 restatement of its sum, bit for bit.  Every comparison is exact."""
import pytest
import torch

from tests import builders
from tests import catalogue_ref as C
from tests import topk_draws_ref as DR

pytestmark = pytest.mark.gpu

E_EXCLUDE, E_OFFSETS, E_NAN = 1, 2, 4
NEG_INF = float("-inf")
SHAPES = [(1, 1, 4, 1, 1), (3, 130, 20, 5, 3), (63, 127, 4, 4, 2), (65, 129, 4, 4, 32), (64, 128, 4, 128, 1), (70, 700, 36, 10, 12),
          (130, 1000, 300, 10, 8), (5, 128, 1024, 7, 18)]
INV_TEMPS = (1.0, 0.5, 0.0)
SEEDS = (0, 2 ** 40 + 7, 2 ** 64 - 2)                       # (seed + r wraps under the last)


def _cuda(t):
    return t.cuda() if t is not None else None


def _keys(B, seed=0):
    """One int64 key per user: small ones, negative ones and ones above 2^32."""
    g = torch.Generator().manual_seed(900 + seed)
    keys = torch.randint(-2 ** 62, 2 ** 62, (B,), generator=g)
    keys[::3] = torch.arange(B)[::3] + 1
    return keys


def _masks(excl, excl_off):
    if excl is None:
        return None, None
    ei, eo = C.ragged(excl)
    return ei.cuda(), (excl_off if excl_off is not None else eo).cuda()


def _draws(U, T, k, R, keys, seed, inv_temp, excl=None, eligible=None, slices=0, excl_off=None):
    from newsreclib_amd import ops
    ei, eo = _masks(excl, excl_off)
    idx, key, score, status = ops.topk_sampled_draws(U.cuda(), T.cuda(), k, R, keys.cuda(), seed, inv_temp, ei, eo, _cuda(eligible), slices)
    assert idx.shape == key.shape == score.shape == (U.shape[0], R, k)
    return idx.cpu(), key.cpu(), score.cpu(), int(status)


def _singles(U, T, k, R, keys, seed, inv_temp, excl=None, eligible=None, excl_off=None):
    """R calls of the single entry under seed + r mod 2^64, stacked to (B, R, k), and the OR of their status words"""
    from newsreclib_amd import ops
    ei, eo = _masks(excl, excl_off)
    Uc, Tc, kc, el = U.cuda(), T.cuda(), keys.cuda(), _cuda(eligible)
    per = [ops.topk_sampled_scores(Uc, Tc, k, kc, s, inv_temp, ei, eo, el) for s in DR.draw_seeds(seed, R)]
    word = 0
    for p in per:
        word |= int(p[3])
    return tuple(torch.stack([p[i] for p in per], dim=1).cpu() for i in range(3)) + (word,)


def _case(B, V, D):
    """Integer vectors (ties occur), exclusion lists (0 to 9 rows, duplicates allowed; user 0's longer than the 64 entries a
    workgroup caches), a mixed mask, keys."""
    seed = B * 7 + V + D
    U, T = C.int_vectors(seed, B, V, D)
    g = torch.Generator().manual_seed(seed + 1)
    excl = [torch.randint(0, V, (int(n),), generator=g).tolist() for n in torch.randint(0, 10, (B,), generator=g)]
    excl[-1] = (excl[-1] + [0, 0])[:9]
    excl[0] = torch.randint(0, V, (100,), generator=g).tolist()
    eligible = (torch.rand(V, generator=g) > 0.15).to(torch.uint8)
    return U, T, excl, eligible, _keys(B, seed)


# ---- 1. equality with R single calls ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_the_draws_are_the_single_calls_under_seed_plus_r(shape):
    """All three outputs and the status word, under every inv_temp and seed: without masks, with exclusion lists (one longer than
    64), with an eligibility mask, with both."""
    B, V, D, k, R = shape
    U, T, excl, eligible, keys = _case(B, V, D)
    masks = ((None, None), (excl, None), (None, eligible), (excl, eligible))
    for inv_temp in INV_TEMPS:
        for n, seed in enumerate(SEEDS):
            for ex, el in (masks[n], masks[3]):
                got = _draws(U, T, k, R, keys, seed, inv_temp, ex, el)
                want = _singles(U, T, k, R, keys, seed, inv_temp, ex, el)
                assert got[3] == want[3] == 0, (inv_temp, seed)
                assert C.same(got[:3], want[:3]), (inv_temp, seed, ex is not None, el is not None)
    if R > 1 and V > 4 * k:                                      # another seed is another draw: the lists of a call differ
        assert not torch.equal(got[0][:, 0], got[0][:, 1])


def test_one_case_against_the_restatement():
    """(3, 130, 20, 5, 3) against ``topk_sampled_ref.expected`` per draw with the device's own noise given, seeds wrapping."""
    from newsreclib_amd import ops
    B, V, D, k, R = 3, 130, 20, 5, 3
    U, T, excl, eligible, keys = _case(B, V, D)
    seed = 2 ** 64 - 2
    noise = []
    for s in DR.draw_seeds(seed, R):
        g = ops.gumbel_noise(keys.cuda().repeat_interleave(V), torch.arange(V).cuda().repeat(B), s)[1]
        noise.append(g.cpu().reshape(B, V))
    for inv_temp in (1.0, 0.5):
        want = DR.expected(U.double() @ T.double().T, noise, inv_temp, k, excl, eligible)
        got = _draws(U, T, k, R, keys, seed, inv_temp, excl, eligible)
        assert got[3] == 0 and C.same(got[:3], want)


# ---- 2. slices, the batch ---------------------------------------------------------------------------------------------------------------
def test_the_draws_do_not_depend_on_the_slicing_or_the_place_in_the_batch():
    B, V, D, k, R = 65, 700, 36, 10, 8                           # (eight draws of ten: two walks of the table inside the entry)
    g = torch.Generator().manual_seed(71)
    U, T = torch.randn(B, D, generator=g), torch.randn(V, D, generator=g)
    excl = [torch.randint(0, V, (int(n),), generator=g).tolist() for n in torch.randint(0, 10, (B,), generator=g)]
    eligible = (torch.rand(V, generator=g) > 0.15).to(torch.uint8)
    keys, seed, inv_temp = _keys(B, 5), 424242, 0.8

    def run(users, slices=0):
        users = list(users)
        got = _draws(U[users], T, k, R, keys[users], seed, inv_temp, [excl[b] for b in users], eligible, slices)
        assert got[3] == 0
        return got[:3]

    base = run(range(B))
    assert C.same(base, _singles(U, T, k, R, keys, seed, inv_temp, excl, eligible)[:3])
    for slices in (1, 7):
        assert C.same(run(range(B), slices), base), slices
    for b in (0, 63, 64):                                        # alone: one user, one workgroup per slice
        assert C.same(run([b]), tuple(t[b:b + 1] for t in base)), b
    assert C.same(tuple(t.flip(0) for t in run(reversed(range(B)))), base)


# ---- 3. edges ---------------------------------------------------------------------------------------------------------------------------
def test_fewer_rows_than_k_and_empty_sides():
    from newsreclib_amd import ops
    U, T = C.int_vectors(5, 4, 6, 8)
    keys = _keys(4)
    idx, key, score, status = _draws(U, T, 9, 5, keys, 11, 1.0, [[0], [], [1, 2], []], None)
    assert status == 0 and C.same((idx, key, score), _singles(U, T, 9, 5, keys, 11, 1.0, [[0], [], [1, 2], []], None)[:3])
    left = torch.tensor([5, 6, 4, 6])
    for b in range(4):
        n = int(left[b])
        assert bool((idx[b, :, :n] >= 0).all()) and bool((idx[b, :, n:] == -1).all())
        assert bool((key[b, :, n:] == NEG_INF).all()) and bool((score[b, :, n:] == NEG_INF).all())
        assert all(sorted(idx[b, r, :n].tolist()) == sorted(idx[b, 0, :n].tolist()) for r in range(5))
    # V == 0: every slot empty; B == 0: nothing to do
    idx, key, score, status = _draws(U, T[:0], 3, 4, keys, 1, 1.0)
    assert status == 0 and bool((idx == -1).all()) and bool((key == NEG_INF).all()) and bool((score == NEG_INF).all())
    got = ops.topk_sampled_draws(U[:0].cuda(), T.cuda(), 3, 4, keys[:0].cuda(), 1)
    assert got[0].shape == got[1].shape == got[2].shape == (0, 4, 3) and int(got[3]) == 0


# ---- 4. flags ---------------------------------------------------------------------------------------------------------------------------
def test_flags_and_outputs_equal_the_single_calls():
    B, V, D, k, R = 6, 300, 8, 4, 7
    U, T = C.int_vectors(21, B, V, D)
    keys = _keys(B, 2)
    excl = [[1, 2], [3], [], [4, 5, 6], [], [7]]
    bad = [list(e) for e in excl]
    bad[3] = [4, V + 3, -2]                                      # a bad exclusion index
    got, want = _draws(U, T, k, R, keys, 5, 1.0, bad), _singles(U, T, k, R, keys, 5, 1.0, bad)
    assert got[3] == want[3] == E_EXCLUDE and C.same(got[:3], want[:3])
    off = C.ragged(excl)[1].clone()
    off[2], off[3] = off[3], off[2] - 1                          # decreasing offsets
    got, want = _draws(U, T, k, R, keys, 5, 1.0, excl, None, 0, off), _singles(U, T, k, R, keys, 5, 1.0, excl, None, off)
    assert got[3] == want[3] and got[3] & E_OFFSETS and C.same(got[:3], want[:3])
    assert bool((got[0] == -1).reshape(B, -1).all(dim=1).any())            # (such a user's lists are blank in every draw)
    Tn = T.clone()
    Tn[17] = float("nan")                                        # a NaN table row
    for inv_temp in (1.0, 0.0):
        got, want = _draws(U, Tn, k, R, keys, 5, inv_temp, excl), _singles(U, Tn, k, R, keys, 5, inv_temp, excl)
        assert got[3] == want[3] == E_NAN and C.same(got[:3], want[:3]) and not bool((got[0] == 17).any())


# ---- 5. no read-back --------------------------------------------------------------------------------------------------------------------
def test_the_entries_do_not_synchronise_with_the_host():
    from newsreclib_amd import ops
    U, T = C.int_vectors(3, 5, 200, 12)
    U, T = U.cuda(), T.cuda()
    ei, eo = C.ragged([[1], [], [5, 6], [], []])
    ei, eo, elig, keys = ei.cuda(), eo.cuda(), torch.ones(200, dtype=torch.uint8).cuda(), _keys(5).cuda()
    cls, w = (torch.arange(200) % 5).int().cuda(), torch.ones(4).cuda()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        if not C.sync_debug_honoured():
            pytest.skip("this torch build does not raise on synchronising calls under set_sync_debug_mode('error')")
        idx, key, score, status = ops.topk_sampled_draws(U, T, 4, 20, keys, 3, 0.5, ei, eo, elig)
        exposure, flags = ops.list_class_exposure(idx, cls, w, 5)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert int(status) == 0 and int(flags) == 0 and idx.shape == (5, 20, 4) and exposure.shape == (5, 5)


# ---- 6. through the cache ---------------------------------------------------------------------------------------------------------------
def _cache_case(late_fusion=False):
    from newsreclib_amd.evaluation import DeviceNewsTable, NewsVectorCache
    mod, attrs = builders.tiny("nrms", late_fusion=late_fusion)
    cache = NewsVectorCache(mod, DeviceNewsTable(attrs), chunk=32)
    lists, hist, hs, uidx = builders.hist_batch(50)
    return mod, cache, lists, hist, hs, uidx


@pytest.mark.parametrize("k,draws", [(50, 5), (8, 20)])
def test_recommend_draws_is_recommend_with_a_sample_per_draw(k, draws):
    """k = 50: groups of 2, 2 and 1 draws; k = 8: groups of 16 and 4.  Host keys (through pinned memory) and device keys."""
    mod, cache, lists, hist, hs, uidx = _cache_case()
    eligible = torch.ones(50, dtype=torch.uint8)
    eligible[0] = 0
    keys = torch.tensor([7, 1, 2 ** 40, -3, 5, 6])
    seed = 2 ** 64 - 3
    want = [cache.recommend(hist.cuda(), hs, k, user_idx=uidx, eligible=eligible, sample=(0.5, s, keys.cuda()))
            for s in DR.draw_seeds(seed, draws)]
    for key_tensor in (keys, keys.cuda()):
        idx, score, status = cache.recommend_draws(hist.cuda(), hs, k, draws, (0.5, seed, key_tensor), user_idx=uidx, eligible=eligible)
        assert idx.shape == score.shape == (6, draws, k) and int(status) == 0
        for r in range(draws):
            assert C.same((idx[:, r], score[:, r]), want[r][:2]), r
    assert not torch.equal(idx[:, 0], idx[:, 1])


# ---- 7. sample_recommendations ----------------------------------------------------------------------------------------------------------
def test_sample_recommendations_returns_the_per_draw_lists_from_one_encoder_pass_per_batch(monkeypatch):
    """Draw j is ``recommend_users`` under ``seed + j`` (a late-fusion module: no user sees another user of its batch), the user
    encoder runs once per batch and the single-draw entry is never called."""
    import warnings

    from newsreclib_amd import ops
    from newsreclib_amd.evaluation import recommend_users, sample_recommendations
    mod, cache, lists, hist, hs, uidx = _cache_case(late_fusion=True)
    k = 5
    eligible = torch.ones(50, dtype=torch.uint8)
    eligible[0] = 0
    ids = [11, 3, 2 ** 35, 8, 1, 20]
    users = [{"hist": lists[b], "user_idx": uidx[b], "user_id": ids[b]} for b in range(6)]
    counts = {"user_vectors": 0, "single": 0, "draws": 0}

    def counting(name, fn):
        def wrapper(*args, **kwargs):
            counts[name] += 1
            return fn(*args, **kwargs)
        return wrapper

    cache.build()
    with monkeypatch.context() as m:
        m.setattr(mod, "user_vectors", counting("user_vectors", mod.user_vectors))
        m.setattr(ops, "topk_sampled_scores", counting("single", ops.topk_sampled_scores))
        m.setattr(ops, "topk_sampled_draws", counting("draws", ops.topk_sampled_draws))
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            draws = sample_recommendations(cache, users, k, 3, 2.0, 16, batch_size=4, eligible=eligible)
        assert counts == {"user_vectors": 2, "single": 0, "draws": 2}
    assert draws.shape == (6, 3, k) and draws.dtype == torch.int64 and not draws.is_cuda
    for j in range(3):
        listed = recommend_users(cache, users, k, batch_size=512, eligible=eligible, sample=(2.0, 16 + j))
        for b, uid in enumerate(ids):
            assert ["N" + str(r) for r in draws[b, j].tolist()] == list(listed["U" + str(uid)]), (b, j)
    # more draws than one group holds, and the log-probabilities of what was drawn
    many, logp = sample_recommendations(cache, users, k, 30, 2.0, 16, batch_size=4, eligible=eligible, log_probs=True)
    assert torch.equal(many[:, :3], draws) and logp.shape == (6, 30, k)
    for j in (0, 25, 29):
        lp = cache.list_log_probs(hist.cuda(), hs, many[:, j].contiguous(), 0.5, user_idx=uidx, eligible=eligible)[0]
        assert C.same(logp[:, j], lp.cpu()), j


# ---- 8. / 9. the exposure ---------------------------------------------------------------------------------------------------------------
def _exposure_case(B, L, k, V, S, seed=0):
    g = torch.Generator().manual_seed(1000 + seed + B + L + k)
    lists = torch.randint(0, V, (B, L, k), generator=g)
    lists[torch.rand(B, L, k, generator=g) < 0.1] = -1            # empty slots anywhere
    cls = torch.randint(0, S, (V,), generator=g).int()
    return lists, cls


def _weights(k, how):
    from newsreclib_amd.evaluation import exposure_weights
    if how == "random":
        return torch.rand(k, generator=torch.Generator().manual_seed(k))
    return exposure_weights(k, how)


@pytest.mark.parametrize("shape", [(1, 1, 1, 1, 1), (5, 3, 7, 50, 4), (65, 16, 8, 300, 64), (3, 128, 128, 200, 17)],
                         ids=lambda s: "x".join(map(str, s)))
def test_exposure_over_shapes(shape):
    from newsreclib_amd import ops
    B, L, k, V, S = shape
    lists, cls = _exposure_case(*shape)
    for how in ("rbp", "dcg", "random"):
        w = _weights(k, how)
        out, status = ops.list_class_exposure(lists.cuda(), cls.cuda(), w.cuda(), S)
        want, flags = DR.exposure(lists, cls, w, S)
        assert out.shape == (B, S) and out.dtype == torch.float32 and int(status) == flags == 0
        assert C.same(out.cpu(), want), how
    # every slot of a user carries its weight to exactly one class: the rows sum to the mean listed weight (float64, loosely)
    total = torch.where(lists >= 0, w.double()[None, None, :], torch.zeros((), dtype=torch.float64)).sum(dim=(1, 2)) / L
    assert torch.allclose(out.cpu().double().sum(dim=1), total, rtol=1e-5, atol=1e-6)


def test_exposure_values_flags_and_edges():
    from newsreclib_amd import ops
    B, L, k, V, S = 6, 5, 9, 40, 7
    lists, cls = _exposure_case(B, L, k, V, S, seed=3)
    lists[1] = -1                                                 # a user with empty lists: no exposure at all
    lists[3, 0, 0], lists[4, 1, 1] = 5, 6                         # (the rows whose class is made odd below are listed)
    for how in ("rbp", "dcg", "random"):
        w = _weights(k, how)
        out, status = ops.list_class_exposure(lists.cuda(), cls.cuda(), w.cuda(), S)
        assert int(status) == 0 and C.same(out.cpu(), DR.exposure(lists, cls, w, S)[0]) and bool((out[1] == 0).all())
        # a row outside the table: flagged, no mass
        outside = lists.clone()
        outside[0, 0, 0], outside[2, 4, 8] = V, -2
        got, status = ops.list_class_exposure(outside.cuda(), cls.cuda(), w.cuda(), S)
        want, flags = DR.exposure(outside, cls, w, S)
        assert int(status) == flags == DR.E_ROW and C.same(got.cpu(), want)
        # a class outside [0, S): flagged, no mass
        odd = cls.clone()
        odd[5], odd[6] = S, -1
        got, status = ops.list_class_exposure(lists.cuda(), odd.cuda(), w.cuda(), S)
        want, flags = DR.exposure(lists, odd, w, S)
        assert int(status) == flags == DR.E_CLASS and C.same(got.cpu(), want)
        got, status = ops.list_class_exposure(outside.cuda(), odd.cuda(), w.cuda(), S)
        assert int(status) == DR.E_ROW | DR.E_CLASS and C.same(got.cpu(), DR.exposure(outside, odd, w, S)[0])
    # k = 1, L = 1; (B, k) lists are one list per user; int64 classes
    one = torch.tensor([[[3]], [[-1]], [[0]]])
    w = torch.tensor([0.3])
    for given in (one, one[:, 0]):
        got, status = ops.list_class_exposure(given.cuda(), cls.long().cuda(), w.cuda(), S)
        assert int(status) == 0 and C.same(got.cpu(), DR.exposure(one, cls, w, S)[0])
    assert float(got[0, int(cls[3])]) == float(w[0]) and float(got[1].sum()) == 0.0
    got, status = ops.list_class_exposure(one[:0].cuda(), cls.cuda(), w.cuda(), S)
    assert got.shape == (0, S) and int(status) == 0


# ---- 10. exposure_report ----------------------------------------------------------------------------------------------------------------
def test_exposure_report_is_the_reduction_of_sample_recommendations_lists():
    import warnings

    from newsreclib_amd import ops
    from newsreclib_amd.evaluation import exposure_report, exposure_weights, sample_recommendations
    mod, cache, lists, hist, hs, uidx = _cache_case(late_fusion=True)
    k, draws = 5, 20
    eligible = torch.ones(50, dtype=torch.uint8)
    eligible[0] = 0
    users = [{"hist": lists[b], "user_idx": uidx[b], "user_id": 10 + b} for b in range(6)]
    drawn = sample_recommendations(cache, users, k, draws, 2.0, 16, batch_size=4, eligible=eligible)
    cls = cache.table.attrs["category"].to(torch.int32)
    S = int(cls.max()) + 1
    for how in ("rbp", "dcg", torch.tensor([1.0, 0.0, 0.5, 0.0, 0.25])):
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            report = exposure_report(cache, users, k, draws, 2.0, 16, "category", weights=how, batch_size=4, eligible=eligible)
        want = ops.list_class_exposure(drawn.cuda(), cls, exposure_weights(k, how).cuda(), S)[0].cpu()
        assert report["per_user"].shape == (6, S) and not report["per_user"].is_cuda and C.same(report["per_user"], want)
        assert C.same(report["mean"], want.double().mean(dim=0).float())
        assert report["share"].shape == (S,) and abs(float(report["share"].double().sum()) - 1.0) < 1e-6
        assert float(report["share"][0]) == 0.0                   # (the categories of the tiny table start at 1)
    assert exposure_report(cache, [], k, draws, 2.0, 16, "category")["per_user"].shape == (0, S)
