"""Encode-once NPA evaluation (``evaluation.NpaFeatureCache``: cached conv feature maps + ``nrl_npa_cached_scores``) against the
reference goldens, the module's own ``torch.no_grad()`` forward and the CPU oracle, under both GEMM engines."""
import numpy as np
import pytest
import torch

from tests import npa_oracle as NO
from tests.helpers import batch_to, load_golden

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True, params=["f32", "bf16x3"])
def engine(request):
    from newsreclib_amd import _lib
    prev = _lib.get_gemm_engine()
    _lib.set_gemm_engine(request.param)
    yield request.param
    _lib.set_gemm_engine(prev)


def _tols(engine):
    return (2e-5, 2e-4) if engine == "f32" else (1e-4, 5e-4)


# ---- 1. reference parity from the existing goldens -------------------------------------------------------------------------
def _golden_cached_scores(g, cfg, prefix=""):
    """The golden batch re-expressed as index lists into a SHUFFLED news table: a scorer that ignores the indices fails."""
    from newsreclib_amd.evaluation import DeviceNewsTable
    batch = NO.golden_batch(g, prefix)
    B, nh = batch["batch_size"], batch["batch_hist"].shape[0]
    titles = torch.cat([batch["x_hist"]["title"], batch["x_cand"]["title"]])
    perm = torch.randperm(titles.shape[0], generator=torch.Generator().manual_seed(11))
    inv = torch.argsort(perm)                            # original row i sits at table row inv[i]
    assert not torch.equal(inv, torch.arange(titles.shape[0]))
    table = DeviceNewsTable({"title": titles[perm]}, device="cuda")
    mod = NO.build_module(cfg, NO.golden_params(cfg)).eval()
    cache = mod.feature_cache(table)
    scores = cache.scores(inv[:nh], torch.bincount(batch["batch_hist"], minlength=B), inv[nh:],
                          torch.bincount(batch["batch_cand"], minlength=B), batch["user_idx"])
    return scores.cpu()


def test_cached_scores_match_reference_golden(engine):
    g = load_golden("npa_tiny_eval")
    got = _golden_cached_scores(g, NO.golden_cfg(g))
    err = float((got - torch.from_numpy(g["out_scores"])).abs().max())
    print(f"npa_tiny_eval [{engine}]: max |cached - reference| = {err:.3e}")
    assert err <= 1e-4                                   # the module test's bound, under a 1e-3 contract


def test_cached_scores_keep_the_max_hist_quirk(engine):
    g = load_golden("npa_quirk")
    cfg = NO.golden_cfg(g)
    got = {}
    for tag in ("small", "big"):
        got[tag] = _golden_cached_scores(g, cfg, tag + "/")
        err = float((got[tag] - torch.from_numpy(g[tag + "/out_scores"])).abs().max())
        print(f"npa_quirk/{tag} [{engine}]: max |cached - reference| = {err:.3e}")
        assert err <= 1e-4, tag
    n = got["small"].shape[1]
    assert float((got["small"] - got["big"][:2, :n]).abs().max()) > 1e-3


# ---- 2. cached path against the module's own no_grad forward ---------------------------------------------------------------
HIST_SIZES, CAND_SIZES = [1, 3, 0, 9, 2], [1, 2, 11, 1, 4]
USER_IDX = [1, 4, 1, 2, 5]                               # user 1 twice
NUM_NEWS = 24


def _synthetic(L, F_, late_fusion=False, hist_sizes=HIST_SIZES, seed=0, D=12, num_news=NUM_NEWS, cand_sizes=CAND_SIZES,
               user_idx=USER_IDX, device="cuda"):
    from newsreclib_amd.evaluation import DeviceNewsTable
    vocab, n_users = 60, 7
    cfg = dict(vocab=vocab, n_users=n_users, D=D, U=6, F=F_, W=3, Pw=8, Pn=8, late_fusion=late_fusion)
    params = NO.make_npa_params(vocab, n_users, D, 6, F_, 3, 8, 8, late_fusion=late_fusion, seed=seed)
    gen = torch.Generator().manual_seed(100 + seed)
    titles = torch.randint(1, vocab, (num_news, L), generator=gen)
    titles[:, L - 2:] *= (torch.rand(num_news, 2, generator=gen) > 0.5)        # some pad tokens (id 0) at the end
    hist_idx = torch.randint(0, num_news, (sum(hist_sizes),), generator=gen)
    cand_idx = torch.randint(0, num_news, (sum(cand_sizes),), generator=gen)
    cand_idx[3] = hist_idx[1]                            # one news both clicked and a candidate
    labels = (torch.rand(cand_idx.shape[0], generator=gen) > 0.7).float()
    mod = NO.build_module(cfg, params, device=device).eval()
    table = DeviceNewsTable({"title": titles}, device=device)
    return dict(mod=mod, table=table, params=params, titles=titles, hist_idx=hist_idx, cand_idx=cand_idx,
                hist_sizes=torch.tensor(hist_sizes), cand_sizes=torch.tensor(cand_sizes), labels=labels,
                user_idx=torch.tensor(user_idx))


def _forward(s):
    batch = s["table"].build_batch(s["hist_idx"], s["hist_sizes"], s["cand_idx"], s["cand_sizes"], s["labels"], s["user_idx"])
    with torch.no_grad():
        return s["mod"](batch)


def _cached(s, cache=None):
    cache = cache or s["mod"].feature_cache(s["table"], chunk=10)           # 3 chunks, the last one short
    return cache.scores(s["hist_idx"], s["hist_sizes"], s["cand_idx"], s["cand_sizes"], s["user_idx"])


def _padded(cand_sizes, width):
    return torch.arange(width)[None, :] >= torch.as_tensor(cand_sizes)[:, None]


@pytest.mark.parametrize("L,F_,late_fusion", [(5, 8, False), (30, 400, False), (7, 1024, False), (5, 8, True)])
def test_cached_scores_match_module_forward(L, F_, late_fusion, engine):
    """Both paths see the same conv feature bits; only the fp32 summation order of the poolings differs."""
    s = _synthetic(L, F_, late_fusion, hist_sizes=[1, 3, 1, 9, 2] if late_fusion else HIST_SIZES)
    want, got = _forward(s).cpu(), _cached(s).cpu()
    assert got.shape == want.shape == (5, max(CAND_SIZES))
    err = float((got - want).abs().max())
    print(f"(L, F) = ({L}, {F_}) late_fusion={late_fusion} [{engine}]: max |cached - forward| = {err:.3e}, "
          f"max |score| = {float(want.abs().max()):.3f}")
    assert err <= 1e-4
    assert float(want.abs().max()) > 1e-2                # (the comparison is not between zeros)
    assert bool((got[_padded(CAND_SIZES, got.shape[1])] == 0.0).all())
    if not late_fusion:                                  # the empty history: all-zero scores, as the forward
        assert bool((got[2] == 0.0).all()) and bool((want[2] == 0.0).all())


def test_cached_scores_refuse_unsupported_filter_counts():
    from newsreclib_amd import ops_npa
    z = torch.zeros(1, dtype=torch.int64, device="cuda")
    off = torch.tensor([0, 1], device="cuda")
    for F_ in (6, 1028):
        q = torch.zeros(1, F_, device="cuda")
        with pytest.raises(ValueError):
            ops_npa.npa_cached_scores(torch.zeros(2, 3, F_, device="cuda"), z, off, z, off, q, q, q, 1, 1)


# ---- 3. conv features against the CPU oracle ---------------------------------------------------------------------------------
def _check_conv_features(mod, params, ids, engine):
    want = NO._conv_features(ids, params, None, None)
    N, L, F_ = want.shape
    buf = torch.full((N + 2, L, F_), 7.0, device="cuda")          # the encoder fills a slice and nothing beside it
    got = mod.news_encoder.conv_features(ids.cuda(), out=buf[1:N + 1])
    assert got.data_ptr() == buf[1:].data_ptr()
    assert bool((buf[0] == 7.0).all()) and bool((buf[N + 1] == 7.0).all())
    err = float((got.cpu() - want).abs().max())
    print(f"conv features {tuple(want.shape)} [{engine}]: max |gpu - oracle| = {err:.3e}")
    assert err <= 10 * _tols(engine)[0]
    assert torch.equal(mod.news_encoder.conv_features(ids.cuda()), got)


def test_conv_features_match_oracle(engine):
    s = _synthetic(6, 8, D=12)
    _check_conv_features(s["mod"], s["params"], s["titles"], engine)
    g = load_golden("npa_tiny_eval")
    cfg = NO.golden_cfg(g)
    params = NO.golden_params(cfg)
    ids = torch.cat([torch.from_numpy(g["in_title_hist"]), torch.from_numpy(g["in_title_cand"])])
    _check_conv_features(NO.build_module(cfg, params).eval(), params, ids, engine)


# ---- 4. determinism ----------------------------------------------------------------------------------------------------------
def test_cached_scores_are_bit_identical_between_calls(engine):
    s = _synthetic(30, 400)
    cache = s["mod"].feature_cache(s["table"])
    assert torch.equal(_cached(s, cache), _cached(s, cache))


# ---- 5. snapshot semantics ---------------------------------------------------------------------------------------------------
def test_cache_is_a_snapshot_until_rebuilt(engine):
    s = _synthetic(5, 8)
    cache = s["mod"].feature_cache(s["table"])
    old = _cached(s, cache).clone()
    assert cache.engine == engine
    was_training = s["mod"].training
    other = NO.make_npa_params(60, 7, 12, 6, 8, 3, 8, 8, seed=5)
    s["mod"].news_encoder.cnn.weight.data.copy_(other[NO.PRE + "cnn.weight"])
    assert torch.equal(_cached(s, cache), old)           # stale on purpose: nothing is keyed on the weights
    cache.build()
    assert s["mod"].training == was_training
    new, want = _cached(s, cache), _forward(s)
    assert float((new - old).abs().max()) > 1e-3
    assert float((new - want).abs().max()) <= 1e-4


def test_build_restores_training_mode_and_ignores_dropout(engine):
    s = _synthetic(5, 8)
    a = s["mod"].feature_cache(s["table"]).build()
    s["mod"].train()
    b = s["mod"].feature_cache(s["table"]).build()
    assert s["mod"].training
    assert torch.equal(a, b)


# ---- 6. index guard ------------------------------------------------------------------------------------------------------------
def test_out_of_range_index_reads_as_a_zero_feature_map():
    """The table is a view of an allocation one row longer whose extra row is NaN: a missing guard shows as NaN and never reads
    memory the test does not own."""
    from newsreclib_amd import ops_npa
    s = _synthetic(5, 8)
    feats = s["mod"].feature_cache(s["table"]).build()
    n, dev = feats.shape[0], feats.device
    alloc = torch.full((n + 1,) + tuple(feats.shape[1:]), float("nan"), device=dev)
    alloc[:n] = feats
    zero_row = torch.cat([feats, torch.zeros_like(feats[:1])])          # row n exists and is all zero
    text_q, q_news = s["mod"].user_queries(s["user_idx"].to(dev))
    zero = torch.zeros(1, dtype=torch.int64, device=dev)
    offs = [torch.cat([zero, torch.cumsum(s[k].to(dev), 0)]) for k in ("hist_sizes", "cand_sizes")]
    hist_idx, cand_idx = s["hist_idx"].to(dev).clone(), s["cand_idx"].to(dev).clone()
    cand_idx[16] = n                                      # impression 4, slot 1
    hist_idx[6] = n                                       # impression 3's history
    hist_idx[0] = -1                                      # impression 0's only clicked news

    def run(table, fix):
        h, c = hist_idx.clone(), cand_idx.clone()
        if fix:
            h[h < 0] = n
        return ops_npa.npa_cached_scores(table, h, offs[0], c, offs[1], text_q[:5], text_q[5:], q_news, 9, 11).cpu()

    got, want = run(alloc[:n], False), run(zero_row, True)
    assert bool(torch.isfinite(got).all())
    assert torch.equal(got, want)
    assert float(got[4, 1]) == 0.0 and float(got[4].abs().max()) > 0.0 and bool((got[0] == 0.0).all())


# ---- 7. the epoch-end metrics ------------------------------------------------------------------------------------------------
EVAL_SEED = 4                                            # the oracle gap asserted below is 8.4e-3 at this seed
EVAL_NEWS = 40


def _eval_case(device):
    """12 impressions with distinct candidates each; (L, F) = (6, 64)."""
    gen = torch.Generator().manual_seed(EVAL_SEED)
    hist_sizes = torch.randint(1, 7, (12,), generator=gen).tolist()
    cand_sizes = torch.randint(2, 6, (12,), generator=gen).tolist()
    users = torch.randint(1, 7, (12,), generator=gen).tolist()
    s = _synthetic(6, 64, hist_sizes=hist_sizes, cand_sizes=cand_sizes, user_idx=users, seed=EVAL_SEED, num_news=EVAL_NEWS,
                   device=device)
    s["cand_idx"] = torch.cat([torch.randperm(EVAL_NEWS, generator=gen)[:n] for n in cand_sizes])
    s["labels"][:] = 0.0
    s["labels"][torch.tensor([0] + cand_sizes[:-1]).cumsum(0)] = 1.0           # one positive, first in every impression
    batch = s["table"].build_batch(s["hist_idx"], s["hist_sizes"], s["cand_idx"], s["cand_sizes"], s["labels"], s["user_idx"])
    return s, batch, hist_sizes, cand_sizes


def _oracle_min_gap(batch, params, cand_sizes):
    oracle = NO.npa_forward(batch_to(batch, "cpu"), params)["scores"]
    return min(float(torch.pdist(oracle[b, :n, None]).min()) for b, n in enumerate(cand_sizes))


def test_evaluate_impressions_matches_module_forward_metrics(engine):
    from newsreclib_amd.evaluation import evaluate_impressions
    from newsreclib_amd.metrics import ranking_metrics
    s, batch, hist_sizes, cand_sizes = _eval_case("cuda")
    # no ranking can flip inside the tolerance: the oracle's closest pair of scores within an impression is > 1e-3 apart
    gap = _oracle_min_gap(batch, s["params"], cand_sizes)
    assert gap > 1e-3, gap
    ho, co = np.cumsum([0] + hist_sizes), np.cumsum([0] + cand_sizes)
    impressions = [{"hist": s["hist_idx"][ho[b]:ho[b + 1]], "cand": s["cand_idx"][co[b]:co[b + 1]],
                    "labels": s["labels"][co[b]:co[b + 1]], "user_idx": s["user_idx"][b]} for b in range(12)]
    logs = evaluate_impressions(s["mod"].feature_cache(s["table"]), impressions, top_k_list=(2, 5))
    with torch.no_grad():
        loss, preds, targets, sizes, *_ = s["mod"].model_step(batch)
    want = ranking_metrics(preds, targets, sizes, (2, 5))
    assert set(logs) == {"loss"} | set(want)             # the keys the NRMS evaluation returns
    for k, v in want.items():
        assert abs(logs[k] - v) <= 1e-6, (k, logs[k], v)
    assert abs(logs["loss"] - float(loss)) <= 1e-4
