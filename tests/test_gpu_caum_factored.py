"""GPU tests of the factored CAUM evaluation (``UserEncoder.score_ragged`` / ``CAUMModule.factored_eval``): parity with the
float64 restatement (tests/caum_factored_ref.py) next to the default path's own error, the dense layout through the module and
the caches, the across-users coupling, the passes, the refusals, and the untouched default."""
import functools

import pytest
import torch

from tests import builders
from tests import caum_oracle as CO
from tests.caum_factored_ref import factored_scores
from tests.helpers import batch_to, load_golden

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True, params=["f32", "bf16x3"])
def engine(request):
    from newsreclib_amd import _lib
    prev = _lib.get_gemm_engine()
    _lib.set_gemm_engine(request.param)
    yield request.param
    _lib.set_gemm_engine(prev)


def _ftol(engine):
    return builders.head_tols(engine)[0]


def _sizes(B, lo, hi):
    """lists of lo..hi candidates, at least one user at lo and one at hi (B = 1: hi)."""
    s = [lo + (3 * b + 1) % (hi - lo + 1) for b in range(B)]
    s[0] = hi
    if B > 1:
        s[B // 2] = lo
    return s


# name -> (B, H, U, heads, F, h1, h2, candidate sizes)
CASES = {f"edges_B{B}": (B, 5, 80, 4, 40, 24, 16, _sizes(B, 1, 4)) for B in (1, 3, 17, 63, 64, 65, 130)}
CASES.update({
    "padded_head_dim": (9, 50, 48, 4, 40, 24, 16, _sizes(9, 1, 4)),             # dh 12 -> 16
    "H1": (5, 1, 64, 4, 40, 24, 16, _sizes(5, 1, 4)),                           # left = right = self
    "module_widths": (5, 3, 400, 20, 400, 400, 256, [2, 1, 3, 1, 2]),
    "tail_slot": (6, 4, 80, 4, 40, 24, 16, [1, 1, 1, 1, 1, 9]),
    "coupling": (3, 5, 80, 4, 40, 24, 16, [4, 3, 4]),
})


@functools.lru_cache(maxsize=None)
def _case(name):
    """(params, hist (B, H, U), flat candidates (n, U), offsets, float64 reference scores (n,)) on the CPU; built once and shared
    by the engines and the tests."""
    B, H, U, heads, F_, h1, h2, sizes = CASES[name]
    cfg = dict(vocab=8, n_ent=8, n_categ=4, D=8, Dh=heads, Dc=4, Ed=8, Eh=2, Q=8, N=U, F=F_, h1=h1, h2=h2)
    params = {k: v for k, v in CO.make_caum_params(cfg, seed=5).items() if k.startswith(CO.UE)}
    g = torch.Generator().manual_seed(11)
    hist = torch.randn(B, H, U, generator=g) * 0.5
    for b in range(B):
        hist[b, H - (b % (H + 1)):] = 0.0                   # zero-padded tails, an empty history among them
    cand = torch.randn(sum(sizes), U, generator=g) * 0.5
    offs = torch.tensor([0] + sizes).cumsum(0)
    ref = factored_scores(hist.double(), cand.double(), offs.tolist(), {k: v.double() for k, v in params.items()}, heads)
    return params, hist, cand, offs, ref


def _encoder(name):
    from newsreclib_amd.user_encoder_caum import UserEncoder
    B, H, U, heads, F_, h1, h2, sizes = CASES[name]
    enc = UserEncoder(news_embed_dim=U, num_filters=F_, dense_att_hidden_dim1=h1, dense_att_hidden_dim2=h2, user_vector_dim=U,
                      num_heads=heads, dropout_probability=0.2)
    enc.load_state_dict({k[len(CO.UE):]: v for k, v in _case(name)[0].items()}, strict=True)
    return enc.cuda().eval()


def _dense_cand(cand, offs, B):
    sizes = (offs[1:] - offs[:-1]).tolist()
    dense = torch.zeros(B, max(sizes), cand.shape[1])
    for b, n in enumerate(sizes):
        dense[b, :n] = cand[offs[b]:offs[b + 1]]
    return dense


def _flat(dense_scores, offs):
    sizes = (offs[1:] - offs[:-1]).tolist()
    return torch.cat([dense_scores[b, :n] for b, n in enumerate(sizes)])


@pytest.mark.parametrize("name", list(CASES))
def test_factored_scores_match_float64_restatement(name, engine):
    """Both paths against the same float64 values on the same inputs: the factored path within the module's golden bound, and
    within 3x the default path's own error (floor 1e-6 of the score scale)."""
    params, hist, cand, offs, ref = _case(name)
    enc = _encoder(name)
    B = hist.shape[0]
    got, status = enc.score_ragged(hist.cuda(), cand.cuda(), offs.cuda())
    with torch.no_grad():
        default = _flat(enc(hist.cuda(), _dense_cand(cand, offs, B).cuda(), offs.cuda()).cpu(), offs)
    assert int(status) == 0 and got.shape == ref.shape
    scale = max(1.0, float(ref.abs().max()))
    err_f = float((got.cpu().double() - ref).abs().max())
    err_d = float((default.double() - ref).abs().max())
    print(f"{name} {engine}: err_factored {err_f:.3e} err_default {err_d:.3e} |ref|max {float(ref.abs().max()):.3f}")
    assert err_f <= 20 * _ftol(engine) * scale
    assert err_f <= max(3 * err_d, 1e-6 * scale)


def _golden_module(name):
    g = load_golden(name)
    cfg = CO.golden_cfg(g)
    return g, cfg, CO.build_module(cfg, CO.golden_params(cfg)).eval()


def _table_call(batch):
    cat = lambda k: torch.cat([batch["x_hist"][k], batch["x_cand"][k]])  # noqa: E731
    nh, B = batch["batch_hist"].shape[0], batch["batch_size"]
    hs = torch.bincount(batch["batch_hist"], minlength=B)
    cs = torch.bincount(batch["batch_cand"], minlength=B)
    attrs = {k: cat(k) for k in ("title", "category", "title_entities")}
    return attrs, (torch.arange(nh), hs, torch.arange(nh, nh + batch["batch_cand"].shape[0]), cs)


def test_module_layout_cache_and_model_step(engine):
    from newsreclib_amd.evaluation import DeviceNewsTable, NewsVectorCache
    g, cfg, mod = _golden_module("caum_ragged")
    batch = CO.golden_batch(g)
    dev = batch_to(batch, "cuda")
    n_default = mod.model_step(dev)[1].shape[0]
    mod.factored_eval = True
    with torch.no_grad():
        scores = mod(dev)
    sizes = torch.bincount(batch["batch_cand"], minlength=batch["batch_size"]).tolist()
    assert scores.shape == (batch["batch_size"], max(sizes)) and int(mod.factored_status) == 0
    for b, n in enumerate(sizes):
        assert bool((scores[b, n:] == 0).all())
        assert float(scores[b, :n].abs().min()) > 0
    attrs, call = _table_call(batch)
    cache = NewsVectorCache(mod, DeviceNewsTable(attrs, device="cuda"))
    assert torch.equal(cache.scores(*call), scores)
    with torch.no_grad():
        preds = mod.model_step(dev)[1]
    assert preds.shape[0] == n_default == sum(sizes)        # what the metrics are handed
    assert torch.equal(preds, _flat(scores, torch.tensor([0] + sizes).cumsum(0)))
    assert torch.equal(cache.model_step(*call, batch["labels"])[1], preds)


def test_users_of_a_slot_are_coupled_and_slots_are_not(engine):
    name = "coupling"
    params, hist, cand, offs, ref = _case(name)
    sizes = (offs[1:] - offs[:-1]).tolist()
    enc = _encoder(name)
    before, _ = enc.score_ragged(hist.cuda(), cand.cuda(), offs.cuda())
    other = cand.clone()
    other[int(offs[0]) + 2] = torch.randn(cand.shape[1], generator=torch.Generator().manual_seed(3)) * 0.5
    after, _ = enc.score_ragged(hist.cuda(), other.cuda(), offs.cuda())
    p1 = int(offs[1]) + 2                                    # user 1, slot 2
    assert abs(float(after[p1] - before[p1])) > 1e-5
    want = factored_scores(hist.double(), other.double(), offs.tolist(), {k: v.double() for k, v in params.items()}, 4)
    assert float((after.cpu().double() - want).abs().max()) <= 20 * _ftol(engine) * max(1.0, float(want.abs().max()))
    slot2 = torch.zeros(cand.shape[0], dtype=torch.bool)
    for b, n in enumerate(sizes):
        if n > 2:
            slot2[int(offs[b]) + 2] = True
    assert torch.equal(after.cpu()[~slot2], before.cpu()[~slot2])            # every other slot: the same bits
    h2 = hist.clone()
    h2[2] = 0.0                                              # another user's history
    moved, _ = enc.score_ragged(h2.cuda(), cand.cuda(), offs.cuda())
    lo, hi = int(offs[1]), int(offs[2])
    assert float((moved[lo:hi] - before[lo:hi]).abs().min()) > 1e-5


def test_passes_agree(engine):
    """One pair per pass, a pass that ends inside a slot, and the default budget.  Measured bit-equal under both engines (a
    row of a GEMM and a pair of the attention do not depend on which other rows share the launch), so bit equality is what is
    asserted, not the 1e-5 of ``test_caum_slot_chunks_equal_one_pass``."""
    from newsreclib_amd.ops_caum import plan_pair_chunks
    name = "edges_B17"
    params, hist, cand, offs, ref = _case(name)
    enc = _encoder(name)
    H = hist.shape[1]
    args = (hist.cuda(), cand.cuda(), offs.cuda())
    whole, _ = enc.score_ragged(*args)
    single, s1 = enc.score_ragged(*args, row_budget=H)
    inside, s2 = enc.score_ragged(*args, row_budget=5 * H)
    slot_counts = [sum(1 for n in (offs[1:] - offs[:-1]).tolist() if n > i) for i in range(4)]
    ends = {sum(slot_counts[:i + 1]) for i in range(4)}
    assert any(j1 not in ends for _, j1 in plan_pair_chunks(slot_counts, H, 5 * H))
    assert int(s1) == 0 and int(s2) == 0
    print(f"passes {engine}: single {float((single - whole).abs().max()):.3e} inside {float((inside - whole).abs().max()):.3e}")
    assert torch.equal(single, whole)
    assert torch.equal(inside, whole)


def test_at_most_one_read_back_per_call(engine):
    """``score_ragged`` reads the per-slot pair counts back and nothing else: under torch's sync debug mode at most one
    synchronising call is reported for a call of several passes (a torch build that does not report them reports none)."""
    import warnings
    params, hist, cand, offs, ref = _case("edges_B17")
    enc = _encoder("edges_B17")
    args = (hist.cuda(), cand.cuda(), offs.cuda())
    enc.score_ragged(*args, row_budget=5 * hist.shape[1])     # (first use: library load, allocator warm-up)
    torch.cuda.synchronize()
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            got, status = enc.score_ragged(*args, row_budget=5 * hist.shape[1])
        finally:
            torch.cuda.set_sync_debug_mode("default")
    syncs = [w for w in seen if "called a synchronizing" in str(w.message)]      # (not the mode's own "prototype feature" notice)
    assert len(syncs) <= 1, [str(w.message) for w in syncs]
    assert int(status) == 0 and torch.equal(got, enc.score_ragged(*args)[0])


def test_training_mode_with_dropout_is_refused(engine):
    params, hist, cand, offs, ref = _case("edges_B3")
    enc = _encoder("edges_B3").train()
    with pytest.raises(ValueError):
        enc.score_ragged(hist.cuda(), cand.cuda(), offs.cuda())


def test_decreasing_offsets_set_the_status_and_score_zero(engine):
    from newsreclib_amd import ops_caum
    params, hist, cand, offs, ref = _case("edges_B3")
    enc = _encoder("edges_B3")
    bad = offs.clone()
    bad[1], bad[2] = offs[2], offs[1]                        # offsets that go down
    assert bool((bad[1:] < bad[:-1]).any())
    got, status = enc.score_ragged(hist.cuda(), cand.cuda(), bad.cuda())
    assert int(status) & ops_caum.STATUS_BAD_OFFSETS and bool((got == 0).all())


def test_kernel_range_checks_zero_the_pair(engine):
    """The attention kernel handed offsets that disagree with its pair list: the pairs that fail their checks come back as
    zeros with the status bit, the others are finite."""
    from newsreclib_amd import ops_caum
    B, H, heads, dh = 3, 2, 2, 16
    W = 3 * heads * dh
    g = torch.Generator().manual_seed(2)
    qkv_h, qkv_c = torch.randn(B * H, W, generator=g).cuda(), torch.randn(5, W, generator=g).cuda()
    # sizes 2, 1, 2: slot-major pairs (row, user) = (0, 0) (2, 1) (3, 2) | (1, 0) (4, 2)
    pair_row, pair_user = torch.tensor([0, 2, 3, 1, 4]).cuda(), torch.tensor([0, 1, 2, 0, 2]).cuda()
    tab, items = ops_caum.pair_chunk_table([3, 2], 0, 5, H, heads)
    tab = torch.tensor(tab, dtype=torch.int32).cuda()
    outs = []
    for offsets in ([0, 2, 3, 5], [0, 3, 2, 5]):
        status = torch.zeros(1, dtype=torch.int32, device="cuda")
        o = ops_caum.caum_eval_attn(qkv_h, qkv_c, torch.tensor(offsets).cuda(), pair_row, pair_user, tab, items, B, H, 0, 5,
                                    heads, dh, 0.25, status)
        outs.append((o.reshape(5, H, heads * dh).cpu(), int(status)))
    (good, s_good), (bad, s_bad) = outs
    assert s_good == 0 and float(good.abs().sum(dim=(1, 2)).min()) > 0 and bool(torch.isfinite(good).all())
    assert s_bad == ops_caum.STATUS_BAD_INDEX and bool(torch.isfinite(bad).all())
    # user 1's offsets go down and user 2's list no longer starts at its pairs' rows: their pairs are zeros
    assert bool((bad[[1, 2, 4]] == 0).all())
    assert float(bad[[0, 3]].abs().sum(dim=(1, 2)).min()) > 0


def test_late_fusion_ignores_the_attribute(engine):
    g, cfg, mod = _golden_module("caum_tiny_late_fusion")
    batch = batch_to(CO.golden_batch(g), "cuda")
    with torch.no_grad():
        a = mod(batch)
        mod.factored_eval = True
        b = mod(batch)
    assert torch.equal(a, b) and not hasattr(mod, "factored_status")


def test_default_path_is_untouched(engine):
    from newsreclib_amd.caum_module import CAUMModule
    assert CAUMModule.factored_eval is False
    g, cfg, mod = _golden_module("caum_tiny_eval")
    batch = batch_to(CO.golden_batch(g), "cuda")
    with torch.no_grad():
        before = mod(batch)
        mod.factored_eval = True
        factored = mod(batch)
        mod.factored_eval = False
        after = mod(batch)
    assert torch.equal(before, after)
    assert float((factored - before).abs().max()) <= 1e-4 and int(mod.factored_status) == 0
