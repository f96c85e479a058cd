"""MANNeR on the MI355X: the two new kernels against float64 restatements (tests/manner_oracle.py), the modules' wiring, the
encode-once evaluation and an A-Module training step.

Bounds of the kernel checks are not fixed numbers: for each case the same loss / gradient / scores are computed with torch fp32
ops on the same inputs, and that formulation's error against float64 is the yardstick.  The f32 engine may be at most 4x that error
(the factor covers the different summation order over D), the bf16x3 engine at most 3x the f32-engine bound (the ratio the
project uses between its engines: 6e-4 / 2e-4).  The measured errors are printed."""
import pytest
import torch

from tests import manner_oracle as MO
from tests.builders import (N_ENT, a_kwargs, cr_kwargs, entity_table, manner_ensemble, manner_modules, manner_news,
                            manner_table_and_impressions)
from tests.helpers import make_tiny_roberta

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(params=["f32", "bf16x3"])
def engine(request):
    from newsreclib_amd import _lib
    prev = _lib.get_gemm_engine()
    _lib.set_gemm_engine(request.param)
    yield request.param
    _lib.set_gemm_engine(prev)


_supcon_case = MO.supcon_case


def _err(a, ref):
    return float((a.double().cpu() - ref).abs().max())


@pytest.mark.parametrize("N,D,classes,T", [(85, 768, 17, 0.9), (12, 64, 4, 0.1), (3, 8, 2, 0.5), (257, 300, 5, 0.9),
                                           (1024, 1024, 18, 0.9)])
def test_supcon_embed_against_float64(N, D, classes, T, engine):
    """Measured on an MI355X (max |error| against float64; the kernel runs its two products on the exact-fp32 GEMM under both
    engine settings, so both rows of a case carry the same kernel figures):

        case                  torch-fp32 loss / grad    kernel loss / grad      f32 bound loss / grad
        (85, 768, 17, 0.9)    3.59e-08 / 3.88e-09       3.59e-08 / 3.46e-09     1.43e-07 / 1.55e-08
        (12, 64, 4, 0.1)      2.18e-08 / 4.23e-08       2.18e-08 / 2.37e-08     8.71e-08 / 1.69e-07
        (3, 8, 2, 0.5)        6.06e-09 / 3.84e-08       6.06e-09 / 3.07e-08     2.43e-08 / 1.54e-07
        (257, 300, 5, 0.9)    9.93e-08 / 1.97e-10       9.93e-08 / 2.71e-10     3.97e-07 / 7.87e-10
        (1024, 1024, 18, 0.9) 5.51e-07 / 4.07e-11       7.41e-08 / 4.35e-11     2.20e-06 / 1.63e-10

    (With dE = G E as one GEMM the last gradient was 1.93e-10, over its bound: the product is chunked over the anchors since.)"""
    from newsreclib_amd.ops_manner import supcon_embed_fwd_bwd
    E, labels = _supcon_case(N, D, classes, T)
    loss64, grad64 = MO.supcon_embed_with_grad(E, labels, T, torch.float64)
    loss32, grad32 = MO.supcon_embed_with_grad(E, labels, T, torch.float32)
    e_loss, e_grad = abs(float(loss32) - float(loss64)), _err(grad32, grad64)
    b_loss, b_grad = 4 * e_loss, 4 * e_grad
    if engine == "bf16x3":
        b_loss, b_grad = 3 * b_loss, 3 * b_grad
    Ed, ld = E.to(DEV), labels.to(DEV)
    loss, dE = supcon_embed_fwd_bwd(Ed, ld, T)
    got_loss, got_grad = abs(float(loss) - float(loss64)), _err(dE, grad64)
    print(f"supcon_embed N={N} D={D} T={T} {engine}: torch-fp32 error loss {e_loss:.3e} grad {e_grad:.3e} | kernel loss "
          f"{got_loss:.3e} (bound {b_loss:.3e}) grad {got_grad:.3e} (bound {b_grad:.3e}) | max|grad| {float(grad64.abs().max()):.3e}")
    assert got_loss <= b_loss
    assert got_grad <= b_grad
    # run-to-run bit-identical
    loss2, dE2 = supcon_embed_fwd_bwd(Ed, ld, T)
    assert torch.equal(loss, loss2) and torch.equal(dE, dE2)
    # grad_scale is linear (a power of two: exactly)
    _, dE4 = supcon_embed_fwd_bwd(Ed, ld, T, grad_scale=4.0)
    assert torch.allclose(dE4, 4.0 * dE, rtol=1e-6, atol=0.0)
    # rows and labels permuted together: the permuted result.  A permutation reorders fp32 sums of up to N terms (the row
    # reductions, the reducer, the k-order of dE = G E), so the two runs differ by rounding: 4 ulp of the fp32 loss, and
    # sqrt(N) * eps of the largest gradient entry (a random walk of N roundings), times 4.
    perm = torch.randperm(N, generator=torch.Generator().manual_seed(5))
    loss_p, dE_p = supcon_embed_fwd_bwd(Ed[perm.to(DEV)].contiguous(), ld[perm.to(DEV)].contiguous(), T)
    eps = torch.finfo(torch.float32).eps
    assert abs(float(loss_p) - float(loss)) <= 4 * eps * abs(float(loss))
    assert float((dE_p - dE[perm.to(DEV)]).abs().max()) <= 4 * eps * N ** 0.5 * float(dE.abs().max())


@pytest.mark.parametrize("labels", [[4, 4, 4, 4], [0, 1, 2, 3], [5]])
def test_supcon_embed_degenerate_cases_are_exactly_zero(labels, engine):
    from newsreclib_amd.ops_manner import supcon_embed_fwd_bwd
    E = torch.randn(len(labels), 8, generator=torch.Generator().manual_seed(1)).to(DEV)
    loss, dE = supcon_embed_fwd_bwd(E, torch.tensor(labels, device=DEV), 0.9)
    assert float(loss) == 0.0 and float(dE.abs().max()) == 0.0


def test_supcon_embed_autograd_and_singleton_class(engine):
    from newsreclib_amd.ops_manner import SupConEmbedLoss
    # three unbalanced classes with a singleton: its row has no positive and is dropped by the reducer
    labels = torch.tensor([0, 0, 0, 1, 1, 2])
    E = torch.randn(6, 16, generator=torch.Generator().manual_seed(3)) * 0.5
    loss64, grad64 = MO.supcon_embed_with_grad(E, labels, 0.5)
    assert float(MO.supcon_rows(E.double(), labels, 0.5)[5]) == 0.0
    x = E.to(DEV).requires_grad_(True)
    loss = SupConEmbedLoss(0.5)(x, labels.to(DEV))
    (2.0 * loss).backward()
    tol = 2e-4 if engine == "f32" else 6e-4
    assert abs(float(loss) - float(loss64)) <= tol * max(1.0, abs(float(loss64)))
    assert torch.allclose(x.grad.double().cpu(), 2.0 * grad64, rtol=tol, atol=tol * float(grad64.abs().max()))
    assert float(x.grad[5].abs().max()) > 0.0                # the singleton still receives gradient as a negative of others


def _ragged(B, H, C_lo, C_hi, V, seed):
    g = torch.Generator().manual_seed(seed)
    hs = torch.randint(1, H + 1, (B,), generator=g)
    cs = torch.randint(C_lo, C_hi + 1, (B,), generator=g)
    cs[0], cs[1] = C_lo, C_hi
    hist = [torch.randint(0, V, (int(n),), generator=g) for n in hs]
    cand = [torch.randperm(V, generator=g)[:int(n)] if V < 4096 else torch.randint(0, V, (int(n),), generator=g) for n in cs]
    hist[0][0], cand[0][0], cand[1][-1] = 0, V - 1, 0        # the first and the last table row are read
    hist[2][-1] = V - 1
    return hist, cand, hs, cs


def _flat(hist, cand, hs, cs):
    z = torch.zeros(1, dtype=torch.int64)
    return (torch.cat(hist).to(DEV), torch.cat([z, torch.cumsum(hs, 0)]).to(DEV), torch.cat(cand).to(DEV),
            torch.cat([z, torch.cumsum(cs, 0)]).to(DEV))


_tables = MO.random_tables


def _check_scores(tables, weights, hist, cand, hs, cs):
    from newsreclib_amd.ops_manner import manner_scores
    ref = MO.ensemble_scores([t.double() for t in tables], weights, hist, cand)
    f32 = MO.ensemble_scores(tables, weights, hist, cand)
    assert MO.min_std_ratio(tables, hist, cand) >= 1e-2
    e32 = max(float((a.double() - b).abs().max()) for a, b in zip(f32, ref) if len(b) > 1)
    bound = 4 * e32
    out = manner_scores([t.to(DEV) for t in tables], weights, *_flat(hist, cand, hs, cs), int(cs.max())).cpu()
    assert out.shape == (len(hist), int(cs.max())) and bool(torch.isfinite(out[:, 0][cs > 1]).all())
    worst = 0.0
    for b, r in enumerate(ref):
        got = out[b, :len(r)].double()
        if len(r) == 1:
            assert bool(torch.isnan(r).all()) and torch.allclose(got, r, equal_nan=True)      # the reference's NaN row
            continue
        worst = max(worst, float((got - r).abs().max()))
    print(f"manner_scores k={len(tables)} B={len(hist)} D={tables[0].shape[1]}: torch-fp32 error {e32:.3e}, kernel error "
          f"{worst:.3e}, bound {bound:.3e}")
    assert worst <= bound
    return out


@pytest.mark.parametrize("weights", [(1.0,), (1.0, -0.3), (1.0, 0.2, -0.25)])
def test_manner_scores_tiny_with_a_single_candidate_row(weights):
    V, D = 64, 32
    hist, cand, hs, cs = _ragged(6, 5, 2, 9, V, seed=2)
    cand[3], cs[3] = cand[3][:1], 1                          # one single-candidate impression: a NaN row, pinned
    # (table seed 1: the first, counting up from 1, under which every impression meets the std condition _check_scores asserts)
    out = _check_scores(_tables(len(weights), V, D, 1), list(weights), hist, cand, hs, cs)
    assert bool(torch.isnan(out[3, 0])) and bool((out[3, 1:] == 0).all())


@pytest.mark.parametrize("k", [1, 2, 3])
def test_manner_scores_mind_like(k):
    V, D = 65536, 768
    hist, cand, hs, cs = _ragged(512, 50, 2, 300, V, seed=7)
    _check_scores(_tables(k, V, D, 9), [1.0, -0.3, 0.25][:k], hist, cand, hs, cs)


# ---- modules ----------------------------------------------------------------------------------------------------------------------


def _rec_batch(hs, cs, seed=1):
    B = len(hs)
    g = torch.Generator().manual_seed(seed)
    labels = torch.cat([(torch.arange(c) == int(torch.randint(0, c, (1,), generator=g))).float() for c in cs])
    batch = {"x_hist": manner_news(sum(hs), 12, seed), "x_cand": manner_news(sum(cs), 10, seed + 1),
             "batch_hist": torch.repeat_interleave(torch.arange(B), torch.tensor(hs)).to(DEV),
             "batch_cand": torch.repeat_interleave(torch.arange(B), torch.tensor(cs)).to(DEV),
             "labels": labels.to(DEV), "user_ids": (torch.arange(B) + 1).to(DEV), "user_idx": torch.arange(B).to(DEV),
             "batch_size": B}
    for side, n in (("x_hist", sum(hs)), ("x_cand", sum(cs))):
        batch[side]["category"] = torch.randint(1, 5, (n,), generator=g).to(DEV)
        batch[side]["sentiment"] = torch.randint(1, 4, (n,), generator=g).to(DEV)
    return batch


def test_ensemble_forward_matches_the_loops(tmp_path, engine):
    cr, ac, asent = manner_modules(tmp_path)
    hs, cs = [3, 1, 4], [4, 2, 5]
    batch = _rec_batch(hs, cs)
    ens = manner_ensemble(cr, ac, asent)
    with torch.no_grad():
        scores = ens(batch).cpu()
        tables = [torch.cat([m.news_encoder(batch["x_hist"]), m.news_encoder(batch["x_cand"])]).double().cpu() for m in (cr, ac, asent)]
    ho, co = [0, 3, 4, 8], [8, 12, 14, 19]
    hist = [torch.arange(ho[b], ho[b + 1]) for b in range(3)]
    cand = [torch.arange(co[b], co[b + 1]) for b in range(3)]
    ref = MO.ensemble_scores(tables, [1.0, 0.2, -0.25], hist, cand)
    for b, r in enumerate(ref):
        assert torch.allclose(scores[b, :len(r)].double(), r, rtol=1e-4, atol=1e-4)
    assert float(scores[1, 2:].abs().max()) == 0.0
    out = ens.model_step(batch)
    assert len(out) == 10 and out[0].shape == (11,) and torch.equal(out[2].cpu(), torch.tensor(cs))
    only_cr = manner_ensemble(cr, None, None, cw=0, sw=0)
    with torch.no_grad():
        s1 = only_cr(batch).cpu()
    ref1 = MO.ensemble_scores(tables[:1], [1.0], hist, cand)
    assert all(torch.allclose(s1[b, :len(r)].double(), r, rtol=1e-4, atol=1e-4) for b, r in enumerate(ref1))


def test_vector_cache_equals_forward_and_metrics(tmp_path, engine):
    from newsreclib_amd.evaluation import MannerVectorCache, NewsVectorCache, evaluate_impressions
    from newsreclib_amd.metrics import aspect_metrics, ranking_metrics
    cr, ac, asent = manner_modules(tmp_path)
    ens = manner_ensemble(cr, ac, asent)
    table, imps = manner_table_and_impressions()
    cache = MannerVectorCache(ens, table)
    hs, cs = torch.tensor([len(i["hist"]) for i in imps]), torch.tensor([len(i["cand"]) for i in imps])
    hidx, cidx = torch.cat([i["hist"] for i in imps]), torch.cat([i["cand"] for i in imps])
    got = cache.scores(hidx, hs, cidx, cs)
    batch = table.build_batch(hidx, hs, cidx, cs, torch.cat([i["labels"] for i in imps]))
    with torch.no_grad():
        want = ens(batch)
    # The cached vector of a news is bit-identical to the one a batch computes (eval mode, rows independent) only when the GEMMs
    # see the same row count per tile; the combine layer runs over 40 table rows here and over the batch's rows there, and the
    # engines' split of the reduction does not depend on the row count, so the scores agree to rounding: 1e-6 relative.
    from newsreclib_amd.nrms_module import prepare_batch
    flat = prepare_batch(batch, None, need_order=False)["cand_flat_idx"]
    a, b = got.reshape(-1)[flat], want.reshape(-1)[flat]
    assert torch.allclose(a, b, rtol=1e-6, atol=1e-6 * float(b.abs().max()))
    # metrics: evaluate_impressions on the cache == the metric functions on the float64 loops' scores
    logs = evaluate_impressions(cache, imps, batch_size=4, top_k_list=(5, 10), num_categ_classes=5, num_sent_classes=4)
    tables = [v.double().cpu() for v in cache.vectors]
    ref = MO.ensemble_scores(tables, cache.weights, [i["hist"] for i in imps], [i["cand"] for i in imps])
    preds, targets = torch.cat(ref).float().to(DEV), torch.cat([i["labels"] for i in imps]).to(DEV)
    want_m = ranking_metrics(preds, targets, cs.to(DEV), (5, 10))
    cat, sent = table.attrs["category"], table.attrs["sentiment"]
    want_m.update(aspect_metrics(preds, cat[cidx.to(DEV)], cat[hidx.to(DEV)], cs.to(DEV), hs.to(DEV), 5, (5, 10), prefix="categ"))
    want_m.update(aspect_metrics(preds, sent[cidx.to(DEV)], sent[hidx.to(DEV)], cs.to(DEV), hs.to(DEV), 4, (5, 10), prefix="sent"))
    assert logs["loss"] == 0.0
    for k, v in want_m.items():
        assert logs[k] == pytest.approx(v, rel=1e-5, abs=1e-6), k
    # CRModule through NewsVectorCache, unchanged
    cr_cache = NewsVectorCache(cr, table)
    s = cr_cache.scores(hidx, hs, cidx, cs)
    with torch.no_grad():
        s_fwd = cr(batch)
    assert torch.allclose(s.reshape(-1)[flat], s_fwd.reshape(-1)[flat], rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("loss", ["cross_entropy_loss", "sup_con_loss"])
@pytest.mark.parametrize("late_fusion", [False, True])
def test_cr_module_train_step_runs_and_reaches_every_trainable_parameter(tmp_path, loss, late_fusion, engine):
    from newsreclib_amd.manner_cr_module import CRModule
    torch.manual_seed(5)
    mod = CRModule(**cr_kwargs(make_tiny_roberta(str(tmp_path)), loss=loss, late_fusion=late_fusion),
                   pretrained_entity_embeddings=entity_table()).to(DEV).train()
    out = mod.model_step(_rec_batch([3, 2, 4], [4, 3, 5]))
    assert len(out) == 11 and bool(torch.isfinite(out[0]))
    out[0].backward()
    grads = {n: p.grad for n, p in mod.named_parameters()}
    assert all(g is None for n, g in grads.items() if "layer.0." in n)          # frozen_layers=[0]
    assert all(bool(torch.isfinite(g).all()) for g in grads.values() if g is not None)
    must = ["news_encoder.combine_layer.weight", "news_encoder.entity_encoders.entities.additive_attention.query",
            "news_encoder.text_encoders.text.plm_model.encoder.layer.1.output.dense.weight"]
    must += [] if late_fusion else ["user_encoder.additive_attention.query"]
    assert all(grads[n] is not None and float(grads[n].abs().max()) > 0.0 for n in must)


def test_a_module_adam_lowers_the_loss(tmp_path, engine):
    from newsreclib_amd.manner_a_module import AModule
    from newsreclib_amd.synthetic import make_news_batch
    torch.manual_seed(7)
    mod = AModule(**a_kwargs(make_tiny_roberta(str(tmp_path)), temperature=0.9, p_drop=0.0),
                  pretrained_entity_embeddings=entity_table()).to(DEV).train()
    b = make_news_batch(4, 3, vocab_size=200, n_entities=N_ENT, L=12, seed=2)
    batch = {"news": {k: ({kk: vv.to(DEV) for kk, vv in v.items()} if isinstance(v, dict) else v.to(DEV))
                      for k, v in b["news"].items()}, "labels": b["labels"].to(DEV)}
    opt = torch.optim.Adam([p for p in mod.parameters() if p.requires_grad], lr=1e-3)
    losses = []
    for _ in range(5):
        opt.zero_grad(set_to_none=True)
        loss, emb, labels = mod.model_step(batch)
        loss.backward()
        opt.step()
        losses.append(float(loss))
    print("AModule losses over 5 Adam steps:", losses)
    assert emb.shape == (12, 96) and losses[-1] < losses[0]
    frozen = [(n, p) for n, p in mod.named_parameters() if not p.requires_grad]
    assert frozen and all("layer.0." in n and p.grad is None for n, p in frozen)
    mod.validation_step(batch, 0)
    assert len(mod.val_step_outputs["embeddings"]) == 1
    mod.on_validation_epoch_end()
    assert mod.val_step_outputs["embeddings"] == []
