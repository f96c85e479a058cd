"""GPU parity of the MINER module (newsreclib_amd.miner_module) against the golden vectors made from the reference's own
components, under both GEMM engines, plus its training / evaluation behaviour.

Bounds: head-only quantities take ``_tols`` (test_gpu_caum.py: 5e-5 absolute / 5e-4 relative under f32, 1e-4 / 1e-3 under
bf16x3) and ``check_lstur_grads(rtol=2e-3, atol=1e-5)``; fixtures that run the tiny transformer body take the bounds of the
``plm_tiny`` test of test_gpu_parity.py: 2e-4 ABSOLUTE on every output (scores, loss, user vectors, news vectors), 5e-4
relative on gradients.  (The ``no_reduce`` fixture runs the body with its last LayerNorm scaled by 0.25,
``tests/miner_oracle.make_body``: at the unscaled body its scores reach 75 and the bf16x3 engine measured 2.9e-4 there.)"""
import numpy as np
import pytest
import torch

from oracle import losses_oracle as LO
from oracle.nrms_oracle import to_dense_batch
from tests import builders
from tests import miner_oracle as MO
from tests.helpers import batch_to, check_lstur_grads, load_golden, make_tiny_roberta, module_grads

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True, params=["f32", "bf16x3"])
def engine(request):
    from newsreclib_amd import _lib
    prev = _lib.get_gemm_engine()
    _lib.set_gemm_engine(request.param)
    yield request.param
    _lib.set_gemm_engine(prev)


def _close(got, ref, atol, rtol):
    got, ref = torch.as_tensor(got).detach().cpu().double(), torch.as_tensor(ref).double()
    err = float((got - ref).abs().max())
    assert err <= atol + rtol * float(ref.abs().max()), (err, float(ref.abs().max()))


def _dense(preds, sizes, shape):
    dense = np.zeros(shape, dtype=np.float32)
    p, o = preds.detach().cpu().numpy(), 0
    for b, n in enumerate(sizes.cpu().numpy()):
        dense[b, :n] = p[o:o + n]
        o += n
    return dense


def _cpu_oracle(mod, cfg, tmp_path):
    """(body, params) on the CPU holding the module's CURRENT weights."""
    from transformers import AutoModel
    body = AutoModel.from_pretrained(MO.make_body(str(tmp_path), cfg)).eval()
    sd = {k: v.detach().cpu().clone() for k, v in mod.state_dict().items()}
    pre = MO.TXT + "plm_model."
    res = body.load_state_dict({k[len(pre):]: v for k, v in sd.items() if k.startswith(pre)}, strict=False)
    assert not res.unexpected_keys
    for name, prm in body.named_parameters():
        prm.requires_grad = not any(f"layer.{i}." in name for i in MO.BODY_FROZEN)
    return body, {k: v.requires_grad_(True) for k, v in sd.items() if not k.startswith(pre)}


@pytest.mark.parametrize("name", MO.MINER_TINY_CASES)
def test_miner_module_matches_reference_golden(name, engine, tmp_path, monkeypatch):
    g, cfg, mod = builders.miner_golden_module(name, tmp_path, monkeypatch)
    seen = {}
    fwd = mod.forward
    mod.forward = lambda *a, **kw: seen.setdefault("out", fwd(*a, **kw))
    enc = mod.news_encoder.forward
    mod.news_encoder.forward = lambda *a, **kw: seen.setdefault("news", []).append(enc(*a, **kw)) or seen["news"][-1]
    batch = batch_to(MO.golden_batch(g), "cuda")
    loss, preds, targets, cand_news_size, *_ = mod.model_step(batch)
    ref = g["out_scores"]
    got = _dense(preds, cand_news_size, ref.shape)
    print(name, engine, "scores err", float(np.abs(got - ref).max()), "of", float(np.abs(ref).max()),
          "loss", float(loss.detach()), float(g["out_loss"]))
    assert float(np.abs(got - ref).max()) <= 2e-4
    assert abs(float(loss.detach()) - float(g["out_loss"])) <= 2e-4
    uv = seen["out"][1].detach().cpu().numpy()
    assert float(np.abs(uv - g["out_user_vector"]).max()) <= 2e-4
    for vec, key in zip(seen["news"], ("out_hist_vec", "out_cand_vec")):
        assert float(np.abs(vec.detach().cpu().numpy() - g[key]).max()) <= 2e-4, key
    loss.backward()
    grads = module_grads(mod)
    assert {k[len("gnorm/"):] for k in g if k.startswith("gnorm/")} <= set(grads)
    check_lstur_grads(g, grads, tol=5e-4, rtol=2e-3, atol=1e-5)


def _head_inputs(g, cfg):
    hist_vec, cand_vec, batch, _ = MO.head_full_case(g, cfg)
    return hist_vec, cand_vec, batch


def test_miner_head_matches_reference_golden_at_config_widths(engine, tmp_path, monkeypatch):
    """User encoder, category bias, target-aware scorer and disagreement loss at the miner.yaml widths (D = 256, K = 32,
    Cd = 200, 200 candidates, histories 50 / 23 / 1 / 37), forward and every gradient."""
    from newsreclib_amd.nrms_module import prepare_batch
    g, cfg, mod = builders.miner_golden_module("miner_head_full", tmp_path, monkeypatch)
    hist_vec, cand_vec, batch = _head_inputs(g, cfg)
    hv, cv = hist_vec.cuda().requires_grad_(True), cand_vec.cuda().requires_grad_(True)
    pb = prepare_batch(batch_to(batch, "cuda"))
    scores, uv = mod.score_news_vectors(hv, cv, pb, seed=cfg["seed"], with_aux=True)
    loss = mod._loss(scores, torch.from_numpy(g["out_y_true"]).cuda(), pb) + mod._aux_loss(pb, uv)
    ftol, gtol = builders.head_tols(engine)
    stride = int(g["cfg_sample_stride"])
    print("head", engine, "scores err", float((scores.detach().cpu() - torch.from_numpy(g["out_scores"])).abs().max()),
          "loss", float(loss.detach()), float(g["out_loss"]))
    _close(scores, g["out_scores"], ftol, gtol)
    _close(loss, g["out_loss"], ftol, gtol)
    _close(uv.reshape(-1)[::stride], g["out_user_vector"], ftol, gtol)
    sizes = torch.bincount(batch["batch_cand"])
    for b, n in enumerate(sizes.tolist()):
        assert bool((scores[b, n:] == 0).all())
    loss.backward()
    check_lstur_grads(g, module_grads(mod), tol=gtol, rtol=2e-3, atol=1e-5)
    for t, key in ((hv, "gin_hist_vec"), (cv, "gin_cand_vec")):
        ref = torch.from_numpy(g[key])
        err = float((t.grad.cpu().reshape(-1)[::stride] - ref).abs().max())
        assert err <= gtol * max(1.0, float(ref.abs().max())), (key, err)


@pytest.mark.parametrize("max_hist", [50, 64])
def test_closed_form_padded_rows_equal_materialised_rows(max_hist, engine):
    """``PolyFn`` never sees a padded row; the reference's dense run (tests/miner_oracle.poly_attention, padded rows in the
    softmax with logit 1e-30) gives the same user vectors and gradients, at the batch's own max_hist and at a wider one."""
    from newsreclib_amd import ops_miner
    from newsreclib_amd.ops_blocks import LinearActFn
    torch.manual_seed(5)
    sizes = torch.tensor([50, 3, 1, 17])
    B, D, Cd, K = 4, 64, 24, 8
    bh = torch.repeat_interleave(torch.arange(B), sizes)
    E = (torch.randn(int(sizes.sum()), D) * 0.5).requires_grad_(True)
    W, codes = (torch.randn(Cd, D) * 0.2).requires_grad_(True), (torch.randn(K, Cd) * 0.5).requires_grad_(True)
    bias = (torch.randn(int(sizes.sum())) * 0.3).requires_grad_(True)
    d_out = torch.randn(B, K, D)
    dense, mask = to_dense_batch(E, bh, B, max_hist)
    bd, _ = to_dense_batch(bias, bh, B, max_hist)
    want, _ = MO.poly_attention(dense, mask, W, codes, bd.unsqueeze(2))
    (want * d_out).sum().backward()
    dev = [t.detach().cuda().requires_grad_(True) for t in (E, W, codes, bias)]
    off = torch.cat([torch.zeros(1, dtype=torch.int64), sizes.cumsum(0)]).cuda()
    P = LinearActFn.apply(dev[0], dev[1], torch.zeros(Cd, device="cuda"), "tanh", None)
    got = ops_miner.PolyFn.apply(dev[0], P, dev[2], dev[3], off, B, max_hist)
    (got * d_out.cuda()).sum().backward()
    ftol, gtol = builders.head_tols(engine)
    _close(got, want.detach(), ftol, gtol)
    for a, b, name in zip(dev, (E, W, codes, bias), ("E", "W", "codes", "bias")):
        _close(a.grad, b.grad, 1e-5, gtol)


@pytest.mark.parametrize("score_type", MO.SCORE_TYPES)
def test_scores_over_300_candidates_in_tiles(score_type, engine):
    """An evaluation impression with 300 candidates beside one with 7: forward and backward of all three aggregations against
    the dense restatement; padded slots score exactly 0."""
    from newsreclib_amd import ops_miner
    from newsreclib_amd.ops_blocks import LinearFn
    torch.manual_seed(11)
    sizes = torch.tensor([300, 7])
    B, D, K = 2, 64, 8
    bc = torch.repeat_interleave(torch.arange(B), sizes)
    cand = (torch.randn(int(sizes.sum()), D) * 0.4).requires_grad_(True)
    uv = (torch.randn(B, K, D) * 0.4).requires_grad_(True)
    wt = (torch.randn(D, D) * 0.2).requires_grad_(True)
    d_out = torch.randn(B, 300)
    dense, mask = to_dense_batch(cand, bc, B)
    want = MO.aggregate(dense @ uv.permute(0, 2, 1), score_type, uv, dense, wt)
    (want * d_out * mask).sum().backward()
    c, u, w = (t.detach().cuda().requires_grad_(True) for t in (cand, uv, wt))
    off = torch.cat([torch.zeros(1, dtype=torch.int64), sizes.cumsum(0)]).cuda()
    z = LinearFn.apply(u.reshape(B * K, D), w, torch.zeros(D, device="cuda"), None).view(B, K, D) \
        if score_type == "weighted" else None
    got = ops_miner.ScoreFn.apply(c, u, z, off, B, 300, score_type)
    assert bool((got[1, 7:] == 0).all())
    (got * d_out.cuda()).sum().backward()
    ftol, gtol = builders.head_tols(engine)
    _close(got, (want * mask).detach(), ftol, gtol)
    _close(c.grad, cand.grad, 1e-5, gtol)
    _close(u.grad, uv.grad, 1e-5, gtol)
    if score_type == "weighted":
        _close(w.grad, wt.grad, 1e-5, gtol)


def test_miner_batch_of_one_and_full_histories(engine, tmp_path):
    g, cfg, mod = builders.miner_golden_module("miner_tiny_eval", tmp_path)
    body, params = _cpu_oracle(mod, cfg, tmp_path)
    batch = MO.golden_batch(g)
    one = {"batch_hist": torch.zeros(5, dtype=torch.int64), "batch_cand": torch.zeros(7, dtype=torch.int64),
           "labels": batch["labels"][5:12], "batch_size": 1, "user_idx": torch.arange(1), "user_ids": torch.arange(1) + 1,
           "x_hist": {"category": batch["x_hist"]["category"][2:7],
                      "title": {k: v[2:7] for k, v in batch["x_hist"]["title"].items()}},
           "x_cand": {"category": batch["x_cand"]["category"][5:12],
                      "title": {k: v[5:12] for k, v in batch["x_cand"]["title"].items()}}}
    full = dict(batch, batch_hist=torch.repeat_interleave(torch.arange(4), 3), batch_size=4)          # 12 rows: 3 per user
    head = [k for k in params if not k.startswith(MO.TXT)]
    for b, shape in ((one, (1, 7)), (full, (4, 7))):          # (both have no padded history row: the pad == 0 branch)
        mod.zero_grad()
        for p in params.values():
            p.grad = None
        scores, uv = mod(batch_to(b, "cuda"))
        want = MO.miner_forward(b, body, params, cfg)
        assert scores.shape == shape
        assert float((scores.detach().cpu() - want["scores"].detach()).abs().max()) <= 2e-4
        assert float((uv.detach().cpu() - want["user_vector"].detach()).abs().max()) <= 2e-4
        d = torch.randn(shape, generator=torch.Generator().manual_seed(3))
        ((scores * d.cuda()).sum() + uv.square().sum()).backward()
        ((want["scores"] * d).sum() + want["user_vector"].square().sum()).backward()
        grads = module_grads(mod)
        for k in head:
            ref = params[k].grad
            err = float((grads[k].detach().cpu() - ref).abs().max())
            assert err <= 5e-4 * max(1.0, float(ref.abs().max())), (k, shape, err)


def test_miner_padded_candidates_score_exactly_zero(engine, tmp_path):
    for name in ("miner_tiny_eval", "miner_tiny_max", "miner_tiny_mean", "miner_tiny_late_fusion"):
        g, cfg, mod = builders.miner_golden_module(name, tmp_path)
        mod.eval()
        batch = MO.golden_batch(g)
        with torch.no_grad():
            scores = mod(batch_to(batch, "cuda"))[0].cpu()
        sizes = torch.bincount(batch["batch_cand"], minlength=batch["batch_size"])
        assert int(sizes.min()) < scores.shape[1]
        for b, n in enumerate(sizes.tolist()):
            assert bool((scores[b, n:] == 0).all())
            assert float(scores[b, :n].abs().min()) > 0


def test_miner_steps_are_bit_reproducible(engine, tmp_path, monkeypatch):
    """Two identical steps: identical loss, and bit-identical gradients of the three parameters whose gradients are reductions
    over users in the MINER kernels (context codes, the poly projection, the target-aware projection: fixed-order two-pass
    reductions).  ``reduce_dim``, the category table and the transformer body keep the library's existing paths (the GEMM
    engines' split-K weight gradients, the sorted-segment table gradient), which add partial sums atomically."""
    runs = []
    for _ in range(2):
        g, cfg, mod = builders.miner_golden_module("miner_tiny_train", tmp_path, monkeypatch)
        loss = mod.model_step(batch_to(MO.golden_batch(g), "cuda"))[0]
        loss.backward()
        runs.append((loss.detach().cpu(), {k: v.detach().cpu().clone() for k, v in module_grads(mod).items()}))
    assert torch.equal(runs[0][0], runs[1][0])
    for k in runs[0][1]:
        a, b = runs[0][1][k], runs[1][1][k]
        if k in ("user_encoder.context_codes", "user_encoder.linear.weight", "target_aware_attn.linear.weight"):
            assert float(a.abs().max()) > 0 and torch.equal(a, b), k
        else:
            assert float((a - b).abs().max()) <= 1e-5 * max(1.0, float(a.abs().max())), k


def test_miner_dual_loss_step_matches_oracle(engine, tmp_path):
    from newsreclib_amd.nrms_module import prepare_batch
    g = load_golden("miner_tiny_eval")
    cfg = MO.golden_cfg(g)
    mod = MO.build_module(cfg, MO.golden_params(cfg), MO.make_body(str(tmp_path), cfg), dual_loss_training=True,
                          dual_loss_coef=0.3, loss="dual_loss").eval()
    batch = MO.golden_batch(g)
    got = mod.model_step(prepare_batch(batch_to(batch, "cuda")))[0]
    # the reference on the CPU, independent of the module: the oracle's forward, the losses oracle, autograd
    body, params = _cpu_oracle(mod, cfg, tmp_path)
    out = MO.miner_forward(batch, body, params, cfg)
    y_true, mask = to_dense_batch(batch["labels"], batch["batch_cand"], batch["batch_size"])
    want = LO.dual_loss(out["scores"], y_true, mask, 0.3) + out["disagreement"]
    assert abs(float(got.detach()) - float(want.detach())) <= 2e-4
    got.backward()
    want.backward()
    grads = module_grads(mod)
    for k, p in params.items():
        ref = p.grad if p.grad is not None else torch.zeros_like(p)
        err = float((grads[k].detach().cpu() - ref).abs().max())
        assert err <= 5e-4 * max(1.0, float(ref.abs().max())), (k, err)
    k = MO.TXT + "plm_model.embeddings.word_embeddings.weight"
    ref = body.embeddings.word_embeddings.weight.grad
    assert float((grads[k].detach().cpu() - ref).abs().max()) <= 5e-4 * max(1.0, float(ref.abs().max()))


def test_miner_frozen_body_layers_get_no_gradient(engine, tmp_path, monkeypatch):
    g, cfg, mod = builders.miner_golden_module("miner_tiny_train", tmp_path, monkeypatch)
    mod.model_step(batch_to(MO.golden_batch(g), "cuda"))[0].backward()
    frozen = [(k, p) for k, p in mod.named_parameters() if any(f"layer.{i}." in k for i in MO.BODY_FROZEN)]
    assert frozen and all(not p.requires_grad and p.grad is None for _, p in frozen)
    grads = module_grads(mod)
    assert float(grads[MO.TXT + "plm_model.embeddings.word_embeddings.weight"].norm()) > 0
    assert float(grads[MO.TXT + "plm_model.encoder.layer.1.attention.self.query.weight"].norm()) > 0


def _adam_oracle_step(mod, cfg, batch, tmp_path, lr):
    body, params = _cpu_oracle(mod, cfg, tmp_path)
    train = list(params.values()) + [p for p in body.parameters() if p.requires_grad]
    opt = torch.optim.Adam(train, lr=lr)
    out = MO.miner_forward(batch, body, params, cfg, p=cfg["p_drop"], seed=cfg["seed"])
    out["loss"].backward()
    opt.step()
    want = {k: v.detach() for k, v in params.items()}
    want.update({MO.TXT + "plm_model." + k: v.detach() for k, v in body.state_dict().items()})
    return float(out["loss"].detach()), want


def test_miner_trainer_step_matches_oracle_adam_and_refreshes_images(engine, tmp_path, monkeypatch):
    """One ``NRMSTrainer`` step against the oracle's Adam step from the same weights (the criterion of ``smoke()``: an element
    whose gradient is rounding noise may step the other way, 2 lr apart); then evaluation, a second step and evaluation again,
    each against the oracle at the module's CURRENT weights -- nothing derived from a weight (matrix-core images of the body's
    and the head's projections) may survive the optimizer's write."""
    from newsreclib_amd.trainer import NRMSTrainer
    g, cfg, mod = builders.miner_golden_module("miner_tiny_train", tmp_path, monkeypatch)
    batch = MO.golden_batch(g)
    lr = 1e-4
    trainer = NRMSTrainer(mod, lr=lr)
    for step in range(2):
        if step == 0:
            want_loss, want = _adam_oracle_step(mod, cfg, batch, tmp_path, lr)
        mod.train()
        mod.news_encoder.text_encoders["title"].plm_model.eval()
        loss = float(trainer.step(batch_to(batch, "cuda")))
        trainer.flush()
        torch.cuda.synchronize()
        if step == 0:
            assert abs(loss - want_loss) <= 1e-3, (loss, want_loss)
            worst, off, total = 0.0, 0, 0
            for k, p in mod.named_parameters():
                if "pooler" in k:
                    continue
                d = (p.detach().cpu() - want[k]).abs()
                worst, off, total = max(worst, float(d.max())), off + int((d > 2e-5).sum()), total + d.numel()
            print("adam step: worst", worst, "off", off, "of", total)
            assert worst <= 2.1e-4 and off <= 0.01 * total, (worst, off, total)
        mod.eval()
        body, params = _cpu_oracle(mod, cfg, tmp_path)
        with torch.no_grad():
            scores = mod(batch_to(batch, "cuda"))[0]
            ref = MO.miner_forward(batch, body, params, cfg)["scores"]
        assert float((scores.cpu() - ref).abs().max()) <= 2e-4


@pytest.mark.parametrize("name", ["miner_tiny_eval", "miner_tiny_no_bias", "miner_tiny_late_fusion"])
def test_miner_news_vector_cache_matches_forward(name, engine, tmp_path):
    from newsreclib_amd.evaluation import DeviceNewsTable, NewsVectorCache
    g, cfg, mod = builders.miner_golden_module(name, tmp_path)
    mod.eval()
    batch, title, categ = builders.miner_table_case(g)
    table = DeviceNewsTable({"title": title, "category": categ}, device="cuda")
    nh, nc, B = batch["batch_hist"].shape[0], batch["batch_cand"].shape[0], batch["batch_size"]
    hs, cs = torch.bincount(batch["batch_hist"], minlength=B), torch.bincount(batch["batch_cand"], minlength=B)
    hi, ci = torch.arange(nh), torch.arange(nh, nh + nc)
    cache = NewsVectorCache(mod, table, chunk=5)          # several chunks, the last one short
    got = cache.scores(hi, hs, ci, cs)
    own = table.build_batch(hi, hs, ci, cs, batch["labels"])
    seen = []
    enc = mod.news_encoder.forward
    mod.news_encoder.forward = lambda *a, **kw: seen.append(enc(*a, **kw)) or seen[-1]
    with torch.no_grad():
        want = mod(own)[0]
    mod.news_encoder.forward = enc
    assert torch.equal(cache.vectors, torch.cat(seen, dim=0))
    ftol, gtol = builders.head_tols(engine)
    _close(got, want.cpu(), ftol, gtol)
    if cfg["p_drop"] == 0.0:          # (the other fixtures hold train-mode scores)
        assert float((got.cpu() - torch.from_numpy(g["out_scores"])).abs().max()) <= 2e-4


def test_cache_still_refuses_an_nrms_plm_module(tmp_path):
    from functools import partial

    from newsreclib_amd.evaluation import DeviceNewsTable, NewsVectorCache
    from newsreclib_amd.nrms_module import NRMSModule
    from tests.helpers import PLM_HEADS, PLM_Q
    mod = NRMSModule(dataset_attributes=["title", "abstract"], attributes2encode=["title"],
                     outputs={"train": ["preds", "targets", "cand_news_size"], "val": [], "test": []},
                     dual_loss_training=False, dual_loss_coef=None, loss="cross_entropy_loss", late_fusion=False,
                     temperature=None, use_plm=True, pretrained_embeddings_path=None,
                     plm_model=make_tiny_roberta(str(tmp_path)), frozen_layers=[0], embed_dim=96, num_heads=PLM_HEADS,
                     query_dim=PLM_Q, dropout_probability=0.2, top_k_list=[5, 10], num_categ_classes=18, num_sent_classes=3,
                     save_recs=False, recs_fpath=None, optimizer=partial(torch.optim.Adam, lr=1e-4), scheduler=None).cuda()
    table = DeviceNewsTable({"title": {"input_ids": torch.ones(4, 6, dtype=torch.int64),
                                       "attention_mask": torch.ones(4, 6, dtype=torch.int64)}}, device="cuda")
    with pytest.raises(NotImplementedError, match="attends across the news of one call"):
        NewsVectorCache(mod, table).build()
