"""GPU parity of the SentiDebias drop-in (``senti_debias_module`` / ``ops_sentidebias`` / ``trainer.SentiDebiasTrainer``) against
the goldens of the reference's components, its kernels against float64, and the two-optimizer step's cache coherence."""
from functools import partial

import numpy as np
import pytest
import torch

from tests import sentidebias_oracle as SO
from tests.helpers import batch_to, check_grads_against_golden, load_golden, module_grads
from tests.sentidebias_helpers import CASES, build_module, golden_batch, golden_params, pinned_seeds

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True, params=["f32", "bf16x3"])
def engine(request):
    from newsreclib_amd import _lib
    prev = _lib.get_gemm_engine()
    _lib.set_gemm_engine(request.param)
    yield request.param
    _lib.set_gemm_engine(prev)


def _module(g, **kw):
    p_drop = float(g["cfg_p_drop"])
    mod = build_module(golden_params(g), p_drop=p_drop, late_fusion=bool(int(g["cfg_late_fusion"])), alpha=float(g["cfg_alpha"]),
                       beta=float(g["cfg_beta"]), **kw)
    mod.train() if p_drop > 0 else mod.eval()
    return mod


def _phase_g(mod, pb, seed):
    """Phase G up to the backward, flags toggled as the train step toggles them."""
    from newsreclib_amd.dense_batch import dense_rows
    og, _ = mod.optimizers()
    mod.toggle_optimizer(og)
    with pinned_seeds([seed]):
        (combined, free, loss_orth, hv, cv), news, pb = mod.generator.forward_full(pb)
    n_hist = pb["batch_hist"].shape[0]
    adv = mod.discriminator.losses(news, pb["x_all"]["sentiment"], n_hist)
    y = dense_rows(pb["labels"], pb["batch_cand"], pb["batch_size"], pb["max_cand"], pb["cand_offsets"], pb["cand_flat_idx"],
                   max_is_exact=True).float()
    g_loss = mod.rec_loss(combined, y) + mod.hparams.beta_coefficient * loss_orth - mod.hparams.alpha_coefficient * (adv[0] + adv[1])
    return dict(combined=combined, bias_free=free, loss_orth=loss_orth, hist_vec=hv, cand_vec=cv, g_loss=g_loss, opt=og)


def _close(got, want, tol):
    return float(np.abs(got.detach().cpu().double().numpy() - want).max()) <= tol


@pytest.mark.parametrize("name", CASES)
def test_both_phases_match_reference_golden(name, engine):
    g = load_golden(name)
    mod = _module(g)
    pb = mod._prepare(batch_to(golden_batch(g), "cuda"))
    tol = 2e-4 if engine == "f32" else 6e-4
    out = _phase_g(mod, pb, int(g["cfg_seed_g"]))
    rs = int(g["cfg_row_stride"])
    assert _close(out["combined"], g["out_combined"], 1e-4) and _close(out["bias_free"], g["out_bias_free"], 1e-4)
    assert _close(out["hist_vec"][::rs], g["out_hist_vec"], 1e-4) and _close(out["cand_vec"][::rs], g["out_cand_vec"], 1e-4)
    assert abs(float(out["loss_orth"]) - float(g["out_loss_orth"])) <= 2e-4
    assert abs(float(out["g_loss"]) - float(g["out_g_loss"])) <= 2e-4 * max(1.0, abs(float(g["out_g_loss"])))
    mod.manual_backward(out["g_loss"])
    grads = module_grads(mod)
    # gradient ownership: phase G leaves every discriminator gradient None (or exactly zero)
    for k, p in mod.named_parameters():
        if k.startswith("discriminator."):
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, k
    check_grads_against_golden(g, {k: v for k, v in grads.items() if k.startswith("generator.")}, rtol=tol)
    emb = grads["generator.news_encoder.text_encoders.title.embedding_layer.weight"]
    assert float(emb[0].abs().max()) == 0.0 and float(grads["generator.sentiment_encoder.embedding_layer.weight"][0].abs().max()) == 0.0
    mod.untoggle_optimizer(out["opt"])
    mod.zero_grad(set_to_none=True)

    # phase D at the same weights
    _, od = mod.optimizers()
    mod.toggle_optimizer(od)
    with pinned_seeds([int(g["cfg_seed_d"])]):
        adv = mod.discriminator.losses(mod.generator.encode_news(pb), pb["x_all"]["sentiment"], pb["batch_hist"].shape[0])
    d_loss = adv[0] + adv[1]
    assert abs(float(d_loss) - float(g["out_d_loss"])) <= 2e-4 * max(1.0, abs(float(g["out_d_loss"])))
    mod.manual_backward(d_loss)
    for k, p in mod.named_parameters():
        if k.startswith("generator."):
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, k
    gd = {k[2:]: v for k, v in g.items() if k.startswith("d_g")}
    gd["cfg_sample_stride"] = g["cfg_sample_stride"]
    check_grads_against_golden(gd, {k: v for k, v in module_grads(mod).items() if k.startswith("discriminator.")}, rtol=tol)
    mod.untoggle_optimizer(od)


def _check_params(g, mod, scale):
    stride = int(g["cfg_sample_stride"])
    for k, p in mod.state_dict().items():
        ref = g["psample/" + k].astype(np.float64)
        got = p.detach().cpu().double().reshape(-1)[::stride].numpy()
        assert float(np.abs(got - ref).max()) <= scale, (k, float(np.abs(got - ref).max()))


def test_tiny_step_with_sgd(engine):
    g = load_golden("sentidebias_tiny_step")
    lr_g, lr_d = float(g["cfg_lr_g"]), float(g["cfg_lr_d"])
    mod = _module(g, opt_g=partial(torch.optim.SGD, lr=lr_g), opt_d=partial(torch.optim.SGD, lr=lr_d))
    batch = batch_to(golden_batch(g), "cuda")
    tol = 2e-4 if engine == "f32" else 6e-4
    with pinned_seeds(g["cfg_seeds"].tolist()):
        mod.training_step(batch, 0)
        first = [float(x) for x in mod.last_losses]
        # a parameter moved by lr * gradient: the gradient bounds (relative to a gradient of magnitude up to ~10) times the lr
        _check_params(g, mod, 10.0 * tol * max(lr_g, lr_d))
        mod.training_step(batch, 1)
        second = [float(x) for x in mod.last_losses]
    for got, want in zip(first + second, g["out_losses"].reshape(-1).tolist()):
        assert abs(got - want) <= 2e-4 * max(1.0, abs(want))
    assert len(mod.training_step_outputs["preds"]) == 2
    assert all(p.grad is None or float(p.grad.abs().max()) == 0.0 for p in mod.parameters())


def test_trainer_matches_float64_adam(engine):
    """``SentiDebiasTrainer`` (two flat fused-Adam pairs) against an independent float64 Adam (``oracle.nrms_oracle.adam_step``)
    fed the gradients of the same module under plain autograd, one whole step.  In its first step Adam moves a coordinate by
    lr * g / (|g| + eps).  Wherever |g| >= 1e-4 -- far above the run-to-run noise of the fp32 atomic accumulations in the weight
    gradients (~1e-7 of gradients of magnitude up to ~10) -- its sign is the gradient's and its size lr to within eps / |g| = 1e-4:
    there the comparison is held to 1e-3 lr plus the fp32 rounding of the stored parameter.  Everywhere else two runs can at
    worst move a coordinate by lr in opposite directions: 2 lr.  The losses are held to the loss bound."""
    from newsreclib_amd.trainer import SentiDebiasTrainer
    from oracle.nrms_oracle import adam_step
    g = load_golden("sentidebias_tiny_train")
    batch = batch_to(golden_batch(g), "cuda")
    lr_g, lr_d = 1e-3, 2e-3
    seeds = [20, 21]
    # the float64 expectation: gradients of each phase from a module without any optimizer step in between is NOT the step
    # (phase D sees phase G's update), so phase G's update is applied by the oracle before phase D's gradients are taken
    ref = _module(g)
    init = {k: v.detach().clone() for k, v in ref.state_dict().items()}
    pb = ref._prepare(batch)
    out = _phase_g(ref, pb, seeds[0])
    ref.manual_backward(out["g_loss"])
    want, g_abs = {}, {}
    for k, p in ref.named_parameters():
        if k.startswith("generator."):
            gr = p.grad.double() if p.grad is not None else torch.zeros_like(p).double()
            p64, m, v = p.detach().double().clone(), torch.zeros_like(gr), torch.zeros_like(gr)
            adam_step(p64, gr, m, v, 1, lr_g)
            want[k], g_abs[k] = p64, gr.abs()
    ref.untoggle_optimizer(out["opt"])
    ref.zero_grad(set_to_none=True)
    with torch.no_grad():
        for k, p in ref.named_parameters():
            if k in want:
                p.copy_(want[k].float())
    _, od = ref.optimizers()
    ref.toggle_optimizer(od)
    with pinned_seeds([seeds[1]]):
        adv = ref.discriminator.losses(ref.generator.encode_news(pb), pb["x_all"]["sentiment"], pb["batch_hist"].shape[0])
    d_ref = adv[0] + adv[1]
    ref.manual_backward(d_ref)
    for k, p in ref.named_parameters():
        if k.startswith("discriminator."):
            gr = p.grad.double()
            p64, m, v = p.detach().double().clone(), torch.zeros_like(gr), torch.zeros_like(gr)
            adam_step(p64, gr, m, v, 1, lr_d)
            want[k], g_abs[k] = p64, gr.abs()
    ref.untoggle_optimizer(od)

    mod = _module(g)
    mod.load_state_dict(init)
    tr = SentiDebiasTrainer(mod, lr_generator=lr_g, lr_discriminator=lr_d)
    with pinned_seeds(seeds):
        g_loss, d_loss = tr.step(batch)
    assert abs(float(g_loss) - float(out["g_loss"])) <= 2e-4 * max(1.0, abs(float(out["g_loss"])))
    assert abs(float(d_loss) - float(d_ref)) <= 2e-4 * max(1.0, abs(float(d_ref)))
    for k, p in mod.named_parameters():
        lr = lr_g if k.startswith("generator.") else lr_d
        err = (p.detach().double() - want[k]).abs()
        assert float(err.max()) <= 2 * lr + 1e-6, k
        big = g_abs[k] >= 1e-4
        if bool(big.any()):
            # (|p| up to ~5: half an ulp is 2.4e-7)
            assert float(err[big].max()) <= 1e-3 * lr + 5e-7, (k, float(err[big].max()))


@pytest.mark.parametrize("optim", ["adam", "adam_fused", "fused_flat"])
def test_caches_hold_across_the_two_phases(optim, engine):
    """After phase G's step phase D's news vectors, and the first validation forward after the step (token table), are
    ``torch.equal`` to those of a freshly built module loaded with the post-step state dict."""
    from newsreclib_amd.trainer import SentiDebiasTrainer
    g = load_golden("sentidebias_tiny_train")
    batch = batch_to(golden_batch(g), "cuda")
    kw = {} if optim != "adam_fused" else {"fused": True}
    mod = _module(g, opt_g=partial(torch.optim.Adam, lr=1e-2, **kw), opt_d=partial(torch.optim.Adam, lr=1e-2, **kw))
    if optim == "fused_flat":
        SentiDebiasTrainer(mod, lr_generator=1e-2, lr_discriminator=1e-2)
    pb = mod._prepare(batch)
    seen = {}
    enc = mod.generator.encode_news
    calls = []

    def spy(b):
        out = enc(b)
        calls.append(out.detach().clone())
        if len(calls) == 3:       # phase D's forward: the generator's weights as phase G's step left them
            seen["state"] = {k: v.detach().clone() for k, v in mod.state_dict().items()}
        return out

    mod.generator.encode_news = spy
    with pinned_seeds([32, 32]):
        mod.eval()
        with torch.no_grad():
            mod.model_step(pb)                         # a validation forward BEFORE the step (may build caches)
        mod.train()
        mod.training_step(pb, 0)
    mod.generator.encode_news = enc
    fresh = _module(g)
    fresh.load_state_dict(seen["state"])
    fresh.train()
    fresh.toggle_optimizer(fresh.optimizers()[1])      # phase D's flags: the generator's parameters are switched off
    with pinned_seeds([32]):
        want = fresh.generator.encode_news(fresh._prepare(batch))
    fresh.untoggle_optimizer(fresh.optimizers()[1])
    # phase G and phase D drew the SAME dropout mask here, so their news vectors differ only because phase G's step moved the
    # weights in between
    assert not torch.equal(calls[1], calls[2])
    assert torch.equal(calls[2], want)
    fresh.load_state_dict(mod.state_dict())
    mod.eval(), fresh.eval()
    with torch.no_grad():
        for _ in range(3):                             # (the automatic token table builds once enough positions were seen)
            got, want = mod.model_step(pb)[0], fresh.model_step(fresh._prepare(batch))[0]
            assert torch.equal(got, want)


# ---- kernel units against float64 --------------------------------------------------------------------------------------------
def _sizes(rng, B, mx):
    return [mx] + [int(x) for x in rng.integers(1, mx + 1, B - 1)] if B > 1 else [mx]


@pytest.mark.parametrize("B,H,C", [(1, 5, 7), (7, 13, 9), (33, 50, 5)])
def test_kernels_against_float64(B, H, C, engine):
    from newsreclib_amd import ops_sentidebias as SD
    rng = np.random.default_rng(B)
    D, S = 300, 4
    hs, cs = _sizes(rng, B, H), _sizes(rng, B, C)
    nh, nc = sum(hs), sum(cs)
    N = nh + nc
    ids = torch.from_numpy(rng.integers(0, S, N))
    ids[:hs[0]] = 2                                    # a user whose history is all one class
    dev = "cuda"
    off = lambda s: torch.tensor([0] + np.cumsum(s).tolist(), device=dev)  # noqa: E731
    news64 = torch.from_numpy(rng.standard_normal((N, D)))
    T64 = torch.tanh(torch.from_numpy(rng.standard_normal((S, D))))
    w = torch.from_numpy(rng.standard_normal(2))

    def leaf(x):
        return x.float().to(dev).requires_grad_(True)

    # row cosines
    news, T = leaf(news64), leaf(T64)
    out = SD.RowCosFn.apply(news, T, ids.to(dev), nh)
    (out * w.float().to(dev)).sum().backward()
    n64, t64 = news64.clone().requires_grad_(True), T64.clone().requires_grad_(True)
    c = SO.cos_rows(n64, t64[ids])
    ref = torch.stack([c[:nh].mean(), c[nh:].mean()])
    (ref * w).sum().backward()
    assert float((out.detach().cpu().double() - ref.detach()).abs().max()) <= 1e-6
    assert float((news.grad.cpu().double() - n64.grad).abs().max()) <= 1e-6 * max(1.0, float(n64.grad.abs().max()))
    assert float((T.grad.cpu().double() - t64.grad).abs().max()) <= 1e-5 * max(1.0, float(t64.grad.abs().max()))
    T2 = leaf(T64)
    out2 = SD.RowCosFn.apply(news.detach().requires_grad_(True), T2, ids.to(dev), nh)
    (out2 * w.float().to(dev)).sum().backward()
    assert torch.equal(T2.grad, T.grad)                # bit-reproducible

    # dense sentiment history and late fusion
    T = leaf(T64)
    dh = SD.SentHistFn.apply(T, ids[:nh].to(dev), off(hs), B, H)
    gh = torch.from_numpy(rng.standard_normal((B, H, D)))
    (dh * gh.float().to(dev)).sum().backward()
    t64 = T64.clone().requires_grad_(True)
    ref = SO.dense(t64[ids[:nh]], hs)
    (ref * gh).sum().backward()
    assert torch.equal(dh.detach().cpu(), ref.detach().float())
    assert float((T.grad.cpu().double() - t64.grad).abs().max()) <= 1e-5 * max(1.0, float(t64.grad.abs().max()))
    T2 = leaf(T64)
    (SD.SentHistFn.apply(T2, ids[:nh].to(dev), off(hs), B, H) * gh.float().to(dev)).sum().backward()
    assert torch.equal(T2.grad, T.grad)                # bit-reproducible
    T = leaf(T64)
    u = SD.LateUserFn.apply(T, ids[:nh].to(dev), off(hs), B)
    gu = torch.from_numpy(rng.standard_normal((B, D)))
    (u * gu.float().to(dev)).sum().backward()
    t64 = T64.clone().requires_grad_(True)
    ref = SO.dense(t64[ids[:nh]], hs).sum(1) / torch.tensor(hs, dtype=torch.float64).unsqueeze(1)
    (ref * gu).sum().backward()
    assert float((u.detach().cpu().double() - ref.detach()).abs().max()) <= 1e-6
    assert float((T.grad.cpu().double() - t64.grad).abs().max()) <= 1e-5 * max(1.0, float(t64.grad.abs().max()))
    T2 = leaf(T64)
    (SD.LateUserFn.apply(T2, ids[:nh].to(dev), off(hs), B) * gu.float().to(dev)).sum().backward()
    assert torch.equal(T2.grad, T.grad)                # bit-reproducible (nrl_sd_bt_matmul)

    # bias-aware scores
    free64, u64 = torch.from_numpy(rng.standard_normal((B, C))), torch.from_numpy(rng.standard_normal((B, D)))
    free, uu, T = leaf(free64), leaf(u64), leaf(T64)
    sc = SD.CombinedScoresFn.apply(free, uu, T, ids[nh:].to(dev), off(cs))
    gs = torch.from_numpy(rng.standard_normal((B, C)))
    (sc * gs.float().to(dev)).sum().backward()
    f64, u6, t64 = (x.clone().requires_grad_(True) for x in (free64, u64, T64))
    ref = f64 + torch.einsum("bd,bcd->bc", u6, SO.dense(t64[ids[nh:]], cs))
    (ref * gs).sum().backward()
    assert float((sc.detach().cpu().double() - ref.detach()).abs().max()) <= 1e-4
    for a, b in ((free, f64), (uu, u6), (T, t64)):
        assert float((a.grad.cpu().double() - b.grad).abs().max()) <= 1e-5 * max(1.0, float(b.grad.abs().max()))
    T2 = leaf(T64)
    (SD.CombinedScoresFn.apply(leaf(free64), leaf(u64), T2, ids[nh:].to(dev), off(cs)) * gs.float().to(dev)).sum().backward()
    assert torch.equal(T2.grad, T.grad)                # bit-reproducible

    # discriminator: tanh(linear1) on the engine, fused tail
    p = {k: v.double() for k, v in SO.make_head_params(3).items() if k.startswith("discriminator.")}
    leaves = {k: leaf(v) for k, v in p.items()}
    x = leaf(0.3 * news64)
    out = SD.DiscriminatorLossFn.apply(x, *(leaves["discriminator." + k] for k in ("linear1.weight", "linear1.bias", "linear2.weight",
                                                                                  "linear2.bias")), ids.to(dev), nh)
    (out * w.float().to(dev)).sum().backward()
    p64 = {k: v.clone().requires_grad_(True) for k, v in p.items()}
    x64 = (0.3 * news64).clone().requires_grad_(True)
    a, b = SO.discriminator_losses(p64, x64[:nh], x64[nh:], ids[:nh], ids[nh:])
    (a * w[0] + b * w[1]).backward()
    tol = 1e-5 if engine == "f32" else 1e-4
    assert float((out.detach().cpu().double() - torch.stack([a, b]).detach()).abs().max()) <= tol
    assert float((x.grad.cpu().double() - x64.grad).abs().max()) <= tol * max(1.0, float(x64.grad.abs().max()))
    for k in p:
        assert float((leaves[k].grad.cpu().double() - p64[k].grad).abs().max()) <= tol * max(1.0, float(p64[k].grad.abs().max())), k
    # requires_grad decides what is computed: phase G (no weight gradients), phase D (no activation gradient)
    frozen = {k: v.detach() for k, v in leaves.items()}
    order = ("linear1.weight", "linear1.bias", "linear2.weight", "linear2.bias")
    x2 = x.detach().requires_grad_(True)
    SD.DiscriminatorLossFn.apply(x2, *(frozen["discriminator." + k] for k in order), ids.to(dev), nh).sum().backward()
    assert x2.grad is not None
    l2 = {k: v.detach().requires_grad_(True) for k, v in leaves.items()}
    o1 = SD.DiscriminatorLossFn.apply(x.detach(), *(l2["discriminator." + k] for k in order), ids.to(dev), nh)
    (o1 * w.float().to(dev)).sum().backward()
    for k in ("discriminator.linear2.weight", "discriminator.linear2.bias"):
        assert torch.equal(l2[k].grad, leaves[k].grad), k          # bit-reproducible over two runs


def test_no_grad_forward_matches_grad_forward(engine):
    """The forward under ``torch.no_grad()`` (nothing saved; the evaluation shapes of the encoder kernels) against the forward that
    a backward can follow.  Same arithmetic in another kernel order: held to the project's output bound (1e-4 on scores and news
    vectors, 2e-4 on the loss term), not to bit equality."""
    g = load_golden("sentidebias_tiny_eval")
    mod = _module(g)
    pb = mod._prepare(batch_to(golden_batch(g), "cuda"))
    a = mod(pb)
    with torch.no_grad():
        b = mod(pb)
        preds = mod.model_step(pb)[0]
    diffs = [float((x.detach() - y).abs().max()) for x, y in zip(a, b)]
    assert all(d <= (2e-4 if i == 2 else 1e-4) for i, d in enumerate(diffs))
    assert float((preds - a[1].detach().reshape(-1)[pb["cand_flat_idx"]]).abs().max()) <= 1e-4


@pytest.mark.parametrize("late_fusion", [False, True])
def test_news_vector_cache_matches_model_step(late_fusion, engine):
    """Encode-once evaluation (``evaluation.NewsVectorCache`` / ``evaluate_impressions``) against the module's own per-batch
    ``model_step`` on the same impressions: ``preds`` equal, ranking and aspect metrics equal."""
    from newsreclib_amd.evaluation import DeviceNewsTable, NewsVectorCache, evaluate_impressions
    from newsreclib_amd.metrics import aspect_metrics, ranking_metrics
    rng = np.random.default_rng(17)
    vocab, n_news, n_imp, bs = 300, 211, 21, 8
    mod = build_module(SO.make_params(vocab, 4, 1, late_fusion), p_drop=0.2, late_fusion=late_fusion).eval()
    lens = rng.integers(3, 31, n_news)
    ids = rng.integers(1, vocab, (n_news, 30))
    ids[np.arange(30)[None, :] >= lens[:, None]] = 0
    ids[0] = 0
    table = DeviceNewsTable({"title": torch.from_numpy(ids), "category": torch.from_numpy(rng.integers(1, 19, n_news)),
                             "sentiment": torch.from_numpy(rng.integers(0, SO.N_SENT, n_news))})
    imps = []
    for _ in range(n_imp):
        nh, nc = int(rng.integers(1, 13)), int(rng.integers(2, 41))
        lab = np.zeros(nc, dtype=np.float32)
        lab[rng.integers(0, nc)] = 1.0
        imps.append({"hist": torch.from_numpy(rng.integers(1, n_news, nh)), "cand": torch.from_numpy(rng.integers(1, n_news, nc)),
                     "labels": torch.from_numpy(lab)})
    cache = NewsVectorCache(mod, table, chunk=64)
    assert cache.build().shape == (n_news, SO.D)
    outs = []
    for lo in range(0, n_imp, bs):
        ch = imps[lo:lo + bs]
        hist, cand = torch.cat([i["hist"] for i in ch]), torch.cat([i["cand"] for i in ch])
        hs, cs = torch.tensor([len(i["hist"]) for i in ch]), torch.tensor([len(i["cand"]) for i in ch])
        labels = torch.cat([i["labels"] for i in ch])
        batch = table.build_batch(hist, hs, cand, cs, labels)
        with torch.no_grad():
            ref = mod.model_step(batch)                       # the reference's 10-tuple: no loss in front
        assert len(ref) == 10
        outs.append(ref)
        got = cache.model_step(hist, hs, cand, cs, labels)   # (loss, then the same ten)
        scores = cache.scores(hist, hs, cand, cs)
        assert scores.shape == (len(ch), int(cs.max()))
        assert torch.equal(got[1], ref[0]) and torch.equal(got[2], ref[1]) and torch.equal(got[3], ref[2])
        assert torch.equal(got[4], ref[3]) and torch.equal(got[6], ref[5]) and torch.equal(got[8], ref[7])
    logs = evaluate_impressions(cache, imps, batch_size=bs, num_categ_classes=19, num_sent_classes=SO.N_SENT)
    cat = lambda j: torch.cat([o[j] for o in outs])  # noqa: E731
    want = ranking_metrics(cat(0), cat(1), cat(2), (5, 10))
    want.update(aspect_metrics(cat(0), cat(4), cat(6), cat(2), cat(3), 19, (5, 10), prefix="categ"))
    want.update(aspect_metrics(cat(0), cat(5), cat(7), cat(2), cat(3), SO.N_SENT, (5, 10), prefix="sent"))
    for k, v in want.items():
        assert logs[k] == v, (k, logs[k], v)
