"""GPU parity of the NPA module (newsreclib_amd.npa_module) against the golden vectors made from the reference's own
components, under both GEMM engines, plus its training / evaluation behaviour."""
import numpy as np
import pytest
import torch

from oracle import losses_oracle as LO
from oracle.nrms_oracle import to_dense_batch
from tests import npa_oracle as NO
from tests.helpers import batch_to, check_lstur_grads, load_golden, module_grads

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


def _seeded(mod, seed):
    orig = mod.forward
    mod.forward = lambda b, seed_=None, **kw: orig(b, seed=seed)
    return mod


def _dense(preds, sizes, shape):
    dense = np.zeros(shape, dtype=np.float32)
    p, o = preds.detach().cpu().numpy(), 0
    for b, n in enumerate(sizes.cpu().numpy()):
        dense[b, :n] = p[o:o + n]
        o += n
    return dense


@pytest.mark.parametrize("name", NO.NPA_CASES)
def test_npa_module_matches_reference_golden(name, engine):
    g = load_golden(name)
    cfg = NO.golden_cfg(g)
    mod = NO.build_module(cfg, NO.golden_params(cfg))
    mod.train() if cfg["p_drop"] > 0 else mod.eval()
    _seeded(mod, cfg["seed"])
    seen = {}
    enc_fwd = mod.news_encoder.forward
    mod.news_encoder.forward = lambda *a, **kw: seen.setdefault("news", enc_fwd(*a, **kw))
    if not cfg["late_fusion"]:
        ue_fwd = mod.user_encoder.forward
        mod.user_encoder.forward = lambda *a, **kw: seen.setdefault("user", ue_fwd(*a, **kw))
    batch = batch_to(NO.golden_batch(g), "cuda")
    loss, preds, targets, cand_news_size, *_ = mod.model_step(batch)
    ftol, gtol = _tols(engine)
    assert float(np.abs(_dense(preds, cand_news_size, g["out_scores"].shape) - g["out_scores"]).max()) <= \
        max(ftol * 5, 1e-4)                                                          # contract 1e-3
    assert abs(float(loss) - float(g["out_loss"])) <= 2e-4
    stride, nh = int(g["cfg_row_stride"]), batch["batch_hist"].shape[0]
    news = seen["news"].detach().cpu().numpy()
    assert float(np.abs(news[:nh][::stride] - g["out_hist_vec"]).max()) <= 10 * ftol
    assert float(np.abs(news[nh:][::stride] - g["out_cand_vec"]).max()) <= 10 * ftol
    if not cfg["late_fusion"]:
        assert float(np.abs(seen["user"].detach().cpu().numpy() - g["out_user_vec"]).max()) <= 10 * ftol
    loss.backward()
    check_lstur_grads(g, module_grads(mod), tol=gtol, rtol=5e-4)


def test_npa16_repeated_user_row_gradient(engine):
    """user 17 appears in three impressions: its table row gets the sum of their gradients."""
    g = load_golden("npa16_train")
    cfg = NO.golden_cfg(g)
    mod = _seeded(NO.build_module(cfg, NO.golden_params(cfg)).train(), cfg["seed"])
    loss = mod.model_step(batch_to(NO.golden_batch(g), "cuda"))[0]
    loss.backward()
    key = "user_projection.user_embed"
    rows = torch.from_numpy(g["grows_idx/" + key])
    assert 17 in rows.tolist() and (torch.from_numpy(g["in_user_idx"]) == 17).sum() == 3
    got = module_grads(mod)[key].detach().cpu()[rows]
    assert float((got - torch.from_numpy(g["grows/" + key])).abs().max()) <= _tols(engine)[1]
    untouched = torch.ones(got.new_empty(cfg["n_users"]).shape, dtype=torch.bool)
    untouched[torch.from_numpy(g["in_user_idx"])] = False
    assert float(module_grads(mod)[key].detach().cpu()[untouched].abs().max()) == 0.0


def test_npa_max_hist_quirk(engine):
    """The same users score differently beside a user with a longer history, exactly as the reference."""
    g = load_golden("npa_quirk")
    cfg = NO.golden_cfg(g)
    mod = NO.build_module(cfg, NO.golden_params(cfg)).eval()
    got = {}
    with torch.no_grad():
        for tag in ("small", "big"):
            got[tag] = mod(batch_to(NO.golden_batch(g, tag + "/"), "cuda")).cpu()
            assert float((got[tag] - torch.from_numpy(g[tag + "/out_scores"])).abs().max()) <= 1e-4, tag
    n = got["small"].shape[1]
    assert float((got["small"] - got["big"][:2, :n]).abs().max()) > 1e-3


def test_npa_batch_of_one_returns_2d_scores(engine):
    g = load_golden("npa_quirk")
    cfg = NO.golden_cfg(g)
    full = NO.golden_batch(g, "small/")
    nh, nc = int((full["batch_hist"] == 0).sum()), int((full["batch_cand"] == 0).sum())
    one = {"batch_hist": full["batch_hist"][:nh], "batch_cand": full["batch_cand"][:nc],
           "x_hist": {"title": full["x_hist"]["title"][:nh]}, "x_cand": {"title": full["x_cand"]["title"][:nc]},
           "labels": full["labels"][:nc], "user_idx": full["user_idx"][:1], "user_ids": full["user_ids"][:1],
           "batch_size": 1}
    params = NO.golden_params(cfg)
    mod = NO.build_module(cfg, params).eval()
    with torch.no_grad():
        scores = mod(batch_to(one, "cuda")).cpu()
    assert scores.shape == (1, nc)
    want = NO.npa_forward(one, params)["scores"]
    assert float((scores - want).abs().max()) <= 1e-4


def test_npa_dual_loss_step_matches_oracle(engine):
    from newsreclib_amd.nrms_module import prepare_batch
    g = load_golden("npa_tiny_eval")
    cfg = NO.golden_cfg(g)
    mod = NO.build_module(cfg, NO.golden_params(cfg), dual_loss_training=True, dual_loss_coef=0.3,
                          loss="dual_loss").eval()
    pb = prepare_batch(batch_to(NO.golden_batch(g), "cuda"))
    got = mod.model_step(pb)[0]
    with torch.no_grad():
        scores = mod(pb).cpu()
    y_true, mask = to_dense_batch(pb["labels"].cpu(), pb["batch_cand"].cpu(), pb["batch_size"])
    want = LO.dual_loss(scores, y_true, mask, 0.3)
    assert abs(float(got.detach()) - float(want)) <= 5e-5 * max(1.0, abs(float(want)))
    got.backward()
    assert all(p.grad is not None and float(p.grad.norm()) > 0 for p in mod.parameters())


def test_npa_trainer_updates_every_parameter():
    from newsreclib_amd.trainer import NRMSTrainer
    g = load_golden("npa_tiny_train")
    cfg = NO.golden_cfg(g)
    mod = NO.build_module(cfg, NO.golden_params(cfg)).train()
    before = {k: p.detach().clone() for k, p in mod.named_parameters()}
    loss = NRMSTrainer(mod, lr=1e-3).step(batch_to(NO.golden_batch(g), "cuda"))
    assert np.isfinite(float(loss))
    for k, p in mod.named_parameters():
        assert float((p.detach() - before[k]).abs().max()) > 0.0, k


def test_npa_no_grad_forward_equals_eval_training_forward(engine):
    g = load_golden("npa16_train")
    cfg = NO.golden_cfg(g)
    mod = NO.build_module(cfg, NO.golden_params(cfg)).eval()
    batch = batch_to(NO.golden_batch(g), "cuda")
    with torch.no_grad():
        a = mod(batch)
    b = mod(batch)
    assert b.requires_grad
    assert torch.equal(a, b.detach())


def test_npa_seeded_steps_are_bit_identical(engine):
    g = load_golden("npa16_train")
    cfg = NO.golden_cfg(g)
    params = NO.golden_params(cfg)
    runs = []
    for _ in range(2):
        mod = _seeded(NO.build_module(cfg, params).train(), 1234)
        loss = mod.model_step(batch_to(NO.golden_batch(g), "cuda"))[0]
        loss.backward()
        runs.append((loss.detach().cpu(), {k: v.detach().cpu().clone() for k, v in module_grads(mod).items()}))
    assert torch.equal(runs[0][0], runs[1][0])
    for k in runs[0][1]:
        if k.startswith("news_encoder.cnn.") or k.endswith("embedding_layer.weight"):
            # the convolution stages shared with the CNN encoders (split-K weight gradient, table gradient) add
            # partial sums atomically: equal to rounding, not to the bit
            a, b = runs[0][1][k], runs[1][1][k]
            assert float((a - b).abs().max()) <= 1e-5 * max(1.0, float(a.abs().max())), k
        else:                   # every NPA kernel reduces in a fixed order
            assert torch.equal(runs[0][1][k], runs[1][1][k]), k
