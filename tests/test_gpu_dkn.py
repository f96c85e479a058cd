"""GPU parity of the DKN module (newsreclib_amd.dkn_module) against the golden vectors made from the reference's own
components, under both GEMM engines, plus its training / evaluation behaviour."""
import numpy as np
import pytest
import torch

from oracle import losses_oracle as LO
from oracle.nrms_oracle import to_dense_batch
from tests import dkn_oracle as DO
from tests.helpers import batch_to, check_lstur_grads, load_golden, module_grads

pytestmark = pytest.mark.gpu

# the user encoder's DNN is affine: these three gradients are zero in exact arithmetic (round-off in the reference)
ZERO_GRAD_KEYS = ("user_encoder.dnn.0.bias", "user_encoder.dnn.1.bias")


@pytest.fixture(autouse=True, params=["f32", "bf16x3"])
def engine(request):
    from newsreclib_amd import _lib
    prev = _lib.get_gemm_engine()
    _lib.set_gemm_engine(request.param)
    yield request.param
    _lib.set_gemm_engine(prev)


def _tols(engine):
    return (2e-5, 2e-4) if engine == "f32" else (1e-4, 5e-4)


def _dense(preds, sizes, shape):
    dense = np.zeros(shape, dtype=np.float32)
    p, o = preds.detach().cpu().numpy(), 0
    for b, n in enumerate(sizes.cpu().numpy()):
        dense[b, :n] = p[o:o + n]
        o += n
    return dense


def _check_quirk4(g, grads, dim):
    for k in ZERO_GRAD_KEYS:
        ref = float(np.abs(g["gfull/" + k]).max()) if "gfull/" + k in g else 0.0
        assert float(grads[k].abs().max()) <= 1e-6 + ref, k
    assert float(grads["user_encoder.dnn.0.weight"][:, :dim].abs().max()) <= 1e-6


@pytest.mark.parametrize("name", DO.DKN_CASES)
def test_dkn_module_matches_reference_golden(name, engine):
    g = load_golden(name)
    cfg = DO.golden_cfg(g)
    mod = DO.build_module(cfg, DO.golden_params(cfg)).train()
    seen = {}
    enc_fwd = mod.news_encoder.forward
    mod.news_encoder.forward = lambda *a, **kw: seen.setdefault("news", enc_fwd(*a, **kw))
    batch = batch_to(DO.golden_batch(g), "cuda")
    loss, preds, targets, cand_news_size, *_ = mod.model_step(batch)
    ftol, gtol = _tols(engine)
    assert float(np.abs(_dense(preds, cand_news_size, g["out_scores"].shape) - g["out_scores"]).max()) <= max(ftol * 5, 1e-4)
    assert abs(float(loss) - float(g["out_loss"])) <= 2e-4
    stride, nh = int(g["cfg_row_stride"]), batch["batch_hist"].shape[0]
    news = seen["news"].detach().cpu().numpy()
    assert float(np.abs(news[:nh][::stride] - g["out_hist_vec"]).max()) <= 10 * ftol
    assert float(np.abs(news[nh:][::stride] - g["out_cand_vec"]).max()) <= 10 * ftol
    loss.backward()
    grads = module_grads(mod)
    skip = set(ZERO_GRAD_KEYS) | {"user_encoder.dnn.0.weight"}
    check_lstur_grads({k: v for k, v in g.items() if not any(k.endswith("/" + s) for s in skip)}, grads, tol=gtol,
                      rtol=5e-4)
    for key in (DO.WORD, DO.ENT, DO.CTX):            # padding rows never receive a gradient
        if key in grads:
            assert float(grads[key][0].abs().max()) == 0.0, key
    if not cfg["late_fusion"]:
        _check_quirk4(g, grads, len(cfg["windows"]) * cfg["F"])
        # the history half of the attention's first layer and its second layer do get the reference's gradient
        ref = torch.from_numpy(g["gfull/user_encoder.dnn.0.weight"] if "gfull/user_encoder.dnn.0.weight" in g else
                               np.zeros(1, np.float32))
        if ref.dim() == 2:
            dim = len(cfg["windows"]) * cfg["F"]
            got = grads["user_encoder.dnn.0.weight"].detach().cpu()[:, dim:]
            assert float((got - ref[:, dim:]).abs().max()) <= gtol * max(1.0, float(ref.abs().max()))


def test_dkn_batch_of_one(engine):
    g = load_golden("dkn_tiny_train")
    cfg = DO.golden_cfg(g)
    full = DO.golden_batch(g)
    nh, nc = int((full["batch_hist"] == 0).sum()), int((full["batch_cand"] == 0).sum())
    one = {"batch_hist": full["batch_hist"][:nh], "batch_cand": full["batch_cand"][:nc],
           "x_hist": {k: v[:nh] for k, v in full["x_hist"].items()},
           "x_cand": {k: v[:nc] for k, v in full["x_cand"].items()},
           "labels": full["labels"][:nc], "user_idx": full["user_idx"][:1], "user_ids": full["user_ids"][:1],
           "batch_size": 1}
    params = DO.golden_params(cfg)
    mod = DO.build_module(cfg, params).eval()
    with torch.no_grad():
        scores = mod(batch_to(one, "cuda")).cpu()
    assert scores.shape == (1, nc)
    want = DO.dkn_forward(one, params, cfg["windows"])["scores"]
    assert float((scores - want).abs().max()) <= 1e-4


def test_dkn_padded_candidates_score_exactly_zero(engine):
    g = load_golden("dkn_tiny_train")
    cfg = DO.golden_cfg(g)
    mod = DO.build_module(cfg, DO.golden_params(cfg)).eval()
    batch = DO.golden_batch(g)
    with torch.no_grad():
        scores = mod(batch_to(batch, "cuda")).cpu()
    sizes = torch.bincount(batch["batch_cand"], minlength=batch["batch_size"])
    for b, n in enumerate(sizes.tolist()):
        assert bool((scores[b, n:] == 0).all())
    assert float(scores[0, :int(sizes[0])].abs().min()) > 0


def test_dkn_dual_loss_step_matches_oracle(engine):
    from newsreclib_amd.nrms_module import prepare_batch
    g = load_golden("dkn_tiny_eval")
    cfg = DO.golden_cfg(g)
    mod = DO.build_module(cfg, DO.golden_params(cfg), dual_loss_training=True, dual_loss_coef=0.3,
                          loss="dual_loss").eval()
    pb = prepare_batch(batch_to(DO.golden_batch(g), "cuda"))
    got = mod.model_step(pb)[0]
    with torch.no_grad():
        scores = mod(pb).cpu()
    y_true, mask = to_dense_batch(pb["labels"].cpu(), pb["batch_cand"].cpu(), pb["batch_size"])
    want = LO.dual_loss(scores, y_true, mask, 0.3)
    assert abs(float(got.detach()) - float(want)) <= 5e-5 * max(1.0, abs(float(want)))
    got.backward()
    zero = {"user_encoder.dnn.0.bias", "user_encoder.dnn.1.bias"}
    assert all(p.grad is not None and float(p.grad.norm()) > 0 for k, p in mod.named_parameters() if k not in zero)


def test_dkn_trainer_updates_every_parameter():
    from newsreclib_amd.trainer import NRMSTrainer
    g = load_golden("dkn_tiny_train")
    cfg = DO.golden_cfg(g)
    mod = DO.build_module(cfg, DO.golden_params(cfg)).train()
    before = {k: p.detach().clone() for k, p in mod.named_parameters()}
    loss = NRMSTrainer(mod, lr=1e-3).step(batch_to(DO.golden_batch(g), "cuda"))
    assert np.isfinite(float(loss))
    for k, p in mod.named_parameters():
        if k in ZERO_GRAD_KEYS:
            continue                                    # (a zero gradient: Adam leaves them where they are)
        assert float((p.detach() - before[k]).abs().max()) > 0.0, k


def test_dkn_no_grad_forward_equals_training_forward(engine):
    g = load_golden("dkn16_train")
    cfg = DO.golden_cfg(g)
    mod = DO.build_module(cfg, DO.golden_params(cfg)).eval()
    batch = batch_to(DO.golden_batch(g), "cuda")
    with torch.no_grad():
        a = mod(batch)
    b = mod(batch)
    assert b.requires_grad
    assert torch.equal(a, b.detach())


def test_dkn_news_vector_cache_matches_forward(engine):
    from newsreclib_amd.evaluation import DeviceNewsTable, NewsVectorCache
    g = load_golden("dkn_tiny_eval")
    cfg = DO.golden_cfg(g)
    mod = DO.build_module(cfg, DO.golden_params(cfg)).eval()
    batch = DO.golden_batch(g)
    title = torch.cat([batch["x_hist"]["title"], batch["x_cand"]["title"]])
    ents = torch.cat([batch["x_hist"]["title_entities"], batch["x_cand"]["title_entities"]])
    table = DeviceNewsTable({"title": title, "title_entities": ents}, device="cuda")
    nh = batch["batch_hist"].shape[0]
    B = batch["batch_size"]
    hs = torch.bincount(batch["batch_hist"], minlength=B)
    cs = torch.bincount(batch["batch_cand"], minlength=B)
    cache = NewsVectorCache(mod, table)
    got = cache.scores(torch.arange(nh), hs, torch.arange(nh, title.shape[0]), cs).cpu()
    with torch.no_grad():
        want = mod(batch_to(batch, "cuda")).cpu()
    assert float((got - want).abs().max()) <= 1e-5


def test_dkn_steps_are_bit_identical(engine):
    g = load_golden("dkn16_train")
    cfg = DO.golden_cfg(g)
    params = DO.golden_params(cfg)
    runs = []
    for _ in range(2):
        mod = DO.build_module(cfg, params).train()
        loss = mod.model_step(batch_to(DO.golden_batch(g), "cuda"))[0]
        loss.backward()
        runs.append((loss.detach().cpu(), {k: v.detach().cpu().clone() for k, v in module_grads(mod).items()}))
    assert torch.equal(runs[0][0], runs[1][0])
    for k in runs[0][1]:
        a, b = runs[0][1][k], runs[1][1][k]
        if ".conv_filters." in k or k.endswith("embedding_layer.weight"):
            # the convolution weight gradient (split-K) and the library's sorted table gradient add partial sums
            # atomically: equal to rounding, not to the bit
            assert float((a - b).abs().max()) <= 1e-5 * max(1.0, float(a.abs().max())), k
        else:                   # every DKN kernel reduces in a fixed order
            assert torch.equal(a, b), k


@pytest.mark.parametrize("how", ["load_state_dict", "optimizer_step", "copy_"])
def test_dkn_conv_image_follows_weight_writes(how, engine):
    g = load_golden("dkn_tiny_train")
    cfg = DO.golden_cfg(g)
    params = DO.golden_params(cfg)
    mod = DO.build_module(cfg, params).eval()
    batch = batch_to(DO.golden_batch(g), "cuda")
    with torch.no_grad():
        mod(batch)                                       # builds the images
    w = mod.news_encoder.conv_filters["2"].weight
    new = {k: v.clone() for k, v in params.items()}
    new[DO.conv_key(2, "weight")] = new[DO.conv_key(2, "weight")] * -1.5
    if how == "load_state_dict":
        mod.load_state_dict(new, strict=True)
    elif how == "copy_":
        with torch.no_grad():
            w.copy_(new[DO.conv_key(2, "weight")].cuda())
    else:
        opt = torch.optim.SGD([w], lr=1.0)
        w.grad = (w.detach() - new[DO.conv_key(2, "weight")].cuda())
        opt.step()
        new[DO.conv_key(2, "weight")] = w.detach().cpu().clone()
    with torch.no_grad():
        got = mod(batch).cpu()
    want = DO.dkn_forward(DO.golden_batch(g), new, cfg["windows"])["scores"]
    assert float((got - want).abs().max()) <= 1e-4
    img = mod.news_encoder.conv_images()[1]
    assert torch.equal(img, w.detach().permute(0, 2, 1, 3).contiguous())
