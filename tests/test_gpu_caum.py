"""GPU parity of the CAUM module (newsreclib_amd.caum_module) against the golden vectors made from the reference's own
components, under both GEMM engines, plus its training / evaluation behaviour."""
import numpy as np
import pytest
import torch

from oracle import losses_oracle as LO
from oracle.nrms_oracle import to_dense_batch
from tests import builders
from tests import caum_oracle as CO
from tests.helpers import batch_to, check_lstur_grads, load_golden, module_grads

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True, params=["f32", "bf16x3"])
def engine(request):
    from newsreclib_amd import _lib
    prev = _lib.get_gemm_engine()
    _lib.set_gemm_engine(request.param)
    yield request.param
    _lib.set_gemm_engine(prev)


def _dense(preds, sizes, shape):
    dense = np.zeros(shape, dtype=np.float32)
    p, o = preds.detach().cpu().numpy(), 0
    for b, n in enumerate(sizes.cpu().numpy()):
        dense[b, :n] = p[o:o + n]
        o += n
    return dense


def _golden_module(name, monkeypatch=None):
    g = load_golden(name)
    cfg = CO.golden_cfg(g)
    mod = CO.build_module(cfg, CO.golden_params(cfg))
    mod.train() if cfg["p_drop"] > 0 else mod.eval()
    if monkeypatch is not None:
        from newsreclib_amd import caum_module
        monkeypatch.setattr(caum_module, "_draw_seed", lambda: cfg["seed"])
    return g, cfg, mod


@pytest.mark.parametrize("name", CO.CAUM_CASES)
def test_caum_module_matches_reference_golden(name, engine, monkeypatch):
    g, cfg, mod = _golden_module(name, monkeypatch)
    seen = {}
    enc_fwd = mod.news_encoder.forward
    mod.news_encoder.forward = lambda *a, **kw: seen.setdefault("news", enc_fwd(*a, **kw))
    batch = batch_to(CO.golden_batch(g), "cuda")
    loss, preds, targets, cand_news_size, *_ = mod.model_step(batch)
    ftol, gtol = builders.head_tols(engine)
    ref = g["out_scores"]
    got = _dense(preds, cand_news_size, ref.shape)
    assert float(np.abs(got - ref).max()) <= 20 * ftol * max(1.0, float(np.abs(ref).max())), float(np.abs(got - ref).max())
    assert abs(float(loss.detach()) - float(g["out_loss"])) <= 1e-3
    stride, nh = int(g["cfg_row_stride"]), batch["batch_hist"].shape[0]
    news = seen["news"].detach().cpu().numpy()
    assert float(np.abs(news[:nh][::stride] - g["out_hist_vec"]).max()) <= 10 * ftol
    assert float(np.abs(news[nh:][::stride] - g["out_cand_vec"]).max()) <= 10 * ftol
    loss.backward()
    check_lstur_grads(g, module_grads(mod), tol=gtol, rtol=2e-3, atol=1e-5)


@pytest.mark.parametrize("dim", [300, 100])
def test_padded_head_mhsa_addatt_matches_reference(dim, engine):
    """MHSAAddAtt at the reference's head dims 300 / 20 = 15 and 100 / 20 = 5 (not built: padded to 16 per head)."""
    from newsreclib_amd.news_encoder import MHSAAddAtt
    torch.manual_seed(3)
    V, Q, N, L = 50, 200, 6, 10
    enc = MHSAAddAtt(pretrained_embeddings=torch.randn(V, dim) * 0.3, embed_dim=dim, num_heads=20, query_dim=Q,
                     dropout_probability=0.2).cuda().eval()
    assert enc.padded_heads
    ids = torch.randint(1, V, (N, L))
    ids[:, 7:] = 0
    params = {k: v.detach().cpu().clone().requires_grad_(True) for k, v in enc.state_dict().items()}
    want = CO.mhsa_addatt(ids, params, "", 20)
    got = enc(ids.cuda())
    assert float((got.detach().cpu() - want.detach()).abs().max()) <= 1e-4
    w = torch.randn(N, dim)
    (got * w.cuda()).sum().backward()
    (want * w).sum().backward()
    for k, p in enc.named_parameters():
        ref = params[k].grad.clone()
        if k == "embedding_layer.weight":
            ref[0] = 0.0
        scale = max(1.0, float(ref.abs().max()))
        assert float((p.grad.cpu() - ref).abs().max()) <= 1e-3 * scale, k


def test_caum_padded_candidates_score_exactly_zero(engine):
    g, cfg, mod = _golden_module("caum_ragged")
    batch = CO.golden_batch(g)
    with torch.no_grad():
        scores = mod(batch_to(batch, "cuda")).cpu()
    sizes = torch.bincount(batch["batch_cand"], minlength=batch["batch_size"])
    for b, n in enumerate(sizes.tolist()):
        assert bool((scores[b, n:] == 0).all())
        assert float(scores[b, :n].abs().min()) > 0


def test_caum_users_of_a_batch_are_coupled(engine):
    """The seq-first attention runs across the users of the batch, as in the reference: another user's history moves
    user 1's scores."""
    g, cfg, mod = _golden_module("caum_tiny_eval")
    batch = CO.golden_batch(g)
    other = {k: (dict(v) if isinstance(v, dict) else v) for k, v in batch.items()}
    nh0 = int((batch["batch_hist"] == 0).sum())
    t = batch["x_hist"]["title"].clone()
    t[:nh0] = torch.flip(t[:nh0], dims=[1]) % 7 + 1
    other["x_hist"]["title"] = t
    with torch.no_grad():
        a = mod(batch_to(batch, "cuda")).cpu()
        b = mod(batch_to(other, "cuda")).cpu()
    n1 = int((batch["batch_cand"] == 1).sum())
    assert float((a[1, :n1] - b[1, :n1]).abs().max()) > 1e-5
    params = CO.golden_params(cfg)
    want = CO.caum_forward(other, params, cfg)["scores"]
    assert float((b - want).abs().max()) <= 1e-4


def test_caum_slot_chunks_equal_one_pass(engine):
    g, cfg, mod = _golden_module("caum_tiny_eval")
    batch = batch_to(CO.golden_batch(g), "cuda")
    with torch.no_grad():
        mod.user_encoder.slot_chunk = None
        whole = mod(batch)
        mod.user_encoder.slot_chunk = 3
        chunked = mod(batch)
    assert whole.shape == chunked.shape == (3, 10)
    assert float((whole - chunked).abs().max()) <= 1e-5


def test_caum_batch_of_one(engine):
    g, cfg, mod = _golden_module("caum_one_user")
    mod.eval()
    batch = CO.golden_batch(g)
    with torch.no_grad():
        scores = mod(batch_to(batch, "cuda")).cpu()
    want = CO.caum_forward(batch, CO.golden_params(cfg), cfg)["scores"]
    assert scores.shape == want.shape == (1, 4)
    assert float((scores - want).abs().max()) <= 1e-4


def test_caum_news_vector_cache_matches_forward(engine):
    from newsreclib_amd.evaluation import DeviceNewsTable, NewsVectorCache
    g, cfg, mod = _golden_module("caum_tiny_eval")
    batch = CO.golden_batch(g)
    cat = lambda k: torch.cat([batch["x_hist"][k], batch["x_cand"][k]])  # noqa: E731
    table = DeviceNewsTable({k: cat(k) for k in ("title", "category", "title_entities")}, device="cuda")
    nh, B = batch["batch_hist"].shape[0], batch["batch_size"]
    hs = torch.bincount(batch["batch_hist"], minlength=B)
    cs = torch.bincount(batch["batch_cand"], minlength=B)
    got = NewsVectorCache(mod, table).scores(torch.arange(nh), hs, torch.arange(nh, nh + batch["batch_cand"].shape[0]),
                                             cs).cpu()
    with torch.no_grad():
        want = mod(batch_to(batch, "cuda")).cpu()
    assert float((got - want).abs().max()) <= 1e-5


def test_caum_dual_loss_step_matches_oracle(engine):
    from newsreclib_amd.nrms_module import prepare_batch
    g = load_golden("caum_tiny_eval")
    cfg = CO.golden_cfg(g)
    mod = CO.build_module(cfg, CO.golden_params(cfg), dual_loss_training=True, dual_loss_coef=0.3,
                          loss="dual_loss").eval()
    pb = prepare_batch(batch_to(CO.golden_batch(g), "cuda"))
    got = mod.model_step(pb)[0]
    with torch.no_grad():
        scores = mod(pb).cpu()
    y_true, mask = to_dense_batch(pb["labels"].cpu(), pb["batch_cand"].cpu(), pb["batch_size"])
    want = LO.dual_loss(scores, y_true, mask, 0.3)
    assert abs(float(got.detach()) - float(want)) <= 5e-5 * max(1.0, abs(float(want)))
    got.backward()
    assert all(p.grad is not None and float(p.grad.norm()) > 0 for p in mod.parameters())


def test_caum_trainer_updates_every_parameter():
    from newsreclib_amd.trainer import NRMSTrainer
    g, cfg, mod = _golden_module("caum_tiny_train")
    before = {k: p.detach().clone() for k, p in mod.named_parameters()}
    loss = NRMSTrainer(mod, lr=1e-3).step(batch_to(CO.golden_batch(g), "cuda"))
    assert np.isfinite(float(loss))
    for k, p in mod.named_parameters():
        assert float((p.detach() - before[k]).abs().max()) > 0.0, k


def test_caum_steps_are_reproducible(engine, monkeypatch):
    runs = []
    for _ in range(2):
        g, cfg, mod = _golden_module("caum_full_train", monkeypatch)
        loss = mod.model_step(batch_to(CO.golden_batch(g), "cuda"))[0]
        loss.backward()
        runs.append((loss.detach().cpu(), {k: v.detach().cpu().clone() for k, v in module_grads(mod).items()}))
    assert torch.equal(runs[0][0], runs[1][0])
    for k in runs[0][1]:
        a, b = runs[0][1][k], runs[1][1][k]
        if k.startswith("user_encoder.dense_att.linear3."):
            assert torch.equal(a, b), k            # the CAUM score kernel reduces in a fixed order
        else:
            # GEMM weight gradients and the sorted table gradients add split partial sums atomically
            assert float((a - b).abs().max()) <= 1e-5 * max(1.0, float(a.abs().max())), k


@pytest.mark.parametrize("how", ["load_state_dict", "optimizer_step", "copy_"])
def test_caum_padded_weights_follow_weight_writes(how, engine):
    g, cfg, mod = _golden_module("caum_tiny_eval")
    params = CO.golden_params(cfg)
    batch = CO.golden_batch(g)
    with torch.no_grad():
        mod(batch_to(batch, "cuda"))
    key = CO.TXT + "multihead_attention.in_proj_weight"
    w = mod.news_encoder.text_encoders["title"].multihead_attention.in_proj_weight
    new = {k: v.clone() for k, v in params.items()}
    new[key] = new[key] * -1.5
    if how == "load_state_dict":
        mod.load_state_dict(new, strict=True)
    elif how == "copy_":
        with torch.no_grad():
            w.copy_(new[key].cuda())
    else:
        opt = torch.optim.SGD([w], lr=1.0)
        w.grad = (w.detach() - new[key].cuda())
        opt.step()
        new[key] = w.detach().cpu().clone()
    with torch.no_grad():
        got = mod(batch_to(batch, "cuda")).cpu()
    want = CO.caum_forward(batch, new, cfg)["scores"]
    assert float((got - want).abs().max()) <= 1e-4
