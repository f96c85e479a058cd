"""MANNeR modules against goldens computed by the REFERENCE's own components (tests/golden/make_golden_manner.py): CRModule on a
train step (early fusion, sup_con_loss, dropout 0.2), a late-fusion CE step and an eval forward; AModule on four label layouts;
the ensemble on ragged impressions with a single-candidate NaN row.  Bounds are the project's: outputs and embeddings 1e-4,
losses 2e-4 max(1, |loss|), gradients through helpers.check_grads_against_golden at rtol 2e-4 (f32) / 6e-4 (bf16x3)."""
import pytest
import torch

from tests import manner_oracle as MO
from tests.helpers import check_grads_against_golden, load_golden, module_grads
from tests.builders import a_kwargs, cr_kwargs

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(params=["f32", "bf16x3"])
def engine(request):
    from newsreclib_amd import _lib
    prev = _lib.get_gemm_engine()
    _lib.set_gemm_engine(request.param)
    yield request.param
    _lib.set_gemm_engine(prev)


def _news(g, tag):
    return {"text": {k: torch.from_numpy(g[f"in_{tag}_text_{k}"]).to(DEV) for k in ("input_ids", "attention_mask")},
            "entities": torch.from_numpy(g[f"in_{tag}_entities"]).to(DEV)}


def _rec_batch(g):
    return {"x_hist": _news(g, "hist"), "x_cand": _news(g, "cand"), "batch_hist": torch.from_numpy(g["in_batch_hist"]).to(DEV),
            "batch_cand": torch.from_numpy(g["in_batch_cand"]).to(DEV), "labels": torch.from_numpy(g["in_labels"]).to(DEV),
            "batch_size": int(g["in_batch_size"]), "user_ids": torch.arange(int(g["in_batch_size"])).to(DEV) + 1,
            "user_idx": torch.arange(int(g["in_batch_size"])).to(DEV)}


def _load(mod, params):
    res = mod.load_state_dict(params, strict=False)
    assert not res.unexpected_keys and all(".plm_model." in k for k in res.missing_keys), res
    return mod.to(DEV)


def _cr(tmp_path, param_seed, loss, late_fusion, p):
    from newsreclib_amd.manner_cr_module import CRModule
    params = MO.make_manner_params(param_seed, True, not late_fusion)
    mod = CRModule(**cr_kwargs(MO.make_body(str(tmp_path)), loss=loss, late_fusion=late_fusion, p_drop=p if p > 0 else 0.2),
                   pretrained_entity_embeddings=params[MO.ENT + "embedding_layer.weight"].clone())
    return _load(mod, params)


def _a(tmp_path, param_seed, temperature, p):
    from newsreclib_amd.manner_a_module import AModule
    params = MO.make_manner_params(param_seed, True, False)
    mod = AModule(**a_kwargs(MO.make_body(str(tmp_path)), temperature=temperature, p_drop=p),
                  pretrained_entity_embeddings=params[MO.ENT + "embedding_layer.weight"].clone())
    return _load(mod, params)


@pytest.mark.parametrize("name", ["manner_cr_tiny_train", "manner_cr_tiny_late_fusion", "manner_cr_tiny_eval"])
def test_cr_module_matches_reference_golden(tmp_path, name, engine):
    from newsreclib_amd.dense_batch import dense_rows
    from newsreclib_amd.nrms_module import prepare_batch
    g = load_golden(name)
    p, seed, late = float(g["cfg_p_drop"]), int(g["cfg_seed"]), bool(g["cfg_late_fusion"])
    loss_name = "sup_con_loss" if int(g["cfg_sup_con"]) else "cross_entropy_loss"
    mod = _cr(tmp_path, int(g["cfg_param_seed"]), loss_name, late, p)
    mod.train(p > 0.0)
    batch = prepare_batch(_rec_batch(g), None, need_order=False)
    # the two encoder calls as forward makes them, kept for comparison
    mod.news_encoder.share_plm_bodies(batch["x_hist"], batch["x_cand"])
    hist_vec = mod.news_encoder(batch["x_hist"], seed=seed)
    cand_vec = mod.news_encoder(batch["x_cand"], seed=seed, stream_base=MO.CAND_STREAM_BASE)
    assert float((hist_vec.detach().cpu() - torch.from_numpy(g["out_hist_vec"])).abs().max()) <= 1e-4
    assert float((cand_vec.detach().cpu() - torch.from_numpy(g["out_cand_vec"])).abs().max()) <= 1e-4
    scores = mod(batch, seed=seed)
    want = torch.from_numpy(g["out_scores"])
    mask = torch.zeros(want.shape, dtype=torch.bool).reshape(-1)
    mask[batch["cand_flat_idx"].cpu()] = True
    mask = mask.reshape(want.shape)
    assert float((scores.detach().cpu() - want)[mask].abs().max()) <= 1e-4
    B = batch["batch_size"]
    y_true = dense_rows(batch["labels"], batch["batch_cand"], B, batch["max_cand"], batch["cand_offsets"], batch["cand_flat_idx"],
                        max_is_exact=True)
    loss = mod._loss(scores, y_true.float(), batch)
    ref_loss = float(g["out_loss"])
    assert abs(float(loss.detach()) - ref_loss) <= 2e-4 * max(1.0, abs(ref_loss))
    loss.backward()
    check_grads_against_golden(g, module_grads(mod), rtol=2e-4 if engine == "f32" else 6e-4)


@pytest.mark.parametrize("name", ["manner_a_tiny_categ", "manner_a_tiny_sent", "manner_a_one_class", "manner_a_all_distinct"])
def test_a_module_matches_reference_golden(tmp_path, name, engine):
    g = load_golden(name)
    p, seed = float(g["cfg_p_drop"]), int(g["cfg_seed"])
    mod = _a(tmp_path, int(g["cfg_param_seed"]), float(g["cfg_temperature"]), p).train()
    batch = {"news": _news(g, "news"), "labels": torch.from_numpy(g["in_labels"]).to(DEV)}
    emb = mod(batch, seed=seed)
    assert float((emb.detach().cpu() - torch.from_numpy(g["out_embeddings"])).abs().max()) <= 1e-4
    loss = mod.criterion(emb, batch["labels"])
    ref_loss = float(g["out_loss"])
    assert abs(float(loss.detach()) - ref_loss) <= 2e-4 * max(1.0, abs(ref_loss))
    loss.backward()
    grads = module_grads(mod)
    if name in ("manner_a_one_class", "manner_a_all_distinct"):
        assert float(loss.detach()) == 0.0 and all(float(v.abs().max()) == 0.0 for v in grads.values())
    if name == "manner_a_tiny_sent":
        assert float(g["out_rows"][4]) == 0.0                # the singleton class: no positive, dropped by the reducer
    check_grads_against_golden(g, grads, rtol=2e-4 if engine == "f32" else 6e-4)


def test_ensemble_matches_reference_golden(tmp_path, engine):
    from newsreclib_amd.manner_module import MANNERModule
    g = load_golden("manner_ens_tiny")
    seeds = [int(s) for s in g["cfg_param_seeds"]]
    subs = [_a(tmp_path / str(i), s, 0.9, 0.2).eval() for i, s in enumerate(seeds)]
    batch = _rec_batch(g)
    mask = torch.from_numpy(g["out_mask_cand"])
    for i, (cw, sw) in enumerate(MO.ENS_WEIGHTS):
        ens = MANNERModule.from_modules(subs[0], subs[1] if cw else None, subs[2] if sw else None, outputs={"test": []},
                                        categ_weight=cw, sent_weight=sw, top_k_list=[5], num_categ_classes=4,
                                        num_sent_classes=3).eval()
        with torch.no_grad():
            got = ens(batch).cpu()
        want = torch.from_numpy(g[f"out_scores_{i}"])
        assert bool(torch.isnan(got[1, 0])) and bool(torch.isnan(want[1, 0]))          # the single-candidate impression
        rows = [b for b in range(want.shape[0]) if b != 1]
        assert float((got[rows] - want[rows])[mask[rows]].abs().max()) <= 1e-4
