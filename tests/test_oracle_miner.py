"""The CPU restatement of MINER (tests/miner_oracle.py, in the reference's materialised form) against the goldens made from the
reference's own components: scores, loss, user vectors, news vectors and every gradient norm, with the library's dropout masks
under the documented streams; plus the two quirks the library's closed forms rest on."""
import pytest
import torch

from tests import miner_oracle as MO
from tests.helpers import load_golden


def _body(tmp_path, cfg):
    from transformers import AutoModel
    body = AutoModel.from_pretrained(MO.make_body(str(tmp_path), cfg))
    for name, prm in body.named_parameters():
        if any(f"layer.{i}." in name for i in MO.BODY_FROZEN):
            prm.requires_grad = False
    return body.eval()


def _check_norms(g, grads):
    for k, gr in grads.items():
        got, ref = float(gr.double().norm()), float(g["gnorm/" + k])
        assert abs(got - ref) <= 1e-4 * ref + 1e-6, (k, got, ref)


@pytest.mark.parametrize("name", MO.MINER_TINY_CASES)
def test_miner_oracle_matches_reference_golden(name, tmp_path):
    g = load_golden(name)
    cfg = MO.golden_cfg(g)
    body = _body(tmp_path, cfg)
    params = {k: v.clone().requires_grad_(True) for k, v in MO.golden_params(cfg).items()}
    out = MO.miner_forward(MO.golden_batch(g), body, params, cfg, p=cfg["p_drop"], seed=cfg["seed"])
    for k in ("scores", "user_vector", "hist_vec", "cand_vec"):
        assert float((out[k].detach() - torch.from_numpy(g["out_" + k])).abs().max()) <= 1e-5, k
    assert abs(float(out["loss"].detach()) - float(g["out_loss"])) <= 1e-5
    assert abs(float(out["disagreement"].detach()) - float(g["out_disagreement"])) <= 1e-6
    out["loss"].backward()
    grads = {k: (p.grad if p.grad is not None else torch.zeros_like(p)) for k, p in params.items()}
    grads.update({MO.TXT + "plm_model." + k: (p.grad if p.grad is not None else torch.zeros_like(p))
                  for k, p in body.named_parameters()})
    assert set(grads) == {k[len("gnorm/"):] for k in g if k.startswith("gnorm/")}
    _check_norms(g, grads)


def test_miner_oracle_matches_head_golden_at_config_widths():
    g = load_golden("miner_head_full")
    cfg = MO.golden_cfg(g)
    hist_vec, cand_vec, batch, masks = MO.head_full_case(g, cfg)
    params = {k: v.clone().requires_grad_(True) for k, v in MO.golden_params(cfg).items() if not k.startswith(MO.TXT)}
    hist_vec.requires_grad_(True)
    cand_vec.requires_grad_(True)
    out = MO.miner_head(hist_vec, cand_vec, batch, params, cfg, masks)
    sizes = torch.bincount(batch["batch_hist"])
    assert int(sizes.max()) == 50 and int(sizes.min()) == 1 and out["scores"].shape == (4, 200)
    assert float((out["scores"].detach() - torch.from_numpy(g["out_scores"])).abs().max()) <= 1e-5
    assert abs(float(out["loss"].detach()) - float(g["out_loss"])) <= 1e-5
    stride = int(g["cfg_sample_stride"])
    assert float((out["user_vector"].detach().reshape(-1)[::stride] - torch.from_numpy(g["out_user_vector"])).abs().max()) <= 1e-6
    out["loss"].backward()
    _check_norms(g, {k: p.grad for k, p in params.items()})
    for k, t in (("hist_vec", hist_vec), ("cand_vec", cand_vec)):
        ref = torch.from_numpy(g["gin_" + k])
        assert float((t.grad.reshape(-1)[::stride] - ref).abs().max()) <= 1e-6 * max(1.0, float(ref.abs().max())), k


def test_padded_rows_dilute_the_weights_when_only_max_hist_changes():
    """attention.py:117 fills masked positions with 1e-30, not -inf: widening the dense history by padded rows lowers every
    real weight of every user, by the closed-form factor den / (den + extra * exp(1e-30 - max))."""
    g = load_golden("miner_head_full")
    cfg = dict(MO.golden_cfg(g), use_categ_bias=False)
    hist_vec, cand_vec, batch, _ = MO.head_full_case(g, cfg)
    params = {k: v for k, v in MO.golden_params(cfg).items() if not k.startswith(MO.TXT)}
    a = MO.miner_head(hist_vec, cand_vec, batch, params, cfg)
    b = MO.miner_head(hist_vec, cand_vec, batch, params, cfg, max_hist=60)
    assert a["weights"].shape[2] == 50 and b["weights"].shape[2] == 60
    ratio = b["weights"][:, :, :50] / a["weights"]
    full = int(torch.argmax(torch.bincount(batch["batch_hist"])))          # the user whose history had no padded row
    assert float(ratio[full].max()) < 1.0 - 1e-3
    assert float((a["scores"] - b["scores"]).abs().max()) > 1e-5
    # a padded position's weight is exp(1e-30 - max) / den, the same for every padded position of a (user, code)
    pad = b["weights"][full, :, 50:]
    assert float((pad - pad[:, :1]).abs().max()) == 0.0 and float(pad.min()) > 0.0
    one = int(torch.argmin(torch.bincount(batch["batch_hist"])))           # a single click: 49 padded rows already
    assert float(a["weights"][one, :, 1:].min()) > 0.0


def test_category_bias_zeroes_own_candidates_and_reassociates():
    """The masked (B, H, n_cand) form equals hh . (S_all - S_own) / n_cand in fp64, and a user's own candidates do not move
    its bias while another user's do."""
    g = load_golden("miner_tiny_eval")
    cfg = MO.golden_cfg(g)
    batch = MO.golden_batch(g)
    B = batch["batch_size"]
    w = MO.golden_params(cfg)["categ_encoder.embedding_layer.weight"].double()
    hc, cc = w[batch["x_hist"]["category"]], w[batch["x_cand"]["category"]]
    dense = MO.categ_bias_dense(hc, cc, batch["batch_hist"], batch["batch_cand"], B)
    own = batch["batch_cand"].unsqueeze(0) == torch.arange(B).unsqueeze(1)
    assert float(dense[own.unsqueeze(1).expand_as(dense)].abs().max()) == 0.0
    flat = MO.categ_bias_flat(hc, cc, batch["batch_hist"], batch["batch_cand"], B)
    mean, _ = MO.to_dense_batch(flat, batch["batch_hist"], B)
    assert float((dense.mean(dim=2) - mean).abs().max()) <= 1e-15
    cc2 = cc.clone()
    cc2[batch["batch_cand"] == 0] = torch.flip(cc2[batch["batch_cand"] == 0], dims=[1]) + 0.3
    flat2 = MO.categ_bias_flat(hc, cc2, batch["batch_hist"], batch["batch_cand"], B)
    rows0 = batch["batch_hist"] == 0
    assert float((flat2[rows0] - flat[rows0]).abs().max()) <= 1e-15
    assert float((flat2[~rows0] - flat[~rows0]).abs().max()) > 1e-4


def test_max_fixture_has_no_near_ties():
    """In every valid slot the reference's largest and second-largest matching scores are >= 1e-3 apart (ten times the loosest
    score tolerance): the argmax is not a matter of rounding, so the GPU test leaves no slot out."""
    g = load_golden("miner_tiny_max")
    assert MO.SCORE_TYPES[int(g["cfg_score_type"])] == "max"
    top = torch.from_numpy(g["out_matching"]).topk(2, dim=2)[0]
    sizes = torch.bincount(torch.from_numpy(g["in_batch_cand"]))
    valid = torch.arange(top.shape[1]).unsqueeze(0) < sizes.unsqueeze(1)
    assert float((top[..., 0] - top[..., 1])[valid].min()) >= 1e-3
    assert float((torch.from_numpy(g["out_matching"]).max(dim=2)[0] - torch.from_numpy(g["out_scores"])).abs().max()) == 0.0
