"""The CPU restatement of CAUM (tests/caum_oracle.py) against the goldens made from the reference's own components: scores,
loss, news vectors and the gradient norms, with the library's dropout masks under the documented streams."""
import pytest
import torch

from tests import caum_oracle as CO
from tests.helpers import load_golden


@pytest.mark.parametrize("name", CO.CAUM_CASES)
def test_caum_oracle_matches_reference_golden(name):
    g = load_golden(name)
    cfg = CO.golden_cfg(g)
    params = {k: v.clone().requires_grad_(True) for k, v in CO.golden_params(cfg).items()}
    out = CO.caum_forward(CO.golden_batch(g), params, cfg, p=cfg["p_drop"], seed=cfg["seed"],
                          late_fusion=cfg["late_fusion"], use_entities=cfg["use_entities"])
    assert float((out["scores"].detach() - torch.from_numpy(g["out_scores"])).abs().max()) <= 1e-5
    assert abs(float(out["loss"].detach()) - float(g["out_loss"])) <= 1e-5
    stride = int(g["cfg_row_stride"])
    for k in ("hist_vec", "cand_vec"):
        assert float((out[k].detach()[::stride] - torch.from_numpy(g["out_" + k])).abs().max()) <= 1e-5
    out["loss"].backward()
    for k, p in params.items():
        gr = p.grad.clone() if p.grad is not None else torch.zeros_like(p)
        if k.endswith("embedding_layer.weight"):
            gr[0] = 0.0                                      # padding_idx = 0
        got = float(gr.double().norm())
        ref = float(g["gnorm/" + k])
        assert abs(got - ref) <= 1e-4 * ref + 1e-6, (k, got, ref)


def test_caum_ragged_case_wraps_onto_pad_rows_and_full_histories():
    g = load_golden("caum_ragged")
    sizes = torch.bincount(torch.from_numpy(g["in_batch_hist"]))
    assert int(sizes.min()) < int(sizes.max()) and int((sizes == sizes.max()).sum()) >= 2
    csizes = torch.bincount(torch.from_numpy(g["in_batch_cand"]))
    assert int(csizes.min()) < int(csizes.max())
    scores = torch.from_numpy(g["out_scores"])
    for b, n in enumerate(csizes.tolist()):
        assert bool((scores[b, n:] == 0).all())
