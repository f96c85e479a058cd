"""The CPU restatement of NPA (tests/npa_oracle.py) against the golden vectors made from the reference's own components."""
import numpy as np
import pytest
import torch

from tests import npa_oracle as NO
from tests.helpers import check_lstur_grads, load_golden


@pytest.mark.parametrize("name", NO.NPA_CASES)
def test_npa_oracle_matches_golden(name):
    g = load_golden(name)
    cfg = NO.golden_cfg(g)
    out, grads = NO.loss_and_grads(NO.golden_batch(g), NO.golden_params(cfg), p_drop=cfg["p_drop"], seed=cfg["seed"],
                                   late_fusion=cfg["late_fusion"])
    stride = int(g["cfg_row_stride"])
    for k in ("scores", "user_vec", "loss"):
        assert float(np.abs(out[k].detach().numpy() - g["out_" + k]).max()) <= 2e-5, k
    for k in ("hist_vec", "cand_vec"):
        assert float(np.abs(out[k].detach().numpy()[::stride] - g["out_" + k]).max()) <= 2e-5, k
    check_lstur_grads(g, grads)


def test_npa_oracle_quirk_max_hist():
    """A user's vector depends on the longest history in the batch (to_dense_batch zero rows in the softmax)."""
    g = load_golden("npa_quirk")
    cfg = NO.golden_cfg(g)
    params = NO.golden_params(cfg)
    scores = {}
    for tag in ("small", "big"):
        out = NO.npa_forward(NO.golden_batch(g, tag + "/"), params)
        assert float(np.abs(out["scores"].numpy() - g[tag + "/out_scores"]).max()) <= 2e-5, tag
        scores[tag] = out["scores"]
    n = scores["small"].shape[1]
    assert float((scores["small"] - scores["big"][:2, :n]).abs().max()) > 1e-3
