"""The CPU restatement of DKN (tests/dkn_oracle.py) against the golden vectors made from the reference's own components."""
import numpy as np
import pytest

from tests import dkn_oracle as DO
from tests.helpers import check_lstur_grads, load_golden


@pytest.mark.parametrize("name", DO.DKN_CASES)
def test_dkn_oracle_matches_golden(name):
    g = load_golden(name)
    cfg = DO.golden_cfg(g)
    out, grads = DO.loss_and_grads(DO.golden_batch(g), DO.golden_params(cfg), cfg["windows"],
                                   late_fusion=cfg["late_fusion"])
    stride = int(g["cfg_row_stride"])
    for k in ("scores", "loss"):
        assert float(np.abs(out[k].detach().numpy() - g["out_" + k]).max()) <= 1e-5, k
    user = out["user_vec"].detach().numpy()
    want = g["out_user_vec"]
    user = user.reshape(want.shape) if cfg["late_fusion"] else user[:, :1]
    assert float(np.abs(user - want).max()) <= 1e-5
    for k in ("hist_vec", "cand_vec"):
        assert float(np.abs(out[k].detach().numpy()[::stride] - g["out_" + k]).max()) <= 1e-5, k
    check_lstur_grads(g, grads, tol=1e-5, rtol=1e-5, atol=1e-6)


def test_dkn_tie_case_has_positive_ties():
    """quirk 3: windows wholly in the padding give identical conv outputs, so the max over time ties at a positive value."""
    import torch
    import torch.nn.functional as F
    g = load_golden("dkn_tie")
    cfg = DO.golden_cfg(g)
    p = DO.golden_params(cfg)
    b = DO.golden_batch(g)
    ids, ents = b["x_hist"]["title"], b["x_hist"]["title_entities"]
    stack = torch.stack([p[DO.WORD][ids], torch.tanh(p[DO.ENT][ents] @ p[DO.TM] + p[DO.TB]),
                         torch.tanh(p[DO.CTX][ents] @ p[DO.TM] + p[DO.TB])], dim=1)
    c = torch.relu(F.conv2d(stack, p[DO.conv_key(2, "weight")], p[DO.conv_key(2, "bias")]).squeeze(3))
    mx = c.max(dim=-1, keepdim=True)[0]
    ties = ((c == mx).sum(-1) > 1) & (mx.squeeze(-1) > 0)
    assert int(ties.sum()) > 0
