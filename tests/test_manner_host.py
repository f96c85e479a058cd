"""MANNeR on the host: constructor signatures against the reference's (tests/golden/manner_contract.json), state-dict keys, the
embedding SupCon restatement against hand-computed answers, its degenerate cases, and checkpoint loading."""
import inspect
import json
import math
import os

import pytest
import torch

from tests import manner_oracle as MO
from tests.builders import MANNER_D as D, MANNER_DE as DE, N_ENT, a_kwargs, cr_kwargs, entity_table
from tests.helpers import make_tiny_roberta

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _contract():
    with open(os.path.join(GOLDEN, "manner_contract.json")) as f:
        return json.load(f)


def test_constructor_kwargs_match_reference():
    from newsreclib_amd import AModule, CRModule, MANNERModule
    c = _contract()
    for cls, key, n, extra in ((CRModule, "CRModule", 22, ["pretrained_entity_embeddings"]),
                               (AModule, "AModule", 16, ["pretrained_entity_embeddings"]),
                               (MANNERModule, "MANNERModule", 13, ["plm_model", "_modules_given"])):
        ours = [p for p in inspect.signature(cls.__init__).parameters if p != "self"]
        assert ours[:n] == c[key]["init_kwargs"] and len(c[key]["init_kwargs"]) == n
        assert ours[n:] == extra


@pytest.mark.parametrize("late_fusion", [False, True])
def test_cr_state_dict_keys(tmp_path, late_fusion):
    from newsreclib_amd.manner_cr_module import CRModule
    mod = CRModule(**cr_kwargs(make_tiny_roberta(str(tmp_path)), late_fusion=late_fusion),
                   pretrained_entity_embeddings=entity_table())
    keys = set(mod.state_dict())
    head = {k for k in keys if ".plm_model." not in k}
    want = set(_contract()["CRModule"]["head_keys_late_fusion" if late_fusion else "head_keys"])
    assert head == want
    assert all(k.startswith("news_encoder.text_encoders.text.plm_model.") for k in keys - head)
    assert mod.news_encoder.combine_layer.weight.shape == (D, D + DE)
    assert mod.news_encoder.text_encoders["text"].news_independent
    assert mod.news_encoder.entity_attrs == ("text", "entities")


def test_a_module_state_dict_and_labels(tmp_path):
    from newsreclib_amd.manner_a_module import AModule
    labels = tmp_path / "categ2index.tsv"
    labels.write_text("news\t1\nsports\t2\n")
    kw = a_kwargs(make_tiny_roberta(str(tmp_path)))
    kw["labels_path"] = str(labels)
    mod = AModule(**kw, pretrained_entity_embeddings=entity_table())
    head = {k for k in mod.state_dict() if ".plm_model." not in k}
    assert head == set(_contract()["AModule"]["head_keys"])
    assert mod.index2label == {1: "news", 2: "sports"}
    assert mod.criterion.temperature == 0.9
    assert AModule(**a_kwargs(make_tiny_roberta(str(tmp_path))), pretrained_entity_embeddings=entity_table()).index2label == {}
    # the epoch-end hooks only clear what the steps collected
    mod.val_step_outputs["embeddings"].append(torch.zeros(2, 4))
    mod.on_validation_epoch_end()
    assert mod.val_step_outputs["embeddings"] == []


def test_cr_module_ignores_temperature_as_the_reference(tmp_path):
    from newsreclib_amd.manner_cr_module import CRModule
    mod = CRModule(**cr_kwargs(make_tiny_roberta(str(tmp_path)), loss="sup_con_loss", use_entities=False))
    assert mod.hparams.temperature == 0.36 and mod.criterion.temperature == 0.1
    with pytest.raises(ValueError):
        CRModule(**cr_kwargs(make_tiny_roberta(str(tmp_path)), loss="dual_loss", use_entities=False))


def test_checkpoint_round_trip_and_weight_zero_loads_nothing(tmp_path):
    from newsreclib_amd.manner_a_module import AModule
    from newsreclib_amd.manner_cr_module import CRModule
    from newsreclib_amd.manner_module import MANNERModule
    plm = make_tiny_roberta(str(tmp_path))
    cr = CRModule(**cr_kwargs(plm, use_entities=False))
    am = AModule(**a_kwargs(plm, use_entities=False))
    with torch.no_grad():
        cr.news_encoder.text_encoders["text"].plm_model.embeddings.word_embeddings.weight[5, :4] = torch.tensor([1., 2., 3., 4.])
        am.news_encoder.text_encoders["text"].plm_model.embeddings.word_embeddings.weight[6, :2] = torch.tensor([7., 8.])
    for name, m in (("cr.ckpt", cr), ("a.ckpt", am)):
        hp = dict(vars(m.hparams))
        hp["plm_model"] = "roberta-base"                    # what a real checkpoint records: not resolvable offline
        torch.save({"state_dict": m.state_dict(), "hyper_parameters": hp}, str(tmp_path / name))
    back = CRModule.load_from_checkpoint(str(tmp_path / "cr.ckpt"), plm_model=plm)
    assert back.hparams.plm_model == plm and back.hparams.loss == "cross_entropy_loss"
    for k, v in cr.state_dict().items():
        assert torch.equal(v, back.state_dict()[k]), k
    kw = dict(outputs={"test": ["preds", "targets"]}, cr_module_module_ckpt=str(tmp_path / "cr.ckpt"), a_module_categ_ckpt=None,
              a_module_sent_ckpt=str(tmp_path / "a.ckpt"), categ_weight=0, sent_weight=-0.25, top_k_list=[5], num_categ_classes=18,
              num_sent_classes=3, save_recs=False, recs_fpath=None, optimizer=None, scheduler=None)
    ens = MANNERModule(**kw, plm_model=plm)
    assert not hasattr(ens, "a_module_categ") and isinstance(ens.a_module_sent, AModule)
    assert [w for _, w in ens.submodels()] == [1.0, -0.25]
    w = ens.a_module_sent.news_encoder.text_encoders["text"].plm_model.embeddings.word_embeddings.weight
    assert w[6, :2].tolist() == [7.0, 8.0]
    assert ens.training_step({}, 0) is None and ens.validation_step({}, 0) is None
    ens2 = MANNERModule.from_modules(cr, a_module_categ=am, outputs={"test": []}, categ_weight=0.2, sent_weight=0,
                                     top_k_list=[5], num_categ_classes=18, num_sent_classes=3)
    assert ens2.cr_module is cr and ens2.a_module_categ is am and not hasattr(ens2, "a_module_sent")
    with pytest.raises(ValueError):
        MANNERModule.from_modules(cr, outputs={"test": []}, categ_weight=0.2, sent_weight=0, top_k_list=[5],
                                  num_categ_classes=18, num_sent_classes=3)
    with pytest.raises(KeyError):
        torch.save({"weights": {}}, str(tmp_path / "bad.ckpt"))
        CRModule.load_from_checkpoint(str(tmp_path / "bad.ckpt"))


def test_supcon_restatement_hand_computed():
    # three embeddings on a line: e0 = (1, 0), e1 = (2, 0) share label 0, e2 = (0, 1) has label 1.  T = 0.5.
    # Gram / T: s01 = 4, s02 = 0, s12 = 0.  Row 0: positives {1}: loss = log(e^4 + e^0) - 4.  Row 1: the same by symmetry.
    # Row 2: no positive -> 0, dropped.  Loss = log(1 + e^-4).
    E = torch.tensor([[1., 0.], [2., 0.], [0., 1.]], dtype=torch.float64)
    labels = torch.tensor([0, 0, 1])
    rows = MO.supcon_rows(E, labels, 0.5)
    want = math.log(1.0 + math.exp(-4.0))
    assert rows.tolist() == pytest.approx([want, want, 0.0], abs=1e-14)
    loss, grad = MO.supcon_embed_with_grad(E, labels, 0.5)
    assert float(loss) == pytest.approx(want, abs=1e-14)
    # d loss / d s01 (per row, mean of two rows): (softmax_01 - 1) with softmax_01 = 1 / (1 + e^-4); s02 / s12 get softmax_02.
    q = 1.0 / (1.0 + math.exp(-4.0))
    c = 0.5 * (1.0 / 0.5)                                   # 1 / n_kept * 1 / T
    dS = torch.tensor([[0., q - 1., 1. - q], [q - 1., 0., 1. - q], [0., 0., 0.]], dtype=torch.float64) * c
    assert torch.allclose(grad, (dS + dS.t()) @ E, atol=1e-14)


def test_supcon_restatement_four_points_two_classes():
    # orthonormal embeddings: every off-diagonal score is 0, so softmax over the three others is 1/3 and every row with one
    # positive has loss log 3
    E = torch.eye(4, dtype=torch.float64)
    loss, grad = MO.supcon_embed_with_grad(E, torch.tensor([3, 7, 3, 7]), 0.9)
    assert float(loss) == pytest.approx(math.log(3.0), abs=1e-14)
    # dS_ij = (1/4) (1/0.9) (1/3 - pos_ij); dE = (dS + dS^T) E = dS + dS^T for E = I
    base = torch.full((4, 4), 1.0 / 3.0, dtype=torch.float64)
    base.fill_diagonal_(0.0)
    pos = torch.tensor([[0, 0, 1, 0], [0, 0, 0, 1], [1, 0, 0, 0], [0, 1, 0, 0]], dtype=torch.float64)
    dS = (base - pos) / (4 * 0.9)
    assert torch.allclose(grad, dS + dS.t(), atol=1e-14)


@pytest.mark.parametrize("labels", [[4, 4, 4, 4], [0, 1, 2, 3], [5]])
def test_supcon_restatement_degenerate_cases_are_exactly_zero(labels):
    E = torch.randn(len(labels), 8, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    loss, grad = MO.supcon_embed_with_grad(E, torch.tensor(labels), 0.9)
    assert float(loss) == 0.0 and float(grad.abs().max()) == 0.0


def test_ensemble_restatement_known_answer():
    # one table, D = 1: history mean 2, candidates 1, 2, 3 -> scores 2, 4, 6 -> mean 4, unbiased std 2 -> z = -1, 0, 1
    table = torch.tensor([[1.], [2.], [3.]], dtype=torch.float64)
    z = MO.ensemble_scores([table], [1.0], [torch.tensor([0, 2])], [torch.tensor([0, 1, 2])])
    assert z[0].tolist() == pytest.approx([-1.0, 0.0, 1.0], abs=1e-14)
    # second table 4 - x: history mean 2, candidates 3, 2, 1 -> scores 6, 4, 2 -> z = 1, 0, -1; weight 0.5 -> -0.5, 0, 0.5 in total
    two = MO.ensemble_scores([table, 4.0 - table], [1.0, 0.5], [torch.tensor([0, 2])], [torch.tensor([0, 1, 2])])
    assert two[0].tolist() == pytest.approx([-0.5, 0.0, 0.5], abs=1e-14)
    one = MO.ensemble_scores([table], [1.0], [torch.tensor([1])], [torch.tensor([2])])
    assert bool(torch.isnan(one[0]).all())                  # a single candidate: torch.std is NaN, the row is NaN


def test_make_news_batch_shapes():
    from newsreclib_amd.synthetic import make_news_batch
    b = make_news_batch(17, 5, vocab_size=200, n_entities=N_ENT, L=12)
    assert b["news"]["text"]["input_ids"].shape == (85, 12) and b["news"]["entities"].shape == (85, 10)
    assert sorted(b["labels"].tolist()) == sorted(list(range(17)) * 5)
    assert int(b["news"]["entities"].max()) < N_ENT and "entities" not in make_news_batch(2, 2, use_entities=False)["news"]
