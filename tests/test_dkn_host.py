"""DKN drop-in contract on the host: constructor, state-dict keys and shapes against the reference
(tests/golden/dkn_contract.json), the context table's initialisation, and the shapes the kernels refuse."""
import json
import os

import pytest
import torch

from tests import dkn_oracle as DO

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _contract():
    with open(os.path.join(GOLDEN, "dkn_contract.json")) as f:
        return json.load(f)


def _module(**over):
    c = _contract()["config"]
    cfg = dict(vocab=c["vocab"], n_ent=c["num_entities"], D=c["text_embed_dim"], Ed=c["entity_embed_dim"],
               F=c["num_filters"], Hd=c["hidden_dim_dnn"], windows=c["window_sizes"], use_context=c["use_context"],
               late_fusion=False)
    from newsreclib_amd.dkn_module import DKNModule
    kw = DO.module_kwargs(cfg, pretrained_word_embeddings=torch.randn(cfg["vocab"], cfg["D"]),
                          pretrained_entity_embeddings=torch.randn(cfg["n_ent"], cfg["Ed"]))
    kw.update(over)
    return DKNModule(**kw)


def test_dkn_module_kwargs_match_reference():
    import inspect

    from newsreclib_amd.dkn_module import DKNModule
    ours = [p for p in inspect.signature(DKNModule.__init__).parameters if p != "self"]
    assert ours[:-2] == _contract()["init_kwargs"]
    assert ours[-2:] == ["pretrained_word_embeddings", "pretrained_entity_embeddings"]


def test_dkn_state_dict_matches_reference():
    got = {k: list(v.shape) for k, v in _module().state_dict().items()}
    assert got == _contract()["state_dict"]


def test_dkn_context_table_starts_equal_but_is_its_own_parameter():
    enc = _module().news_encoder
    ent, ctx = enc.entity_embedding_layer.weight, enc.context_embedding_layer.weight
    assert torch.equal(ent, ctx)
    assert ent is not ctx and ent.data_ptr() != ctx.data_ptr()
    with torch.no_grad():
        ent[1, 0] += 1.0
    assert not torch.equal(ent, ctx)


def test_dkn_without_context_has_two_channels():
    mod = _module(use_context=False)
    assert not any("context_embedding_layer" in k for k in mod.state_dict())
    assert mod.news_encoder.conv_filters["3"].weight.shape[1] == 2


def test_dkn_late_fusion_has_no_user_encoder():
    mod = _module(late_fusion=True)
    assert not any(k.startswith("user_encoder.") for k in mod.state_dict())
    assert not any(k.startswith("click_predictor.") for k in mod.state_dict())


@pytest.mark.parametrize("over", [dict(num_filters=102), dict(window_sizes=[1, 2, 3, 4, 5]), dict(window_sizes=[2, 2]),
                                  dict(hidden_dim_dnn=65), dict(entity_embed_dim=98)])
def test_dkn_unsupported_shapes_raise(over):
    with pytest.raises(NotImplementedError):
        _module(**over)


def test_dkn_window_longer_than_title_raises():
    mod = _module(window_sizes=[1, 5])
    news = {"title": torch.ones(2, 4, dtype=torch.int64), "title_entities": torch.zeros(2, 4, dtype=torch.int64)}
    with pytest.raises(NotImplementedError):
        mod.news_encoder(news)


def test_dkn_encoder_declares_entity_inputs():
    assert "title_entities" in _module().news_encoder.entity_attrs


def test_add_dkn_fields_pads_after_leading_entities():
    from newsreclib_amd.synthetic import add_dkn_fields, make_batch
    b = add_dkn_fields(make_batch(4, vocab=500, mode="ragged", seed=3), n_entities=1000, seed=4)
    for side in ("x_hist", "x_cand"):
        t, e = b[side]["title"], b[side]["title_entities"]
        assert e.shape == t.shape and e.dtype == torch.int64
        assert int(e.max()) < 1000 and int(e.min()) >= 0
        assert bool((e[t == 0] == 0).all())
        nz = (e != 0).int()
        assert bool((nz[:, 1:] <= nz[:, :-1]).all())           # leading entities, then zeros


# ---- input generators of the op-level shape sweep (tests/sweep_inputs.py, run on the GPU by test_gpu_npa_dkn_sweep.py) ------
def test_sweep_dkn_fragile_share_is_within_the_cap_for_every_seed():
    """The float64 oracle alone: at most 2 % of a case's pooled outputs have a top-two gap or a |max| below 10x either
    engine's forward tolerance; the L = 255 case holds a maximum at the last valid position of every window."""
    from tests import sweep_inputs as S
    for i, case in enumerate(S.DKN_ENCODER_CASES):
        for engine in S.TOL:
            ref = S.cached("dkn_encoder", i, "float64", engine)
            assert float(ref["fragile"].float().mean()) <= S.FRAGILE_CAP, (case["name"], engine)
        if case["last"]:
            F_ = case["F"]
            for j, w in enumerate(case["windows"]):
                assert int(ref["argmax"][0, j * F_]) == case["L"] - w == (254, 251)[j]
                assert not bool(ref["fragile"][0, j * F_]) and float(ref["out"][0, j * F_]) > 0


def test_sweep_dkn_click_gates_are_clear_of_zero():
    """No pre-activation of the predictor's ReLU is within 1e-4 of zero (fp32 rounding there is ~1e-6): the gate decides
    the same in fp32 and float64.  Every case has an empty history, whose user vector is exactly zero."""
    from tests import sweep_inputs as S
    assert {c["Hd"] for c in S.DKN_CLICK_CASES} >= {1, 16, 64} and {c["dim"] for c in S.DKN_CLICK_CASES} >= {4, 32, 400, 1024}
    for i, case in enumerate(S.DKN_CLICK_CASES):
        ref = S.cached("dkn_click", i, "float64")
        assert ref["min_pre"] >= 1e-4, (case["name"], ref["min_pre"])
        assert bool(torch.isfinite(ref["scores"]).all())
        assert bool((ref["user"][case["hist"].index(0)] == 0).all())
