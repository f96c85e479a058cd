"""CAUM drop-in contract on the host: constructor, state-dict keys and shapes against the reference
(tests/golden/caum_contract.json), and the configurations the module refuses."""
import inspect
import json
import os

import pytest
import torch

from tests import caum_oracle as CO

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _contract():
    with open(os.path.join(GOLDEN, "caum_contract.json")) as f:
        return json.load(f)


def _cfg(**over):
    c = _contract()["config"]
    cfg = dict(vocab=c["vocab"], n_ent=c["num_entities"], n_categ=c["num_categ_classes"] + 1, D=c["text_embed_dim"],
               Dh=c["text_num_heads"], Dc=c["categ_embed_dim"], Ed=c["entity_embed_dim"], Eh=c["entity_num_heads"],
               Q=c["query_dim"], N=c["news_embed_dim"], F=c["num_filters"], h1=c["dense_att_hidden_dim1"],
               h2=c["dense_att_hidden_dim2"], p_drop=0.2, use_entities=True, late_fusion=False)
    cfg.update(over)
    return cfg


def _module(cfg=None, **over):
    from newsreclib_amd.caum_module import CAUMModule
    cfg = cfg or _cfg()
    kw = CO.module_kwargs(cfg, pretrained_word_embeddings=torch.randn(cfg["vocab"], cfg["D"]),
                          pretrained_entity_embeddings=torch.randn(cfg["n_ent"], cfg["Ed"]))
    kw.update(over)
    return CAUMModule(**kw)


def test_caum_module_kwargs_match_reference():
    from newsreclib_amd.caum_module import CAUMModule
    ours = [p for p in inspect.signature(CAUMModule.__init__).parameters if p != "self"]
    assert ours[:-2] == _contract()["init_kwargs"]
    assert len(ours[:-2]) == 33
    assert ours[-2:] == ["pretrained_word_embeddings", "pretrained_entity_embeddings"]


def test_caum_state_dict_matches_reference():
    got = {k: list(v.shape) for k, v in _module().state_dict().items()}
    assert got == _contract()["state_dict"]


def test_caum_use_plm_raises():
    with pytest.raises(NotImplementedError):
        _module(use_plm=True, plm_model="roberta-base")


def test_caum_news_dim_must_equal_user_dim():
    with pytest.raises(ValueError):
        _module(user_vector_dim=200)


def test_caum_without_entities_and_late_fusion():
    mod = _module(_cfg(use_entities=False, late_fusion=True))
    keys = mod.state_dict().keys()
    assert not any(k.startswith("user_encoder.") for k in keys)
    assert not any("entity_encoders" in k for k in keys)
    assert mod.news_encoder.combine_layer.weight.shape == (400, 400)
    assert mod.news_encoder.entity_attrs == ()


def test_caum_encoder_declares_entity_inputs():
    enc = _module().news_encoder
    assert enc.entity_attrs == ("title_entities",)
    # the reference head dims (300 / 20, 100 / 20) run the head-padded attention; the user encoder's 400 / 20 is built
    assert enc.text_encoders["title"].padded_heads and enc.entity_encoders["title_entities"].padded_heads


def test_padded_attention_params_keep_reference_layout():
    from newsreclib_amd.ops_caum import padded_attention_params
    mha = torch.nn.MultiheadAttention(embed_dim=100, num_heads=20)
    w_in, b_in, w_o, dhp, scale = padded_attention_params(mha, 20)
    assert dhp == 16 and w_in.shape == (3 * 320, 100) and w_o.shape == (100, 320)
    assert abs(scale - 5 ** -0.5) < 1e-9
    # head 3, feature 2 of q / k / v and of the out-projection's input
    for part in range(3):
        assert torch.equal(w_in[part * 320 + 3 * 16 + 2], mha.in_proj_weight[part * 100 + 3 * 5 + 2])
    assert torch.equal(w_o[:, 3 * 16 + 2], mha.out_proj.weight[:, 3 * 5 + 2])
    assert float(w_in[5].abs().sum()) == 0.0 and float(w_o[:, 15].abs().sum()) == 0.0
    (w_in.sum() + 2 * w_o.sum() + b_in.sum()).backward()
    assert torch.equal(mha.in_proj_weight.grad, torch.ones_like(mha.in_proj_weight))
    assert torch.equal(mha.out_proj.weight.grad, torch.full_like(mha.out_proj.weight, 2.0))


def test_category_encoder_with_dropout_builds():
    from newsreclib_amd.news_encoder import LinearEncoder
    enc = LinearEncoder(pretrained_embeddings=None, from_pretrained=False, freeze_pretrained_emb=False, num_categories=19,
                        embed_dim=100, use_dropout=True, dropout_probability=0.2, linear_transform=True, output_dim=100)
    assert sorted(enc.state_dict()) == ["embedding_layer.weight", "linear.bias", "linear.weight"]
    assert enc.dropout.p == 0.2
