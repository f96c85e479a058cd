"""NPA drop-in contract on the host: constructor, state-dict keys and shapes against the reference
(tests/golden/npa_contract.json), the window-size restriction, and the encode-once cache's refusal."""
import pytest
import torch

from tests import builders
from tests import npa_oracle as NO


def test_npa_module_kwargs_match_reference():
    import inspect

    from newsreclib_amd.npa_module import NPAModule
    ours = [p for p in inspect.signature(NPAModule.__init__).parameters if p != "self"]
    assert ours[:-1] == builders.npa_contract()["init_kwargs"]
    assert ours[-1] == "pretrained_embeddings"
    assert set(builders.npa_contract()["init_kwargs"]) >= set(builders.npa_contract()["yaml_keys"]) - {"_target_"}


def test_npa_state_dict_matches_reference():
    mod = builders.npa_contract_module()
    got = {k: list(v.shape) for k, v in mod.state_dict().items()}
    assert got == builders.npa_contract()["state_dict"]
    assert float(mod.user_projection.user_embed.detach().min()) >= 0.0     # torch.rand, as projection.py:40


def test_npa_late_fusion_has_no_user_encoder():
    mod = builders.npa_contract_module(late_fusion=True)
    assert not any(k.startswith("user_encoder.") for k in mod.state_dict())


def test_npa_window_size_other_than_3_raises():
    with pytest.raises(NotImplementedError):
        builders.npa_contract_module(window_size=5)


def test_news_vector_cache_refuses_npa():
    from newsreclib_amd.evaluation import DeviceNewsTable, NewsVectorCache
    mod = builders.npa_contract_module()
    table = DeviceNewsTable({"title": torch.ones(4, 6, dtype=torch.int64)}, device="cpu")   # refused before any device work
    with pytest.raises(NotImplementedError):
        NewsVectorCache(mod, table).build()


# ---- input generators of the op-level shape sweep (tests/sweep_inputs.py, run on the GPU by test_gpu_npa_dkn_sweep.py) ------
def test_sweep_npa_conv_inputs_are_exact_in_float32():
    """Grid-valued inputs: the float32 oracle's conv features equal the float64 ones bit for bit, with and without the
    dropout multipliers, and no pre-activation is closer to zero than 1/256 -- no ReLU can decide differently."""
    from tests import sweep_inputs as S
    assert {c["F"] for c in S.NPA_ENCODER_CASES} >= {4, 64, 256, 260, 516, 772, 1024}
    assert {c["L"] for c in S.NPA_ENCODER_CASES} >= {1, 2, 3, 4, 5, 30}
    # the GPU test's "d_queries of a query without rows is exactly 0" needs such a query: in the F sweep and in the L sweep
    for sweep in "FL":
        assert any(0 in S.cached_inputs("npa_encoder", i)["counts"]
                   for i, c in enumerate(S.NPA_ENCODER_CASES) if c["name"].startswith(sweep)), sweep
    assert {c["layout"] for c in S.NPA_ENCODER_CASES} >= {"module", "one", "gaps"}
    for i, case in enumerate(S.NPA_ENCODER_CASES):
        assert 3 * case["D"] <= 1536 and case["p"] in (0.0, 0.5)
        inp = S.cached_inputs("npa_encoder", i)
        assert int((inp["ids"] == 0).sum()) >= 1
        z = S.npa_conv_pre(inp, torch.float64)
        assert float(z.abs().min()) >= 1.0 / 256, case["name"]
        assert torch.equal(S.npa_conv_pre(inp, torch.float32).double(), z), case["name"]
        r64, r32 = S.cached("npa_encoder", i, "float64"), S.cached("npa_encoder", i, "float32")
        for k in ("features", "c"):                                   # eval features; the training ones (dropout 0 / 1)
            assert torch.equal(r32[k].double(), r64[k]), (case["name"], k)


def test_sweep_npa_query_gates_are_exact_in_float32():
    from tests import sweep_inputs as S
    for i, case in enumerate(S.NPA_QUERY_CASES):
        inp = S.cached_inputs("npa_query", i)
        for z64, z32 in zip(S.npa_query_pre(case, inp, torch.float64), S.npa_query_pre(case, inp, torch.float32)):
            assert float(z64.abs().min()) >= 1.0 / 256, case["name"]
            assert torch.equal(z32.double(), z64), case["name"]
    rep = [c for c in S.NPA_QUERY_CASES if c["repeat"]]
    assert rep and int((S.cached_inputs("npa_query", S.NPA_QUERY_CASES.index(rep[0]))["user_idx"] == 4).sum()) == 3
