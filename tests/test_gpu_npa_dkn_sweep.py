"""Op-level shape sweep of the NPA and DKN kernels against a float64 evaluation of their CPU restatements
(tests/npa_oracle.py, tests/dkn_oracle.py): every float4-chunk count of the NPA pooling kernels and both sides of their
boundaries, fewer tokens / features / history rows than waves, the strided loops past 256 threads and 64 lanes, the query
workspace with either head the wider one, empty histories and candidate lists, the DKN max-pool at W = L and at the limit of
its one-byte argmax, both column slots of the transform reduction, its row chunks and entity slices.

The inputs come from tests/sweep_inputs.py, which makes every ReLU / arg-max decision the same in fp32 and float64 (grid-valued
gate inputs for NPA, the fragile-output mask for DKN; their properties are asserted on the host in test_npa_host.py and
test_dkn_host.py).  Tolerances are the project's own, as test_gpu_shapes.py: forward 5 ftol, gradients
gtol max(1, |want|_max), against float64.  Every comparison prints a ``SWEEP`` line with the kernel's error and the float32
CPU oracle's error at the same case (tools/sweep_errors.py collects them into profiles/npa_dkn_sweep_errors.txt)."""
import pytest
import torch

from tests import dkn_oracle as DO
from tests import sweep_inputs as S
from tests.sweep_inputs import Report

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True, params=["f32", "bf16x3"])
def engine(request):
    from newsreclib_amd import _lib
    prev = _lib.get_gemm_engine()
    _lib.set_gemm_engine(request.param)
    yield request.param
    _lib.set_gemm_engine(prev)


def _ids(cases):
    return [c["name"] for c in cases]


def _run_npa_encoder(inp, case, requires_grad=True):
    from newsreclib_amd import ops_npa
    dev = {k: inp[k].cuda() for k in ("ids", "owner", "offsets", "d_out")}
    leaves = {k: inp[k].cuda().requires_grad_(requires_grad) for k in ("emb", "w", "b", "queries")}
    w_img = leaves["w"].permute(0, 2, 1).contiguous().unsqueeze(1)           # Conv1d (F, D, W) -> the kernels' (F, 1, W, D)
    out = ops_npa.NpaEncoderFn.apply(dev["ids"], leaves["emb"], w_img, leaves["b"], leaves["queries"], dev["owner"],
                                     dev["offsets"], case["p"], S.DROP_SEED, ops_npa.ENCODER_STREAM0, None)
    return out, leaves, dev


@pytest.mark.parametrize("index", range(len(S.NPA_ENCODER_CASES)), ids=_ids(S.NPA_ENCODER_CASES))
def test_npa_encoder_sweep(index, engine):
    from newsreclib_amd import ops_npa
    case, inp = S.NPA_ENCODER_CASES[index], S.cached_inputs("npa_encoder", index)
    r64, r32 = S.cached("npa_encoder", index, "float64"), S.cached("npa_encoder", index, "float32")
    rep = Report("npa_encoder", case["name"], engine)
    # the grid-valued pre-activations are exact under either engine: relu(conv) bit for bit
    feat = ops_npa.npa_conv_features(inp["ids"].cuda(), inp["emb"].cuda(), inp["w"].cuda(), inp["b"].cuda()).cpu()
    rep.check("conv features == float64 oracle, bit for bit", torch.equal(feat, r64["features"].float()))
    out, leaves, dev = _run_npa_encoder(inp, case)
    rep.fwd("out", out, r64["out"], r32["out"])
    out.backward(dev["d_out"])
    for k, name in (("emb", "d_emb"), ("w", "d_w"), ("b", "d_b"), ("queries", "d_queries")):
        rep.grad(name, leaves[k].grad, r64[name], r32[name])
    empty = [i for i, n in enumerate(inp["counts"]) if n == 0]
    rep.check("d_queries of a query without rows is exactly 0", bool((leaves["queries"].grad[empty] == 0).all()))
    rep.done()


def test_npa_encoder_random_values_forward(engine):
    """Random (not grid-valued) inputs: a ReLU may decide differently in fp32, which the forward value absorbs (the feature
    is continuous through the gate) and a gradient would not -- forward only."""
    inp = S.cached_inputs("npa_random", 0)
    r64, r32 = S.cached("npa_random", 0, "float64"), S.cached("npa_random", 0, "float32")
    rep = Report("npa_encoder", "random", engine)
    with torch.no_grad():
        out, _, _ = _run_npa_encoder(inp, S.NPA_RANDOM_CASE, requires_grad=False)
    rep.fwd("out", out, r64["out"], r32["out"])
    rep.done()


@pytest.mark.parametrize("index", range(len(S.NPA_QUERY_CASES)), ids=_ids(S.NPA_QUERY_CASES))
def test_npa_user_queries_sweep(index, engine):
    from newsreclib_amd import ops_npa
    case, inp = S.NPA_QUERY_CASES[index], S.cached_inputs("npa_query", index)
    r64, r32 = S.cached("npa_query", index, "float64"), S.cached("npa_query", index, "float32")
    rep = Report("npa_query", case["name"], engine)
    leaves = {k: inp[k].cuda().requires_grad_(True) for k in S.QUERY_KEYS if k in inp}
    args = [leaves.get(k) for k in S.QUERY_KEYS]
    res = ops_npa.NpaUserQueriesFn.apply(inp["user_idx"].cuda(), *args, case["p"], S.DROP_SEED, ops_npa.QUERY_STREAM0, None)
    if case["Pn"]:
        text, news = res
        rep.fwd("news_q", news, r64["news"], r32["news"])
        torch.autograd.backward([text, news], [inp["d_text"].cuda(), inp["d_news"].cuda()])
    else:
        text = res
        text.backward(inp["d_text"].cuda())
    rep.fwd("text_q", text, r64["text"], r32["text"])
    for k in leaves:
        rep.grad("d_" + k, leaves[k].grad, r64["d_" + k], r32["d_" + k])
    rep.done()


@pytest.mark.parametrize("index", range(len(S.NPA_ATT_CASES)), ids=_ids(S.NPA_ATT_CASES))
def test_npa_user_attention_sweep(index, engine):
    from newsreclib_amd import ops_npa
    case, inp = S.NPA_ATT_CASES[index], S.cached_inputs("npa_att", index)
    r64, r32 = S.cached("npa_att", index, "float64"), S.cached("npa_att", index, "float32")
    rep = Report("npa_att", case["name"], engine)
    hist, q = inp["hist"].cuda().requires_grad_(True), inp["q"].cuda().requires_grad_(True)
    out = ops_npa.PersonalizedUserAttentionFn.apply(hist, inp["offsets"].cuda(), case["max_hist"], q)
    rep.fwd("out", out, r64["out"], r32["out"])
    out.backward(inp["d_out"].cuda())
    # (d_hist comes from the NaN-poisoned pool: a row the kernel misses fails the finiteness check of the comparison)
    rep.grad("d_hist", hist.grad, r64["d_hist"], r32["d_hist"])
    rep.grad("d_q", q.grad, r64["d_q"], r32["d_q"])
    rep.check("the user with an empty history gets a zero vector", bool((out[1] == 0).all()) and bool((out[5] == 0).all()))
    rep.done()


@pytest.mark.parametrize("index", range(len(S.DKN_ENCODER_CASES)), ids=_ids(S.DKN_ENCODER_CASES))
def test_dkn_encoder_sweep(index, engine):
    from newsreclib_amd import ops_dkn
    case, inp = S.DKN_ENCODER_CASES[index], S.cached_inputs("dkn_encoder", index)
    r64, r32 = S.cached("dkn_encoder", index, "float64", engine), S.cached("dkn_encoder", index, "float32", engine)
    rep = Report("dkn_encoder", case["name"], engine)
    share = float(r64["fragile"].float().mean())
    print(f"SWEEP dkn_encoder/{case['name']} {engine} fragile share {share:.4f}")
    rep.check("at most 2 % of the pooled outputs are fragile", share <= S.FRAGILE_CAP)
    keys = list(inp["params"])
    leaves = {k: inp["params"][k].cuda().requires_grad_(True) for k in keys}
    windows = case["windows"]
    convs = [leaves[DO.conv_key(x, what)] for x in windows for what in ("weight", "bias")]
    images = [leaves[DO.conv_key(x, "weight")].detach().permute(0, 2, 1, 3).contiguous() for x in windows]
    out = ops_dkn.DknEncoderFn.apply(inp["ids"].cuda(), inp["ents"].cuda(), None, tuple(windows), images, None,
                                     leaves[DO.WORD], leaves[DO.ENT], leaves.get(DO.CTX), leaves[DO.TM], leaves[DO.TB], *convs)
    rep.fwd("out", out, r64["out"], r32["out"])          # forward values everywhere, fragile outputs included
    out.backward(r64["d_out"].cuda())                    # d_out is zero at the fragile outputs, on both sides
    for k in keys:
        rep.grad(k, leaves[k].grad, r64["grads"][k], r32["grads"][k])
    rep.done()


@pytest.mark.parametrize("index", range(len(S.DKN_CLICK_CASES)), ids=_ids(S.DKN_CLICK_CASES))
def test_dkn_click_sweep(index, engine):
    """Every case holds an impression with an empty history.  The reference's user encoder then takes a softmax over
    padded slots only: uniform weights over all-zero rows, u = 0, in the restated oracle once its ``finfo.min`` fill is
    created in the working dtype (as a float32 scalar it overflowed to -inf under float64 and the row became NaN;
    test_dkn_host.py asserts the oracle's u = 0).  The kernel does not expose u: its documented u = 0 shows in that
    impression's scores matching the oracle's, and their finiteness is asserted beside the comparison."""
    from newsreclib_amd import ops_dkn
    case, inp = S.DKN_CLICK_CASES[index], S.cached_inputs("dkn_click", index)
    r64, r32 = S.cached("dkn_click", index, "float64"), S.cached("dkn_click", index, "float32")
    rep = Report("dkn_click", case["name"], engine)
    keys = ["hist", "cand"] + list(S.CLICK_KEYS)
    leaves = {k: inp[k].cuda().requires_grad_(True) for k in keys}
    max_hist, max_cand = max(case["hist"]), max(case["cand"])
    scores = ops_dkn.DknClickFn.apply(leaves["hist"], inp["hist_offsets"].cuda(), max_hist, leaves["cand"],
                                      inp["cand_offsets"].cuda(), max_cand, *[leaves[k] for k in S.CLICK_KEYS])
    rep.fwd("scores", scores, r64["scores"], r32["scores"])
    rep.check("padded score slots are exactly 0", bool((scores.detach().cpu()[~r64["mask_c"]] == 0).all()))
    b0 = case["hist"].index(0)
    rep.check("empty history: finite scores", bool(torch.isfinite(scores[b0]).all()))
    scores.backward(inp["d_scores"].cuda())
    for k in keys:
        rep.grad("d_" + k, leaves[k].grad, r64["d_" + k], r32["d_" + k])
    rep.done()
