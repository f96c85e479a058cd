"""Op-level shape sweep of the MINER kernels (nrl_miner.hip) and of CAUM's non-attention kernels (nrl_caum.hip) against a
float64 evaluation of their CPU restatements, each op through its autograd Function in ops_miner.py / ops_caum.py.  Inputs,
case tables and references: tests/sweep_inputs_caum_miner.py; the input conditions are asserted on the host in
tests/test_caum_miner_sweep_host.py.  Branches reached (each is named in a case id or in the comment above its case table):

* ``miner_wgrad_kernel``: R = 1, 63, 64, 65, 129 (slabs of 64 rows), N % 16 != 0 (the ``n >= N`` break), 16 K / 4 > 256;
* ``miner_cb_*``: Dc / 4 > 64 and > 256, users without candidates or without history, every n_hist % 4 and n_cand % 4 (the
  padded ``rn_h`` / ``rn_c``), B = 1 (bias and both gradients exactly 0);
* ``miner_poly_*``: n = 0, 1, max_hist - 1 and max_hist in one batch, n > 64 with K n > 256, an LDS request between 64 and
  160 KiB (the ``hipFuncSetAttribute`` raise), exactly 160 KiB (the tile stays in LDS) and one step over it
  (``tile_in_lds = 0``: the history tile read through the caches);
* ``miner_score_*``: K = 1, 2, 63, 64, 65, 255 in all three modes, users with 0 candidates, counts on both sides of the
  four-wave round and of the 32-candidate backward tile, ``max_cand - nc > 256``, the weighted mode 5.5 KiB under the LDS
  limit, an exact tie of the maximum (the whole gradient at the lowest index);
* ``miner_cos_*``: D / 4 > 64 and > 256, R = 1, 2, 4, 5, 32, 65, one group and three, eps = 1e-8 and 0 (late fusion), a zero row;
* ``caum_dropout`` / ``caum_expand_*`` / ``caum_concat_dropout_*``: the per-slot streams base + 3 i + {0, 1, 2} at C > 1 and
  bases that are not the module's, bit for bit; one upstream gradient of two missing;
* ``caum_combine_*``: H = 1 and 2 (coinciding circular neighbours), hs = 1 against hs = C, F and U no multiples of 4;
* ``caum_group_tanh_*``; ``caum_score_*``: H > 256 and H = 8192, N2 and U on both sides of 64 and 256, slot0 > 0 with ragged
  lists, the column sum's chunks at R = 1, 63, 64, 65, 129, ``grad_bufs`` given and not given.

Bounds: ``Report.fwd`` / ``Report.grad``; a case wider than a configured width (MINER Dn 256, K 32, Cd 200, Dc 100, max_hist
50; CAUM U = F = 400, N2 = 200) goes through ``Report.bound`` over the same two numbers.  The vector ops are plain fp32
under both engines and run once, under the f32 tolerances; ``BiasFreeLinearFn`` runs under both engines.  Every comparison
prints a ``SWEEP`` line (``tools/sweep_errors.py --tests caum_miner`` collects them into
profiles/caum_miner_sweep_errors.txt).

``BiasFreeLinearFn``: the GEMM entries refuse N % 4 != 0 on the host (``nrl_linear_bwd_img``, ``nrl_linear_act_fwd``), so
N = 1, 15, 17, 33 of the planned shapes run at 4, 12, 20, 36 (see ``LIN_CASES``); the weight-gradient entry takes any N and
runs at the planned shapes unchanged (``test_miner_wgrad_entry_sweep``).

Out of scope: ``ops_caum.AttnFn`` and the attention kernels (``test_gpu_mins.py::test_mha_matches_oracle`` and
``test_gpu_parity.py::test_long_sequence_attention_on_matrix_cores`` cover every head dim and dispatch edge); the factored
evaluation kernels (``test_gpu_caum_factored.py`` compares them with float64); the grid-stride wrap of the element-wise
kernels (more than 16.7 M elements: not a few-second test); module-level behaviour."""
import pytest
import torch

from tests import sweep_inputs_caum_miner as S
from tests.sweep_inputs import Report

pytestmark = pytest.mark.gpu
DEV = "cuda"
VEC = "f32"                      # the engine name the vector-only ops report under: their tolerances


def _ids(cases):
    return [c["name"] for c in cases]


def _leaf(x):
    return x.to(DEV).requires_grad_(True)


def _refs(family, index):
    return S.cached(family, index, "float64"), S.cached(family, index, "float32")


def _fwd(rep, case, what, got, want, want32):
    if case["wide"]:
        rep.bound(what, got, want, want32, 5 * rep.ftol)
    else:
        rep.fwd(what, got, want, want32)


def _grad(rep, case, what, got, want, want32):
    if case["wide"]:
        rep.bound(what, got, want, want32, rep.gtol, rel=True)
    else:
        rep.grad(what, got, want, want32)


@pytest.fixture
def engine(request):
    from newsreclib_amd import _lib
    prev = _lib.get_gemm_engine()
    _lib.set_gemm_engine(request.param)
    yield request.param
    _lib.set_gemm_engine(prev)


# ---- MINER ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("engine", ["f32", "bf16x3"], indirect=True)
@pytest.mark.parametrize("act", S.LIN_ACTS, ids=["none", "tanh"])
@pytest.mark.parametrize("index", range(len(S.LIN_CASES)), ids=_ids(S.LIN_CASES))
def test_miner_bias_free_linear_sweep(index, act, engine):
    """N is a multiple of 4 in every case: the GEMM entries refuse anything else on the host (module docstring)."""
    from newsreclib_amd import ops_miner as OM
    case, inp = S.LIN_CASES[index], S.cached_inputs("lin", index)
    r64, r32 = (r[act] for r in _refs("lin", index))
    rep = Report("miner_linear", f"{case['name']}/{act or 'none'}", engine)

    def run():
        x, w = _leaf(inp["x"]), _leaf(inp["w"])
        c = OM.BiasFreeLinearFn.apply(x, w, act)
        c.backward(inp["d_out"].to(DEV))
        return c.detach(), x.grad, w.grad

    c, d_x, d_w = run()
    _fwd(rep, case, "out", c, r64["out"], r32["out"])
    _grad(rep, case, "d_x", d_x, r64["d_x"], r32["d_x"])
    _grad(rep, case, "d_w", d_w, r64["d_w"], r32["d_w"])
    rep.check("d_w bit-identical over two backward runs", torch.equal(run()[2], d_w))
    rep.done()


@pytest.mark.parametrize("index", range(len(S.WGRAD_CASES)), ids=_ids(S.WGRAD_CASES))
def test_miner_wgrad_entry_sweep(index):
    """``nrl_miner_wgrad`` as ``BiasFreeLinearFn.backward`` calls it, at the widths the Function cannot reach because its GEMM
    entries refuse them (N = 1, 15, 17, 33): plain fp32, so once, under the f32 tolerances."""
    from newsreclib_amd import _lib, ops
    case, inp = S.WGRAD_CASES[index], S.cached_inputs("wgrad", index)
    r64, r32 = _refs("wgrad", index)
    rep = Report("miner_wgrad", case["name"], VEC)
    lib = _lib.load()
    M, N, K = case["M"], case["N"], case["K"]
    g, x = inp["d_out"].to(DEV), inp["x"].to(DEV)

    def run():
        d_w = torch.empty((N, K), dtype=torch.float32, device=DEV)
        ws = ops.workspace(lib.nrl_miner_wgrad_workspace_bytes(M, N, K), g.device)
        _lib.check(lib.nrl_miner_wgrad(g.data_ptr(), x.data_ptr(), M, N, K, d_w.data_ptr(), ws.data_ptr(), ws.numel(),
                                       ops._stream()), "nrl_miner_wgrad")
        return d_w

    d_w = run()
    _grad(rep, case, "d_w", d_w, r64["d_w"], r32["d_w"])
    rep.check("d_w bit-identical over two runs", torch.equal(run(), d_w))
    rep.done()


@pytest.mark.parametrize("index", range(len(S.CB_CASES)), ids=_ids(S.CB_CASES))
def test_miner_categ_bias_sweep(index):
    from newsreclib_amd import ops_miner as OM
    case, inp = S.CB_CASES[index], S.cached_inputs("cb", index)
    r64, r32 = _refs("cb", index)
    rep = Report("miner_categ_bias", case["name"], VEC)
    hc, cc = _leaf(inp["hc"]), _leaf(inp["cc"])
    bias = OM.CategBiasFn.apply(hc, cc, inp["batch_hist"].to(DEV), inp["batch_cand"].to(DEV), inp["hist_off"].to(DEV),
                                inp["cand_off"].to(DEV), case["B"])
    bias.backward(inp["d_bias"].to(DEV))
    _fwd(rep, case, "bias", bias, r64["bias"], r32["bias"])
    _grad(rep, case, "d_hc", hc.grad, r64["d_hc"], r32["d_hc"])
    _grad(rep, case, "d_cc", cc.grad, r64["d_cc"], r32["d_cc"])
    if case["B"] == 1:           # every candidate is the user's own: s_all - s_own and q_all - q_own are exactly 0
        rep.check("B = 1: bias, d_hc and d_cc exactly 0", all(float(t.detach().abs().max()) == 0.0 for t in (bias, hc.grad, cc.grad)))
    rep.done()


@pytest.mark.parametrize("index", range(len(S.POLY_CASES)), ids=_ids(S.POLY_CASES))
def test_miner_poly_attention_sweep(index):
    """P is an input tensor (not the GEMM's output).  ``lds_160k_tile`` and ``lds_over_cache_path`` differ by one float4 of D:
    the first keeps the history tile in LDS, the second reads it through the caches; both go through the same bound."""
    from newsreclib_amd import ops_miner as OM
    case, inp = S.POLY_CASES[index], S.cached_inputs("poly", index)
    r64, r32 = _refs("poly", index)
    rep = Report("miner_poly", case["name"], VEC)
    E, P, codes = _leaf(inp["E"]), _leaf(inp["P"]), _leaf(inp["codes"])
    bias = _leaf(inp["bias"]) if case["bias"] else None
    uv = OM.PolyFn.apply(E, P, codes, bias, inp["hist_off"].to(DEV), case["B"], case["max_hist"])
    uv.backward(inp["d_uv"].to(DEV))
    _fwd(rep, case, "user_vector", uv, r64["uv"], r32["uv"])
    empty = [b for b, n in enumerate(case["hs"]) if n == 0]
    if empty:
        rep.check("an empty history gives a zero user vector", float(uv.detach()[empty].abs().max()) == 0.0)
    for name, t in (("d_E", E), ("d_P", P), ("d_codes", codes)) + ((("d_bias", bias),) if case["bias"] else ()):
        _grad(rep, case, name, t.grad, r64[name], r32[name])
    rep.done()


SCORE_PARAMS = [(i, m) for i, c in enumerate(S.SCORE_CASES) for m in c["modes"]]


@pytest.mark.parametrize("index,mode", SCORE_PARAMS, ids=[f"{S.SCORE_CASES[i]['name']}-{m}" for i, m in SCORE_PARAMS])
def test_miner_score_sweep(index, mode):
    """``tie_K5_D8``: two identical interest rows win for three candidates; the reference is the explicit lowest-index maximum
    (``lowest_index_max``), not ``torch.max``."""
    from newsreclib_amd import ops_miner as OM
    case, inp = S.SCORE_CASES[index], S.cached_inputs("score", index)
    r64, r32 = (r[mode] for r in _refs("score", index))
    rep = Report("miner_score", f"{case['name']}/{mode}", VEC)
    cand, uv = _leaf(inp["cand"]), _leaf(inp["uv"])
    Z = _leaf(inp["Z"]) if mode == "weighted" else None
    scores = OM.ScoreFn.apply(cand, uv, Z, inp["cand_off"].to(DEV), case["B"], case["max_cand"], mode)
    scores.backward(inp["d_scores"].to(DEV))
    _fwd(rep, case, "scores", scores, r64["scores"], r32["scores"])
    rep.check("padded slots are exactly 0", float(scores.detach().cpu()[~r64["mask"]].abs().max()) == 0.0)
    _grad(rep, case, "d_cand", cand.grad, r64["d_cand"], r32["d_cand"])
    _grad(rep, case, "d_uv", uv.grad, r64["d_uv"], r32["d_uv"])
    if mode == "weighted":
        _grad(rep, case, "d_Z", Z.grad, r64["d_Z"], r32["d_Z"])
    empty = [b for b, n in enumerate(case["cs"]) if n == 0]
    if empty:
        rep.check("a user without candidates: d_uv exactly 0", float(uv.grad[empty].abs().max()) == 0.0)
        if mode == "weighted":
            rep.check("a user without candidates: d_Z exactly 0", float(Z.grad[empty].abs().max()) == 0.0)
    if case["tie"]:
        b, k1, k2 = case["tie"]
        rep.check("the tie's higher index takes no gradient", float(uv.grad[b, k2].abs().max()) == 0.0)
        rep.check("the tie's lower index takes some", float(uv.grad[b, k1].abs().max()) > 0.0)
    rep.done()


@pytest.mark.parametrize("index", range(len(S.COSD_CASES)), ids=_ids(S.COSD_CASES))
def test_miner_cos_disagreement_sweep(index):
    from newsreclib_amd import ops_miner as OM
    case, inp = S.COSD_CASES[index], S.cached_inputs("cosd", index)
    r64, r32 = _refs("cosd", index)
    rep = Report("miner_cos", case["name"], VEC)
    x = _leaf(inp["x"])
    loss = OM.CosDisagreementFn.apply(x, case["eps"])
    (loss * inp["w"].to(DEV)).backward()
    _fwd(rep, case, "loss", loss.reshape(1), r64["loss"].reshape(1), r32["loss"].reshape(1))
    if case["zero_row"]:
        # the zero row's gradient is S / eps (finite, ~1e6): compared on its own, so that its size does not loosen the others
        g, r = case["zero_row"]
        rest = torch.ones(case["G"], case["R"], dtype=torch.bool)
        rest[g, r] = False
        _grad(rep, case, "d_x (zero row)", x.grad[g, r], r64["d_x"][g, r], r32["d_x"][g, r])
        _grad(rep, case, "d_x (other rows)", x.grad.cpu()[rest], r64["d_x"][rest], r32["d_x"][rest])
    else:
        _grad(rep, case, "d_x", x.grad, r64["d_x"], r32["d_x"])
    rep.done()


# ---- CAUM -------------------------------------------------------------------------------------------------------------------
def _bits(rep, what, got, want32):
    rep.check(what + " equals the float32 restatement bit for bit", torch.equal(got.detach().cpu(), want32))


@pytest.mark.parametrize("index", range(len(S.DROP_CASES)), ids=_ids(S.DROP_CASES))
def test_caum_dropout_sweep(index):
    from newsreclib_amd import ops_caum as OC
    case, inp = S.DROP_CASES[index], S.cached_inputs("drop", index)
    r64, r32 = _refs("drop", index)
    rep = Report("caum_dropout", case["name"], VEC)
    x = _leaf(inp["h"])
    y = OC.DropoutFn.apply(x, case["p"], S.DROP_SEED, case["base"])
    y.backward(inp["d_h"].to(DEV))
    _bits(rep, "y", y, r32["y"])
    if case["p"] in (0.0, 0.5):
        _bits(rep, "d_x", x.grad, r32["d_x"])
    rep.grad("d_x", x.grad, r64["d_x"], r32["d_x"])
    rep.done()


# every case with both upstream gradients; one case (B3_C4_H3, p = 0.2) also with only one of the two
EXPAND_PARAMS = [(i, None) for i in range(len(S.DROP_CASES))] + [(1, "hd"), (1, "cd")]


@pytest.mark.parametrize("index,only", EXPAND_PARAMS,
                         ids=[S.DROP_CASES[i]["name"] + ("" if o is None else "-only_d_" + o) for i, o in EXPAND_PARAMS])
def test_caum_expand_sweep(index, only):
    """``only``: one of the two outputs takes part in the loss, so the other's upstream gradient arrives as ``None``."""
    from newsreclib_amd import ops_caum as OC
    case, inp = S.DROP_CASES[index], S.cached_inputs("drop", index)
    r64, r32 = _refs("drop", index)
    rep = Report("caum_expand", case["name"] + ("" if only is None else "/only_d_" + only), VEC)
    h, c = _leaf(inp["h"]), _leaf(inp["c"])
    hd, cd = OC.ExpandFn.apply(h, c, case["p"], S.DROP_SEED, case["base"])
    _bits(rep, "hd", hd, r32["hd"])
    _bits(rep, "cd", cd, r32["cd"])
    loss = 0.0
    if only in (None, "hd"):
        loss = loss + (hd * inp["d_hd"].to(DEV)).sum()
    if only in (None, "cd"):
        loss = loss + (cd * inp["d_cd"].to(DEV)).sum()
    loss.backward()
    want_h = (r64["d_h"], r32["d_h"]) if only != "cd" else (r64["d_h"] * 0, r32["d_h"] * 0)
    want_c = (r64["d_c"], r32["d_c"]) if only != "hd" else (r64["d_c"] * 0, r32["d_c"] * 0)
    if case["p"] in (0.0, 0.5) and only is None:
        _bits(rep, "d_h", h.grad, r32["d_h"])
        _bits(rep, "d_c", c.grad, r32["d_c"])
    rep.grad("d_h", h.grad, *want_h)
    rep.grad("d_c", c.grad, *want_c)
    if only == "cd":
        rep.check("d_h exactly 0 without d_hd", float(h.grad.abs().max()) == 0.0)
    if only == "hd":
        rep.check("d_c exactly 0 without d_cd", float(c.grad.abs().max()) == 0.0)
    rep.done()


@pytest.mark.parametrize("index", range(len(S.DROP_CASES)), ids=_ids(S.DROP_CASES))
def test_caum_concat_dropout_sweep(index):
    from newsreclib_amd import ops_caum as OC
    case, inp = S.DROP_CASES[index], S.cached_inputs("drop", index)
    r64, r32 = _refs("drop", index)
    rep = Report("caum_concat_dropout", case["name"], VEC)
    cnn, a = _leaf(inp["cnn"]), _leaf(inp["a"])
    z = OC.ConcatDropoutFn.apply(cnn, a, case["B"], case["C"], case["H"], case["p"], S.DROP_SEED, case["base"])
    z.backward(inp["d_z"].to(DEV))
    _bits(rep, "z", z, r32["z"])
    if case["p"] in (0.0, 0.5):
        _bits(rep, "d_cnn", cnn.grad, r32["d_cnn"])
        _bits(rep, "d_a", a.grad, r32["d_a"])
    rep.grad("d_cnn", cnn.grad, r64["d_cnn"], r32["d_cnn"])
    rep.grad("d_a", a.grad, r64["d_a"], r32["d_a"])
    rep.done()


@pytest.mark.parametrize("index", range(len(S.COMB_CASES)), ids=_ids(S.COMB_CASES))
def test_caum_combine_sweep(index):
    from newsreclib_amd import ops_caum as OC
    case, inp = S.COMB_CASES[index], S.cached_inputs("comb", index)
    r64, r32 = _refs("comb", index)
    rep = Report("caum_combine", case["name"], VEC)
    dims = tuple(case[k] for k in ("B", "C", "H", "F", "U", "hs"))

    def run(with_s):
        P, Q = _leaf(inp["P"]), _leaf(inp["Q"])
        cnn, s = OC.CombineFn.apply(P, Q, *dims)
        loss = (cnn * inp["d_cnn"].to(DEV)).sum()
        if with_s:
            loss = loss + (s * inp["d_s"].to(DEV)).sum()
        loss.backward()
        return cnn.detach(), s.detach(), P.grad, Q.grad

    cnn, s, d_P, d_Q = run(True)
    _fwd(rep, case, "cnn", cnn, r64["cnn"], r32["cnn"])
    _fwd(rep, case, "s", s, r64["s"], r32["s"])
    _grad(rep, case, "d_P", d_P, r64["d_P"], r32["d_P"])
    _grad(rep, case, "d_Q", d_Q, r64["d_Q"], r32["d_Q"])
    _, _, d_P, d_Q = run(False)                                      # d_s arrives as None
    _grad(rep, case, "d_P (d_s is None)", d_P, r64["d_P_cnn_only"], r32["d_P_cnn_only"])
    _grad(rep, case, "d_Q (d_s is None)", d_Q, r64["d_Q_cnn_only"], r32["d_Q_cnn_only"])
    rep.done()


@pytest.mark.parametrize("index", range(len(S.GTANH_CASES)), ids=_ids(S.GTANH_CASES))
def test_caum_group_tanh_sweep(index):
    from newsreclib_amd import ops_caum as OC
    case, inp = S.GTANH_CASES[index], S.cached_inputs("gtanh", index)
    r64, r32 = _refs("gtanh", index)
    rep = Report("caum_group_tanh", case["name"], VEC)
    a, g = _leaf(inp["a"]), _leaf(inp["g"])
    z = OC.GroupTanhFn.apply(a, g, case["rows"])
    z.backward(inp["d_z"].to(DEV))
    _fwd(rep, case, "z", z, r64["z"], r32["z"])
    _grad(rep, case, "d_a", a.grad, r64["d_a"], r32["d_a"])
    _grad(rep, case, "d_g", g.grad, r64["d_g"], r32["d_g"])
    rep.done()


@pytest.mark.parametrize("bufs", [False, True], ids=["grads_returned", "grad_bufs_prefilled"])
@pytest.mark.parametrize("index", range(len(S.CSCORE_CASES)), ids=_ids(S.CSCORE_CASES))
def test_caum_score_sweep(index, bufs):
    """``grads_returned``: ``grad_bufs=None``, d_w3 and d_b3 come back through autograd.  ``grad_bufs_prefilled``: they are
    added into caller-owned buffers that hold non-zero values; the buffers must end at prefill + gradient."""
    from newsreclib_amd import ops_caum as OC
    case, inp = S.CSCORE_CASES[index], S.cached_inputs("cscore", index)
    r64, r32 = _refs("cscore", index)
    rep = Report("caum_score", case["name"] + ("/grad_bufs" if bufs else ""), VEC)
    B, C, H = case["B"], case["C"], case["H"]
    z2, w3, b3, x, cd = (_leaf(inp[k]) for k in ("z2", "w3", "b3", "x", "cd"))
    grad_bufs = [inp["prefill_w3"].to(DEV).clone(), inp["prefill_b3"].to(DEV).clone()] if bufs else None
    scores = OC.ScoreFn.apply(z2, w3, b3, x, cd, inp["cand_off"].to(DEV), B, C, case["slot0"], grad_bufs)
    scores.backward(inp["d_scores"].to(DEV))
    _fwd(rep, case, "scores", scores, r64["scores"], r32["scores"])
    pad = ~inp["valid"]
    if bool(pad.any()):
        rep.check("a padded slot scores exactly 0", float(scores.detach().cpu()[pad].abs().max()) == 0.0)
        rows = pad.reshape(-1).repeat_interleave(H)
        rep.check("the rows of a padded slot take exactly 0 in d_z2, d_x and d_cd",
                  float(z2.grad.cpu()[rows].abs().max()) == 0.0 and float(x.grad.cpu()[rows].abs().max()) == 0.0 and
                  float(cd.grad.cpu()[pad.reshape(-1)].abs().max()) == 0.0)
    for k, t in (("d_z2", z2), ("d_x", x), ("d_cd", cd)):
        _grad(rep, case, k, t.grad, r64[k], r32[k])
    if bufs:
        rep.check("no gradient is handed to autograd beside the buffers", w3.grad is None and b3.grad is None)
        for k, buf in (("w3", grad_bufs[0]), ("b3", grad_bufs[1])):
            pre = inp["prefill_" + k]
            _grad(rep, case, f"prefill + d_{k}", buf, pre.double() + r64["d_" + k], pre + r32["d_" + k])
    else:
        _grad(rep, case, "d_w3", w3.grad, r64["d_w3"], r32["d_w3"])
        _grad(rep, case, "d_b3", b3.grad, r64["d_b3"], r32["d_b3"])
    rep.done()


# ---- refused on the host, before any launch of the refused kernel: each refusal is the last thing its test does -------------
def _poly_args(K, max_hist, D, n):
    g = torch.Generator().manual_seed(7)
    E, P, codes = (torch.randn(s, generator=g) * 0.5 for s in ((n, D), (n, 4), (K, 4)))
    return _leaf(E), _leaf(torch.tanh(P)), _leaf(codes), None, torch.tensor([0, n], device=DEV), 1, max_hist


def test_miner_poly_fwd_refuses_weights_over_160k():
    """K max_hist 4 = 164,000 bytes: the weights alone exceed the LDS, with or without the history tile."""
    from newsreclib_amd import ops_miner as OM
    with pytest.raises(RuntimeError, match="nrl_miner_poly_fwd: needs 164000 bytes of LDS"):
        OM.PolyFn.apply(*_poly_args(41, 1000, 4, 2))


def test_miner_poly_bwd_refuses_a_shape_the_forward_accepts():
    """K = 21, max_hist = 1000, D = 4: the forward needs (K + D) max_hist 4 = 100,000 bytes and runs; the backward keeps the
    weights and their gradients, 2 K max_hist 4 = 168,000 bytes, and is refused by ``_lib.check`` naming the LDS need.  Pinned
    as it is today."""
    from newsreclib_amd import ops_miner as OM
    args = _poly_args(21, 1000, 4, 3)
    uv = OM.PolyFn.apply(*args)
    assert uv.shape == (1, 21, 4) and bool(torch.isfinite(uv).all())
    with pytest.raises(RuntimeError, match="nrl_miner_poly_bwd: needs 168000 bytes of LDS"):
        uv.sum().backward()


def _score_args(K, D, mode):
    g = torch.Generator().manual_seed(8)
    cand, uv, Z = (torch.randn(s, generator=g).to(DEV) for s in ((2, D), (1, K, D), (1, K, D)))
    return cand, uv, Z if mode == "weighted" else None, torch.tensor([0, 2], device=DEV), 1, 3, mode


def test_miner_score_weighted_refuses_K255_D80():
    """(2 K (D + 1) + 4 D) 4 = 166,520 bytes; D = 76 (158,296 bytes) runs in the sweep."""
    from newsreclib_amd import ops_miner as OM
    with pytest.raises(RuntimeError, match="nrl_miner_score_fwd: needs 166520 bytes of LDS"):
        OM.ScoreFn.apply(*_score_args(255, 80, "weighted"))


@pytest.mark.parametrize("mode", S.MO.SCORE_TYPES)
def test_miner_score_refuses_256_codes(mode):
    """The saved arg-max is one byte."""
    from newsreclib_amd import ops_miner as OM
    with pytest.raises(NotImplementedError, match="at most 255 context codes"):
        OM.ScoreFn.apply(*_score_args(256, 4, mode))


def test_caum_score_refuses_H8193():
    from newsreclib_amd import ops_caum as OC
    H = 8193
    g = torch.Generator().manual_seed(9)
    z2, w3, b3, x, cd = (torch.randn(s, generator=g).to(DEV) for s in ((H, 1), (1, 1), (1,), (H, 1), (1, 1)))
    with pytest.raises(RuntimeError, match="max_hist <= 8192"):
        OC.ScoreFn.apply(z2, w3, b3, x, cd, torch.tensor([0, 1], device=DEV), 1, 1, 0, None)
