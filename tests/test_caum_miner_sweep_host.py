"""Host tier of the CAUM / MINER shape sweep (tests/sweep_inputs_caum_miner.py, run on the GPU by
tests/test_gpu_caum_miner_sweep.py): the coverage the case tables promise, the input conditions for every committed seed
(each a property of the float64 reference alone), the float32 CPU restatement of every case inside that case's bound -- the
yardstick the GPU test prints beside the kernel's error -- and the restatements themselves: the CAUM pieces composed into
``caum_oracle.user_encoder_slot``, the poly attention's detour through ``atanh`` against its projection."""
import pytest
import torch

from tests import caum_oracle as CO
from tests import sweep_inputs_caum_miner as S

F64, F32 = torch.float64, torch.float32


def _ids(cases):
    return [c["name"] for c in cases]


def _refs(family, i):
    return S.cached(family, i, "float64"), S.cached(family, i, "float32")


def _inside(case, r64, r32, fwd=(), grad=()):
    """The float32 restatement stays inside the bound the GPU test asserts under the f32 engine."""
    for kind, keys in (("fwd", fwd), ("grad", grad)):
        for k in keys:
            a, b = r64[k], r32[k]
            assert bool(torch.isfinite(a).all()) and bool(torch.isfinite(b).all()), k
            e32 = float((b.double() - a).abs().max()) if a.numel() else 0.0
            assert e32 <= S.tolerance(case, kind, a, b), (k, e32)


def test_case_tables_reach_what_they_promise():
    lin = S.LIN_CASES
    assert {c["M"] for c in lin} >= {1, 63, 64, 65, 129, 70} and {c["K"] for c in lin} >= {4, 64, 68, 256, 260}
    assert all(c["N"] % 4 == 0 and c["K"] % 4 == 0 for c in lin) and {c["N"] % 16 for c in lin} >= {0, 4, 8, 12}
    assert any(16 * c["K"] // 4 > 256 for c in lin) and any(c["N"] > 32 and c["N"] % 16 for c in lin)
    cb = S.CB_CASES
    assert {c["Dc"] for c in cb} == {4, 100, 256, 260, 1028} and {c["B"] for c in cb} == {1, 3, 5}
    assert {sum(c["hs"]) % 4 for c in cb} == {0, 1, 2, 3} and {sum(c["cs"]) % 4 for c in cb} == {0, 1, 2, 3}
    assert any(0 in c["hs"] for c in cb) and any(0 in c["cs"] for c in cb)
    assert any(h > 4 and k > 4 for c in cb for h, k in zip(c["hs"], c["cs"]))
    assert all(sum(c["hs"]) > 0 and sum(c["cs"]) > 0 for c in cb)
    po = S.POLY_CASES
    assert {c["K"] for c in po} >= {1, 4, 5, 32} and {c["bias"] for c in po} == {True, False}
    assert sum({0, 1, c["max_hist"] - 1, c["max_hist"]} <= set(c["hs"]) for c in po) >= 2
    assert any(max(c["hs"]) == 70 and c["K"] == 5 for c in po)                           # lane loops, K n > 256
    assert all(max(c["hs"]) <= c["max_hist"] and c["D"] % 4 == 0 and c["Cd"] % 4 == 0 for c in po)
    by = {c["name"]: c for c in po}
    assert S.LDS_RAISE < by["lds_82k_raise"]["lds"] < S.LDS_MAX
    tile, over = by["lds_160k_tile"], by["lds_over_cache_path"]
    assert (tile["max_hist"], tile["D"], tile["Cd"], tile["K"]) == (128, 316, 8, 4) and tile["lds"] == S.LDS_MAX
    assert (over["max_hist"], over["D"], over["Cd"], over["K"]) == (128, 320, 8, 4) and over["lds"] > S.LDS_MAX
    assert over["K"] * over["max_hist"] * 4 <= S.LDS_MAX                                 # accepted: only the tile leaves LDS
    assert all(c["lds"] <= S.LDS_MAX or c is over for c in po)
    assert all(2 * c["K"] * c["max_hist"] * 4 <= S.LDS_MAX for c in po)                  # every backward is accepted
    for c in (tile, over):                                                              # one full history, the rest short
        assert sorted(c["hs"])[-1] == c["max_hist"] and sorted(c["hs"])[-2] <= 1
    sc = S.SCORE_CASES
    for mode in S.MO.SCORE_TYPES:
        mine = [c for c in sc if mode in c["modes"] and not c["tie"]]
        assert {c["K"] for c in mine} >= {1, 2, 63, 64, 65, 255} and {c["D"] for c in mine} >= {4, 64, 68, 256}, mode
        assert {n for c in mine for n in c["cs"]} >= {0, 1, 3, 4, 5, 31, 32, 33, 65}, mode
        assert any(c["max_cand"] - min(c["cs"]) > 256 and min(c["cs"]) > 0 for c in mine), mode
    assert all(c["max_cand"] > max(c["cs"]) and c["K"] <= 255 for c in sc)
    assert all(c["D"] >= 32 for c in sc if c["K"] == 255)
    lds = lambda c, mode: ((2 if mode == "weighted" else 1) * c["K"] * (c["D"] + 1) + 4 * c["D"]) * 4  # noqa: E731
    assert all(lds(c, m) <= S.LDS_MAX for c in sc for m in c["modes"])
    assert max(lds(c, "weighted") for c in sc if "weighted" in c["modes"]) == 158296
    co = S.COSD_CASES
    assert {c["R"] for c in co} >= {1, 2, 4, 5, 32, 65} and {c["D"] for c in co} >= {4, 256, 260, 1028}
    assert {c["G"] for c in co} == {1, 3} and {c["eps"] for c in co} == {1e-8, 0.0}
    assert any((c["G"], c["R"], c["eps"]) == (1, 65, 0.0) for c in co) and sum(c["zero_row"] is not None for c in co) == 1
    dr = S.DROP_CASES
    assert {c["B"] for c in dr} == {1, 3} and {c["C"] for c in dr} == {1, 4} and {c["H"] for c in dr} == {1, 3}
    for k in ("D", "F", "U"):
        assert {c[k] for c in dr} == {1, 3, 4, 5, 8}, k
    assert {c["p"] for c in dr} == {0.0, 0.2, 0.5} and all(c["base"] != 0 for c in dr)
    cm = S.COMB_CASES
    assert {c["H"] for c in cm} >= {1, 2, 3, 7} and {c["C"] for c in cm} >= {1, 3}
    assert {c["F"] for c in cm} >= {1, 3, 4, 5} and {c["U"] for c in cm} >= {1, 3, 4, 5}
    assert any(c["hs"] == 1 and c["C"] == 3 for c in cm) and any(c["hs"] == 3 and c["C"] == 3 for c in cm)
    assert any((c["B"], c["C"], c["H"], c["F"], c["U"]) == (2, 2, 5, 400, 400) for c in cm)
    assert [(c["G"], c["rows"], c["N"]) for c in S.GTANH_CASES] == [(1, 1, 1), (3, 7, 5), (4, 50, 200)]
    cs = S.CSCORE_CASES
    assert {c["H"] for c in cs} >= {1, 3, 4, 5, 64, 257, 8192} and {c["N2"] for c in cs} >= {1, 63, 64, 65, 200}
    assert {c["U"] for c in cs} >= {1, 63, 64, 65, 257, 400} and {c["B"] * c["C"] * c["H"] for c in cs} >= {1, 63, 64, 65, 129}
    assert {c["slot0"] for c in cs} == {0, 2} and any(0 in c["counts"] for c in cs) and all(c["H"] <= 8192 for c in cs)
    assert any(c["slot0"] == 2 and 0 in c["counts"] and len(set(c["counts"])) > 2 for c in cs)          # slot0 > 0, ragged
    assert all(len(c["counts"]) == c["B"] for c in cs)
    for family, (cases, _, _) in S.FAMILIES.items():                # committed seeds and names, distinct inside a family
        assert len({c["seed"] for c in cases}) == len(cases) == len({c["name"] for c in cases}), family


# ---- MINER ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", range(len(S.LIN_CASES)), ids=_ids(S.LIN_CASES))
def test_linear_float32_restatement(index):
    case = S.LIN_CASES[index]
    r64, r32 = _refs("lin", index)
    for act in S.LIN_ACTS:
        _inside(case, r64[act], r32[act], fwd=("out",), grad=("d_x", "d_w"))


@pytest.mark.parametrize("index", range(len(S.WGRAD_CASES)), ids=_ids(S.WGRAD_CASES))
def test_wgrad_float32_restatement(index):
    case = S.WGRAD_CASES[index]
    assert (case["M"], case["N"], case["K"]) == [(1, 1, 4), (63, 15, 64), (64, 16, 64), (65, 17, 68), (129, 33, 260), (70, 200, 256)][index]
    _inside(case, *_refs("wgrad", index), grad=("d_w",))


@pytest.mark.parametrize("index", range(len(S.CB_CASES)), ids=_ids(S.CB_CASES))
def test_categ_bias_inputs_and_float32_restatement(index):
    case, inp = S.CB_CASES[index], S.cached_inputs("cb", index)
    r64, r32 = _refs("cb", index)
    assert float(inp["hc"].double().norm(dim=1).min()) >= S.MIN_NORM and float(inp["cc"].double().norm(dim=1).min()) >= S.MIN_NORM
    _inside(case, r64, r32, fwd=("bias",), grad=("d_hc", "d_cc"))
    if case["B"] == 1:
        # every candidate is the user's own.  bias and d_hc are exact zeros; d_cc is the difference of one sum taken in two
        # orders (a broadcast and an index_add), 0 or one rounding of it -- the kernel's q_all - q_own is the same float twice
        assert float(r64["bias"].abs().max()) == 0.0 and float(r64["d_hc"].abs().max()) == 0.0
        assert float(r64["d_cc"].abs().max()) <= 1e-15 and float(r32["bias"].abs().max()) == 0.0
    # the flat form is the materialised (B, H, n_cand) bias of the reference, averaged over the whole candidate axis
    dense = S.MO.categ_bias_dense(inp["hc"].double(), inp["cc"].double(), inp["batch_hist"], inp["batch_cand"], case["B"])
    flat = dense.mean(dim=2)[inp["batch_hist"], torch.cat([torch.arange(n) for n in case["hs"]])]
    assert torch.allclose(flat, r64["bias"], rtol=0.0, atol=1e-14)


@pytest.mark.parametrize("index", range(len(S.POLY_CASES)), ids=_ids(S.POLY_CASES))
def test_poly_inputs_and_float32_restatement(index):
    case, inp = S.POLY_CASES[index], S.cached_inputs("poly", index)
    r64, r32 = _refs("poly", index)
    keys = ("d_E", "d_P", "d_codes") + (("d_bias",) if case["bias"] else ())
    _inside(case, r64, r32, fwd=("uv",), grad=keys)
    P = inp["P"].double()
    assert float(P.abs().max()) < 1.0 and float((torch.tanh(torch.atanh(P)) - P).abs().max()) <= 1e-15
    w = r64["weights"]                                               # (B, K, max_hist): padded positions take part
    assert torch.allclose(w.sum(-1), torch.ones(case["B"], case["K"], dtype=F64), atol=1e-12)
    for b, n in enumerate(case["hs"]):
        if n == 0:
            assert float(r64["uv"][b].abs().max()) == 0.0            # every position padded: zero embeddings
        if n < case["max_hist"]:                                     # the 1e-30 fill is a logit, not -inf
            assert float(w[b, :, n:].min()) > 0.0
    # the closed form the kernel computes: n logits and (max_hist - n) times exp(1e-30 - m) in the denominator
    logits = P @ inp["codes"].double().t() + (inp["bias"].double().unsqueeze(1) if case["bias"] else 0.0)
    off = inp["hist_off"].tolist()
    for b, n in enumerate(case["hs"]):
        lg = logits[off[b]:off[b + 1]].t()                            # (K, n)
        den = torch.exp(lg).sum(-1) + (case["max_hist"] - n) * torch.exp(torch.tensor(1e-30, dtype=F64))
        uv = (torch.exp(lg) / den.unsqueeze(1)) @ inp["E"].double()[off[b]:off[b + 1]]
        assert torch.allclose(uv, r64["uv"][b], rtol=0.0, atol=1e-12)


@pytest.mark.parametrize("index", range(len(S.SCORE_CASES)), ids=_ids(S.SCORE_CASES))
def test_score_inputs_and_float32_restatement(index):
    case, inp = S.SCORE_CASES[index], S.cached_inputs("score", index)
    r64, r32 = _refs("score", index)
    if "max" in case["modes"]:
        gaps = S.score_gaps(case, inp)
        assert gaps.numel() == sum(case["cs"]) and float(gaps.min()) >= S.MAX_GAP
    for mode in case["modes"]:
        a, b = r64[mode], r32[mode]
        _inside(case, a, b, fwd=("scores",), grad=("d_cand", "d_uv") + (("d_Z",) if mode == "weighted" else ()))
        assert float(a["scores"][~a["mask"]].abs().max()) == 0.0 and int(a["mask"].sum()) == sum(case["cs"])
        for u, n in enumerate(case["cs"]):
            if n == 0:
                assert float(a["d_uv"][u].abs().max()) == 0.0 and (mode != "weighted" or float(a["d_Z"][u].abs().max()) == 0.0)
    if case["tie"]:
        u, k1, k2 = case["tie"]
        assert k1 < k2 and torch.equal(inp["uv"][u, k1], inp["uv"][u, k2])
        S64, _, mask = S.score_matching(case, inp, F64)
        S32, _, _ = S.score_matching(case, inp, F32)
        assert torch.equal(S64[u, :, k1], S64[u, :, k2]) and torch.equal(S32[u, :, k1], S32[u, :, k2])
        won = (r64["max"]["argmax"][u] == k1) & mask[u]
        assert int(won.sum()) >= S.TIE_ROWS and not bool(((r64["max"]["argmax"][u] == k2) & mask[u]).any())
        assert torch.equal(r64["max"]["argmax"][mask], r32["max"]["argmax"][mask])
        assert float(r64["max"]["d_uv"][u, k2].abs().max()) == 0.0 and float(r64["max"]["d_uv"][u, k1].abs().max()) > 0.0
        # away from the tie the explicit lowest-index maximum is torch.max
        assert torch.equal(r64["max"]["scores"][mask], S64.max(dim=2)[0][mask])
    elif "max" in case["modes"]:
        Smat, _, mask = S.score_matching(case, inp, F64)
        assert torch.equal(S.lowest_index_max(Smat)[0][mask], r64["max"]["scores"][mask])


@pytest.mark.parametrize("index", range(len(S.COSD_CASES)), ids=_ids(S.COSD_CASES))
def test_cos_disagreement_inputs_and_float32_restatement(index):
    case, inp = S.COSD_CASES[index], S.cached_inputs("cosd", index)
    r64, r32 = _refs("cosd", index)
    norms = inp["x"].double().norm(dim=-1)
    zero = norms == 0
    assert bool(((norms >= S.MIN_NORM) | zero).all()) and int(zero.sum()) == (1 if case["zero_row"] else 0)
    _inside(case, r64, r32, fwd=("loss",))
    if case["zero_row"]:
        assert case["eps"] == 1e-8 and bool(zero[case["zero_row"]])
        g, r = case["zero_row"]
        row = r64["d_x"][g, r]
        assert bool(torch.isfinite(r64["d_x"]).all()) and 1e5 < float(row.abs().max()) < 1e9      # of order w / eps / (G R R)
        rest = ~zero
        for a, b in ((row, r32["d_x"][g, r]), (r64["d_x"][rest], r32["d_x"][rest])):
            _inside(case, {"x": a}, {"x": b}, grad=("x",))
        assert float(r64["d_x"][rest].abs().max()) < 100.0
    else:
        _inside(case, r64, r32, grad=("d_x",))
    if case["eps"] == 0.0 and case["G"] == 1:                        # the late-fusion form is ONE 2-D cosine matrix
        want = S.MO.cosine_2d(inp["x"][0].double(), inp["x"][0].double(), zero_diagonal=True).mean()
        assert float(want) == float(r64["loss"])


# ---- CAUM -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", range(len(S.DROP_CASES)), ids=_ids(S.DROP_CASES))
def test_dropout_masks_and_float32_restatement(index):
    case, inp = S.DROP_CASES[index], S.cached_inputs("drop", index)
    r64, r32 = _refs("drop", index)
    B, C, H, D, W, p = case["B"], case["C"], case["H"], case["D"], case["F"] + case["U"], case["p"]
    scale = 1.0 / (1.0 - p)
    for i in range(C):
        m = S.slot_masks(case, i)
        assert [tuple(x.shape) for x in m] == [(B, D), (B, H, D), (B, H, W)]
        for j, x in enumerate(m):
            assert x.dtype == F32 and bool(((x == 0) | (x == torch.tensor(scale, dtype=F32))).all())
            assert torch.equal(x, S.dropout_multiplier(S.DROP_SEED, case["base"] + 3 * i + j, p, x.shape))
    if p == 0.5 and B * H * W >= 24:                                 # slots draw different masks
        assert C == 1 or not torch.equal(S.slot_masks(case, 0)[2], S.slot_masks(case, 1)[2])
    keys = ("y", "d_x", "hd", "cd", "d_h", "d_c", "z", "d_cnn", "d_a")
    _inside(case, r64, r32, grad=keys)
    if p in (0.0, 0.5):                                              # multipliers 1 and 2: every product is exact
        for k in keys:
            if k != "d_h":                                           # (d_h adds C products: rounded, in slot order)
                assert torch.equal(r32[k].double(), r64[k]), k


@pytest.mark.parametrize("index", range(len(S.COMB_CASES)), ids=_ids(S.COMB_CASES))
def test_combine_float32_restatement(index):
    case = S.COMB_CASES[index]
    r64, r32 = _refs("comb", index)
    _inside(case, r64, r32, fwd=("cnn", "s"), grad=("d_P", "d_Q", "d_P_cnn_only", "d_Q_cnn_only"))


@pytest.mark.parametrize("index", range(len(S.GTANH_CASES)), ids=_ids(S.GTANH_CASES))
def test_group_tanh_float32_restatement(index):
    r64, r32 = _refs("gtanh", index)
    _inside(S.GTANH_CASES[index], r64, r32, fwd=("z",), grad=("d_a", "d_g"))


@pytest.mark.parametrize("index", range(len(S.CSCORE_CASES)), ids=_ids(S.CSCORE_CASES))
def test_caum_score_inputs_and_float32_restatement(index):
    case, inp = S.CSCORE_CASES[index], S.cached_inputs("cscore", index)
    r64, r32 = _refs("cscore", index)
    _inside(case, r64, r32, fwd=("scores",), grad=("d_z2", "d_w3", "d_b3", "d_x", "d_cd"))
    pad = ~inp["valid"]
    assert inp["valid"].shape == (case["B"], case["C"])
    for b, n in enumerate(case["counts"]):
        assert inp["valid"][b].tolist() == [case["slot0"] + i < n for i in range(case["C"])]
    if bool(pad.any()):
        rows = pad.reshape(-1).repeat_interleave(case["H"])
        assert float(r64["scores"][pad].abs().max()) == 0.0
        assert all(float(r64[k][rows].abs().max()) == 0.0 for k in ("d_z2", "d_x")) and float(r64["d_cd"][pad.reshape(-1)].abs().max()) == 0.0
    if case["H"] > 256:                                              # the peaked rows carry the softmax: each is visible
        G, H = case["B"] * case["C"], case["H"]
        w = torch.softmax((inp["z2"].double() @ inp["w3"].double().t() + inp["b3"].double()).reshape(G, H), dim=-1)
        peaks = list(S.cscore_peaks(H))
        assert float(w[:, peaks].min()) >= 0.01 and float(w[:, peaks].sum(-1).min()) >= 0.5
    assert float(inp["prefill_w3"].abs().min()) > 0.0 and float(inp["prefill_b3"].abs().min()) > 0.0


@pytest.mark.parametrize("p", [0.0, 0.5])
def test_caum_pieces_compose_to_the_oracle_slot(p):
    """``combine``, ``group_tanh`` and ``dense_att_score`` with the projections between them are
    ``caum_oracle.user_encoder_slot`` (float64), masks of ``slot_masks`` included: the pieces the sweep compares the kernels
    with are the oracle's, not a second opinion."""
    cfg = dict(vocab=11, n_ent=7, n_categ=5, D=8, Dh=2, Dc=4, Ed=8, Eh=2, Q=6, N=8, F=6, h1=5, h2=4)
    prm = {k: v.double() for k, v in CO.make_caum_params(cfg, seed=3).items()}
    B, H, N, F_, U, heads = 3, 4, cfg["N"], cfg["F"], cfg["N"], cfg["Dh"]
    g = torch.Generator().manual_seed(4)
    h, c = torch.randn(B, H, N, generator=g).double(), torch.randn(B, N, generator=g).double()
    m = [x.double() for x in S.slot_masks(dict(B=B, H=H, D=N, F=F_, U=U, p=p, base=19), 1)]
    want = CO.user_encoder_slot(h, c, prm, heads, *(m if p > 0 else (None, None, None)))
    ue = CO.UE
    hd, cd = h * m[1], c * m[0]
    w1, b1, w2, b2 = prm[ue + "linear1.weight"], prm[ue + "linear1.bias"], prm[ue + "linear2.weight"], prm[ue + "linear2.bias"]
    rows = hd.reshape(B * H, N)
    P = torch.cat([rows @ w1[:, :N].t() + b1, rows @ w1[:, N:2 * N].t(), rows @ w1[:, 2 * N:3 * N].t(),
                   rows @ w2[:, N:].t() + b2], dim=1)
    Q = torch.cat([cd @ w1[:, 3 * N:].t(), cd @ w2[:, :N].t()], dim=1)
    cnn, s = S.combine(P, Q, B, 1, H, F_, U, 1)
    a = CO.mha_batch_first(s.reshape(B, H, U).transpose(0, 1), prm, ue + "multihead_attention.", heads).transpose(0, 1)
    z = torch.cat([cnn.reshape(B, H, F_), a], dim=-1) * m[2]
    x = (z @ prm[ue + "linear3.weight"].t() + prm[ue + "linear3.bias"]).reshape(B * H, U)
    d = ue + "dense_att."
    wd = prm[d + "linear.weight"]
    t1 = S.group_tanh(x @ wd[:, :U].t(), cd @ wd[:, U:].t() + prm[d + "linear.bias"], H)
    t2 = torch.tanh(t1 @ prm[d + "linear2.weight"].t() + prm[d + "linear2.bias"])
    got = S.dense_att_score(t2, prm[d + "linear3.weight"], prm[d + "linear3.bias"], x, cd, B, H)
    assert torch.allclose(got, want, rtol=1e-12, atol=1e-13)
