"""Host tier of the LSTUR / NAML op sweep (tests/sweep_inputs_lstur_naml.py, run on the GPU by
tests/test_gpu_lstur_naml_sweep.py): the coverage the case tables promise, with the library's shape predicates recomputed in
Python; the exactness of the grid-valued ReLU gate inputs for every committed seed; the float32 CPU restatement of every case
against the float64 one -- the yardstick the GPU test prints beside the kernel's error; the arithmetic of the live-row list
around the seven one-title shapes."""
import pytest
import torch

from tests import sweep_inputs_lstur_naml as S

F64, F32 = torch.float64, torch.float32


def _ids(cases):
    return [c["name"] for c in cases]


def _both(preds, key):
    return {p[key] for p in preds} == {True, False}


def test_case_names_are_unique():
    for cases, _, _ in S.FAMILIES.values():
        assert len({c["name"] for c in cases}) == len(cases)


def test_case_tables_reach_what_they_promise():
    # ---- CNN encoder ----
    cnn = S.CNN_CASES
    base = [c for c in cnn if (c["D"], c["F"], c["W"], c["Q"]) == (16, 12, 3, 12)]
    assert {c["L"] for c in base} >= {1, 2, 3, 15, 16, 17, 31, 32, 33, 63, 64, 65}
    assert {(c["W"], c["L"]) for c in cnn} >= {(1, 3), (5, 9), (7, 2), (7, 9), (5, 2)}
    assert {c["F"] for c in cnn} >= {12, 28, 16, 32, 300, 304, 316, 320, 324, 400}
    assert {c["Q"] for c in cnn} >= {4, 8, 12, 208, 212, 224, 228, 320, 324}
    assert {c["D"] for c in cnn} >= {4, 12, 16, 28, 32, 300, 304, 308, 320, 324}
    assert {c["N"] * c["L"] for c in cnn if c["F"] == 12} >= {32, 33, 64}
    assert {(c["N"], c["L"]) for c in cnn} >= {(1, 9), (2049, 1), (2049, 2)}
    assert {c["ids"] for c in cnn if tuple(c[k] for k in "NLDFWQ") == S.CNN_BASE} == set(S.ID_PATTERNS)
    assert any(c["ids"] == "all_pad" and c["N"] == 1 for c in cnn)
    tiny = {(c["N"], c["L"], c["Q"]) for c in cnn if c["name"].startswith("tiny")}
    assert tiny == set(S.CNN_TINY_REFUSED) | set(S.CNN_TINY_ACCEPTED)
    assert any(tuple(c[k] for k in "NLDFWQ") + (c["p"],) == (5, 30, 300, 300, 3, 200, 0.5) for c in cnn)
    assert {c["p"] for c in cnn} == {0.0, 0.5}
    assert all(c[k] % 4 == 0 for c in cnn for k in "DFQ") and all(c["W"] in (1, 3, 5, 7) for c in cnn)
    pr = [S.cnn_predicates(c) for c in cnn]
    for key in ("conv_planes", "rp", "x_planes", "aa_planes", "m_rem", "ncb_x_padded", "ncb_dc_padded", "persistent_pool"):
        assert _both(pr, key), key
    assert {p["kt"] for p in pr if p["conv_planes"]} == {1, 2}
    for axis in range(3):                                                        # D, F, Q: each at all three image widths
        assert {p["nblk"][axis] for p in pr if p["rp"]} == {13, 19, 20}, axis
    # each way out of a predicate on its own: W, L, F for the conv planes; D, F, Q for the row-panel; F % 16, F > 304, Q > 224 for aa
    by = {c["name"]: S.cnn_predicates(c) for c in cnn}
    assert not by["W7_L2"]["conv_planes"] and by["W7_L2"]["rp"] and not by["L64"]["conv_planes"] and by["L63"]["conv_planes"]
    assert by["F320"]["conv_planes"] and not by["F324"]["conv_planes"] and not by["F324"]["rp"]
    assert by["D320"]["rp"] and not by["D324"]["rp"] and by["Q320"]["rp"] and not by["Q324"]["rp"]
    assert by["F300"]["aa_planes"] and not by["F304"]["aa_planes"] and not by["F316"]["aa_planes"] and by["F28"]["aa_planes"]
    assert by["Q224"]["aa_planes"] and not by["Q228"]["aa_planes"] and by["Q228"]["x_planes"]
    assert by["M33"]["aa_planes"] and by["M33"]["m_rem"] and by["M32"]["aa_planes"] and not by["M32"]["m_rem"]
    assert by["L31"]["kt"] == 1 and by["L32"]["kt"] == 2
    # ---- GRU ----
    gru = S.GRU_CASES
    assert {c["Hd"] for c in gru} >= {4, 16, 20, 32, 36, 128, 132, 168, 172, 508, 512, 768, 772}
    assert {c["B"] for c in gru if c["Hd"] == 16} >= {1, 15, 16, 17, 33} and {c["B"] for c in gru if c["Hd"] == 512} >= {31, 32, 33}
    assert {c["Din"] for c in gru} >= {4, 36, 324} and {c["T"] for c in gru} >= {1, 2, 3, 4, 5}
    assert {c["lengths"] for c in gru} == {"mixed", "ones", "full"}
    assert any(c["lengths"] == "ones" and c["T"] == 5 for c in gru)
    pairs = {}
    for c in gru:
        pairs.setdefault((c["B"], c["T"], c["Din"], c["Hd"], c["lengths"], c["seed"]), set()).add(c["with_h0"])
    assert sum(v == {True, False} for v in pairs.values()) >= 3
    assert all(c["Hd"] % 4 == 0 and c["Din"] % 4 == 0 and c["T"] <= 5 and c["B"] <= 33 for c in gru)
    assert any((c["Hd"], c["B"], c["T"], c["Din"]) == (772, 3, 2, 4) for c in gru)
    gp = [S.gru_predicates(c) for c in gru]
    for key in ("fused", "wgrad_big", "row_clamp", "unit_clamp", "k_tail"):
        assert _both(gp, key), key
    assert {p["tr"] for p in gp if p["fused"]} == {1, 2} and {p["slots"] for p in gp if p["fused"]} >= {1, 2, 6}
    grids = {p["grid"] for p in gp if p["fused"] and p["tr"] == 1}
    assert grids >= {1, 7, 8, 9, 17}
    assert {g // 8 for g in grids} >= {0, 1, 2} and any(g % 8 for g in grids) and any(g % 8 == 0 for g in grids)
    assert any(p["fused"] and p["row_tiles"] > 1 and p["grid"] % 8 for p in gp)
    gby = {c["name"]: S.gru_predicates(c) for c in gru}
    assert gby["Hd768"]["fused"] and gby["Hd768"]["slots"] == 6 and not gby["Hd772_two_launch"]["fused"]
    assert gby["Hd508"]["tr"] == 1 and gby["Hd512"]["tr"] == 2 and not gby["Hd168"]["wgrad_big"] and gby["Hd172"]["wgrad_big"]
    assert gby["Hd128"]["slots"] == 1 and gby["Hd132"]["slots"] == 2
    # ---- additive attention ----
    aa = S.AA_CASES
    assert {c["S"] for c in aa} >= {1, 2, 15, 16, 17, 63, 64, 65, 129, 8192} and max(c["S"] for c in aa) == 8192
    assert {c["D"] for c in aa} >= {4, 12, 300, 1020, 1024, 1028} and {c["Q"] for c in aa} >= {4, 12, 200, 1024, 1028, 4096}
    assert max(c["Q"] for c in aa) == 4096
    assert {c["G"] for c in aa if (c["S"], c["D"], c["Q"]) == (2, 4, 4)} >= {0, 1, 2047, 2048, 2049}
    assert any((c["G"], c["S"], c["D"], c["Q"]) == (1, 8192, 4, 4) for c in aa)
    ap = [S.aa_predicates(c) for c in aa]
    assert {p["rg_fwd"] for p in ap} >= {256, 85, 3, 1} and {p["rg_bwd"] for p in ap} >= {256, 85, 3, 1}
    for key in ("idle_fwd", "idle_bwd", "second_pass_fwd", "persistent", "s16", "s64", "unroll_wrap", "flush_strides"):
        assert _both(ap, key), key
    assert any(256 < c["Q"] <= 512 for c in cnn)                                 # ... and through the CNN encoder's backward
    assert {p["accq_slots"] for p in ap} >= {1, 2, 4}
    assert any(p["rg_fwd"] == 1 and p["idle_fwd"] for p in ap)                   # 129 <= D / 4 <= 255: idle threads beside RG = 1
    assert all(c["peaked"] == (c["S"] > 256) for c in aa)
    # ---- linear + activation ----
    lin = S.LIN_CASES
    for act in S.ACTS:
        mine = [c for c in lin if c["act"] == act]
        assert {c["N"] for c in mine} >= {4, 208, 212, 224, 228, 512, 516} and {c["M"] for c in mine} >= {0, 1, 255, 256, 257}, act
    assert {c["K"] for c in lin if c["act"] == "relu"} >= {4, 28, 32, 36, 900}
    assert sum(not c["need_da"] for c in lin) == 1
    lp = [S.lin_predicates(c) for c in lin]
    for key in ("q_tile_f32", "q_tile_x3", "wgrad_big", "empty"):
        assert _both(lp, key), key
    assert any(p["q_tile_x3"] and not p["q_tile_f32"] for p in lp)
    # ---- embedding rows ----
    emb = S.EMB_CASES
    assert {(c["n"], c["D"], c["p"]) for c in emb} >= {(n, d, p) for n in (0, 1, 300) for d in (4, 100) for p in (0.0, 0.5)}
    assert {c["ids"] for c in emb} == {"random", "hot_row", "all_zero"}


def test_live_list_arithmetic_of_the_one_title_shapes():
    """M Q >= 2 M + ceil(M / 2048) + 8, the room the backward used to demand of the tanh buffer: four one-title shapes miss
    it, their first neighbours meet it."""
    assert [S.live_list_fits(*s) for s in S.CNN_TINY_REFUSED] == [False] * 4
    assert [S.live_list_fits(*s) for s in S.CNN_TINY_ACCEPTED] == [True] * 3
    for n, l, q in S.CNN_TINY_REFUSED:                      # each accepted neighbour is one step of L or Q away from a refused shape
        assert any((n, l2, q2) in S.CNN_TINY_ACCEPTED for l2, q2 in ((l + 1, q), (l, q + 4), (l, q + 8), (l + 3, q), (l + 4, q)))
    # every other CNN case had room, so the fix changes no path of theirs
    assert all(S.live_list_fits(c["N"], c["L"], c["Q"]) for c in S.CNN_CASES if not c["name"].startswith("tiny"))


def _exact_and_odd(pre32, pre64):
    assert torch.equal(pre32.double(), pre64)
    k = pre64 * 256.0
    assert torch.equal(k, k.round()) and bool((k.abs() % 2 == 1).all())           # odd multiples of 1 / 256: never 0


@pytest.mark.parametrize("index", range(len(S.CNN_CASES)), ids=_ids(S.CNN_CASES))
def test_cnn_grid_pre_activations_are_exact(index):
    case, inp = S.CNN_CASES[index], S.cached_inputs("cnn", index)
    _exact_and_odd(S.cnn_pre(case, inp, F32), S.cnn_pre(case, inp, F64))
    # the operands fit a bf16 (8 significant bits), so the low plane of the bf16x3 split is zero
    for k in S.CNN_KEYS[:3]:
        v = inp["params"][k]
        assert torch.equal(v.bfloat16().float(), v), k
    ids = inp["ids"]
    assert int(ids.min()) >= 0 and int(ids.max()) < S.VOCAB
    if case["ids"] == "all_pad":
        assert int(ids.abs().max()) == 0
    elif case["ids"] == "no_pad":
        assert int(ids.min()) > 0
    elif case["ids"] == "one_all_pad_title":
        assert int((ids == 0).all(dim=1).sum()) == 1
    else:
        assert int(ids[0, 0]) == 0 and int(ids[1 % case["N"], case["L"] // 2]) == 0 and int(ids[-1, -1]) == 0
        assert int((ids != 0).sum()) > 0


RELU = [i for i, c in enumerate(S.LIN_CASES) if c["act"] == "relu"]


@pytest.mark.parametrize("index", RELU, ids=[S.LIN_CASES[i]["name"] for i in RELU])
def test_linear_relu_grid_pre_activations_are_exact(index):
    case, inp = S.LIN_CASES[index], S.cached_inputs("lin", index)
    _exact_and_odd(S.lin_pre(case, inp, F32), S.lin_pre(case, inp, F64))
    for k in ("a", "w", "b"):
        assert torch.equal(inp[k].bfloat16().float(), inp[k]), k


def _flat(ref):
    for k, v in ref.items():
        if isinstance(v, dict):
            for k2, v2 in v.items():
                yield f"{k}/{k2}", v2
        else:
            yield k, v


PARAMS = [(f, i) for f, (cases, _, _) in S.FAMILIES.items() for i in range(len(cases))]


@pytest.mark.parametrize("family,index", PARAMS, ids=[f"{f}-{S.FAMILIES[f][0][i]['name']}" for f, i in PARAMS])
def test_float32_reference_agrees_with_float64(family, index):
    """Every reference is finite, stays in its dtype, and the float32 one is within 1e-5 max(1, |want|_max) of the float64
    one -- the float32 oracle's usual error (a few ulps of the largest value through sums of up to ~1000 terms)."""
    r64, r32 = S.cached(family, index, "float64"), S.cached(family, index, "float32")
    for (k, a), (_, b) in zip(_flat(r64), _flat(r32)):
        assert a.dtype == F64 and b.dtype == F32 and a.shape == b.shape, k
        assert bool(torch.isfinite(a).all()) and bool(torch.isfinite(b).all()), k
        if a.numel():
            err, top = float((b.double() - a).abs().max()), float(a.abs().max())
            assert err <= 1e-5 * max(1.0, top), (k, err, top)


def test_exact_zeros_of_the_references():
    """What the GPU file asserts as exact zeros is exactly zero in the reference too."""
    for i, c in enumerate(S.CNN_CASES):
        g = S.cached("cnn", i, "float64")["grads"][S.CNN_KEYS[0]]
        assert float(g[0].abs().max()) == 0.0
        if c["ids"] == "all_pad":
            assert float(g.abs().max()) == 0.0
    for i, c in enumerate(S.GRU_CASES):
        inp, ref = S.cached_inputs("gru", i), S.cached("gru", i, "float64")
        pad = torch.arange(c["T"])[None, :] >= inp["lengths"][:, None]
        if bool(pad.any()):
            assert float(ref["d_hist"][pad].abs().max()) == 0.0
    for i, c in enumerate(S.AA_CASES):
        if c["G"] == 0:
            ref = S.cached("aa", i, "float64")
            assert ref["out"].shape == (0, c["D"]) and all(float(ref["d_" + k].abs().sum()) == 0.0 for k in ("w", "b", "q"))
    for i, c in enumerate(S.LIN_CASES):
        if c["M"] == 0:
            ref = S.cached("lin", i, "float64")
            assert ref["out"].shape == (0, c["N"]) and float(ref["d_w"].abs().sum()) == 0.0 and float(ref["d_b"].abs().sum()) == 0.0


def test_peaked_softmax_of_the_long_rows():
    """S = 8192: the six constructed rows hold most of the weight, so a dropped or doubled row shows in the output."""
    for i, c in enumerate(S.AA_CASES):
        if not c["peaked"]:
            continue
        inp = S.cached_inputs("aa", i)
        a = torch.tanh(inp["y"].double() @ inp["w"].double().t() + inp["b"].double()) @ inp["q"].double()
        w = torch.softmax(a, dim=1)
        assert float(w[:, list(S.AA_PEAKS(c["S"]))].sum(dim=1).min()) > 0.9
        assert float(w[:, list(S.AA_PEAKS(c["S"]))].min()) > 0.1
