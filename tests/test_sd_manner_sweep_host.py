"""Host tier of the SentiDebias / MANNeR shape sweep (tests/sweep_inputs_sd_manner.py, run on the GPU by
tests/test_gpu_sd_manner_sweep.py): the input conditions, each a property of the float64 reference, for every committed seed;
the coverage the case lists promise; and the float32 CPU restatement of each case inside that case's bound, so that the
reference alone stays inside it."""
import pytest
import torch

from tests import manner_oracle as MO
from tests import sweep_inputs_sd_manner as S


def _e32(r64, r32, key):
    return float((r32[key].double() - r64[key]).abs().max()) if r64[key].numel() else 0.0


def _bound(r64, r32, key, tol, rel=False):
    scale = max(1.0, float(r64[key].abs().max())) if rel and r64[key].numel() else 1.0
    return max(tol * scale, 4 * _e32(r64, r32, key))


def _refs(family, i):
    return S.cached(family, i, "float64"), S.cached(family, i, "float32")


def test_case_lists_reach_what_they_promise():
    c = S.ROWCOS_CASES
    assert {x["D"] for x in c} >= {4, 252, 256, 260, 300} and {x["S"] for x in c} >= {1, 2, 4, 8}
    assert {x["N"] for x in c} >= {1, 63, 64, 65, 129}
    assert {(x["N"], x["n_hist"]) for x in c} >= {(1, 0), (1, 1), (63, 1), (64, 63), (64, 64), (65, 0), (129, 66), (129, 128)}
    assert all(x["S"] * x["D"] <= 3072 for x in c) and any(x["S"] * x["D"] == 3072 for x in c)
    h = S.HIST_CASES
    assert {(x["B"], x["H"]) for x in h} >= {(1, 1), (1, 64), (1, 65), (5, 13), (3, 43), (2, 130)}
    assert {x["B"] for x in h} >= {1, 3, 4, 5} and {x["S"] for x in h} >= {1, 4, 8} and {x["D"] for x in h} >= {4, 260, 384}
    assert any(x["S"] * x["D"] == 3072 for x in h) and all(x["S"] * x["D"] <= 3072 for x in h)
    assert any(0 in x["hs"] for x in h) and any(1 in x["hs"] for x in h) and all(max(x["hs"]) <= x["H"] for x in h)
    sc = S.SCORE_CASES
    assert {x["C"] for x in sc} >= {1, 63, 64, 65, 130} and {x["B"] for x in sc} >= {1, 4, 5} and {x["S"] for x in sc} >= {1, 8}
    assert any(0 in x["cs"] for x in sc) and any(max(x["cs"]) < x["C"] for x in sc)
    d = S.DISC_CASES
    assert {x["Hd"] for x in d} >= {4, 252, 256, 260, 380} and {x["O"] for x in d} == {1, 2, 3, 8}
    assert {(x["O"] * x["Hd"] + x["O"]) % 4 for x in d} == {0, 1, 2, 3}
    assert {x["N"] for x in d} >= {1, 63, 64, 65, 129}
    for i, x in enumerate(d):
        ids = S.cached_inputs("disc", i)["ids"]
        assert int(ids.min()) >= 0 and int(ids.max()) <= x["O"]
        if x["N"] > 1:
            assert 0 in ids.tolist() and x["O"] in ids.tolist()
    m = S.MANNER_CASES
    assert {x["D"] for x in m} >= {4, 252, 256, 260, 1024} and {x["k"] for x in m} == {1, 2, 3}
    assert {x["max_cand"] for x in m} >= {255, 256, 257, 513, 2048} and all(max(x["cs"]) == x["max_cand"] for x in m)
    assert {n for x in m for n in x["hs"]} >= {0, 1, 65, 300} and {len(x["hs"]) for x in m} == {1, 5}
    assert {n for x in m for n in x["cs"]} >= {0, 1}
    sup = S.SUPCON_CASES
    assert {x["N"] for x in sup} >= {1, 2, 5, 6, 7, 125, 128, 129, 132} and {x["D"] for x in sup} == {4, 8}
    assert {x["T"] for x in sup} == {0.05, 0.9}


@pytest.mark.parametrize("index", range(len(S.ROWCOS_CASES)), ids=[c["name"] for c in S.ROWCOS_CASES])
def test_rowcos_inputs_and_float32_restatement(index):
    case, inp = S.ROWCOS_CASES[index], S.cached_inputs("rowcos", index)
    r64, r32 = _refs("rowcos", index)
    assert float(S.rowcos_norm_products(case, inp).min()) >= 1e-3
    if case["special"] == "zero_row":
        z = S.ZERO_ROW
        side = 0 if z < case["n_hist"] else 1
        n_side = case["n_hist"] if side == 0 else case["N"] - case["n_hist"]
        want = float(inp["w"][side]) / n_side * inp["T"].double()[inp["ids"][z]] / S.SO.COS_EPS
        assert float(r64["out"].abs().max()) < 1.0
        assert torch.allclose(r64["d_news"][z], want, rtol=1e-12, atol=0.0)
        rest = torch.arange(case["N"]) != z
        assert _e32({"x": r64["d_news"][rest]}, {"x": r32["d_news"][rest]}, "x") <= _bound(
            {"x": r64["d_news"][rest]}, {"x": r32["d_news"][rest]}, "x", S.COS_DNEWS, rel=True)
    if case["special"] == "bad_ids":
        rows = list(S.BAD_ROWS)
        assert float(r64["d_news"][rows].abs().max()) == 0.0 and float(r32["d_news"][rows].abs().max()) == 0.0
        assert any(r < case["n_hist"] for r in rows) and any(r >= case["n_hist"] for r in rows)
        assert any(r >= 64 for r in rows) and any(r < 64 for r in rows)
    for key, tol, rel in (("out", S.COS_VALUE, False), ("d_news", S.COS_DNEWS, True), ("d_T", S.D_TABLE, True)):
        assert _e32(r64, r32, key) <= _bound(r64, r32, key, tol, rel), key
    if case["n_hist"] == 0:
        assert float(r64["out"][0]) == 0.0                      # the mean of an empty side is 0
    if case["n_hist"] == case["N"]:
        assert float(r64["out"][1]) == 0.0


@pytest.mark.parametrize("index", range(len(S.HIST_CASES)), ids=[c["name"] for c in S.HIST_CASES])
def test_hist_and_late_float32_restatement(index):
    case = S.HIST_CASES[index]
    r64, r32 = _refs("hist", index)
    assert torch.equal(r32["dense"], r64["dense"].float())      # a gather: the float32 restatement is the float64 one cast
    empty = torch.tensor([n == 0 for n in case["hs"]])
    assert bool(torch.isnan(r64["u"][empty]).all()) and bool(torch.isfinite(r64["u"][~empty]).all())
    assert bool(torch.isnan(r32["u"][empty]).all())
    a, b = {"u": r64["u"][~empty]}, {"u": r32["u"][~empty]}
    assert _e32(a, b, "u") <= _bound(a, b, "u", S.LATE_U)
    assert _e32(r64, r32, "d_T_dense") <= _bound(r64, r32, "d_T_dense", S.D_TABLE, rel=True)
    assert ("d_T_late" in r64) == (min(case["hs"]) > 0)
    if "d_T_late" in r64:
        assert _e32(r64, r32, "d_T_late") <= _bound(r64, r32, "d_T_late", S.D_TABLE, rel=True)


@pytest.mark.parametrize("index", range(len(S.SCORE_CASES)), ids=[c["name"] for c in S.SCORE_CASES])
def test_scores_float32_restatement(index):
    inp = S.cached_inputs("scores", index)
    r64, r32 = _refs("scores", index)
    assert torch.equal(r64["out"][~inp["mask"]], inp["free"].double()[~inp["mask"]])       # padded slots equal `free`
    assert _e32(r64, r32, "out") <= _bound(r64, r32, "out", S.SCORES)
    for key in ("d_free", "d_u", "d_T"):
        assert _e32(r64, r32, key) <= _bound(r64, r32, key, S.SCORES_GRAD, rel=True), key


@pytest.mark.parametrize("index", range(len(S.DISC_CASES)), ids=[c["name"] for c in S.DISC_CASES])
def test_disc_float32_restatement(index):
    case = S.DISC_CASES[index]
    r64, r32 = _refs("disc", index)
    for key in ["out", "d_x"] + ["d_" + k for k in S.DISC_KEYS]:
        assert bool(torch.isfinite(r64[key]).all())
        assert _e32(r64, r32, key) <= _bound(r64, r32, key, S.DISC["f32"], rel=key != "out"), key
    if case["O"] == 1:                                           # one output: log-softmax is 0, loss and gradients exactly 0
        assert all(float(r64[k].abs().max()) == 0.0 for k in r64)


@pytest.mark.parametrize("index", range(len(S.MANNER_CASES)), ids=[c["name"] for c in S.MANNER_CASES])
def test_manner_scorer_inputs(index):
    case, inp = S.MANNER_CASES[index], S.cached_inputs("manner", index)
    r64, r32 = _refs("manner", index)
    kinds = inp["kinds"]
    skip = [b for b, k in enumerate(kinds) if k != "real"]
    assert "real" in kinds
    assert MO.min_std_ratio(inp["tables"], inp["hist"], inp["cand"], skip=skip) >= 1e-2
    for b, kind in enumerate(kinds):
        for r in (r64, r32):
            row = r["rows"][b]
            assert len(row) == case["cs"][b]
            if kind == "nan":
                assert bool(torch.isnan(row).all())
            elif kind == "real":
                assert bool(torch.isfinite(row).all())
    e32, top = S.manner_errors(case, inp, r64, r32)
    assert 0.25 * S.EPS32 * top <= e32 <= 4 * e32                # a yardstick that is 0 would bound nothing
    V = case["V"]
    for raw, used in ((inp["raw_hist"], inp["hist"]), (inp["raw_cand"], inp["cand"])):
        for a, b in zip(raw, used):
            assert torch.equal(a.clamp(0, V - 1), b) and int(b.min() if len(b) else 0) >= 0 and int(b.max() if len(b) else 0) < V
    if case["clamp"]:
        flat = torch.cat(inp["raw_hist"] + inp["raw_cand"])
        assert -3 in flat.tolist() and V + 7 in flat.tolist()


@pytest.mark.parametrize("index", range(len(S.SUPCON_CASES)), ids=[c["name"] for c in S.SUPCON_CASES])
def test_supcon_row_losses(index):
    case, inp = S.SUPCON_CASES[index], S.cached_inputs("supcon", index)
    r64, r32 = _refs("supcon", index)
    if case["labels"] is not None:
        assert r64["rows"] is None and float(r64["loss"]) == 0.0 and float(r64["grad"].abs().max()) == 0.0
        return
    rows = r64["rows"]
    assert bool(((rows == 0) | (rows >= 1e-3)).all()) and bool((rows > 0).any())
    assert bool(torch.equal(r32["rows"] > 0, rows > 0))          # the keep-decision is the same in fp32
    if case["singleton"]:
        assert int((inp["labels"] == inp["labels"][-1]).sum()) == 1 and float(rows[-1]) == 0.0
    e_loss, e_grad = abs(float(r32["loss"]) - float(r64["loss"])), _e32(r64, r32, "grad")
    assert e_loss >= 0.25 * S.EPS32 * abs(float(r64["loss"])) and e_grad >= 0.25 * S.EPS32 * float(r64["grad"].abs().max())
    assert e_loss <= 4 * e_loss and e_grad <= 4 * e_grad
