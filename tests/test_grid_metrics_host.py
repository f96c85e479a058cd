"""Host tier of the weight grid (``nrl_manner_zscores`` / ``nrl_grid_metrics`` / ``ops.grid_metrics`` /
``metrics.GridStreamingMetrics`` / ``evaluate_weight_grid``): the CPU restatement against hand-worked impressions, the launch
plan, the workspace size without a device, the C entry's refusals before any launch, and the Python refusals."""
import ctypes
import json
import math
import os
import re

import pytest
import torch

from tests import grid_metrics_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("nrl_manner_zscores", "nrl_grid_metrics_configs_per_block", "nrl_grid_metrics_workspace_size", "nrl_grid_metrics")
P = 256                    # a placeholder pointer: non-null, aligned, never read (every refusal is before a launch)


def _lib_or_skip():
    from newsreclib_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("library not built")
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES + ("nrl_last_error", "nrl_abi_version"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    return lib


# ---- the restatement on impressions worked by hand ----------------------------------------------------------------------------------
def test_scores_skip_zero_weights_and_round_like_the_scorer():
    comp = torch.tensor([[1.0, -0.5, 0.25], [float("nan"), 2.0, -1.0], [0.5, 0.5, 0.5]])
    assert R.scores(comp, torch.tensor([1.0, 0.0, -0.5])).tolist() == [0.75, -0.75, 0.0]          # the NaN component is not used
    assert R.scores(comp, torch.tensor([0.0, 0.0, 2.0])).tolist() == [1.0, 1.0, 1.0]
    assert math.isnan(R.scores(comp, torch.tensor([1.0, 1.0, 0.0]))[0])
    assert R.scores(comp, torch.tensor([0.0, 0.0, 0.0])).tolist() == [0.0, 0.0, 0.0]
    # one rounding for the second term: (1 + 2^-12)^2 - (1 + 2^-11) is 2^-24 under an fma, 0 under a product and a sum
    a, c = 1.0 + 2.0 ** -12, -(1.0 + 2.0 ** -11)
    fused = R.scores(torch.tensor([[c], [a]]), torch.tensor([1.0, a]))
    assert float(fused) == 2.0 ** -24
    assert float(torch.tensor(c) + torch.tensor(a) * torch.tensor(a)) == 0.0


def test_rows_of_a_hand_worked_impression():
    # two components, five candidates; row 0 ranks by the first component, row 1 by the second, row 2 by their difference
    comp = torch.tensor([[0.5, 1.0, -1.0, 0.0, 0.5], [1.0, -1.0, 0.5, 0.5, 0.0]])
    targets = torch.tensor([0.0, 1.0, 0.0, 2.0, 0.0])
    ca, ha = torch.tensor([1, 2, 2, 0, 1]), torch.tensor([2, 2, 1])
    w = torch.tensor([[1.0, 0.0], [0.0, 1.0], [1.0, -1.0]])
    rows = R.rows(comp, w, targets, torch.tensor([5]), (2, 5), [(ca, ha, 3)], torch.tensor([3]))
    assert rows.shape == (3, 1, 7)
    ideal2, ideal5 = 2 + 1 / math.log2(3), 2 + 1 / math.log2(3)
    # row 0: order 1, 0, 4, 3, 2 (the tie 0.5 / 0.5 by position): targets 1, 0, 0, 2, 0
    want0 = [1.0, 1 / ideal2, (1 + 2 / math.log2(5)) / ideal5]
    # row 1: order 0, 2, 3, 4, 1: targets 0, 0, 2, 0, 1
    want1 = [1 / 3, 0.0, (2 / math.log2(4) + 1 / math.log2(6)) / ideal5]
    # row 2: scores -0.5, 2, -1.5, -0.5, 0.5 -> order 1, 4, 0, 3, 2: targets 1, 0, 0, 2, 0
    want2 = [1.0, 1 / ideal2, (1 + 2 / math.log2(5)) / ideal5]
    for g, want in enumerate((want0, want1, want2)):
        assert rows[g, 0, :3].tolist() == pytest.approx(want, abs=1e-15), g
    # aspects of row 0: top 2 = classes 2, 1 -> entropy log 2 / log 3; against the history {1: 1, 2: 2}: min 2 / max 3
    assert rows[0, 0, 3] == pytest.approx(math.log(2) / math.log(3), abs=1e-15)
    assert rows[0, 0, 5] == pytest.approx(2 / 3, abs=1e-15)
    # top 5 = all: counts {0: 1, 1: 2, 2: 2} against {1: 1, 2: 2}: min 3 / max 5, the same under every row
    assert all(rows[g, 0, 6] == pytest.approx(3 / 5, abs=1e-15) for g in range(3))
    # candidate ids all 0: both 0; an empty history: personalization 0
    zero = R.rows(comp, w, targets, torch.tensor([5]), (2,), [(torch.zeros(5, dtype=torch.long), ha, 3)], torch.tensor([3]))
    assert float(zero[:, :, 2:].abs().max()) == 0.0
    none = R.rows(comp, w, targets, torch.tensor([5]), (2,), [(ca, ha[:0], 3)], torch.tensor([0]))
    assert float(none[:, :, 3].abs().max()) == 0.0 and float(none[0, 0, 2]) > 0


def test_rank_is_the_stable_descending_order_with_nan_first():
    p = torch.tensor([0.0, -0.0, float("nan"), 1.0, -0.0, float("inf")])
    assert R.rank(p)[1].tolist() == [3, 4, 0, 2, 5, 1]


def test_shared_inputs_are_not_vacuous():
    for T, G in ((1, 2), (2, 7), (3, 65), (4, 7)):
        comp, _, csz, _, _ = R.case(T, T, [1, 2, 127, 128, 129, 300])
        w = R.grid_weight_rows(G, T)
        assert not bool((w == 0).all(1).any()) and bool(torch.isfinite(w).all())
        n = R.assert_not_vacuous(comp, w, csz)
        print(f"T = {T}, G = {G}: {n} rows rank some impression differently from row 0")
    w = R.grid_weight_rows(65, 3)
    assert all(bool((w[:, t] == 0).any()) for t in range(3)) and bool((w < 0).any()) and torch.equal(w[64], w[0])
    comp = R.case(1, 3, [40])[0]
    assert len(torch.unique(comp)) == R.LEVELS                       # tie-heavy


# ---- ABI surface -------------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_typed_and_exported_without_an_abi_bump():
    from newsreclib_amd import _lib, ops
    header = open(os.path.join(ROOT, "include", "newsreclib_amd.h")).read()
    assert _lib.ABI_VERSION == 19 and re.search(r"#define NRL_ABI_VERSION 19\b", header)
    for name in NAMES:
        assert re.search(r"\b%s\(" % name, header) and name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["nrl_grid_metrics"][1]) == 28 and len(_lib.SIGNATURES["nrl_manner_zscores"][1]) == 13
    assert re.search(r"#define NRL_GRID_MAX_COMPONENTS %d\b" % ops.GRID_MAX_COMPONENTS, header)
    assert re.search(r"#define NRL_GRID_MAX_CONFIGS %d\b" % ops.GRID_MAX_CONFIGS, header)
    assert (ops.GRID_MAX_COMPONENTS, ops.GRID_MAX_CONFIGS) == (4, 4096)
    assert _lib_or_skip().nrl_abi_version() == 19


def test_the_launch_plan_depends_on_G_and_B_alone():
    lib = _lib_or_skip()
    plan = lib.nrl_grid_metrics_configs_per_block
    for B in (1, 3, 4, 5, 9, 512, 513, 4096, 8192, 8193, 73152, 1 << 20):
        for G in (1, 2, 7, 21, 65, 441, 4096):
            got = plan(B, G)
            assert got == R.configs_per_block(B, G), (B, G, got)
            assert 1 <= got <= G
    assert plan(512, 441) == 28 and plan(512, 21) == 2 and plan(512, 1) == 1          # 16 ranges of 128 workgroups each
    assert plan(9, 65) == 1 and plan(1 << 20, 441) == 441
    assert plan(0, 5) == 1 and plan(5, 0) == 1 and plan(-1, -1) == 1


def test_workspace_size_without_a_device():
    lib = _lib_or_skip()
    ws = lib.nrl_grid_metrics_workspace_size
    base = ws(512, 441, 2, 2, 0)
    cols = 1 + 2 + 2 * 2 * 2
    assert base % 256 == 0 and base >= 441 * 512 * cols * 4 + 512 * 4 + 441 * (cols + 1) * 8
    assert ws(513, 441, 2, 2, 0) > base and ws(512, 442, 2, 2, 0) > base and ws(512, 441, 2, 3, 0) > base and ws(512, 441, 1, 2, 0) < base
    assert ws(4097, 7, 0, 1, 0) > ws(4096, 7, 0, 1, 0)
    # the rows are set aside only when the caller keeps none
    kept = ws(512, 441, 2, 2, 1)
    assert kept % 256 == 0 and 512 * 4 + 441 * (cols + 1) * 8 <= kept < 64 << 10 and base - kept >= 441 * 512 * cols * 4
    assert ws(9, 4096, 2, 4, 1) < 2 << 20
    for args in ((0, 4, 0, 2), (-1, 4, 0, 2), (4, 0, 0, 2), (4, 4097, 0, 2), (4, 4, 3, 2), (4, 4, -1, 2), (4, 4, 0, 5), (4, 4, 0, -1),
                 (1 << 31, 4, 0, 2)):
        assert ws(*args, 0) == 256 and ws(*args, 1) == 256, args
    table = json.load(open(os.path.join(ROOT, "tests", "data", "grid_metrics_workspace_sizes.json")))
    assert len(table) >= 5 and {row["args"][4] for row in table} == {0, 1}
    for row in table:
        assert ws(*row["args"]) == row["bytes"], row


def test_the_c_entries_refuse_before_any_launch():
    lib = _lib_or_skip()
    st = ctypes.c_int32(0)
    ks = (ctypes.c_int32 * 4)(5, 10, 0, 0)

    def call(T=3, G=7, N=20, B=4, n_asp=0, nc0=0, nc1=0, n_hist=0, n_k=2, cpb=0, comp=P, weights=P, targets=P, off=P, ca0=None, ha0=None,
             hoff=None, sums=P, count=P, status=True, ws=P, ws_bytes=1 << 24, top_k=ks):
        return lib.nrl_grid_metrics(comp, T, weights, G, targets, off, N, B, n_asp, ca0, ha0, nc0, None, None, nc1, hoff, n_hist, top_k,
                                    n_k, cpb, None, None, sums, count, ctypes.addressof(st) if status else None, ws, ws_bytes, None)

    for kw, word in (({"T": 0}, "components"), ({"T": 5}, "components"), ({"G": 0}, "weight rows"), ({"G": 4097}, "weight rows"),
                     ({"N": -1}, "negative"), ({"B": -1}, "negative"), ({"B": 1 << 31}, "2^31"), ({"n_asp": 3}, "n_aspects"),
                     ({"n_k": 5}, "top_k"), ({"n_k": 2, "top_k": None}, "top_k"), ({"cpb": -1}, "configs_per_block"),
                     ({"count": None}, "go together"), ({"status": False}, "status"), ({"weights": None}, "null weights"),
                     ({"off": None}, "null argument"), ({"comp": None}, "null argument"), ({"targets": None}, "null argument"),
                     ({"n_asp": 1, "nc0": 1, "ca0": P, "ha0": P, "hoff": P}, "num_classes"),
                     ({"n_asp": 1, "nc0": 1025, "ca0": P, "ha0": P, "hoff": P}, "num_classes"),
                     ({"n_asp": 1, "nc0": 4, "ca0": None, "ha0": P, "hoff": P}, "aspect 0"),
                     ({"n_asp": 1, "nc0": 4, "ca0": P, "ha0": P, "hoff": None}, "aspect 0")):
        assert call(**kw) == -1, kw                                       # NRL_E_INVALID
        assert word in lib.nrl_last_error().decode(), (kw, lib.nrl_last_error())
    bad_k = (ctypes.c_int32 * 4)(5, 1025, 0, 0)
    assert call(top_k=bad_k) == -1 and "every k" in lib.nrl_last_error().decode()
    assert call(B=0) == 0                                                 # B == 0: success, nothing launched
    need = lib.nrl_grid_metrics_workspace_size(4, 7, 0, 2, 0)
    assert need > 256
    assert call(ws_bytes=need - 1) == -2                                  # NRL_E_WORKSPACE
    assert "workspace too small: %d < %d bytes" % (need - 1, need) in lib.nrl_last_error().decode()
    assert call(ws=None) == -1 and "workspace" in lib.nrl_last_error().decode()
    assert call(ws=P + 16) == -1

    ptrs = (ctypes.c_void_p * 3)(P, P, P)

    def zs(k=3, V=10, N=20, B=4, max_cand=8, D=8, tables=ptrs, hoff=P, coff=P):
        return lib.nrl_manner_zscores(tables, k, V, P, hoff, P, coff, N, B, max_cand, D, P, None)

    for kw, word in (({"k": 0}, "tables"), ({"k": 4}, "tables"), ({"V": 0}, "bad sizes"), ({"B": -1}, "bad sizes"), ({"N": -1}, "bad sizes"),
                     ({"D": 6}, "multiple of 4"), ({"D": 1028}, "multiple of 4"), ({"max_cand": 0}, "max_cand"),
                     ({"max_cand": 2049}, "max_cand"), ({"tables": None}, "null argument"), ({"coff": None}, "null argument"),
                     ({"tables": (ctypes.c_void_p * 3)(P, None, P)}, "table 1"), ({"tables": (ctypes.c_void_p * 3)(P, P + 4, P)}, "table 1")):
        assert zs(**kw) == -1, kw
        assert word in lib.nrl_last_error().decode(), (kw, lib.nrl_last_error())
    assert zs(B=0) == 0 and zs(N=0) == 0


# ---- Python refusals (no device is touched before they return) ------------------------------------------------------------------------
def test_grid_weights_are_checked_on_the_host():
    from newsreclib_amd import ops
    ok = ops.grid_weights([[1.0, 0.0, -0.25], [1, 0.5, 0]])
    assert ok.dtype == torch.float32 and ok.shape == (2, 3) and not ok.is_cuda
    with pytest.raises(ValueError, match="row 1 of the grid is all zeros"):
        ops.grid_weights([[1.0, 0.0], [0.0, 0.0]])
    with pytest.raises(ValueError, match="non-finite"):
        ops.grid_weights([[1.0, float("nan")]])
    with pytest.raises(ValueError, match="non-finite"):
        ops.grid_weights([[float("inf"), 1.0]])
    with pytest.raises(ValueError, match=r"\(G, T\)"):
        ops.grid_weights([1.0, 2.0])
    with pytest.raises(ValueError, match="one entry per component: 3, got 2"):
        ops.grid_weights([[1.0, 2.0]], 3)
    with pytest.raises(NotImplementedError, match="at most 4 components and 4096 rows"):
        ops.grid_weights(torch.ones(2, 5))
    with pytest.raises(NotImplementedError, match="at most 4 components and 4096 rows"):
        ops.grid_weights(torch.ones(4097, 2))


def test_python_entries_refuse_before_any_device_work():
    from newsreclib_amd import evaluation as E
    from newsreclib_amd import metrics, ops
    from newsreclib_amd.ops_manner import manner_zscores
    comp, t, off = torch.zeros(2, 5), torch.zeros(5), torch.tensor([0, 5])
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.grid_metrics(comp, [[1.0, 0.5]], t, off, (5,))
    with pytest.raises(RuntimeError, match="no CPU path"):
        manner_zscores([torch.zeros(4, 8)], torch.tensor([1]), torch.tensor([0, 1]), torch.tensor([2, 3]), torch.tensor([0, 2]), 2)
    with pytest.raises(ValueError, match="1 to 3 news-vector tables"):
        manner_zscores([], torch.tensor([1]), torch.tensor([0, 1]), torch.tensor([2, 3]), torch.tensor([0, 2]), 2)
    with pytest.raises(ValueError, match="all zeros"):
        metrics.GridStreamingMetrics([[0.0, 0.0]])
    with pytest.raises(NotImplementedError):
        metrics.GridStreamingMetrics(torch.ones(1, 5))
    gm = metrics.GridStreamingMetrics([[1.0, 0.5], [1.0, 0.0]], (5, 10), 19, 4)
    assert gm.compute() == {} and gm.weights.shape == (2, 2)
    with pytest.raises(RuntimeError, match="no CPU path"):
        gm.update(comp, (None, None, t, torch.tensor([5]), torch.tensor([0]), off[:0], off[:0], off[:0], off[:0]))
    with pytest.raises(ValueError, match="configured differently"):
        gm.merge(metrics.GridStreamingMetrics([[1.0, 0.5], [1.0, 0.25]], (5, 10), 19, 4))
    with pytest.raises(ValueError, match="configured differently"):
        gm.merge(metrics.GridStreamingMetrics([[1.0, 0.5], [1.0, 0.0]], (5,), 19, 4))
    assert gm.merge(metrics.GridStreamingMetrics([[1.0, 0.5], [1.0, 0.0]], (5, 10), 19, 4)) is gm
    assert "no AUC" in metrics.GridStreamingMetrics.__doc__
    imps = [{"hist": torch.tensor([1, 2]), "cand": torch.tensor([3, 4]), "labels": torch.tensor([1.0, 0.0])}]
    from newsreclib_amd.nrms_module import NRMSModule
    with pytest.raises(TypeError, match="zscores"):
        E.evaluate_weight_grid(E.NewsVectorCache(object.__new__(NRMSModule), None), imps, [[1.0, 0.5]])
    cache = object.__new__(E.MannerVectorCache)
    cache.weights = [1.0, 0.2, -0.25]
    with pytest.raises(ValueError, match=r"one entry per loaded sub-model, in module.submodels\(\) order: 3 here"):
        E.evaluate_weight_grid(cache, imps, [[1.0, 0.5]])
    with pytest.raises(ValueError, match="all zeros"):
        E.evaluate_weight_grid(cache, imps, [[1.0, 0.5, 0.0], [0.0, 0.0, 0.0]])
