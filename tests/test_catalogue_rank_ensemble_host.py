"""Host tier of the full-catalogue rank under MANNeR's ensemble (``nrl_catalogue_ensemble_ranks`` /
``ops.catalogue_ensemble_ranks`` / ``MannerVectorCache.rank_clicks_ensemble`` / ``evaluate_full_rank(ensemble=True)``): ABI surface,
workspace sizing, host-side refusals (no device is touched before they return), and the conditions the GPU tier's references
must meet on their own."""
import ctypes
import json
import os
import re
import subprocess

import pytest
import torch

from tests import catalogue_rank_ensemble_ref as ER
from tests import catalogue_ref as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("nrl_catalogue_ensemble_ranks_workspace_size", "nrl_catalogue_ensemble_ranks")


def _lib_or_skip():
    from newsreclib_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("library not built")
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES + ("nrl_catalogue_ranks_workspace_size", "nrl_last_error", "nrl_abi_version"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    return lib


def test_symbols_are_declared_typed_and_exported_without_an_abi_bump():
    from newsreclib_amd import _lib, ops
    header = open(os.path.join(ROOT, "include", "newsreclib_amd.h")).read()
    assert _lib.ABI_VERSION == 19 and re.search(r"#define NRL_ABI_VERSION 19\b", header)
    for name in NAMES:
        assert re.search(r"\b%s\(" % name, header) and name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES[NAMES[1]][1]) == 23 and len(_lib.SIGNATURES[NAMES[0]][1]) == 6
    assert set(ops.ENSEMBLE_RANK_FLAGS) == set(ops.RANK_FLAGS) | {8} and set(ops.RANK_FLAGS) == {1, 2, 4, 16, 32}
    assert all(ops.ENSEMBLE_RANK_FLAGS[b] == ops.RANK_FLAGS[b] for b in ops.RANK_FLAGS)
    assert "ranks and population are 0" in ops.ENSEMBLE_RANK_FLAGS[8] and re.search(r"#define NRL_TOPK_E_STATS 8\b", header)
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("library not built")
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(NAMES) <= exported
    assert not any(n.startswith("nrl_catalogue_ensemble") and n.endswith("_workspace_bytes") for n in exported)
    assert _lib_or_skip().nrl_abi_version() == 19


def test_workspace_size():
    lib = _lib_or_skip()
    ws, one = lib.nrl_catalogue_ensemble_ranks_workspace_size, lib.nrl_catalogue_ranks_workspace_size
    base = ws(3, 512, 65536, 768, 1536, 8)
    assert base % 256 == 0 and base >= 3 * 1536 * 768 * 4 + (512 + 1536) * 8 * 4
    # the layout of nrl_catalogue_ranks with T gathered blocks: T = 1 is that entry's size, every further table adds one block
    for T in (1, 2, 3):
        assert ws(T, 512, 65536, 768, 1536, 8) == one(512, 65536, 768, 1536, 8) + (T - 1) * 1536 * 768 * 4
    assert ws(3, 1024, 65536, 768, 1536, 8) > base and ws(3, 512, 65536, 768, 3072, 8) > base and ws(3, 512, 65536, 768, 1536, 16) > base
    for args in ((1, 1, 1, 4, 1, 0), (3, 3, 1000, 300, 0, 7), (2, 130, 63, 4, 5, 2), (3, 512, 65536, 768, 1536, 0), (3, 4, 0, 8, 3, 0)):
        assert ws(*args) % 256 == 0 and ws(*args) >= 256
    # never O(B V): the table length does not enter once the slice count is fixed, and B V = 2^40 stays small
    assert base == ws(3, 512, 1 << 20, 768, 1536, 8) == ws(3, 512, (1 << 31) - 1, 768, 1536, 8)
    big = ws(3, 1 << 20, 1 << 20, 768, 1536, 0)
    assert big < 64 << 20                                    # (one (B, V) fp32 matrix there is 4 TiB)
    for args in ((0, 4, 100, 8, 3, 0), (4, 4, 100, 8, 3, 0), (3, -1, 100, 8, 3, 0), (3, 4, -1, 8, 3, 0), (3, 4, 100, 6, 3, 0),
                 (3, 4, 100, 1028, 3, 0), (3, 4, 1 << 31, 8, 3, 0), (3, 4, 100, 8, -1, 0), (3, 4, 100, 8, 3, -1), (3, 4, 100, 8, 1 << 31, 0)):
        assert ws(*args) == 256, args


def test_workspace_sizes_match_the_committed_table():
    """The size function is named ``_size`` (``tests/data/workspace_sizes.json`` pins the set of ``*_workspace_bytes`` functions)
    and has a table of its own: a layout change on purpose regenerates it."""
    ws = _lib_or_skip().nrl_catalogue_ensemble_ranks_workspace_size
    table = json.load(open(os.path.join(ROOT, "tests", "data", "catalogue_ensemble_rank_workspace_sizes.json")))
    assert len(table) >= 5 and {row["args"][0] for row in table} == {1, 2, 3}
    for row in table:
        assert ws(*row["args"]) == row["bytes"], row


def test_host_side_refusals_need_no_device():
    lib = _lib_or_skip()
    st = ctypes.c_int32(0)
    P = 256                                                  # a placeholder pointer: never read, every refusal is before a launch
    ptrs = (ctypes.c_void_p * 3)(P, P, P)
    wts = (ctypes.c_float * 3)(1.0, 0.2, -0.25)

    def call(T, B, V, D, n, slices=0, users=ptrs, tables=ptrs, weights=wts, tgt_idx=P, tgt_off=P, stats=P, moments=P, status=True,
             ws=P, ws_bytes=1 << 20):
        return lib.nrl_catalogue_ensemble_ranks(users, tables, weights, T, B, V, D, tgt_idx, tgt_off, n, None, None, None, slices, P, P,
                                                P, stats, moments, ctypes.addressof(st) if status else None, ws, ws_bytes, None)

    for args, word in (((3, -1, 100, 8, 3), "negative"), ((3, 4, -2, 8, 3), "negative"), ((3, 4, 100, 8, -3), "negative"),
                       ((3, 4, 100, 8, 3, -1), "negative"), ((0, 4, 100, 8, 3), "T in [1, 3]"), ((4, 4, 100, 8, 3), "T in [1, 3]"),
                       ((3, 4, 100, 6, 3), "multiple of 4"), ((3, 4, 100, 1028, 3), "multiple of 4"), ((3, 4, 1 << 31, 8, 3), "2^31"),
                       ((3, 4, 100, 8, 1 << 31), "2^31")):
        assert call(*args) == -1, args
        assert word in lib.nrl_last_error().decode(), lib.nrl_last_error()
    assert call(3, 4, 100, 8, 3, status=False) == -1 and "status" in lib.nrl_last_error().decode()
    assert call(3, 4, 100, 8, 3, tgt_off=None) == -1 and "tgt_idx without tgt_off" in lib.nrl_last_error().decode()
    assert call(3, 4, 100, 8, 0, tgt_off=None) == -1 and "tgt_idx without tgt_off" in lib.nrl_last_error().decode()
    for kw in ({"users": None}, {"tables": None}, {"weights": None}):
        assert call(3, 4, 100, 8, 3, **kw) == -1 and "null users / tables / weights" in lib.nrl_last_error().decode(), kw
    hole = (ctypes.c_void_p * 3)(P, None, P)
    assert call(3, 4, 100, 8, 3, users=hole) == -1 and "sub-model 1" in lib.nrl_last_error().decode()
    assert call(3, 4, 100, 8, 3, tables=hole) == -1 and "sub-model 1" in lib.nrl_last_error().decode()
    assert call(3, 4, 100, 8, 3, stats=None) == -1 and "out_stats" in lib.nrl_last_error().decode()
    assert call(3, 4, 100, 8, 3, moments=None) == -1 and "moments" in lib.nrl_last_error().decode()
    assert call(3, 0, 100, 8, 3) == 0                        # B == 0: success, nothing launched
    need = lib.nrl_catalogue_ensemble_ranks_workspace_size(3, 4, 100, 8, 3, 0)
    assert call(3, 4, 100, 8, 3, ws_bytes=need - 1) == -2 and "workspace too small" in lib.nrl_last_error().decode()
    assert call(3, 4, 100, 8, 3, ws=None) == -1 and "workspace" in lib.nrl_last_error().decode()


def test_python_entries_refuse_before_any_device_work():
    from newsreclib_amd import evaluation as E
    from newsreclib_amd import ops
    u, t = torch.zeros(2, 8), torch.zeros(5, 8)
    ti, to = torch.tensor([1]), torch.tensor([0, 1, 1])
    with pytest.raises(ValueError, match="1 to 3 sub-models"):
        ops.catalogue_ensemble_ranks([], [], [], ti, to)
    with pytest.raises(ValueError, match="1 to 3 sub-models"):
        ops.catalogue_ensemble_ranks([u] * 4, [t] * 4, [1.0] * 4, ti, to)
    with pytest.raises(ValueError, match="1 to 3 sub-models"):
        ops.catalogue_ensemble_ranks([u, u], [t, t], [1.0], ti, to)
    with pytest.raises(ValueError, match="of one shape each"):
        ops.catalogue_ensemble_ranks([u, torch.zeros(3, 8)], [t, t], [1.0, 1.0], ti, to)
    with pytest.raises(ValueError, match="of one shape each"):
        ops.catalogue_ensemble_ranks([u], [torch.zeros(5, 12)], [1.0], ti, to)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.catalogue_ensemble_ranks([u], [t], [1.0], ti, to)
    cache = object.__new__(E.MannerVectorCache)
    args = (torch.tensor([1, 2, 3]), torch.tensor([2, 1]), torch.tensor([4]), torch.tensor([1, 0]))
    with pytest.raises(RuntimeError, match="no CPU path"):
        cache.rank_clicks_ensemble(*args)
    with pytest.raises(ValueError, match="rank_clicks_ensemble takes at most 32 clicks"):
        cache.rank_clicks_ensemble(args[0], args[1], torch.ones(33, dtype=torch.int64), torch.tensor([33, 0]))
    with pytest.raises(ValueError, match="one entry per user"):
        cache.rank_clicks_ensemble(args[0], args[1], args[2], torch.tensor([1]))
    # `rank_clicks` itself keeps refusing and says where to go
    with pytest.raises(NotImplementedError, match="only the dot-product families are served.*rank_clicks_ensemble"):
        cache.rank_clicks(*args)


def test_evaluate_full_rank_ensemble_needs_a_cache_with_the_method():
    from newsreclib_amd import evaluation as E
    from newsreclib_amd.nrms_module import NRMSModule
    users = [{"hist": torch.tensor([1, 2]), "clicks": torch.tensor([3])}]
    with pytest.raises(TypeError, match="rank_clicks_ensemble"):
        E.evaluate_full_rank(E.NewsVectorCache(object.__new__(NRMSModule), None), users, ensemble=True)
    with pytest.raises(TypeError, match="rank_clicks_ensemble"):
        E.evaluate_full_rank(object.__new__(E.NpaFeatureCache), users, ensemble=True)


# ---- the references on their own ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,V,D", ER.INTERVAL_SHAPES)
def test_the_float64_intervals_are_sharp_on_the_inputs_used(B, V, D):
    """The condition the GPU tier's float64 check rests on, on the reference alone: at least two thirds of the targets in the
    population have a one-point interval and none is wider than 2."""
    assert D <= 64
    *_, intervals = ER.interval_case(B, V, D)
    inside = [iv for iv in intervals if iv is not None]
    points = sum(lo == hi for lo, hi in inside)
    print(f"B = {B}, V = {V}, D = {D}: {points} of {len(inside)} intervals are one point, widest {max(hi - lo for lo, hi in inside)}")
    assert len(inside) >= 20 and 3 * points >= 2 * len(inside) and max(hi - lo for lo, hi in inside) <= 2


def test_exact_reference_against_a_stable_sort():
    """``ranks_from_bits`` on tie-heavy integer scores against a stable descending sort; a refused user and a NaN row."""
    g = torch.Generator().manual_seed(4)
    B, V = 6, 90
    raw = [torch.randint(-2, 3, (B, V), generator=g).float() for _ in range(2)]
    raw[0][:, 17] = float("nan")
    stats = torch.tensor([[0.5, 2.0], [-1.0, 0.5]]).expand(B, 2, 2).clone()
    stats[4, 1, 1] = 0.0                                             # user 4 cannot be standardised
    eligible = (torch.rand(V, generator=g) > 0.2).to(torch.uint8)
    excl = [torch.randint(0, V, (int(n),), generator=g).tolist() for n in (0, 3, 10, 1, 25, 7)]
    rank, score, ranked = ER.ranks_from_bits(raw, stats, (1.0, -0.25), [list(range(V))] * B, excl, eligible)
    rank, score = rank.reshape(B, V), score.reshape(B, V)
    z = ER.ensemble_from_bits(raw, stats, (1.0, -0.25))
    pop = C.allowed(B, V, excl, eligible)
    pop[:, 17] = False
    assert len(torch.unique(z[pop])) < 60                            # tie-heavy
    for b in range(B):
        if b == 4:
            assert int(ranked[b]) == 0 and not bool(rank[b].any()) and bool((score[b] == ER.NEG_INF).all())
            continue
        order = torch.sort(torch.where(pop[b], -z[b], torch.full((V,), float("inf"))), stable=True)[1]
        n = int(pop[b].sum())
        assert int(ranked[b]) == n and torch.equal(rank[b, order[:n]], torch.arange(1, n + 1, dtype=torch.int32))
        assert not bool(rank[b, order[n:]].any())
        assert torch.equal(score[b][pop[b]], z[b][pop[b]])
