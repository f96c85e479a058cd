"""Host tier of the full-catalogue rank of held-out clicks: ABI surface, workspace sizing, host-side refusals (no device is touched
before they return), ``metrics.full_rank_metrics`` against ``ranking_metrics`` and a brute-force loop, and the reference itself
against a stable sort."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from tests import catalogue_ref as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("nrl_catalogue_ranks_workspace_size", "nrl_catalogue_ranks")


def _lib_or_skip():
    from newsreclib_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("library not built")
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES + ("nrl_last_error", "nrl_abi_version"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    return lib


def test_symbols_are_declared_typed_and_exported_without_an_abi_bump():
    from newsreclib_amd import _lib, ops
    header = open(os.path.join(ROOT, "include", "newsreclib_amd.h")).read()
    assert _lib.ABI_VERSION == 19 and re.search(r"#define NRL_ABI_VERSION 19\b", header)
    assert re.search(r"#define NRL_RANK_MAX_TARGETS 32\b", header) and ops.RANK_MAX_TARGETS == 32
    assert re.search(r"#define NRL_RANK_E_TARGETS 16\b", header) and re.search(r"#define NRL_RANK_E_TARGET_ROW 32\b", header)
    assert set(ops.RANK_FLAGS) == {1, 2, 4, 16, 32}
    for name in NAMES:
        assert re.search(r"\b%s\(" % name, header) and name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["nrl_catalogue_ranks"][1]) == 19 and len(_lib.SIGNATURES[NAMES[0]][1]) == 5
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("library not built")
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(NAMES) <= exported
    assert _lib_or_skip().nrl_abi_version() == 19


def test_workspace_bytes():
    ws = _lib_or_skip().nrl_catalogue_ranks_workspace_size
    base = ws(512, 65536, 400, 1536, 8)
    assert base % 256 == 0 and base >= 1536 * 400 * 4 + (512 + 1536) * 8 * 4
    assert ws(1024, 65536, 400, 1536, 8) > base and ws(512, 65536, 400, 3072, 8) > base and ws(512, 65536, 400, 1536, 16) > base
    for args in ((1, 1, 4, 1, 0), (3, 1000, 300, 0, 7), (130, 63, 4, 5, 2), (512, 65536, 400, 1536, 0), (4, 0, 8, 3, 0)):
        assert ws(*args) % 256 == 0 and ws(*args) >= 256
    # O(n_targets D + (B + n_targets) slices): the table length does not enter once the slice count is fixed (and reachable)
    assert base == ws(512, 1 << 20, 400, 1536, 8) == ws(512, (1 << 31) - 1, 400, 1536, 8)
    assert ws(512, 1 << 24, 400, 1536, 0) == ws(512, 65536, 400, 1536, 0) < 512 * 65536 * 4 / 8
    for args in ((-1, 100, 8, 3, 0), (4, -1, 8, 3, 0), (4, 100, 6, 3, 0), (4, 100, 1028, 3, 0), (4, 1 << 31, 8, 3, 0),
                 (4, 100, 8, -1, 0), (4, 100, 8, 3, -1), (4, 100, 8, 1 << 31, 0)):
        assert ws(*args) == 256, args


def test_workspace_sizes_match_the_committed_table():
    """``tests/data/workspace_sizes.json`` pins the set of ``*_workspace_bytes`` functions, so this entry's size function is named
    ``_size`` and has a table of its own: a layout change on purpose regenerates it."""
    import json
    ws = _lib_or_skip().nrl_catalogue_ranks_workspace_size
    table = json.load(open(os.path.join(ROOT, "tests", "data", "catalogue_rank_workspace_sizes.json")))
    assert len(table) >= 4
    for row in table:
        assert ws(*row["args"]) == row["bytes"], row


def test_host_side_refusals_need_no_device():
    lib = _lib_or_skip()
    st = ctypes.c_int32(0)
    P = 256                                                  # a placeholder pointer: never read, every refusal is before a launch

    def call(B, V, D, n, slices=0, tgt_idx=P, tgt_off=P, status=True, ws=P, ws_bytes=1 << 20):
        return lib.nrl_catalogue_ranks(P, P, B, V, D, tgt_idx, tgt_off, n, None, None, None, slices, P, P, P,
                                       ctypes.addressof(st) if status else None, ws, ws_bytes, None)

    for args, word in (((-1, 100, 8, 3), "negative"), ((4, -2, 8, 3), "negative"), ((4, 100, 8, -3), "negative"),
                       ((4, 100, 8, 3, -1), "negative"), ((4, 100, 6, 3), "multiple of 4"), ((4, 100, 1028, 3), "multiple of 4"),
                       ((4, 1 << 31, 8, 3), "2^31"), ((4, 100, 8, 1 << 31), "2^31")):
        assert call(*args) == -1, args
        assert word in lib.nrl_last_error().decode(), lib.nrl_last_error()
    assert call(4, 100, 8, 3, status=False) == -1 and "status" in lib.nrl_last_error().decode()
    assert call(4, 100, 8, 3, tgt_off=None) == -1 and "tgt_idx without tgt_off" in lib.nrl_last_error().decode()
    assert call(4, 100, 8, 0, tgt_off=None) == -1 and "tgt_idx without tgt_off" in lib.nrl_last_error().decode()
    assert call(0, 100, 8, 3) == 0                           # B == 0: success, nothing launched
    need = lib.nrl_catalogue_ranks_workspace_size(4, 100, 8, 3, 0)
    assert call(4, 100, 8, 3, ws_bytes=need - 1) == -2 and "workspace too small" in lib.nrl_last_error().decode()
    assert call(4, 100, 8, 3, ws=None) == -1 and "workspace" in lib.nrl_last_error().decode()


def test_python_entries_refuse_before_any_device_work():
    from newsreclib_amd import evaluation as E
    from newsreclib_amd import ops
    from newsreclib_amd.nrms_module import NRMSModule
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.catalogue_ranks(torch.zeros(2, 8), torch.zeros(5, 8), torch.tensor([1]), torch.tensor([0, 1, 1]))
    cache = E.NewsVectorCache(object.__new__(NRMSModule), None)
    with pytest.raises(RuntimeError, match="no CPU path"):
        cache.rank_clicks(torch.tensor([1, 2, 3]), torch.tensor([2, 1]), torch.tensor([4]), torch.tensor([1, 0]))


# ---- the reference against a stable sort ---------------------------------------------------------------------------------------
def test_reference_against_a_stable_sort():
    g = torch.Generator().manual_seed(4)
    B, V = 6, 90
    U, T = torch.randint(-1, 2, (B, 4), generator=g).float(), torch.randint(-1, 2, (V, 4), generator=g).float()      # few values
    eligible = (torch.rand(V, generator=g) > 0.2).to(torch.uint8)
    excl = [torch.randint(0, V, (int(n),), generator=g).tolist() for n in (0, 3, 10, 1, 25, 7)]
    targets = [list(range(V)) for _ in range(B)]                     # every row of every user
    raw = U.double() @ T.double().T
    rank, score, ranked = C.expected_ranks(raw, targets, excl, eligible)
    s = C.masked(raw, C.population(raw, excl, eligible)[0])
    assert len(torch.unique(s)) < 12                                 # tie-heavy
    neg, order = torch.sort(-s, dim=1, stable=True)                  # score descending, equal scores by ascending row
    rank = rank.reshape(B, V)
    for b in range(B):
        n = int(torch.isfinite(s[b]).sum())
        assert int(ranked[b]) == n
        assert torch.equal(rank[b, order[b, :n]], torch.arange(1, n + 1, dtype=torch.int32))
        assert bool((rank[b, order[b, n:]] == 0).all())
    assert bool((score.reshape(B, V)[rank == 0] == float("-inf")).all())
    assert C.expected_ranks(raw, [[-1, V], [], [], [], [], []])[0].tolist() == [0, 0]


# ---- full_rank_metrics -----------------------------------------------------------------------------------------------------------
def _metric_case():
    """7 users over V = 40 with integer scores (many ties): user 2 has no clicks, every click of user 3 is invalid, user 5's
    population is exactly its clicks (N = P)."""
    g = torch.Generator().manual_seed(9)
    B, V = 7, 40
    s = torch.randint(-3, 4, (B, V), generator=g).double()
    s[:, [0, 11]] = float("-inf")                                    # ineligible for everyone
    for b in range(B):
        s[b, torch.randint(1, V, (4,), generator=g)] = float("-inf")     # the user's history
    clicks = [torch.randperm(V, generator=g)[:n].tolist() for n in (1, 4, 0, 3, 12, 5, 2)]
    clicks[3] = [0, 11, V + 2]                                       # ineligible, ineligible, outside the table
    clicks[0] = [int(torch.isfinite(s[0]).nonzero()[3])]
    clicks[4][0] = 11                                                # one invalid click among valid ones
    keep = torch.zeros(V, dtype=torch.bool)
    keep[clicks[5]] = True
    s[5, ~keep] = float("-inf")
    s[5, keep] = s[5, keep].nan_to_num(neginf=1.0)
    return s, clicks


def test_full_rank_metrics_against_ranking_metrics_and_brute_force():
    from newsreclib_amd.metrics import full_rank_metrics, ranking_metrics
    s, clicks = _metric_case()
    B, V = s.shape
    rank, _, ranked = C.ranks(s, torch.isfinite(s), clicks)
    sizes = torch.tensor([len(c) for c in clicks])
    top_k = (1, 5, 10)
    got = full_rank_metrics(rank, sizes, ranked, top_k)
    assert int(ranked[5]) == len(clicks[5]) and sizes[2] == 0 and not bool(rank[sizes[:3].sum():sizes[:4].sum()].any())

    # ranking_metrics on one impression per user: the qualifying rows in ascending row order
    preds, labels, csz = [], [], []
    for b in range(B):
        ok = torch.isfinite(s[b])
        lab = torch.zeros(V)
        lab[[c for c in clicks[b] if 0 <= c < V]] = 1.0
        preds.append(s[b][ok].float())
        labels.append(lab[ok])
        csz.append(int(ok.sum()))
    want = ranking_metrics(torch.cat(preds), torch.cat(labels), torch.tensor(csz), top_k)
    assert abs(got["mrr"] - want["mrr"]) <= 1e-6
    for k in top_k:
        assert abs(got[f"ndcg@{k}"] - want[f"ndcg@{k}"]) <= 1e-6, k

    # brute force: positions in the stable descending order of the qualifying rows
    recall, hit, auc, mrr = {k: [] for k in top_k}, {k: [] for k in top_k}, [], []
    for b in range(B):
        rows = [v for v in range(V) if math.isfinite(float(s[b, v]))]
        order = sorted(rows, key=lambda v: (-float(s[b, v]), v))
        pos = sorted(order.index(c) + 1 for c in clicks[b] if c in order)
        for k in top_k:
            recall[k].append(sum(p <= k for p in pos) / len(pos) if pos else 0.0)
            hit[k].append(float(bool(pos) and pos[0] <= k))
        mrr.append(1.0 / pos[0] if pos else 0.0)
        others = [v for v in order if v not in clicks[b]]
        if pos and others:
            right = sum(order.index(c) < order.index(o) for c in clicks[b] if c in order for o in others)
            auc.append(right / (len(pos) * len(others)))
        else:
            auc.append(0.0)
    assert abs(got["mrr"] - np.mean(mrr)) <= 1e-12
    assert abs(got["auc_user"] - np.mean(auc)) <= 1e-12
    for k in top_k:
        assert abs(got[f"recall@{k}"] - np.mean(recall[k])) <= 1e-12 and abs(got[f"hit@{k}"] - np.mean(hit[k])) <= 1e-12
    assert set(got) == {"mrr", "auc_user"} | {f"{m}@{k}" for m in ("ndcg", "recall", "hit") for k in top_k}


def test_full_rank_metrics_edges():
    from newsreclib_amd.metrics import full_rank_metrics
    empty = full_rank_metrics(torch.zeros(0, dtype=torch.int32), torch.zeros(0, dtype=torch.int64), torch.zeros(0, dtype=torch.int32))
    assert empty["mrr"] == 0.0 and empty["ndcg@5"] == 0.0 and empty["auc_user"] == 0.0
    none = full_rank_metrics(torch.zeros(0, dtype=torch.int32), torch.tensor([0, 0]), torch.tensor([10, 20]))
    assert all(v == 0.0 for v in none.values())
    one = full_rank_metrics(torch.tensor([1, 0, 3], dtype=torch.int32), torch.tensor([1, 2]), torch.tensor([10, 10]), (2,))
    assert one["mrr"] == pytest.approx((1 + 1 / 3) / 2) and one["hit@2"] == 0.5 and one["recall@2"] == 0.5
    assert one["ndcg@2"] == pytest.approx(0.5) and one["auc_user"] == pytest.approx((1 + (1 - 2 / 9)) / 2)
