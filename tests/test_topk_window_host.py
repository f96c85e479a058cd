"""CPU tier of the per-user time windows on the full-catalogue top-k and rank: the ABI (header against ``_lib.SIGNATURES`` and,
when the library is built, its exports), the pinned flag dictionaries, the float64 reference (``tests/topk_window_ref.py``)
against a brute-force loop, the refusals of the two ``ops`` wrappers that come before any device work, and the host-side window
arithmetic of ``recommend_users``."""
import os
import re

import pytest
import torch

from tests import catalogue_ref as C
from tests import topk_window_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("nrl_topk_window_scores", "nrl_catalogue_window_ranks")


def _header():
    return open(os.path.join(ROOT, "include", "newsreclib_amd.h")).read()


def _declared_arguments(header, name):
    m = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
    assert m, name + " is not declared in the header"
    return [a.strip().split()[-1].lstrip("*") for a in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")]


def test_the_two_entries_are_in_the_header_and_in_the_signatures():
    from newsreclib_amd import _lib, ops
    assert callable(ops.topk_window_scores) and callable(ops.catalogue_window_ranks)
    header = _header()
    scores, ranks = (_declared_arguments(header, n) for n in NAMES)
    assert scores[:9] == ["user_vec", "table", "B", "V", "D", "k", "row_time", "win_lo", "win_hi"]
    assert scores[9:] == _declared_arguments(header, "nrl_topk_scores")[6:]
    assert ranks[:11] == ["user_vec", "table", "B", "V", "D", "tgt_idx", "tgt_off", "n_targets", "row_time", "win_lo", "win_hi"]
    assert ranks[11:] == _declared_arguments(header, "nrl_catalogue_ranks")[8:]
    for name, args in zip(NAMES, (scores, ranks)):
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == len(args), name
    assert len(scores) == 19 and len(ranks) == 22
    assert _lib.ABI_VERSION == 19 and re.search(r"#define NRL_ABI_VERSION 19\b", header)


def test_the_built_library_exports_the_two_entries():
    from newsreclib_amd import _build, ops
    assert callable(ops.topk_window_scores)
    if not os.path.exists(_build.LIB):
        return                                                   # (nothing built here: the GPU tier loads it)
    data = open(_build.LIB, "rb").read()
    for name in NAMES:
        assert name.encode() + b"\0" in data, name


def test_the_flag_dictionaries_are_unchanged():
    from newsreclib_amd import ops
    assert callable(ops.topk_window_scores)
    assert set(ops.TOPK_FLAGS) == {1, 2, 4, 8} and set(ops.RANK_FLAGS) == {1, 2, 4, 16, 32}
    assert ops.INT32_MIN == R.INT32_MIN == -2 ** 31 and ops.INT32_MAX == R.INT32_MAX == 2 ** 31 - 1


def test_the_reference_agrees_with_a_brute_force_loop():
    from newsreclib_amd import ops
    assert callable(ops.topk_window_scores)
    B, V, D, k = 4, 40, 8, 6
    U, T = C.int_vectors(9, B, V, D)
    s = U.double() @ T.double().T
    row_time = torch.arange(V) // 4
    lo = torch.tensor([R.INT32_MIN, 3, 6, 2], dtype=torch.int32)
    hi = torch.tensor([R.INT32_MAX, 3, 5, 7], dtype=torch.int32)
    excl = [[1, 2], [], [24], [8, 9, 99]]
    eligible = torch.ones(V, dtype=torch.uint8)
    eligible[[0, 12, 13]] = 0
    targets = [[0, 5], [12, 14, 2], [24], [9, 10, 31, 32]]
    idx, score = R.expected_topk(s, k, row_time, lo, hi, excl, eligible)
    rank, rscore, ranked = R.expected_ranks(s, targets, row_time, lo, hi, excl, eligible)
    at = 0
    for b in range(B):
        rows = [v for v in range(V) if eligible[v] and v not in excl[b] and int(lo[b]) <= int(row_time[v]) <= int(hi[b])]
        rows.sort(key=lambda v: (-float(s[b, v]), v))
        assert idx[b].tolist() == (rows + [-1] * k)[:k] and int(ranked[b]) == len(rows), b
        assert score[b].tolist() == ([float(s[b, v]) for v in rows] + [float("-inf")] * k)[:k], b
        for t in targets[b]:
            assert int(rank[at]) == (rows.index(t) + 1 if t in rows else 0), (b, t)
            assert float(rscore[at]) == (float(s[b, t]) if t in rows else float("-inf")), (b, t)
            at += 1
    assert ranked.tolist()[2] == 0 and idx[2].tolist() == [-1] * k    # the empty window
    assert R.window_mask(row_time, lo, hi).sum(1).tolist() == [40, 4, 0, 24]


def _wrappers():
    from newsreclib_amd import ops
    U, T = torch.zeros(3, 8), torch.zeros(10, 8)
    ti, to = torch.zeros(2, dtype=torch.int64), torch.tensor([0, 1, 2, 2])
    return ((lambda rt, lo, hi: ops.topk_window_scores(U, T, 2, rt, lo, hi)),
            (lambda rt, lo, hi: ops.catalogue_window_ranks(U, T, ti, to, rt, lo, hi)))


def test_the_wrappers_refuse_dtypes_lengths_and_the_cpu():
    rt, b = torch.zeros(10, dtype=torch.int32), torch.zeros(3, dtype=torch.int32)
    for call in _wrappers():
        for bad in ((rt.long(), b, b), (rt, b.long(), b), (rt, b, b.float()), (rt.tolist(), b, b)):
            with pytest.raises(TypeError, match="int32"):
                call(*bad)
        for bad in ((rt[:9], b, b), (rt, b[:2], b), (rt, b, torch.zeros(4, dtype=torch.int32)), (rt.reshape(2, 5), b, b)):
            with pytest.raises(ValueError, match="one entry per"):
                call(*bad)
        with pytest.raises(RuntimeError, match="must live on the GPU"):
            call(rt, b, b)


def test_user_windows_clamp_at_both_int32_ends_and_need_a_time():
    from newsreclib_amd.evaluation import user_windows
    users = [{"hist": [1], "time": 100}, {"hist": [1], "time": R.INT32_MAX - 3}, {"hist": [1], "time": R.INT32_MIN + 2},
             {"hist": [1], "time": 2 ** 40}, {"hist": [1], "time": torch.tensor(7)}]
    lo, hi = user_windows(users, 24, 5)
    assert lo.dtype == hi.dtype == torch.int32
    assert lo.tolist() == [76, R.INT32_MAX - 27, R.INT32_MIN, R.INT32_MAX, -17]
    assert hi.tolist() == [105, R.INT32_MAX, R.INT32_MIN + 7, R.INT32_MAX, 12]
    lo, hi = user_windows(users[:2], None, 0)                    # the window of ``evaluate_full_rank(until_request=True)``
    assert lo.tolist() == [R.INT32_MIN] * 2 and hi.tolist() == [100, R.INT32_MAX - 3]
    lo, hi = user_windows(users[:1], 2 ** 33, None)
    assert lo.tolist() == [R.INT32_MIN] and hi.tolist() == [R.INT32_MAX]
    with pytest.raises(ValueError, match='user 1 of the list has no "time"'):
        user_windows([users[0], {"hist": [1]}], 24, 0)


def test_recommend_users_refuses_before_any_device_work():
    from types import SimpleNamespace

    from newsreclib_amd import evaluation as E
    plain = SimpleNamespace(module=SimpleNamespace(dot_product_scorer=True), table=SimpleNamespace(attrs={}, device="cpu"),
                            _row_time=None)
    with pytest.raises(ValueError, match='no "time"'):
        E.recommend_users(plain, [{"hist": [1]}], 3, window=(24, 0))
    with pytest.raises(ValueError, match="integer news attribute `time`"):
        E.recommend_users(plain, [{"hist": [1], "time": 5}], 3, window=(24, 0))
    with pytest.raises(NotImplementedError, match="class-capped"):
        E.recommend_users(plain, [{"hist": [1], "time": 5}], 3, window=(24, 0), cap=("category", 2))
    for marker in ("multi_interest_scorer", "dnn_predictor_scorer", "personalized_pooling_scorer", "class_biased_scorer"):
        other = SimpleNamespace(module=SimpleNamespace(**{marker: True}), table=plain.table, _row_time=None)
        with pytest.raises(NotImplementedError, match="tkw_scores_kernel"):
            E.recommend_users(other, [{"hist": [1], "time": 5}], 3, window=(24, 0))
        with pytest.raises(NotImplementedError, match="tkw_scores_kernel"):
            E.evaluate_full_rank(other, [{"hist": [1], "clicks": [2], "time": 5}], until_request=True)
    manner = SimpleNamespace(module=SimpleNamespace(), table=plain.table, recommend_ensemble=None, _row_time=None)
    with pytest.raises(NotImplementedError, match="MannerVectorCache"):
        E.recommend_users(manner, [{"hist": [1], "time": 5}], 3, window=(24, 0))
    with pytest.raises(ValueError, match='no "time"'):
        E.evaluate_full_rank(plain, [{"hist": [1], "clicks": [2]}], until_request=True)


def test_only_the_served_methods_take_a_window():
    """A filter argument must never be accepted and ignored: ``window`` is a parameter of the two methods that apply it and of no
    other ``recommend*`` / ``rank_clicks*`` of any cache."""
    import inspect

    from newsreclib_amd import evaluation as E
    takes = {(cls.__name__, name) for cls in (E.NewsVectorCache, E.MannerVectorCache, E.NpaFeatureCache)
             for name, fn in inspect.getmembers(cls, inspect.isfunction)
             if name.startswith(("recommend", "rank_clicks")) and "window" in inspect.signature(fn).parameters}
    assert takes == {("NewsVectorCache", "recommend"), ("NewsVectorCache", "rank_clicks")}
