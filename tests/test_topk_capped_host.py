"""CPU tier of the class-capped top-k: the greedy definition against the restated streaming insertion and slice merge
(``tests/topk_capped_ref.py``), and the native entries' argument checks, which run before anything touches a device."""
import random

import pytest
import torch

from tests import topk_capped_ref as R

NAMES = ("nrl_topk_scores_capped", "nrl_topk_ensemble_scores_capped")


def _case(rng):
    V = rng.choice([1, 2, 5, 17, 64, 65, 130, 300])
    k = rng.choice([1, 2, 5, 10, 63, 64])
    n_cls = rng.choice([1, 3, 19])
    m = rng.choice([1, 2, 3, k, k + 5])
    spread = rng.choice([1, 3, 50])                     # few distinct scores: ties everywhere
    scores = [None if rng.random() < 0.1 else float(rng.randint(-spread, spread)) for _ in range(V)]
    if rng.random() < 0.3:
        scores = [(-0.0 if s == 0.0 and rng.random() < 0.5 else s) for s in scores]
    classes = [rng.randint(-1, n_cls - 2) * 1000003 for _ in range(V)]          # any int32 is a class
    return V, k, m, scores, classes


def test_streaming_and_slice_merge_equal_the_greedy_definition():
    rng = random.Random(20)
    for _ in range(1500):
        V, k, m, scores, classes = _case(rng)
        want = R.greedy(scores, classes, k, m)
        order = list(range(V))
        rng.shuffle(order)
        assert R.stream(scores, classes, k, m, order).rows() == want
        n_sl = rng.randint(1, 5)
        cuts = sorted(rng.randint(0, V) for _ in range(n_sl - 1))
        parts = [list(range(a, b)) for a, b in zip([0] + cuts, cuts + [V])]
        rng.shuffle(parts)                              # the merge does not depend on the order of the slices either
        lists = [R.stream(scores, classes, k, m, p) for p in parts]
        assert R.merge(lists, scores, classes, k, m).rows() == want


def test_the_list_never_holds_more_than_m_of_a_class_and_fills_up_when_it_can():
    rng = random.Random(21)
    for _ in range(300):
        V, k, m, scores, classes = _case(rng)
        rows = R.stream(scores, classes, k, m, list(range(V))).rows()
        per = {}
        for v in rows:
            per[classes[v]] = per.get(classes[v], 0) + 1
        assert all(n <= m for n in per.values())
        avail = {}
        for v in range(V):
            if scores[v] is not None:
                avail[classes[v]] = avail.get(classes[v], 0) + 1
        assert len(rows) == min(k, sum(min(m, n) for n in avail.values()))


def test_a_cap_of_k_or_more_is_the_uncapped_top_k():
    rng = random.Random(22)
    for _ in range(300):
        V, k, _, scores, classes = _case(rng)
        plain = sorted((v for v in range(V) if scores[v] is not None), key=lambda v: (-scores[v], v))[:k]
        for m in (k, k + 1, 2 ** 31 - 1):
            assert R.greedy(scores, classes, k, m) == plain
            assert R.stream(scores, classes, k, m, list(range(V))).rows() == plain


def test_tensor_reference_is_the_greedy_definition():
    g = torch.Generator().manual_seed(5)
    B, V, k, m = 4, 90, 8, 2
    s = torch.randint(-3, 4, (B, V), generator=g).double()
    s[0, 5:40] = float("-inf")
    s[1, 7] = float("nan")
    cls = torch.randint(0, 5, (V,), generator=g)
    idx, score = R.reference(s, torch.isfinite(s), cls, k, m)
    for b in range(B):
        row = [None if (x != x or x == float("-inf")) else x for x in s[b].tolist()]
        want = R.greedy(row, cls.tolist(), k, m)
        assert idx[b, :len(want)].tolist() == want and bool((idx[b, len(want):] == -1).all())
        assert score[b, :len(want)].tolist() == [row[v] for v in want]
    # a walk over the uncapped order finds the same lists
    neg, order = torch.sort(-torch.where(torch.isnan(s), torch.full_like(s, float("-inf")), s), dim=1, stable=True)
    listed = torch.where(neg < float("inf"), order, torch.full_like(order, -1))
    w_idx, w_score, decided = R.walk_listed(listed, (-neg).float(), cls, k, m)
    assert decided and torch.equal(w_idx, idx) and torch.equal(w_score, score)


# ---- the native entries refuse bad arguments before they launch anything (no device is touched: the pointers are never read) ------
def _lib():
    from newsreclib_amd import _build, _lib
    _build.build(verbose=False)
    return _lib.load()


def _dot_args(k=5, m=2, row_class=64, status=64, V=100):
    # user, table, B, V, D, k, row_class, m, excl_idx, excl_off, eligible, slices, out_idx, out_score, status, ws, ws_bytes, stream
    return [64, 64, 4, V, 8, k, row_class, m, None, None, None, 0, 64, 64, status, None, 0, None]


def test_limits_are_declared_once():
    import os
    import re
    from newsreclib_amd import ops
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "newsreclib_amd.h")).read()
    assert re.search(r"#define NRL_TOPK_CAP_MAX_K 64\b", header) and ops.TOPK_CAP_MAX_K == 64


@pytest.mark.parametrize("change,needle", [(dict(k=65), "k in [1, 64]"), (dict(k=0), "k in [1, 128]"), (dict(m=0), "max_per_class"),
                                           (dict(m=-3), "max_per_class"), (dict(row_class=None), "row_class"),
                                           (dict(status=None), "status")])
def test_dot_entry_refuses_bad_arguments(change, needle):
    lib = _lib()
    assert lib.nrl_topk_scores_capped(*_dot_args(**change)) == -1
    assert needle in lib.nrl_last_error().decode() and "topk_scores_capped" in lib.nrl_last_error().decode()


def test_the_uncapped_checks_come_first_and_the_workspace_is_the_uncapped_one():
    lib = _lib()
    # k = 200 breaks the family's limit and the cap's: the family's message wins, as in the uncapped entry
    assert lib.nrl_topk_scores_capped(*_dot_args(k=200)) == -1 and "k in [1, 128]" in lib.nrl_last_error().decode()
    # every check passes: the next refusal is the workspace's (null), still before any launch
    assert lib.nrl_topk_scores_capped(*_dot_args()) != 0
    assert "max_per_class" not in lib.nrl_last_error().decode() and "row_class" not in lib.nrl_last_error().decode()
    # B == 0 returns success without a launch once the arguments are sound, and refuses when they are not
    args = _dot_args()
    args[2] = 0
    assert lib.nrl_topk_scores_capped(*args) == 0
    args[7] = 0
    assert lib.nrl_topk_scores_capped(*args) == -1


def test_ensemble_entry_refuses_bad_arguments():
    import ctypes
    lib = _lib()
    ptrs = (ctypes.c_void_p * 2)(64, 64)
    wts = (ctypes.c_float * 2)(1.0, 0.5)

    def args(k=5, m=2, row_class=64, T=2):
        return [ptrs, ptrs, wts, T, 4, 100, 8, k, row_class, m, None, None, None, 0, 64, 64, 64, 64, 64, None, 0, None]

    for kw, needle in ((dict(k=65), "k in [1, 64]"), (dict(m=0), "max_per_class"), (dict(row_class=None), "row_class"),
                       (dict(T=4), "T in [1, 3]")):
        assert lib.nrl_topk_ensemble_scores_capped(*args(**kw)) == -1
        msg = lib.nrl_last_error().decode()
        assert needle in msg and "topk_ensemble_scores_capped" in msg, msg


def test_wrappers_check_row_class_on_the_host():
    from newsreclib_amd import ops
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.topk_scores_capped(torch.zeros(2, 4), torch.zeros(9, 4), 3, torch.zeros(9, dtype=torch.int32), 1)
