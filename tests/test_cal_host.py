"""CPU tier of the calibrated greedy re-ranking (``nrl_calibrated_rerank``): the ABI (header against ``_lib.SIGNATURES`` and the
library), the limits and the flags, every native refusal and their order through ctypes without a device, the Python-side
refusals, hand-worked cases and the header's five properties on the two restatements (``tests/cal_ref.py``) the GPU tests compare
against, and ``ops.class_targets`` against ``numpy.bincount``."""
import ctypes
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import cal_ref as R
from tests import mmr_ref as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
ARGS = ["pool_idx", "pool_score", "table", "B", "N", "V", "D", "row_class", "target", "S", "k", "lambda", "mu", "gamma", "similarity",
        "normalize", "out_idx", "out_score", "out_obj", "out_cal", "status", "stream"]


def _header():
    return open(os.path.join(ROOT, "include", "newsreclib_amd.h")).read()


def _native():
    from newsreclib_amd import _build, _lib
    _build.build(verbose=False)
    return _lib.load()


def test_the_entry_is_in_the_header_in_the_signatures_and_in_the_library():
    from newsreclib_amd import _lib
    header = _header()
    m = re.search(r"\bint nrl_calibrated_rerank\(([^;]*)\);", header)
    assert m, "nrl_calibrated_rerank is not declared in the header"
    assert [a.strip().split()[-1].lstrip("*") for a in m.group(1).split(",")] == ARGS
    types = _lib.SIGNATURES["nrl_calibrated_rerank"][1]
    assert len(types) == len(ARGS)
    assert [ARGS[i] for i, t in enumerate(types) if t is ctypes.c_float] == ["lambda", "mu", "gamma"]
    assert [ARGS[i] for i, t in enumerate(types) if t is ctypes.c_int64] == ["B", "V"]
    assert [ARGS[i] for i, t in enumerate(types) if t is ctypes.c_int32] == ["N", "D", "S", "k", "similarity", "normalize"]
    assert _lib.ABI_VERSION == 19 and re.search(r"#define NRL_ABI_VERSION 19\b", header)      # one new symbol, the number stays
    assert hasattr(_native(), "nrl_calibrated_rerank")


def test_limits_and_flags():
    from newsreclib_amd import ops
    header = _header()
    assert re.search(r"#define NRL_CAL_MAX_CLASSES 64\b", header) and ops.CAL_MAX_CLASSES == 64 == R.MAX_CLASSES
    assert re.search(r"#define NRL_CAL_E_TARGET 128\b", header) and re.search(r"#define NRL_TOPK_E_CLASS 64\b", header)
    assert (R.E_ROW, R.E_NAN, R.E_CLASS, R.E_TARGET) == (1, 4, 64, 128)
    assert set(ops.CAL_FLAGS) == {1, 4, 64, 128}
    assert "outside [0, V)" in ops.CAL_FLAGS[1] and "non-finite" in ops.CAL_FLAGS[4] and "class id" in ops.CAL_FLAGS[64]
    assert "target" in ops.CAL_FLAGS[128]
    # a dictionary of its own: the pinned key sets are untouched
    assert set(ops.MMR_FLAGS) == {1, 4} and set(ops.TOPK_FLAGS) == {1, 2, 4, 8} and set(ops.RANK_FLAGS) == {1, 2, 4, 16, 32}


# ---- the native entry refuses bad arguments before it launches anything (no device is touched: the pointers are never read) ---------
def _args(pool_idx=64, pool_score=64, table=64, B=4, N=16, V=100, D=8, row_class=64, target=64, S=19, k=5, lam=0.5, mu=0.25,
          gamma=0.5, similarity=0, normalize=1, out_idx=64, out_score=64, out_obj=64, out_cal=64, status=64):
    return [pool_idx, pool_score, table, B, N, V, D, row_class, target, S, k, lam, mu, gamma, similarity, normalize, out_idx,
            out_score, out_obj, out_cal, status, None]


NAN = float("nan")


@pytest.mark.parametrize("change,needle", [
    (dict(B=-1), "negative size"), (dict(V=-1), "negative size"), (dict(N=-1), "negative size"), (dict(S=-1), "negative size"),
    (dict(k=-1), "negative size"),
    (dict(N=0), "N in [1, 128]"), (dict(N=129), "N in [1, 128]"),
    (dict(k=0), "k in [1, N = 16]"), (dict(k=17), "k in [1, N = 16]"),
    (dict(S=0), "S in [1, 64]"), (dict(S=65), "S in [1, 64]"),
    (dict(V=2 ** 31), "table rows"), (dict(B=2 ** 31), "users per call"),
    (dict(lam=-0.01), "lambda in [0, 1]"), (dict(lam=1.01), "lambda in [0, 1]"), (dict(lam=NAN), "lambda in [0, 1]"),
    (dict(mu=-0.01), "mu in [0, 1]"), (dict(mu=1.01), "mu in [0, 1]"), (dict(mu=NAN), "mu in [0, 1]"),
    (dict(gamma=-0.01), "gamma in [0, 1]"), (dict(gamma=1.01), "gamma in [0, 1]"), (dict(gamma=NAN), "gamma in [0, 1]"),
    (dict(normalize=2), "normalize"), (dict(normalize=-1), "normalize"),
    (dict(D=0), "D a multiple of 4"), (dict(D=6), "D a multiple of 4"), (dict(D=1028), "D a multiple of 4"), (dict(D=-4), "D a multiple"),
    (dict(similarity=2), "similarity"), (dict(similarity=-1), "similarity"),
    (dict(status=None), "status"),
    (dict(pool_idx=None), "null argument"), (dict(pool_score=None), "null argument"), (dict(table=None), "null argument"),
    (dict(row_class=None), "null argument"), (dict(target=None), "null argument"), (dict(out_idx=None), "null argument"),
    (dict(out_score=None), "null argument"), (dict(out_obj=None), "null argument"), (dict(out_cal=None), "null argument"),
    (dict(mu=0.0, row_class=None), "null argument"), (dict(mu=0.0, out_cal=None), "null argument")])
def test_every_refusal(change, needle):
    lib = _native()
    assert lib.nrl_calibrated_rerank(*_args(**change)) == -1
    msg = lib.nrl_last_error().decode()
    assert needle in msg and msg.startswith("calibrated_rerank:"), msg


def test_the_order_of_the_checks():
    lib = _native()
    # each argument list breaks every later check as well: the message is that of the earliest one
    chain = [(dict(B=-1), "negative size"), (dict(N=200), "N in [1, 128]"), (dict(k=17), "k in [1, N"), (dict(S=65), "S in [1, 64]"),
             (dict(V=2 ** 31), "table rows"), (dict(lam=2.0), "lambda in"), (dict(mu=2.0), "mu in"), (dict(gamma=2.0), "gamma in"),
             (dict(normalize=3), "normalize"), (dict(status=None), "status")]
    for i, (_, needle) in enumerate(chain):
        broken = {}
        for change, _ in chain[i:]:
            broken.update(change)
        assert lib.nrl_calibrated_rerank(*_args(**broken)) == -1
        assert needle in lib.nrl_last_error().decode(), (needle, lib.nrl_last_error().decode())
    # D and similarity come behind normalize and before the status word, and only with mu != 0
    for broken, needle in ((dict(D=6, similarity=3, status=None), "D a multiple"), (dict(similarity=3, status=None), "similarity"),
                           (dict(normalize=3, D=6), "normalize")):
        assert lib.nrl_calibrated_rerank(*_args(**broken)) == -1 and needle in lib.nrl_last_error().decode()
    # B == 0 returns success without a launch once the checks pass (null pointers included), and refuses when they do not
    assert lib.nrl_calibrated_rerank(*_args(B=0, pool_idx=None, table=None, row_class=None, target=None, out_cal=None)) == 0
    assert lib.nrl_calibrated_rerank(*_args(B=0, gamma=2.0)) == -1
    assert lib.nrl_calibrated_rerank(*_args(B=0, status=None)) == -1


def test_with_mu_zero_neither_the_table_nor_d_nor_the_similarity_is_looked_at():
    lib = _native()
    # B == 0 keeps every accepted call off the device
    assert lib.nrl_calibrated_rerank(*_args(B=0, mu=0.0, D=6, similarity=7, table=None)) == 0
    assert lib.nrl_calibrated_rerank(*_args(B=0, mu=0.0, D=-3)) == 0
    assert lib.nrl_calibrated_rerank(*_args(B=0, mu=0.25, D=6)) == -1
    assert lib.nrl_calibrated_rerank(*_args(B=0, mu=0.25, similarity=7)) == -1
    # the other limits hold all the same
    assert lib.nrl_calibrated_rerank(*_args(B=0, mu=0.0, V=2 ** 31)) == -1 and "table rows" in lib.nrl_last_error().decode()
    assert lib.nrl_calibrated_rerank(*_args(B=0, mu=0.0, S=65)) == -1


def test_python_side_refusals():
    from newsreclib_amd import ops
    from newsreclib_amd.evaluation import NewsVectorCache, NpaFeatureCache, recommend_users
    idx, score, table = torch.zeros(2, 8, dtype=torch.int64), torch.zeros(2, 8), torch.zeros(9, 4)
    cls, tgt = torch.zeros(9, dtype=torch.int32), torch.zeros(2, 3)
    call = ops.calibrated_rerank
    for bad in (lambda: call(idx.int(), score, table, cls, tgt, 3, 0.5, 0.5, 0.5), lambda: call(idx, score.double(), table, cls, tgt, 3, 0.5, 0.5, 0.5),
                lambda: call(idx, score, table.half(), cls, tgt, 3, 0.5, 0.5, 0.5), lambda: call(idx, score, table, cls.float(), tgt, 3, 0.5, 0.5, 0.5),
                lambda: call(idx, score, table, None, tgt, 3, 0.5, 0.5, 0.5), lambda: call(idx, score, table, cls, tgt.double(), 3, 0.5, 0.5, 0.5),
                lambda: call(idx, score[:, :7], table, cls, tgt, 3, 0.5, 0.5, 0.5), lambda: call(idx[0], score[0], table, cls, tgt, 3, 0.5, 0.5, 0.5),
                lambda: call(idx, score, table[0], cls, tgt, 3, 0.5, 0.5, 0.5), lambda: call(idx, score, table, cls[:8], tgt, 3, 0.5, 0.5, 0.5),
                lambda: call(idx, score, table, cls, tgt[:1], 3, 0.5, 0.5, 0.5), lambda: call(idx, score, table, cls, tgt[0], 3, 0.5, 0.5, 0.5),
                lambda: call(idx, score, table, cls, tgt[:, :0], 3, 0.5, 0.5, 0.5),
                lambda: call(idx, score, table, cls, tgt, 0, 0.5, 0.5, 0.5), lambda: call(idx, score, table, cls, tgt, 9, 0.5, 0.5, 0.5),
                lambda: call(idx, score, table, cls, tgt, 3, 1.5, 0.5, 0.5), lambda: call(idx, score, table, cls, tgt, 3, 0.5, -0.5, 0.5),
                lambda: call(idx, score, table, cls, tgt, 3, 0.5, 0.5, float("nan")),
                lambda: call(idx, score, table, cls, tgt, 3, 0.5, 0.5, 0.5, similarity="jaccard"),
                lambda: call(idx, score, None, cls, tgt, 3, 0.5, 0.5, 0.5)):         # mu != 0 without a table
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(NotImplementedError, match="at most 128"):
        call(torch.zeros(2, 129, dtype=torch.int64), torch.zeros(2, 129), table, cls, tgt, 3, 0.5, 0.5, 0.5)
    with pytest.raises(NotImplementedError, match="at most 64 classes"):
        call(idx, score, table, cls, torch.zeros(2, 65), 3, 0.5, 0.5, 0.5)
    for t in (table, None):                                  # with and without a table: the device is required
        with pytest.raises(RuntimeError, match="no CPU path"):
            call(idx, score, t, cls, tgt, 3, 0.5, 0.0, 0.5)
    # NPA: served with mu == 0 only
    with pytest.raises(ValueError, match="mu == 0 only"):
        NpaFeatureCache.rerank_calibrated(SimpleNamespace(), idx, score, 3, "category", tgt, 0.5, 0.25, 0.5)
    npa = SimpleNamespace(module=SimpleNamespace(personalized_pooling_scorer=True), table=None,
                          rerank_calibrated=lambda *a, **kw: NpaFeatureCache.rerank_calibrated(None, *a, **kw))
    with pytest.raises(ValueError, match="mu == 0 only"):
        recommend_users(npa, [{"hist": torch.tensor([1])}], 5, calibrate=dict(pool=8, aspect="category", gamma=0.5, mu=0.5))
    # recommend_users: calibrate and diversify exclude each other; the dictionary is checked before anything is touched
    cache = NewsVectorCache(SimpleNamespace(), None)
    with pytest.raises(ValueError, match="exclude each other"):
        recommend_users(cache, [], 5, diversify=(8, 0.5), calibrate=dict(pool=8, aspect="category", gamma=0.5))
    with pytest.raises(ValueError, match="at least k"):
        recommend_users(cache, [], 10, calibrate=dict(pool=5, aspect="category", gamma=0.5))
    with pytest.raises(ValueError, match="proportional"):
        recommend_users(cache, [], 5, calibrate=dict(pool=8, aspect="category", gamma=0.5, target="uniform"))
    for bad in (dict(pool=8, gamma=0.5), dict(pool=8, aspect="category"), dict(pool=8, aspect="category", gamma=0.5, lamda=1.0)):
        with pytest.raises(ValueError, match="calibrate=dict"):
            recommend_users(cache, [], 5, calibrate=bad)


# ---- hand-worked cases ------------------------------------------------------------------------------------------------------------------
def _hand(gamma, target=(2, 0), classes=(1, 1, 0, 0), scores=(1.0, 0.75, 0.5, 0.25), k=4, S=2):
    # four slots, rows 0 ... 3 with the classes given, lambda = 1, raw scores, mu = 0
    return R.cal_f32(np.arange(4), np.array(scores, dtype=F), None, 4, np.array(classes), np.array(target, dtype=F), k, 1.0, 0.0,
                     gamma, "cosine", False)


def test_hand_worked_the_choice_flips_with_gamma():
    # S = 2, target (2, 0): the user read class 0 twice; slots 0, 1 are of class 1, slots 2, 3 of class 0.
    # step 0: n = (0, 0).  cal_0 = min(1, 2) / max(1, 2) = 1/2;  cal_1 = (min(0, 2) + min(1, 0)) / (max(0, 2) + max(1, 0)) = 0/3
    #   gamma = 0:    obj = 1, .75, .5, .25                       -> slot 0
    #   gamma = 1:    obj = 1 + 0, .75 + 0, .5 + .5, .25 + .5     -> slot 0 again: 1 == 1 is a tie and the lower slot wins
    idx, score, obj, cal, flags, steps = _hand(0.0)
    assert [s[0] for s in steps] == [0, 1, 2, 3] and flags == 0 and obj.tolist() == [1.0, 0.75, 0.5, 0.25]
    idx, score, obj, cal, flags, steps = _hand(1.0)
    # step 1: n = (0, 1).  cal_0 = (min(1, 2) + min(1, 0)) / (2 + 1) = 1/3;  cal_1 = (0 + 0) / (2 + 2) = 0
    #   obj = -, .75, .5 + 1/3, .25 + 1/3 -> slot 2 (0.8333 > 0.75): the choice has flipped
    # step 2: n = (1, 1).  cal_0 = (2 + 0) / (2 + 1) = 2/3;  cal_1 = (1 + 0) / (2 + 2) = 1/4
    #   obj = -, .75 + .25, -, .25 + 2/3 -> slot 1 (1.0 > 0.9167)
    # step 3: n = (1, 2): slot 3 is left; cal_0 = (2 + 0) / (2 + 2) = 1/2
    assert [s[0] for s in steps] == [0, 2, 1, 3] and flags == 0
    third = F(1) / F(3)
    assert obj.tolist() == [1.0, float(F(0.5) + third), 1.0, 0.75]
    assert cal.tolist() == [0.0, float(third), 0.25, 0.5] and score.tolist() == [1.0, 0.5, 0.75, 0.25]
    # between the two: at gamma = 1/2 step 1 gives slot 1 .75 against slot 2 .5 + 1/6: no flip yet
    assert [s[0] for s in _hand(0.5)[5]][:2] == [0, 1]
    # the last term is the finished list's overlap with the target: counts (2, 2) against (2, 0): 2 / 4
    assert cal[3] == R.count_formula([1, 0, 1, 0], np.array([2, 0], dtype=F)) == 0.5


def test_hand_worked_an_all_zero_target_gives_zero_everywhere():
    idx, score, obj, cal, flags, steps = _hand(1.0, target=(0, 0))
    assert [s[0] for s in steps] == [0, 1, 2, 3] and flags == 0 and cal.tolist() == [0.0] * 4 and obj.tolist() == score.tolist()
    assert not np.signbit(cal).any()


def test_hand_worked_a_class_out_of_range_is_live_with_term_zero():
    for bad in (2, -1, 64, -7):
        idx, score, obj, cal, flags, steps = _hand(1.0, classes=(bad, 1, 0, 0))
        # slot 0 still wins step 0 on its score, with term +0, and counts for no class: step 1 sees n = (0, 0) again
        assert flags == R.E_CLASS and steps[0][0] == 0 and cal[0] == 0.0 and obj[0] == 1.0
        assert steps[1][0] == 2 and cal[1] == 0.5 and obj[1] == 1.0          # .5 + 1/2 against slot 1's .75 + 0
        assert sorted(idx.tolist()) == [0, 1, 2, 3]
    # a dead slot's class is never looked at
    out = R.cal_f32(np.array([0, -1, 9, 3]), np.array([1, 1, 1, np.nan], dtype=F), None, 4, np.array([0, 5, 5, 5]),
                    np.array([1, 1], dtype=F), 4, 1.0, 0.0, 1.0, "cosine", False)
    assert out[4] == (R.E_ROW | R.E_NAN) and out[0].tolist() == [0, -1, -1, -1] and np.isneginf(out[3][1:]).all()


@pytest.mark.parametrize("bad", [-1.0, np.nan, np.inf, -np.inf])
def test_hand_worked_a_bad_target_entry_is_zero_and_flagged(bad):
    got = _hand(1.0, target=(bad, 1))
    want = _hand(1.0, target=(0, 1))
    assert got[4] == R.E_TARGET and want[4] == 0
    assert all(np.array_equal(a, b) for a, b in zip(got[:4], want[:4]))
    both = R.cal_f64(np.arange(4), np.array([1.0, 0.75, 0.5, 0.25], dtype=F), None, 4, np.array([1, 1, 0, 0]), np.array([bad, 1]), 4,
                     1.0, 0.0, 1.0, "cosine", False)
    assert both[4] == R.E_TARGET and np.array_equal(both[0], want[0])
    # -0 is a zero like any other
    assert _hand(1.0, target=(-0.0, 1))[4] == 0


# ---- the restatements' own properties ---------------------------------------------------------------------------------------------------
def _case(rng, V=40):
    """``test_mmr_host``'s pools (ties, a zero row, duplicates, bad rows and scores) with classes and a target beside them"""
    N, D = int(rng.choice([1, 2, 5, 9, 16])), int(rng.choice([4, 8]))
    spread = int(rng.choice([1, 3, 16]))
    table = rng.integers(-spread, spread + 1, (V, D)) / 8.0
    table[0] = 0.0
    idx = rng.integers(0, V, N)
    if N > 2 and rng.random() < 0.5:
        idx[1] = idx[0]
    for bad in (-1, -1, -2, V):
        if rng.random() < 0.25:
            idx[int(rng.integers(0, N))] = bad
    score = (rng.integers(-spread, spread + 1, N) / 8.0).astype(F)
    for bad in (np.nan, np.inf, -np.inf):
        if rng.random() < 0.15:
            score[int(rng.integers(0, N))] = bad
    k = int(rng.choice([1, max(1, N // 2), N]))
    S = int(rng.choice([1, 2, 5, 19]))
    row_class = rng.integers(0, S, V)
    if rng.random() < 0.3:
        row_class[rng.integers(0, V, 4)] = rng.choice([-1, S, 99])
    target = rng.integers(0, 4, S).astype(F)
    if rng.random() < 0.2:
        target[int(rng.integers(0, S))] = rng.choice([-1.0, np.nan, np.inf])
    return idx, score, table, k, row_class, target


def _same(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), equal_nan=True)


def _live(idx, score, V):
    return np.isfinite(score) & (idx >= 0) & (idx < V)


def test_f32_equals_f64_where_the_arithmetic_is_exact():
    # gamma = 0 on dot similarity, raw scores and weights on the quarter grid: every operation is exact in float32, so the two
    # restatements agree in everything.  (The calibration term is a quotient and rounds, so it is compared through the choices
    # at gamma > 0 only where it is exact: targets that make every quotient a dyadic number are rare; it has its own test below.)
    rng = np.random.default_rng(60)
    for _ in range(600):
        idx, score, table, k, row_class, target = _case(rng)
        lam, mu = float(rng.choice([0.0, 0.25, 0.5, 1.0])), float(rng.choice([0.0, 0.25, 0.5, 1.0]))
        V = table.shape[0]
        a = R.cal_f32(idx, score, M.gram_f32(idx, table), V, row_class, target, k, lam, mu, 0.0, "dot", False)
        b = R.cal_f64(idx, score, table, V, row_class, target, k, lam, mu, 0.0, "dot", False)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and _same(a[2], b[2]) and a[4] == b[4], (idx, score, k, lam, mu)
        assert [s[0] for s in a[5]] == [s[0] for s in b[5]]
        assert np.allclose(a[3], b[3], rtol=2.0 ** -22, atol=0)                # the terms themselves: one rounding per addition
        live = _live(idx, score, V)
        want = 0
        if ((idx != -1) & ((idx < 0) | (idx >= V))).any():
            want |= R.E_ROW
        if (~np.isfinite(score) & (idx >= 0) & (idx < V)).any():
            want |= R.E_NAN
        cls = row_class[np.where(live, idx, 0)]
        if (live & ((cls < 0) | (cls >= len(target)))).any():
            want |= R.E_CLASS
        if not (np.isfinite(target) & (target >= 0)).all():
            want |= R.E_TARGET
        assert a[4] == want
        n = min(k, int(live.sum()))
        assert int((a[0] >= 0).sum()) == n and all(np.isneginf(a[j][n:]).all() for j in (1, 2, 3)) and np.all(a[0][n:] == -1)


def test_the_term_is_exact_in_both_where_the_quotient_is_dyadic():
    # S = 2, target (1, 1), two slots of different classes: cal = 1/2 then 2/2, exact in both arithmetics, gamma on the grid
    for gamma in (0.25, 0.5, 1.0):
        a = R.cal_f32([0, 1], [0.5, 0.25], None, 2, [0, 1], [1, 1], 2, 0.5, 0.0, gamma, "dot", False)
        b = R.cal_f64([0, 1], [0.5, 0.25], None, 2, [0, 1], [1, 1], 2, 0.5, 0.0, gamma, "dot", False)
        assert a[3].tolist() == [0.5, 1.0] == b[3].tolist() and _same(a[2], b[2]) and a[2].tolist() == [0.25 + gamma / 2, 0.125 + gamma]


def test_f32_is_greedy_in_f64():
    rng = np.random.default_rng(61)
    for _ in range(300):
        idx, score, table, k, row_class, target = _case(rng)
        score = np.where(np.isfinite(score), score, 0).astype(F)
        lam, mu, gamma = (float(rng.choice([0.0, 0.3, 0.5, 1.0])) for _ in range(3))
        sim, norm = str(rng.choice(["cosine", "dot"])), bool(rng.integers(0, 2))
        V, D = table.shape
        tol = (D + 16) * 2.0 ** -23 * (2 + D * 4 + 1)        # as test_mmr_host: |rel| <= 2, |sim| <= D * 2 * 2; and cal <= 1
        a = R.cal_f32(idx, score, M.gram_f32(idx, table), V, row_class, target, k, lam, mu, gamma, sim, norm)
        slots = [s[0] for s in a[5] if s[0] >= 0]
        b = R.cal_f64(idx, score, table, V, row_class, target, k, lam, mu, gamma, sim, norm, forced=slots)
        for t, (c, obj) in enumerate(b[5]):
            if c < 0:
                break
            assert obj[c] >= np.nanmax(obj) - tol and abs(float(a[2][t]) - obj[c]) <= tol and abs(float(a[3][t]) - b[3][t]) <= tol


@pytest.mark.parametrize("which", ["f32", "f64"])
def test_the_five_header_properties(which):
    rng = np.random.default_rng(62)
    seen_full = 0
    for _ in range(300):
        idx, score, table, _, row_class, target = _case(rng)
        N, V, S = len(idx), table.shape[0], len(target)
        lam, mu, gamma = (float(rng.choice([0.0, 0.3, 0.5, 1.0])) for _ in range(3))
        sim, norm = str(rng.choice(["cosine", "dot"])), bool(rng.integers(0, 2))
        if which == "f32":
            G = M.gram_f32(idx, table)
            run = lambda k, lam, mu, gamma, sim, norm: R.cal_f32(idx, score, G, V, row_class, target, k, lam, mu, gamma, sim, norm)  # noqa: E731
            mmr = lambda k, lam: M.mmr_f32(idx, score, G, V, k, lam, sim, norm)  # noqa: E731
            dtype = F
        else:
            run = lambda k, lam, mu, gamma, sim, norm: R.cal_f64(idx, score, table, V, row_class, target, k, lam, mu, gamma, sim, norm)  # noqa: E731
            mmr = lambda k, lam: M.mmr_f64(idx, score, table, k, lam, sim, norm)  # noqa: E731
            dtype = np.float64
        # 1. the result for k is a prefix of the result for k' > k
        full = run(N, lam, mu, gamma, sim, norm)
        for k in {1, max(1, N // 2)}:
            part = run(k, lam, mu, gamma, sim, norm)
            assert all(_same(p, f[:k]) for p, f in zip(part[:4], full[:4]))
        # 2. nothing but the user's own pool enters: the restatements take one user by construction
        # 3. gamma = 0, mu = fl(1 - lambda): nrl_mmr_rerank (lambda < 1 here: at lambda = 1 the mu == 0 form has no Gram matrix)
        # (mmr_f64 takes 1 - lambda in real arithmetic: the float64 comparison keeps to lambdas whose fl(1 - lambda) is exact)
        for l3 in ((0.0, 0.3, 0.5) if which == "f32" else (0.0, 0.25, 0.5)):
            one_minus = float(F(1) - F(l3))
            got, want = run(N, l3, one_minus, 0.0, sim, norm), mmr(N, l3)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
            assert np.array_equal(np.asarray(got[2], dtype=np.float64), np.asarray(want[2], dtype=np.float64), equal_nan=True)
            assert (got[4] & ~(R.E_CLASS | R.E_TARGET)) == want[3]
        # 4. gamma = 0, mu = 0, lambda = 1, normalize = 0: the pool in (score descending, slot ascending) order
        four = run(N, 1.0, 0.0, 0.0, sim, False)
        live = _live(idx, score, V)
        order = sorted(np.nonzero(live)[0], key=lambda i: (-float(score[i]), i))
        assert [s[0] for s in four[5] if s[0] >= 0] == order
        assert np.array_equal(four[1][:len(order)], score[order]) and _same(four[2][:len(order)], score[order])
        # 5. a full list without a flag: the last term is the count formula over the list's classes
        for k in {1, max(1, N // 2), N}:
            five = run(k, lam, mu, gamma, sim, norm)
            if five[4] == 0 and five[0][k - 1] >= 0:
                seen_full += 1
                assert five[3][k - 1] == R.count_formula(row_class[five[0]], target.astype(dtype), dtype)
    assert seen_full > 30


def test_property_five_is_personalization_at_k():
    # with the integer class counts of a history as the target, the last term is aspect_metrics' personalization@k of the list
    from newsreclib_amd.metrics import aspect_metrics
    rng = np.random.default_rng(63)
    V, N, S, k = 60, 24, 6, 10
    row_class = rng.integers(0, S, V)
    row_class[:3] = [1, 2, 3]
    for _ in range(20):
        idx = rng.permutation(V)[:N]
        score = rng.standard_normal(N).astype(F)
        hist = rng.integers(0, V, int(rng.integers(1, 30)))
        target = np.bincount(row_class[hist], minlength=S).astype(F)
        out = R.cal_f32(idx, score, None, V, row_class, target, k, 0.5, 0.0, 0.5)
        assert out[4] == 0 and row_class[out[0]].sum() > 0
        got = aspect_metrics(torch.from_numpy(out[1]), torch.from_numpy(row_class[out[0]]), torch.from_numpy(row_class[hist]),
                             torch.tensor([k]), torch.tensor([len(hist)]), S, (k,))[f"categ_pers@{k}"]
        assert abs(got - float(out[3][k - 1])) <= 2.0 ** -22


def test_class_targets_against_numpy_bincount():
    from newsreclib_amd import ops
    rng = np.random.default_rng(64)
    V, S, B = 50, 7, 9
    row_class = rng.integers(0, S, V)
    row_class[5], row_class[6] = -1, S                       # classes outside [0, S) count for nothing
    sizes = np.array([0, 1, 5, 12, 0, 3, 30, 2, 1])
    hist = rng.integers(0, V, int(sizes.sum()))
    hist[3], hist[7] = 5, 6
    hist[10], hist[11] = -1, V                               # and so do rows outside the table
    off = np.concatenate([[0], np.cumsum(sizes)])
    want = np.zeros((B, S), dtype=np.float32)
    for u in range(B):
        rows = hist[off[u]:off[u + 1]]
        rows = rows[(rows >= 0) & (rows < V)]
        cls = row_class[rows]
        want[u] = np.bincount(cls[(cls >= 0) & (cls < S)], minlength=S)
    for rc in (torch.from_numpy(row_class), torch.from_numpy(row_class).int()):
        got = ops.class_targets(torch.from_numpy(hist), torch.from_numpy(off), rc, S)
        assert got.dtype == torch.float32 and got.shape == (B, S) and np.array_equal(got.numpy(), want)
    quota = ops.class_targets(torch.from_numpy(hist), torch.from_numpy(off), torch.from_numpy(row_class), S, k=10)
    assert np.array_equal(quota.numpy(), (want * np.float32(10.0)) / np.maximum(sizes, 1).astype(np.float32)[:, None])
    assert float(quota[6].sum()) <= 10.0 + 1e-5 and quota[0].tolist() == [0.0] * S
    empty = ops.class_targets(torch.zeros(0, dtype=torch.int64), torch.zeros(1, dtype=torch.int64), torch.from_numpy(row_class), S)
    assert empty.shape == (0, S)
