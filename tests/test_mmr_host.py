"""CPU tier of the greedy MMR re-ranking (``nrl_mmr_rerank``): the ABI (header against ``_lib.SIGNATURES`` and the library), the
limits and the flags, every native refusal and their order through ctypes without a device, the Python-side refusals, the
properties of the two restatements (``tests/mmr_ref.py``) the GPU tests compare against, and ``metrics.intra_list_similarity``."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import mmr_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, "include", "newsreclib_amd.h")).read()


def test_the_entry_is_in_the_header_in_the_signatures_and_in_the_library():
    from newsreclib_amd import _lib
    header = _header()
    m = re.search(r"\bint nrl_mmr_rerank\(([^;]*)\);", header)
    assert m, "nrl_mmr_rerank is not declared in the header"
    args = [a.strip().split()[-1].lstrip("*") for a in m.group(1).split(",")]
    assert args == ["pool_idx", "pool_score", "table", "B", "N", "V", "D", "k", "lambda", "similarity", "normalize", "out_idx",
                    "out_score", "out_mmr", "status", "stream"]
    assert len(_lib.SIGNATURES["nrl_mmr_rerank"][1]) == len(args)
    import ctypes
    assert _lib.SIGNATURES["nrl_mmr_rerank"][1][8] is ctypes.c_float
    assert _lib.ABI_VERSION == 19 and re.search(r"#define NRL_ABI_VERSION 19\b", header)
    assert hasattr(_native(), "nrl_mmr_rerank")


def test_limits_and_flags():
    from newsreclib_amd import ops
    header = _header()
    assert re.search(r"#define NRL_MMR_MAX_POOL 128\b", header) and ops.MMR_MAX_POOL == 128
    assert re.search(r"#define NRL_MMR_E_ROW 1\b", header) and R.E_ROW == 1 and R.E_NAN == 4
    assert set(ops.MMR_FLAGS) == {1, 4} and "outside [0, V)" in ops.MMR_FLAGS[1] and "non-finite" in ops.MMR_FLAGS[4]
    # a dictionary of its own: the pinned key sets are untouched
    assert set(ops.TOPK_FLAGS) == {1, 2, 4, 8} and set(ops.RANK_FLAGS) == {1, 2, 4, 16, 32}
    assert ops.MMR_FLAGS[1] != ops.TOPK_FLAGS[1]


# ---- the native entry refuses bad arguments before it launches anything (no device is touched: the pointers are never read) ---------
def _native():
    from newsreclib_amd import _build, _lib
    _build.build(verbose=False)
    return _lib.load()


def _args(pool_idx=64, pool_score=64, table=64, B=4, N=16, V=100, D=8, k=5, lam=0.5, similarity=0, normalize=1, out_idx=64,
          out_score=64, out_mmr=64, status=64):
    return [pool_idx, pool_score, table, B, N, V, D, k, lam, similarity, normalize, out_idx, out_score, out_mmr, status, None]


@pytest.mark.parametrize("change,needle", [
    (dict(B=-1), "negative size"), (dict(V=-1), "negative size"), (dict(D=-4), "negative size"), (dict(N=-1), "negative size"),
    (dict(k=-1), "negative size"),
    (dict(N=0), "N in [1, 128]"), (dict(N=129, k=5), "N in [1, 128]"),
    (dict(k=0), "k in [1, N = 16]"), (dict(k=17), "k in [1, N = 16]"),
    (dict(D=0), "D a multiple of 4"), (dict(D=6), "D a multiple of 4"), (dict(D=1028), "D a multiple of 4"),
    (dict(V=2 ** 31), "table rows"), (dict(B=2 ** 31), "users per call"),
    (dict(lam=-0.01), "lambda in [0, 1]"), (dict(lam=1.01), "lambda in [0, 1]"), (dict(lam=float("nan")), "lambda in [0, 1]"),
    (dict(similarity=2), "similarity"), (dict(similarity=-1), "similarity"), (dict(normalize=2), "normalize"),
    (dict(status=None), "status"),
    (dict(pool_idx=None), "null argument"), (dict(pool_score=None), "null argument"), (dict(table=None), "null argument"),
    (dict(out_idx=None), "null argument"), (dict(out_score=None), "null argument"), (dict(out_mmr=None), "null argument")])
def test_every_refusal(change, needle):
    lib = _native()
    assert lib.nrl_mmr_rerank(*_args(**change)) == -1
    msg = lib.nrl_last_error().decode()
    assert needle in msg and msg.startswith("mmr_rerank:"), msg


def test_the_order_of_the_checks():
    lib = _native()
    # each argument list breaks every later check as well: the message is that of the earliest one
    later = dict(status=None)
    chain = [(dict(B=-1), "negative size"), (dict(N=200), "N in [1, 128]"), (dict(k=17), "k in [1, N"), (dict(D=6), "D a multiple"),
             (dict(lam=2.0), "lambda in"), (dict(similarity=3), "similarity"), (dict(status=None), "status")]
    for i, (_, needle) in enumerate(chain):
        broken = {}
        for change, _ in chain[i:]:
            broken.update(change)
        broken.update(later)
        assert lib.nrl_mmr_rerank(*_args(**broken)) == -1
        assert needle in lib.nrl_last_error().decode(), (needle, lib.nrl_last_error().decode())
    # B == 0 returns success without a launch once the checks pass (null pointers included), and refuses when they do not
    assert lib.nrl_mmr_rerank(*_args(B=0, pool_idx=None, table=None, out_mmr=None)) == 0
    assert lib.nrl_mmr_rerank(*_args(B=0, lam=2.0)) == -1
    assert lib.nrl_mmr_rerank(*_args(B=0, status=None)) == -1
    # table may be null only when V == 0: with V == 0 the null-pointer check passes (B == 0 keeps the call off the device)
    assert lib.nrl_mmr_rerank(*_args(table=None)) == -1 and "null argument" in lib.nrl_last_error().decode()


def test_python_side_refusals():
    from newsreclib_amd import ops
    from newsreclib_amd.evaluation import NewsVectorCache, NpaFeatureCache, recommend_users
    idx, score, table = torch.zeros(2, 8, dtype=torch.int64), torch.zeros(2, 8), torch.zeros(9, 4)
    for call in (lambda: ops.mmr_rerank(idx.int(), score, table, 3, 0.5), lambda: ops.mmr_rerank(idx, score.double(), table, 3, 0.5),
                 lambda: ops.mmr_rerank(idx, score, table.half(), 3, 0.5), lambda: ops.mmr_rerank(idx, score[:, :7], table, 3, 0.5),
                 lambda: ops.mmr_rerank(idx[0], score[0], table, 3, 0.5), lambda: ops.mmr_rerank(idx, score, table[0], 3, 0.5),
                 lambda: ops.mmr_rerank(idx, score, table, 0, 0.5), lambda: ops.mmr_rerank(idx, score, table, 9, 0.5),
                 lambda: ops.mmr_rerank(idx, score, table, 3, 1.5), lambda: ops.mmr_rerank(idx, score, table, 3, float("nan")),
                 lambda: ops.mmr_rerank(idx, score, table, 3, 0.5, similarity="jaccard")):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(NotImplementedError, match="at most 128"):
        ops.mmr_rerank(torch.zeros(1, 129, dtype=torch.int64), torch.zeros(1, 129), table, 3, 0.5)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.mmr_rerank(idx, score, table, 3, 0.5)
    # NPA: refused, and the reason is the user-dependence of its news vectors
    with pytest.raises(NotImplementedError, match="depends on the user"):
        NpaFeatureCache.rerank_diverse(SimpleNamespace(), idx, score, 3, 0.5)
    npa = SimpleNamespace(module=SimpleNamespace(personalized_pooling_scorer=True), table=None,
                          rerank_diverse=lambda *a, **kw: NpaFeatureCache.rerank_diverse(None, *a, **kw))
    with pytest.raises(NotImplementedError, match="depends on the user"):
        recommend_users(npa, [{"hist": torch.tensor([1])}], 5, diversify=(8, 0.5))
    # recommend_users: a pool smaller than k is refused before anything is touched
    with pytest.raises(ValueError, match="at least k"):
        recommend_users(NewsVectorCache(SimpleNamespace(), None), [], 10, diversify=(5, 0.5))


# ---- the restatements' own properties ---------------------------------------------------------------------------------------------------
def _case(rng, V=40):
    N, D = int(rng.choice([1, 2, 5, 9, 16])), int(rng.choice([4, 8]))
    spread = int(rng.choice([1, 3, 16]))                # few distinct values: ties everywhere
    table = rng.integers(-spread, spread + 1, (V, D)) / 8.0
    table[0] = 0.0                                      # a zero row
    idx = rng.integers(0, V, N)
    if N > 2 and rng.random() < 0.5:
        idx[1] = idx[0]                                 # a duplicated row
    for bad in (-1, -1, -2, V):
        if rng.random() < 0.25:
            idx[int(rng.integers(0, N))] = bad
    score = (rng.integers(-spread, spread + 1, N) / 8.0).astype(np.float32)
    for bad in (np.nan, np.inf, -np.inf):
        if rng.random() < 0.15:
            score[int(rng.integers(0, N))] = bad
    k = int(rng.choice([1, max(1, N // 2), N]))
    return idx, score, table, k


def _same(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), equal_nan=True)


def test_f32_equals_f64_where_the_arithmetic_is_exact():
    # dot similarity, raw scores and lambda on the quarter grid: every product and difference is exact in float32, so the two
    # restatements must agree in everything, the objectives included
    rng = np.random.default_rng(50)
    for _ in range(1000):
        idx, score, table, k = _case(rng)
        lam = float(rng.choice([0.0, 0.25, 0.5, 0.75, 1.0]))
        a = R.mmr_f32(idx, score, R.gram_f32(idx, table), table.shape[0], k, lam, "dot", False)
        b = R.mmr_f64(idx, score, table, k, lam, "dot", False)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and _same(a[2], b[2]) and a[3] == b[3], (idx, score, k, lam)
        assert [s[0] for s in a[4]] == [s[0] for s in b[4]]
        want = 0
        if ((idx != -1) & ((idx < 0) | (idx >= table.shape[0]))).any():
            want |= R.E_ROW
        if (~np.isfinite(score) & (idx >= 0) & (idx < table.shape[0])).any():
            want |= R.E_NAN
        assert a[3] == want
        live = np.isfinite(score) & (idx >= 0) & (idx < table.shape[0])
        assert int((a[0] >= 0).sum()) == min(k, int(live.sum()))
        assert np.all(a[0][int((a[0] >= 0).sum()):] == -1) and np.all(np.isneginf(a[1][a[0] < 0])) and np.all(np.isneginf(a[2][a[0] < 0]))


def test_f32_is_greedy_in_f64_under_cosine_and_normalisation():
    # where the float32 roundings are real, the float32 choice is still a maximiser of the float64 objective up to those roundings
    rng = np.random.default_rng(51)
    tol = (8 + 16) * 2.0 ** -23 * (2 + 8 * 4)            # D + 16 roundings of 2^-24 relative; |rel| <= 2, |sim| <= D * 2 * 2
    for _ in range(300):
        idx, score, table, k = _case(rng)
        score = np.where(np.isfinite(score), score, 0).astype(np.float32)
        lam = float(rng.choice([0.0, 0.3, 0.5, 0.7, 1.0]))
        sim, norm = str(rng.choice(["cosine", "dot"])), bool(rng.integers(0, 2))
        a = R.mmr_f32(idx, score, R.gram_f32(idx, table), table.shape[0], k, lam, sim, norm)
        slots = [s[0] for s in a[4] if s[0] >= 0]
        b = R.mmr_f64(idx, score, table, k, lam, sim, norm, forced=slots)
        for t, (c, obj) in enumerate(b[4]):
            if c < 0:
                break
            assert obj[c] >= np.nanmax(obj) - tol and abs(float(a[2][t]) - obj[c]) <= tol


@pytest.mark.parametrize("which", ["f32", "f64"])
def test_prefix_property_and_lambda_one(which):
    rng = np.random.default_rng(52)
    for _ in range(300):
        idx, score, table, _ = _case(rng)
        N, V = len(idx), table.shape[0]
        lam = float(rng.choice([0.0, 0.3, 0.5, 1.0]))
        sim, norm = str(rng.choice(["cosine", "dot"])), bool(rng.integers(0, 2))
        run = (lambda k, lam, sim, norm: R.mmr_f32(idx, score, R.gram_f32(idx, table), V, k, lam, sim, norm)) if which == "f32" else \
            (lambda k, lam, sim, norm: R.mmr_f64(idx, score, table, k, lam, sim, norm))
        full = run(N, lam, sim, norm)
        for k in {1, max(1, N // 2)}:
            part = run(k, lam, sim, norm)
            assert np.array_equal(part[0], full[0][:k]) and np.array_equal(part[1], full[1][:k]) and _same(part[2], full[2][:k])
        # lambda = 1 without normalisation: the live slots by (score descending, slot ascending)
        one = run(N, 1.0, sim, False)
        live = np.isfinite(score) & (idx >= 0) & (idx < V)
        order = sorted(np.nonzero(live)[0], key=lambda i: (-float(score[i]), i))
        assert [s[0] for s in one[4] if s[0] >= 0] == order
        assert np.array_equal(one[1][:len(order)], score[order]) and _same(one[2][:len(order)], score[order])


def test_a_nan_objective_ranks_below_every_number():
    obj = np.array([np.nan, -np.inf, np.nan, 1.0])
    assert R._pick(obj, np.array([True, True, True, False])) == 1
    assert R._pick(obj, np.array([True, False, True, False])) == 0
    assert R._pick(obj, np.array([False, False, False, False])) == -1
    assert R._pick(np.array([-0.0, 0.0, 0.0]), np.array([True, True, True])) == 0


def test_intra_list_similarity_against_numpy():
    from newsreclib_amd.metrics import intra_list_similarity
    rng = np.random.default_rng(53)
    table = rng.standard_normal((30, 12)).astype(np.float32)
    table[3] = 0.0
    idx = rng.integers(0, 30, (7, 6))
    idx[0, 4:] = -1
    idx[1, 1:] = -1                                     # one valid slot: the user does not count
    idx[2, :] = -1                                      # none
    idx[4, 0] = 3                                       # a zero vector: cosine 0 with everything
    idx[5, 1] = idx[5, 0]                               # a duplicate: cosine 1
    per_user = []
    for row in idx:
        rows = [r for r in row if r >= 0]
        if len(rows) < 2:
            continue
        vec = table[rows].astype(np.float64)
        nrm = np.linalg.norm(vec, axis=1, keepdims=True)
        unit = np.divide(vec, nrm, out=np.zeros_like(vec), where=nrm > 0)
        g = unit @ unit.T
        per_user.append((g.sum() - np.trace(g)) / (len(rows) * (len(rows) - 1)))
    got = intra_list_similarity(torch.from_numpy(idx), torch.from_numpy(table))
    assert abs(got - float(np.mean(per_user))) < 1e-6
    assert intra_list_similarity(torch.full((2, 3), -1), torch.from_numpy(table)) == 0.0
