"""CPU tier of the greedy DPP re-ranking (``nrl_dpp_rerank``): the ABI (header against ``_lib.SIGNATURES`` and the library), the
limits and the flags, every native refusal and their order through ctypes without a device, the Python-side refusals of
``ops.dpp_rerank`` and ``recommend_users(dpp=...)``, and the properties of the two restatements (``tests/dpp_ref.py``) the GPU
tests compare against: the float32 recurrence against the float64 definition, and hand-worked pools."""
import ctypes
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import dpp_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def _header():
    return open(os.path.join(ROOT, "include", "newsreclib_amd.h")).read()


def _native():
    from newsreclib_amd import _build, _lib
    _build.build(verbose=False)
    return _lib.load()


def test_the_entry_is_in_the_header_in_the_signatures_and_in_the_library():
    from newsreclib_amd import _lib
    header = _header()
    m = re.search(r"\bint nrl_dpp_rerank\(([^;]*)\);", header)
    assert m, "nrl_dpp_rerank is not declared in the header"
    decl = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    args = [a.strip().split()[-1].lstrip("*") for a in decl.split(",")]
    assert args == ["pool_idx", "pool_score", "quality", "table", "B", "N", "V", "D", "k", "alpha", "eps", "similarity", "normalize",
                    "out_idx", "out_score", "out_gain", "status", "stream"]
    sig = _lib.SIGNATURES["nrl_dpp_rerank"][1]
    assert len(sig) == len(args) and sig[9] is ctypes.c_float and sig[10] is ctypes.c_float and sig[8] is ctypes.c_int32
    assert sig[4] is ctypes.c_int64 and sig[5] is ctypes.c_int32 and sig[6] is ctypes.c_int64
    assert _lib.ABI_VERSION == 19 and re.search(r"#define NRL_ABI_VERSION 19\b", header)
    assert hasattr(_native(), "nrl_dpp_rerank")


def test_limits_and_flags():
    from newsreclib_amd import ops
    header = _header()
    assert re.search(r"#define NRL_DPP_MAX_K 64\b", header) and ops.DPP_MAX_K == 64
    assert re.search(r"#define NRL_DPP_E_QUALITY 256\b", header) and R.E_QUALITY == 256
    assert re.search(r"#define NRL_DPP_E_RANK 512\b", header) and R.E_RANK == 512
    assert set(ops.DPP_FLAGS) == {1, 4, 256, 512} and ops.DPP_FLAGS[1] == ops.MMR_FLAGS[1] and ops.DPP_FLAGS[4] == ops.MMR_FLAGS[4]
    assert "quality" in ops.DPP_FLAGS[256] and "rank" in ops.DPP_FLAGS[512]
    # a dictionary of its own: the pinned key sets are untouched
    assert set(ops.MMR_FLAGS) == {1, 4} and set(ops.CAL_FLAGS) == {1, 4, 64, 128} and set(ops.TOPK_FLAGS) == {1, 2, 4, 8}


# ---- the native entry refuses bad arguments before it launches anything (no device is touched: the pointers are never read) ---------
def _args(pool_idx=64, pool_score=64, quality=None, table=64, B=4, N=16, V=100, D=8, k=5, alpha=1.0, eps=1e-4, similarity=0,
          normalize=1, out_idx=64, out_score=64, out_gain=64, status=64):
    return [pool_idx, pool_score, quality, table, B, N, V, D, k, alpha, eps, similarity, normalize, out_idx, out_score, out_gain,
            status, None]


@pytest.mark.parametrize("change,needle", [
    (dict(B=-1), "negative size"), (dict(V=-1), "negative size"), (dict(D=-4), "negative size"), (dict(N=-1), "negative size"),
    (dict(k=-1), "negative size"),
    (dict(N=0), "N in [1, 128]"), (dict(N=129, k=5), "N in [1, 128]"),
    (dict(k=0), "k in [1, min(N = 16, 64)]"), (dict(k=17), "k in [1, min(N = 16, 64)]"), (dict(N=128, k=65), "k in [1, min(N = 128, 64)]"),
    (dict(alpha=-0.5), "alpha finite"), (dict(alpha=float("inf")), "alpha finite"), (dict(alpha=float("nan")), "alpha finite"),
    (dict(eps=-1e-3), "eps in [0, 1)"), (dict(eps=1.0), "eps in [0, 1)"), (dict(eps=float("nan")), "eps in [0, 1)"),
    (dict(D=0), "D a multiple of 4"), (dict(D=6), "D a multiple of 4"), (dict(D=1028), "D a multiple of 4"),
    (dict(V=2 ** 31), "table rows"), (dict(B=2 ** 31), "users per call"),
    (dict(similarity=2), "similarity"), (dict(similarity=-1), "similarity"), (dict(normalize=2), "normalize"),
    (dict(status=None), "status"),
    (dict(pool_idx=None), "null argument"), (dict(pool_score=None), "null argument"), (dict(table=None), "null argument"),
    (dict(out_idx=None), "null argument"), (dict(out_score=None), "null argument"), (dict(out_gain=None), "null argument")])
def test_every_refusal(change, needle):
    lib = _native()
    assert lib.nrl_dpp_rerank(*_args(**change)) == -1
    msg = lib.nrl_last_error().decode()
    assert needle in msg and msg.startswith("dpp_rerank:"), msg


def test_the_order_of_the_checks():
    lib = _native()
    # each argument list breaks every later check as well: the message is that of the earliest one
    chain = [(dict(B=-1), "negative size"), (dict(N=200), "N in [1, 128]"), (dict(k=17), "k in [1, min(N"), (dict(alpha=-1.0), "alpha finite"),
             (dict(eps=2.0), "eps in"), (dict(D=6), "D a multiple"), (dict(similarity=3), "similarity"), (dict(status=None), "status")]
    for i, (_, needle) in enumerate(chain):
        broken = {}
        for change, _ in chain[i:]:
            broken.update(change)
        assert lib.nrl_dpp_rerank(*_args(**broken)) == -1
        assert needle in lib.nrl_last_error().decode(), (needle, lib.nrl_last_error().decode())
    # B == 0 returns success without a launch once the checks pass (null pointers included), and refuses when they do not
    assert lib.nrl_dpp_rerank(*_args(B=0, pool_idx=None, table=None, out_gain=None)) == 0
    assert lib.nrl_dpp_rerank(*_args(B=0, eps=1.0)) == -1
    assert lib.nrl_dpp_rerank(*_args(B=0, status=None)) == -1
    # quality may be null or given; table may be null only when V == 0
    assert lib.nrl_dpp_rerank(*_args(B=0, quality=64)) == 0 and lib.nrl_dpp_rerank(*_args(B=0, quality=None)) == 0
    assert lib.nrl_dpp_rerank(*_args(table=None)) == -1 and "null argument" in lib.nrl_last_error().decode()


def test_python_side_refusals():
    from newsreclib_amd import ops
    from newsreclib_amd.evaluation import NewsVectorCache, NpaFeatureCache, recommend_users
    idx, score, table = torch.zeros(2, 8, dtype=torch.int64), torch.zeros(2, 8), torch.zeros(9, 4)
    for call in (lambda: ops.dpp_rerank(idx.int(), score, table, 3), lambda: ops.dpp_rerank(idx, score.double(), table, 3),
                 lambda: ops.dpp_rerank(idx, score, table.half(), 3), lambda: ops.dpp_rerank(idx, score[:, :7], table, 3),
                 lambda: ops.dpp_rerank(idx[0], score[0], table, 3), lambda: ops.dpp_rerank(idx, score, table[0], 3),
                 lambda: ops.dpp_rerank(idx, score, table, 0), lambda: ops.dpp_rerank(idx, score, table, 9),
                 lambda: ops.dpp_rerank(idx, score, table, 3, alpha=-1.0), lambda: ops.dpp_rerank(idx, score, table, 3, alpha=float("inf")),
                 lambda: ops.dpp_rerank(idx, score, table, 3, alpha=float("nan")), lambda: ops.dpp_rerank(idx, score, table, 3, eps=1.0),
                 lambda: ops.dpp_rerank(idx, score, table, 3, eps=-1e-4), lambda: ops.dpp_rerank(idx, score, table, 3, similarity="l2"),
                 lambda: ops.dpp_rerank(idx, score, table, 3, quality=score.double()),
                 lambda: ops.dpp_rerank(idx, score, table, 3, quality=score[:, :7])):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(NotImplementedError, match="at most 128"):
        ops.dpp_rerank(torch.zeros(1, 129, dtype=torch.int64), torch.zeros(1, 129), table, 3)
    with pytest.raises(NotImplementedError, match="at most 64"):
        ops.dpp_rerank(torch.zeros(1, 100, dtype=torch.int64), torch.zeros(1, 100), table, 65)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.dpp_rerank(idx, score, table, 3)
    # NPA: refused, and the reason is the user-dependence of its news vectors
    with pytest.raises(NotImplementedError, match="depends on the user"):
        NpaFeatureCache.rerank_dpp(SimpleNamespace(), idx, score, 3)
    npa = SimpleNamespace(module=SimpleNamespace(personalized_pooling_scorer=True), table=None,
                          rerank_dpp=lambda *a, **kw: NpaFeatureCache.rerank_dpp(None, *a, **kw))
    with pytest.raises(NotImplementedError, match="depends on the user"):
        recommend_users(npa, [{"hist": torch.tensor([1])}], 5, dpp=dict(pool=8))
    # recommend_users: everything is refused before anything is touched
    cache = NewsVectorCache(SimpleNamespace(), None)
    with pytest.raises(ValueError, match="at least k"):
        recommend_users(cache, [], 10, dpp=dict(pool=5))
    with pytest.raises(ValueError, match="excludes"):
        recommend_users(cache, [], 5, diversify=(8, 0.5), dpp=dict(pool=8))
    with pytest.raises(ValueError, match="excludes"):
        recommend_users(cache, [], 5, calibrate=dict(pool=8, aspect="category", gamma=0.5), dpp=dict(pool=8))
    with pytest.raises(ValueError, match="pool=, alpha"):
        recommend_users(cache, [], 5, dpp=dict(pool=8, lam=0.5))
    with pytest.raises(ValueError, match="pool=, alpha"):
        recommend_users(cache, [], 5, dpp=dict(alpha=0.5))


# ---- hand-worked pools ------------------------------------------------------------------------------------------------------------------
def _both(idx, score, table, k, quality, eps, similarity):
    idx, score, table = np.asarray(idx), np.asarray(score, dtype=F), np.asarray(table, dtype=np.float64)
    a = R.dpp_f32(idx, score, R.gram_f32(idx, table), table.shape[0], k, quality, eps, similarity)
    b = R.dpp_f64(idx, score, table, k, quality, eps=eps, similarity=similarity)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[3] == b[3]
    return a, b


@pytest.mark.parametrize("eps", [0.0, 1e-4])
def test_a_duplicated_row_is_only_ever_a_fill(eps):
    table = np.zeros((4, 4))
    table[1], table[2] = [2, 0, 0, 0], [0, 0, 2, 0]            # a and b, orthogonal, squared norms 4: every cosine is exact
    # rows [a, a, b], q = 1: L is [[1, 1, 0], [1, 1, 0], [0, 0, 1]].  Step 0: three gains of 1, the lower slot.  Then e_1 = 1 and
    # d2_1 = 1 - 1 = 0: slot 1 is not eligible; e_2 = 0, d2_2 = 1: slot 2.  Slot 1 is the fill, whatever its score
    a, b = _both([1, 1, 2], [1.0, 3.0, 2.0], table, 3, np.ones(3, dtype=F), eps, "cosine")
    assert a[0].tolist() == [1, 2, 1] and [s[0] for s in a[4]] == [0, 2, 1] and [s[2] for s in a[4]] == [True, True, False]
    assert a[1].tolist() == [1.0, 2.0, 3.0] and a[2].tolist() == [1.0, 1.0, 0.0] and b[2].tolist() == [1.0, 1.0, 0.0]
    assert a[3] == R.E_RANK and not np.signbit(a[2][2])
    short = _both([1, 1, 2], [1.0, 3.0, 2.0], table, 2, np.ones(3, dtype=F), eps, "cosine")[0]
    assert short[0].tolist() == [1, 2] and short[3] == 0     # the flag says that a listed slot was a fill


def test_the_zero_row_is_only_ever_a_fill():
    table = np.zeros((4, 4))
    table[1], table[2], table[3] = [2, 0, 0, 0], [0, 0, 2, 0], [0, 1, 0, 0]
    for sim in ("cosine", "dot"):
        # the zero row has the best score and L_ii = 0: never eligible; the fill lists it last, by score among the fills
        a, _ = _both([0, 1, 0, 2, 3], [9.0, 1.0, 8.0, 2.0, 3.0], table, 5, np.full(5, 2.0, dtype=F), 1e-4, sim)
        assert [s[0] for s in a[4]][3:] == [0, 2] and [s[2] for s in a[4]] == [True, True, True, False, False]
        assert sorted(s[0] for s in a[4][:3]) == [1, 3, 4] and a[3] == R.E_RANK and a[2][3:].tolist() == [0.0, 0.0]
    # a zero quality does what a zero row does
    a, _ = _both([1, 2, 3], [3.0, 2.0, 1.0], table, 3, np.array([0.0, 1.0, 1.0], dtype=F), 1e-4, "cosine")
    assert [s[0] for s in a[4]] == [1, 2, 0] and a[3] == R.E_RANK


def test_a_pool_of_rank_two_lists_its_third_news_as_a_fill():
    table = np.zeros((4, 4))
    table[1], table[2], table[3] = [1, 0, 0, 0], [0, 1, 0, 0], [1, 1, 0, 0]          # the third is the sum of the other two
    # dot, q = 1: L has the diagonal (1, 1, 2).  Step 0: slot 2 (gain 2); the others keep 1 - (1 / sqrt 2)^2 = 1/2 up to rounding;
    # step 1: slot 0 by the tie rule; slot 1 is then spanned: 1/2 - (1/2 / sqrt(1/2))^2 = 0 up to rounding, far below eps L_ii
    a, b = _both([1, 2, 3], [1.0, 2.0, 3.0], table, 3, np.ones(3, dtype=F), 1e-4, "dot")
    assert [s[0] for s in a[4]] == [2, 0, 1] and [s[2] for s in a[4]] == [True, True, False] and a[3] == R.E_RANK
    assert a[2][0] == 2.0 and abs(float(a[2][1]) - 0.5) <= 2.0 ** -22 and a[2][2] == 0.0 and abs(b[2][1] - 0.5) <= 1e-15
    # MMR cannot see this: slot 1 is orthogonal to slot 0 and its cosine with slot 2 is that of slot 0
    left = a[4][1][1]
    assert abs(float(left[0]) - float(left[1])) <= 2.0 ** -22 and np.isnan(left[2])


def test_a_bad_quality_entry_kills_the_slot_and_is_flagged():
    table = np.eye(4)
    for bad in (-1.0, np.nan, np.inf, -np.inf):
        a, _ = _both([0, 1, 2, -1], [1.0, 1.0, 1.0, 1.0], table, 4, np.array([1.0, bad, 1.0, bad], dtype=F), 1e-4, "cosine")
        assert a[0].tolist() == [0, 2, -1, -1] and a[3] == R.E_QUALITY      # (the empty slot's quality is not read)
        assert np.isneginf(a[1][2:]).all() and np.isneginf(a[2][2:]).all()


# ---- the float32 recurrence against the float64 definition ------------------------------------------------------------------------------
def _case(rng, V=60):
    N, D = int(rng.choice([1, 2, 5, 9, 16, 24])), int(rng.choice([4, 8, 16]))
    spread = int(rng.choice([1, 3, 16]))                # few distinct values: ties and low rank
    table = rng.integers(-spread, spread + 1, (V, D)) / 8.0
    table[0] = 0.0
    idx = rng.integers(0, V, N)
    if N > 2 and rng.random() < 0.5:
        idx[1] = idx[0]
    for bad in (-1, -2, V):
        if rng.random() < 0.25:
            idx[int(rng.integers(0, N))] = bad
    score = (rng.integers(-16, 17, N) / 8.0).astype(F)
    if rng.random() < 0.2:
        score[int(rng.integers(0, N))] = np.nan
    quality = (rng.integers(0, 17, N) / 8.0).astype(F) if rng.random() < 0.5 else rng.uniform(0.5, 2.0, N).astype(F)
    return idx, score, table, quality, int(rng.choice([1, max(1, N // 2), N]))


def test_f32_is_greedy_in_f64_and_its_gains_are_the_determinant_ratios():
    """The float32 list, step by step, maximises the float64 marginal gain up to the rounding of the recurrence.  The bound:
    the computed Cholesky rows are the exact ones of L + dL with |dL_ij| <= g max L_ii, g = (t + 5) 2^-23 (t + 2 roundings of
    2^-24 in the chain and the division, 3 in forming L from an exact Gram matrix, doubled for the square), and a perturbation dL
    moves the Schur complement L_ii - L_iS w_i, w_i = L_SS^-1 L_Si, by at most (1 + |w_i|_1)^2 max |dL| to first order."""
    rng = np.random.default_rng(60)
    checked = fills = 0
    for _ in range(400):
        idx, score, table, quality, k = _case(rng)
        sim, eps = str(rng.choice(["cosine", "dot"])), float(rng.choice([1e-2, 1e-4]))
        a = R.dpp_f32(idx, score, R.gram_f32(idx, table), table.shape[0], k, quality, eps, sim)
        slots = [s[0] for s in a[4] if s[2]]
        L, live, flags, _ = R.kernel_matrix_f64(idx, score, table, quality, similarity=sim)
        assert flags == a[3] & ~R.E_RANK
        b = R.dpp_f64(idx, score, table, len(slots), quality, eps=eps, similarity=sim, forced=slots) if slots else None
        lmax = float(np.diagonal(L)[live].max()) if live.any() else 0.0
        for t, c in enumerate(slots):
            S = slots[:t]
            w = np.abs(np.linalg.solve(L[np.ix_(S, S)], L[S, :])).sum(axis=0) if S else np.zeros(len(idx))
            tol = (t + 5) * 2.0 ** -23 * (1 + w) ** 2 * lmax
            gains = b[4][t][1]
            assert abs(float(a[2][t]) - gains[c]) <= tol[c], (t, c)
            avail = ~np.isnan(gains)
            assert np.all(gains[avail] - tol[avail] <= gains[c] + tol[c]), (t, c)
            checked += 1
        # the fill: whatever is listed after the DPP phase has a float64 gain below eps L_ii up to the same bound
        if len(slots) < k and any(not s[2] for s in a[4]):
            S = slots
            g = R.marginal_gains_f64(L, S)
            w = np.abs(np.linalg.solve(L[np.ix_(S, S)], L[S, :])).sum(axis=0) if S else np.zeros(len(idx))
            tol = (len(S) + 5) * 2.0 ** -23 * (1 + w) ** 2 * lmax
            for c in (s[0] for s in a[4] if not s[2]):
                assert g[c] <= max(eps * L[c, c], 0.0) + tol[c]
                fills += 1
            assert a[3] & R.E_RANK
        n_live = int(live.sum())
        assert int((a[0] >= 0).sum()) == min(k, n_live) and np.all(a[0][min(k, n_live):] == -1)
        assert np.all(np.isneginf(a[1][a[0] < 0])) and np.all(np.isneginf(a[2][a[0] < 0]))
    assert checked > 1000 and fills > 100


@pytest.mark.parametrize("which", ["f32", "f64"])
def test_prefix_property_and_the_product_of_the_gains(which):
    rng = np.random.default_rng(61)
    for _ in range(150):
        idx, score, table, quality, _ = _case(rng)
        N, V = len(idx), table.shape[0]
        sim = str(rng.choice(["cosine", "dot"]))
        run = (lambda k: R.dpp_f32(idx, score, R.gram_f32(idx, table), V, k, quality, 1e-3, sim)) if which == "f32" else \
            (lambda k: R.dpp_f64(idx, score, table, k, quality, eps=1e-3, similarity=sim))
        full = run(N)
        for k in {1, max(1, N // 2)}:
            part = run(k)
            assert np.array_equal(part[0], full[0][:k]) and np.array_equal(part[1], full[1][:k])
            assert np.array_equal(np.asarray(part[2], dtype=np.float64), np.asarray(full[2][:k], dtype=np.float64))
        slots = [s[0] for s in full[4] if s[2]]
        if slots:                                           # the product of the DPP-phase gains is det L_S
            L = R.kernel_matrix_f64(idx, score, table, quality, similarity=sim)[0]
            sign, logdet = np.linalg.slogdet(L[np.ix_(slots, slots)])
            gains = np.asarray(full[2][:len(slots)], dtype=np.float64)
            assert sign > 0 and abs(np.log(gains).sum() - logdet) <= len(slots) * (2e-3 if which == "f32" else 1e-9)


def test_alpha_is_the_trade_off_between_relevance_and_diversity():
    rng = np.random.default_rng(62)
    table = rng.standard_normal((50, 16))
    idx, score = np.arange(30), np.sort(rng.standard_normal(30))[::-1].astype(F)
    # a large alpha lists by relevance; alpha = 0 ignores the scores altogether
    by_score = R.dpp_f64(idx, score, table, 5, alpha=40.0)
    assert by_score[0].tolist() == [0, 1, 2, 3, 4]
    flat = R.dpp_f64(idx, score, table, 5, alpha=0.0)
    shuffled = R.dpp_f64(idx, score[::-1].copy(), table, 5, alpha=0.0)
    assert flat[0].tolist() == shuffled[0].tolist() and np.allclose(flat[2], shuffled[2])
    assert flat[2][0] == pytest.approx(1.0) and np.all(np.diff(flat[2]) <= 1e-12)       # gains never grow (submodularity of log det)
