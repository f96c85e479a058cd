"""CPU tier of the class-biased full-catalogue top-k and rank: the ABI (header against ``_lib.SIGNATURES``), the limits and the
flag, the markers of the modules, the refusals that come before any device work, and the properties of the float64
scores (``tests/topk_bias_ref.py``) under the shared contract (``tests/catalogue_ref.py``) the GPU tests compare against."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import catalogue_ref as C
from tests import topk_bias_ref as R
from tests import topk_capped_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("nrl_topk_bias_scores", "nrl_topk_bias_scores_capped", "nrl_catalogue_bias_ranks")


def _header():
    return open(os.path.join(ROOT, "include", "newsreclib_amd.h")).read()


def _declared_arguments(header, name):
    m = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
    assert m, name + " is not declared in the header"
    return [a.strip() for a in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")]


def test_the_three_entries_are_in_the_header_and_in_the_signatures():
    from newsreclib_amd import _lib
    header = _header()
    for name in NAMES:
        args = _declared_arguments(header, name)
        assert name in _lib.SIGNATURES, name
        assert len(_lib.SIGNATURES[name][1]) == len(args), (name, len(args))
        # (bias, row_class, S) directly behind D
        assert [a.split()[-1].lstrip("*") for a in args[4:8]] == ["D", "bias", "row_class", "S"], args[:8]
    capped = [a.split()[-1].lstrip("*") for a in _declared_arguments(header, "nrl_topk_bias_scores_capped")]
    assert capped[8:11] == ["k", "cap_class", "max_per_class"]
    assert _lib.ABI_VERSION == 19 and re.search(r"#define NRL_ABI_VERSION 19\b", header)


def test_limits_and_the_flag_are_declared_once():
    from newsreclib_amd import ops
    header = _header()
    assert re.search(r"#define NRL_TOPK_MAX_BIAS_CLASSES 64\b", header) and ops.TOPK_MAX_BIAS_CLASSES == 64
    assert re.search(r"#define NRL_TOPK_E_CLASS 64\b", header)
    # bit 64 is worded for both families; the earlier keys are unchanged (the key sets of TOPK_FLAGS and RANK_FLAGS themselves are
    # pinned by the host tests of the other scorers, so the biased entries' words are dictionaries of their own)
    assert 64 in ops.TOPK_BIAS_FLAGS and 64 in ops.RANK_BIAS_FLAGS and "class id" in ops.TOPK_BIAS_FLAGS[64]
    assert all(ops.TOPK_BIAS_FLAGS[b] == ops.TOPK_FLAGS[b] for b in ops.TOPK_FLAGS) and set(ops.TOPK_FLAGS) == {1, 2, 4, 8}
    assert all(ops.RANK_BIAS_FLAGS[b] == ops.RANK_FLAGS[b] for b in ops.RANK_FLAGS) and set(ops.RANK_FLAGS) == {1, 2, 4, 16, 32}
    assert set(ops.TOPK_BIAS_FLAGS) == {1, 2, 4, 8, 64} and set(ops.RANK_BIAS_FLAGS) == {1, 2, 4, 16, 32, 64}


def test_sentidebias_is_a_class_biased_scorer_and_still_no_dot_product_scorer():
    from newsreclib_amd.nrms_module import NRMSModule
    from newsreclib_amd.senti_debias_module import SentiDebiasModule
    assert SentiDebiasModule.class_biased_scorer is True and SentiDebiasModule.class_bias_aspect == "sentiment"
    assert not hasattr(SentiDebiasModule, "dot_product_scorer")
    assert callable(SentiDebiasModule.user_vectors_and_bias)
    assert not getattr(NRMSModule, "class_biased_scorer", False)


def test_a_module_with_neither_marker_is_refused_before_any_device_work():
    from newsreclib_amd.evaluation import NewsVectorCache
    cache = NewsVectorCache(SimpleNamespace(), None)        # (no table, no vectors: anything past the refusal would fail otherwise)
    hist, hs = torch.tensor([1, 2, 3]), torch.tensor([3])
    for call in (lambda: cache.recommend_biased(hist, hs, 5),
                 lambda: cache.rank_clicks_biased(hist, hs, torch.tensor([4]), torch.tensor([1]))):
        with pytest.raises(NotImplementedError) as err:
            call()
        assert "class_biased_scorer" in str(err.value) and "dot_product_scorer" in str(err.value)
    # a module with a marker and the wrong keywords is refused as early
    own = NewsVectorCache(SimpleNamespace(class_biased_scorer=True), None)
    with pytest.raises(ValueError, match="brings its own class bias"):
        own.recommend_biased(hist, hs, 5, aspect="category", bias=torch.zeros(1, 3))
    dot = NewsVectorCache(SimpleNamespace(dot_product_scorer=True), None)
    with pytest.raises(ValueError, match="needs `aspect` and `bias`"):
        dot.recommend_biased(hist, hs, 5)


# ---- the native entries refuse bad arguments before they launch anything (no device is touched: the pointers are never read) ------
def _lib():
    from newsreclib_amd import _build, _lib
    _build.build(verbose=False)
    return _lib.load()


def _scores_args(k=5, bias=64, row_class=64, S=4, status=64, V=100, B=4):
    # user, table, B, V, D, bias, row_class, S, k, excl_idx, excl_off, eligible, slices, out_idx, out_score, status, ws, bytes, stream
    return [64, 64, B, V, 8, bias, row_class, S, k, None, None, None, 0, 64, 64, status, None, 0, None]


def _capped_args(k=5, m=2, cap_class=64, **kw):
    a = _scores_args(k=k, **kw)
    return a[:9] + [cap_class, m] + a[9:]


def _rank_args(bias=64, row_class=64, S=4, status=64, V=100, B=4):
    # ..., S, tgt_idx, tgt_off, n_targets, excl_idx, excl_off, eligible, slices, out_rank, out_score, out_ranked, status, ws, bytes, stream
    return [64, 64, B, V, 8, bias, row_class, S, 64, 64, 3, None, None, None, 0, 64, 64, 64, status, None, 0, None]


@pytest.mark.parametrize("change,needle", [(dict(S=0), "S in [1, 64]"), (dict(S=65), "S in [1, 64]"), (dict(S=-1), "S in [1, 64]"),
                                           (dict(bias=None), "bias is required"), (dict(row_class=None), "row_class is required"),
                                           (dict(status=None), "status")])
def test_every_entry_refuses_a_bad_bias(change, needle):
    lib = _lib()
    for name, args in (("topk_bias_scores", _scores_args), ("topk_bias_scores_capped", _capped_args),
                       ("catalogue_bias_ranks", _rank_args)):
        assert getattr(lib, "nrl_" + name)(*args(**change)) == -1
        msg = lib.nrl_last_error().decode()
        assert needle in msg and name + ":" in msg, msg


def test_the_order_of_the_checks():
    lib = _lib()
    # the dot-product entry's checks come first, under the new entry's name
    assert lib.nrl_topk_bias_scores(*_scores_args(k=200, S=0)) == -1
    assert "topk_bias_scores: k in [1, 128]" in lib.nrl_last_error().decode()
    # then the bias, then the cap
    assert lib.nrl_topk_bias_scores_capped(*_capped_args(k=65, S=65)) == -1 and "S in [1, 64]" in lib.nrl_last_error().decode()
    assert lib.nrl_topk_bias_scores_capped(*_capped_args(k=65)) == -1
    assert "topk_bias_scores_capped: k in [1, 64] under a class cap" in lib.nrl_last_error().decode()
    assert lib.nrl_topk_bias_scores_capped(*_capped_args(m=0)) == -1 and "max_per_class" in lib.nrl_last_error().decode()
    assert lib.nrl_topk_bias_scores_capped(*_capped_args(cap_class=None)) == -1 and "row_class" in lib.nrl_last_error().decode()
    # every check passes: the next refusal is the workspace's (null), still before any launch
    for name, args in (("nrl_topk_bias_scores", _scores_args), ("nrl_topk_bias_scores_capped", _capped_args),
                       ("nrl_catalogue_bias_ranks", _rank_args)):
        assert getattr(lib, name)(*args()) != 0
        assert not any(w in lib.nrl_last_error().decode() for w in ("S in", "bias is", "row_class", "max_per_class")), name
        # B == 0 returns success without a launch once the arguments are sound, and refuses when they are not
        assert getattr(lib, name)(*args(B=0)) == 0
        assert getattr(lib, name)(*args(B=0, S=65)) == -1
        # V == 0 needs no classes
        assert getattr(lib, name)(*args(B=0, V=0, row_class=None)) == 0


def test_wrappers_have_no_cpu_path():
    from newsreclib_amd import ops
    U, T, cls = torch.zeros(2, 4), torch.zeros(9, 4), torch.zeros(9, dtype=torch.int32)
    off = torch.zeros(3, dtype=torch.int64)
    for call in (lambda: ops.topk_bias_scores(U, T, torch.zeros(2, 4), cls, 3),
                 lambda: ops.topk_bias_scores_capped(U, T, torch.zeros(2, 4), cls, 3, cls, 1),
                 lambda: ops.catalogue_bias_ranks(U, T, torch.zeros(2, 4), cls, off[:0], off)):
        with pytest.raises(RuntimeError, match="no CPU path"):
            call()


# ---- the restatement's own properties ------------------------------------------------------------------------------------------------
def _case(rng):
    B, V, D = int(rng.choice([1, 2, 5])), int(rng.choice([1, 2, 7, 64, 65, 130])), 4
    S = int(rng.choice([1, 3, 19]))
    spread = int(rng.choice([1, 3, 20]))                # few distinct values: ties everywhere
    U, T = rng.integers(-spread, spread + 1, (B, D)) / 8.0, rng.integers(-spread, spread + 1, (V, D)) / 8.0
    bias = rng.integers(-spread, spread + 1, (B, S)) / 8.0
    cls = rng.integers(-1, S + 1, V)                    # ids -1 and S among them
    excl = [sorted(set(rng.integers(-2, V + 2, int(rng.integers(0, 6))).tolist())) for _ in range(B)]
    elig = (rng.random(V) > 0.15).astype(np.uint8)
    k = int(rng.choice([1, 5, 128]))
    return U, T, bias, cls, excl, elig, k


def test_a_zero_bias_is_the_plain_reference():
    """``topk_bias_ref.scores`` with a zero bias is ``U @ T.T`` whatever the class ids, so the shared order over it returns the
    plain dot-product lists (the order itself is pinned in test_catalogue_ref_host.py), and a bad class id adds nothing."""
    rng = np.random.default_rng(40)
    for _ in range(500):
        U, T, bias, cls, excl, elig, k = _case(rng)
        s, flags = R.scores(U, T, np.zeros_like(bias), cls)
        assert flags == (R.E_CLASS if ((cls < 0) | (cls >= bias.shape[1])).any() else 0)
        pop, nan = C.population(s, excl, elig)
        idx, score = C.topk(s, pop, k)
        want_idx, want_score = C.expected_topk(torch.from_numpy(U) @ torch.from_numpy(T).T, k, excl, elig)
        assert not nan and torch.equal(idx, want_idx) and torch.equal(score, want_score)
        # a bad class id adds nothing: the scores with the bias differ from the plain ones only in the good columns
        sb, _ = R.scores(U, T, bias, cls)
        bad = (cls < 0) | (cls >= bias.shape[1])
        assert torch.equal(sb[:, bad], s[:, bad])


def test_ranks_are_consistent_with_the_lists():
    rng = np.random.default_rng(41)
    for _ in range(500):
        U, T, bias, cls, excl, elig, k = _case(rng)
        B, V = U.shape[0], T.shape[0]
        if rng.random() < 0.2:
            bias[0, 0] = np.nan                         # a NaN bias drops that class for that user
        s, _ = R.scores(U, T, bias, cls)
        pop, nan = C.population(s, excl, elig)
        assert nan == bool((torch.isnan(s) & ~pop & torch.from_numpy(elig.astype(bool))[None, :]
                            & torch.tensor([[v not in excl[b] for v in range(V)] for b in range(B)])).any())
        idx, score = C.topk(s, pop, k)
        targets = [rng.integers(-1, V + 1, int(rng.integers(0, 4))).tolist() for _ in range(B)]
        rank, tscore, ranked = C.ranks(s, pop, targets)
        assert torch.equal(ranked, (idx >= 0).sum(1).to(torch.int32)) or k < V
        j = 0
        for b in range(B):
            assert int(ranked[b]) == int(pop[b].sum())
            for r in targets[b]:
                listed = torch.nonzero((idx[b] == r) & (idx[b] >= 0)).reshape(-1)
                if rank[j] == 0:
                    assert listed.numel() == 0 and tscore[j] == -np.inf
                elif rank[j] <= k:
                    assert listed.numel() == 1 and int(listed[0]) == rank[j] - 1 and score[b, rank[j] - 1] == tscore[j]
                else:
                    assert listed.numel() == 0
                j += 1
        # the capped walk with m >= k is the uncapped list
        kc = min(k, 64)
        c_idx, c_score = topk_capped_ref.reference(s, pop, torch.from_numpy(cls * 3), kc, kc)
        assert torch.equal(c_idx, idx[:, :kc]) and torch.equal(c_score, score[:, :kc])
