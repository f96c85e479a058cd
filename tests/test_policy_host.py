"""CPU tier of the policy entries (``nrl_catalogue_logz`` / ``nrl_list_logprob``): the float64 restatement (``tests/policy_ref.py``)
is a distribution, the ABI (header against ``_lib.SIGNATURES`` and, when the library is built, its exports and the host-side
refusals of the native entries), every argument error of the ``ops`` wrappers and of the cache methods before anything looks at a
device, the refusals on stand-in caches, and ``snips_value`` against a hand computation."""
import ctypes
import itertools
import math
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import policy_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("nrl_catalogue_logz_workspace_size", "nrl_catalogue_logz", "nrl_list_logprob")
NRL_OK, NRL_E_INVALID, NRL_E_WORKSPACE = 0, -1, -2


def _header():
    return open(os.path.join(ROOT, "include", "newsreclib_amd.h")).read()


def _declared_arguments(header, name):
    m = re.search(r"\b(?:int|size_t) " + name + r"\(([^;]*)\);", header)
    assert m, name + " is not declared in the header"
    return [a.strip().split()[-1].lstrip("*") for a in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")]


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
def test_the_reference_is_a_distribution():
    """V = 5, k = 2: the 20 ordered lists have total probability 1; k = V: the last slot is certain."""
    from newsreclib_amd import ops
    assert callable(ops.list_logprob)
    s = np.array([1.5, -0.25, 0.0, 3.0, -2.0])
    pop = np.ones(5, dtype=bool)
    for inv_temp in (1.0, 0.3, 0.0):
        total = sum(math.exp(P.pl_logprobs(s, inv_temp, pop, pair)[1]) for pair in itertools.permutations(range(5), 2))
        assert abs(total - 1.0) <= 1e-12, (inv_temp, total)
        for perm in ([3, 0, 2, 1, 4], [4, 1, 2, 0, 3]):
            logp, tot = P.pl_logprobs(s, inv_temp, pop, perm)
            assert logp[-1] == 0.0 and math.copysign(1.0, logp[-1]) == 1.0 and abs(tot - logp.sum()) <= 1e-15
    # a masked row takes no part, trailing empty slots are +0, and the first slot is the softmax
    pop[2] = False
    logp, _ = P.pl_logprobs(s, 1.0, pop, [3, -1, -1])
    w = np.exp(s[pop])
    assert abs(logp[0] - math.log(w[2] / w.sum())) <= 1e-14 and logp[1] == 0.0 and logp[2] == 0.0
    total = sum(math.exp(P.pl_logprobs(s, 1.0, pop, pair)[1]) for pair in itertools.permutations([0, 1, 3, 4], 2))
    assert abs(total - 1.0) <= 1e-12


def test_the_statistics_of_the_reference():
    from newsreclib_amd import ops
    assert callable(ops.catalogue_logz)
    s = np.array([1.5, -0.25, 0.0, 3.0, -2.0, 7.0])
    pop = np.array([1, 1, 1, 1, 1, 0], dtype=bool)
    m, ls, h, n = P.stats(s, 1.0, pop)
    p = np.exp(s[pop]) / np.exp(s[pop]).sum()
    assert (m, n) == (3.0, 5) and abs(m + ls - math.log(np.exp(s[pop]).sum())) <= 1e-14
    assert abs(h + (p * np.log(p)).sum()) <= 1e-14
    # inv_temp = 0 is the uniform policy: entropy log n, logsum log n
    m, ls, h, n = P.stats(s, 0.0, pop)
    assert m == 0.0 and abs(ls - math.log(5)) <= 1e-15 and abs(h - math.log(5)) <= 1e-15
    assert P.stats(s, 1.0, np.zeros(6, dtype=bool)) == (P.NEG_INF, P.NEG_INF, 0.0, 0)
    m, ls, h, n = P.stats(s, 2.0, np.array([0, 0, 0, 0, 1, 0], dtype=bool))
    assert (m, ls, h, n) == (-4.0, 0.0, 0.0, 1)


def test_the_subtractive_form_breaks_where_the_tail_form_does_not():
    """One row 40 above the rest: after it is drawn, ``Z - exp(t_best)`` is rounding noise or zero in float64."""
    from newsreclib_amd import ops
    assert callable(ops.list_logprob)
    s = np.array([40.0, 0.0, 0.0, -1.0])
    pop = np.ones(4, dtype=bool)
    logp, _ = P.pl_logprobs(s, 1.0, pop, [0, 1])
    want = -math.log(2 + math.exp(-1))
    assert abs(logp[1] - want) <= 1e-14
    bad, _ = P.pl_logprobs_subtractive(s, 1.0, pop, [0, 1])
    assert not (abs(bad[1] - want) <= 1e-3)


# ---- the ABI --------------------------------------------------------------------------------------------------------------------------
def test_the_entries_and_flags_are_in_the_header_and_in_the_signatures():
    from newsreclib_amd import _lib, ops
    header = _header()
    ws, logz, lp = (_declared_arguments(header, n) for n in NAMES)
    assert ws == ["B", "V", "D"]
    assert logz == ["user_vec", "table", "B", "V", "D", "inv_temp", "excl_idx", "excl_off", "eligible", "drop_idx", "kd", "out_max",
                    "out_logsum", "out_entropy", "out_pop", "out_dropped", "status", "ws", "ws_bytes", "stream"]
    assert lp == ["user_vec", "table", "B", "V", "D", "inv_temp", "list_idx", "k", "tail_max", "tail_logsum", "tail_pop",
                  "tail_dropped", "out_score", "out_logp", "out_total", "status", "stream"]
    for name, args in zip(NAMES, (ws, logz, lp)):
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == len(args), name
    assert _lib.SIGNATURES["nrl_catalogue_logz"][1][5] is ctypes.c_float and _lib.SIGNATURES["nrl_list_logprob"][1][5] is ctypes.c_float
    assert re.search(r"#define NRL_POLICY_E_LIST 128\b", header) and re.search(r"#define NRL_POLICY_E_INF 256\b", header)
    assert _lib.ABI_VERSION == 19 and re.search(r"#define NRL_ABI_VERSION 19\b", header)
    assert set(ops.POLICY_FLAGS) == {1, 2, 4, 128, 256}
    assert not any(n.startswith(("nrl_catalogue_logz", "nrl_list_logprob")) and n.endswith("_workspace_bytes") for n in _lib.SIGNATURES)


def test_the_built_library_exports_the_entries_and_refuses_on_the_host():
    from newsreclib_amd import _build, _lib, ops
    assert callable(ops.catalogue_logz)
    if not os.path.exists(_build.LIB):
        return                                                   # (nothing built here: the GPU tier loads it)
    data = open(_build.LIB, "rb").read()
    for name in NAMES:
        assert name.encode() + b"\0" in data, name
    lib = _lib.load()
    # 5 words per (user, chunk), padded to 256 bytes: V = 65536 has 512 tiles in 64 chunks, V = 8320 65 tiles in 33
    assert lib.nrl_catalogue_logz_workspace_size(512, 65536, 300) == 512 * 64 * 5 * 4
    assert lib.nrl_catalogue_logz_workspace_size(65, 8320, 20) == (65 * 33 * 5 * 4 + 255) // 256 * 256
    assert lib.nrl_catalogue_logz_workspace_size(3, 0, 4) == 256 and lib.nrl_catalogue_logz_workspace_size(3, 5, 6) == 256
    status = ctypes.c_int32(0)
    buf = (ctypes.c_char * 1024)()
    ws = (ctypes.addressof(buf) + 255) & ~255
    st = ctypes.addressof(status)

    def logz(B=2, V=10, D=8, inv_temp=1.0, drop=None, kd=0, out=st, dropped=st, status=st, ws_bytes=256):
        return lib.nrl_catalogue_logz(st, st, B, V, D, inv_temp, None, None, None, drop, kd, out, out, out, out, dropped, status, ws,
                                      ws_bytes, None)

    for bad in (dict(inv_temp=float("nan")), dict(inv_temp=float("inf")), dict(inv_temp=-0.5), dict(kd=-1), dict(kd=129, drop=st),
                dict(kd=2), dict(kd=2, drop=st, dropped=None), dict(out=None), dict(status=None), dict(D=6), dict(D=1028), dict(B=-1)):
        assert logz(**bad) == NRL_E_INVALID, bad
    assert logz(ws_bytes=8) == NRL_E_WORKSPACE
    assert logz(B=0, out=None, dropped=None) == NRL_OK           # no users: success without a launch

    def lp(B=2, V=10, D=8, inv_temp=1.0, k=2, lists=st, tail=st, out=st, status=st):
        return lib.nrl_list_logprob(st, st, B, V, D, inv_temp, lists, k, tail, tail, tail, tail, out, out, out, status, None)

    for bad in (dict(inv_temp=float("nan")), dict(inv_temp=-1.0), dict(k=0), dict(k=129), dict(lists=None), dict(tail=None),
                dict(out=None), dict(status=None), dict(D=6), dict(B=2 ** 26, k=64)):
        assert lp(**bad) == NRL_E_INVALID, bad
    assert lp(B=0, lists=None, tail=None, out=None) == NRL_OK


# ---- the wrappers' refusals -------------------------------------------------------------------------------------------------------------
def test_the_wrappers_refuse_before_anything_looks_at_a_device():
    from newsreclib_amd import ops
    U, T = torch.zeros(3, 8), torch.zeros(10, 8)
    lists = torch.zeros(3, 2, dtype=torch.int64)
    for call in (lambda **kw: ops.catalogue_logz(U, T, **kw), lambda **kw: ops.list_logprob(U, T, kw.pop("drop_idx", lists), **kw)):
        for bad in (float("nan"), float("inf"), -1.0, -1e-30, 1e39):
            with pytest.raises(ValueError, match="`inv_temp` must be finite"):
                call(inv_temp=bad)
        for bad in (lists.int(), lists.float(), lists.tolist()):
            with pytest.raises(TypeError, match="must be an int64 tensor"):
                call(drop_idx=bad)
        for bad in (lists[:2], lists[:, 0], torch.zeros(3, 129, dtype=torch.int64)):
            with pytest.raises(ValueError, match="one list per user|at most 128 rows"):
                call(drop_idx=bad)
        for ok in (dict(inv_temp=0.0), dict(inv_temp=0), dict(drop_idx=torch.zeros(3, 128, dtype=torch.int64))):
            with pytest.raises(RuntimeError, match="must live on the GPU"):
                call(**ok)
    with pytest.raises(TypeError, match="`list_idx` must be an int64 tensor"):
        ops.list_logprob(U, T, None)
    with pytest.raises(ValueError, match="at least one slot"):
        ops.list_logprob(U, T, lists[:, :0])
    with pytest.raises(TypeError, match="`user_vec` must be a float32 tensor"):
        ops.catalogue_logz(U.double(), T)
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        ops.catalogue_logz(U, T)


def _stand_in(**markers):
    return SimpleNamespace(module=SimpleNamespace(**markers), table=SimpleNamespace(attrs={}, device="cpu"), _row_time=None)


def test_the_cache_methods_refuse_before_any_device_work():
    from newsreclib_amd import evaluation as E
    cache = object.__new__(E.NewsVectorCache)
    cache.module = SimpleNamespace(dot_product_scorer=True)
    hist, hs = torch.ones(3, dtype=torch.int64), torch.tensor([1, 2])
    lists = torch.zeros(2, 3, dtype=torch.int64)
    lo = torch.zeros(2, dtype=torch.int32)
    with pytest.raises(NotImplementedError, match="tkz_sum_kernel.*tkw_walk"):
        cache.policy_stats(hist, hs, 1.0, window=(lo, lo))
    with pytest.raises(NotImplementedError, match="tkz_sum_kernel.*tkw_walk"):
        cache.list_log_probs(hist, hs, lists, 1.0, window=(lo, lo))
    for bad in (float("nan"), float("inf"), -1.0):
        with pytest.raises(ValueError, match="`inv_temp`"):
            cache.policy_stats(hist, hs, bad)
        with pytest.raises(ValueError, match="`inv_temp`"):
            cache.list_log_probs(hist, hs, lists, bad)
    with pytest.raises(TypeError, match="`lists` must be an int64 tensor"):
        cache.list_log_probs(hist, hs, lists.int(), 1.0)
    for bad in (lists[:1], lists[:, :0], torch.zeros(2, 129, dtype=torch.int64), lists[0]):
        with pytest.raises(ValueError, match="`lists` must be"):
            cache.list_log_probs(hist, hs, bad, 1.0)
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        cache.policy_stats(hist, hs, 1.0)
    users = [{"hist": [1]}]
    for marker in ("multi_interest_scorer", "dnn_predictor_scorer", "personalized_pooling_scorer", "class_biased_scorer"):
        other = object.__new__(E.NewsVectorCache)
        other.module = SimpleNamespace(**{marker: True})
        for call in (lambda: other.policy_stats(hist, hs, 1.0), lambda: other.list_log_probs(hist, hs, lists, 1.0),
                     lambda: E.policy_report(_stand_in(**{marker: True}), users, [1.0])):
            with pytest.raises(NotImplementedError, match="tkz_sum_kernel") as info:
                call()
            assert marker in str(info.value) and "tks_scores_kernel" not in str(info.value)
    for cls in (E.MannerVectorCache, E.NpaFeatureCache):
        other = object.__new__(cls)
        other.module = SimpleNamespace(personalized_pooling_scorer=cls is E.NpaFeatureCache)
        with pytest.raises(NotImplementedError, match="tkz_sum_kernel"):
            other.policy_stats(hist, hs, 1.0)
        with pytest.raises(NotImplementedError, match="tkz_sum_kernel"):
            other.list_log_probs(hist, hs, lists, 1.0)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="temperature must be finite and > 0"):
            E.policy_report(_stand_in(dot_product_scorer=True), users, [1.0, bad])
    assert E.policy_report(_stand_in(dot_product_scorer=True), [], []) == {}


def test_sample_recommendations_asks_for_the_log_probabilities_of_what_it_drew():
    """A stand-in cache: with ``log_probs=True`` every draw's list goes to ``list_log_probs`` under the same inverse temperature and
    the result lands at (user, draw); the default never calls it and returns the tensor alone."""
    from newsreclib_amd import evaluation as E
    asked = []

    def recommend(hist, hs, k, user_idx=None, eligible=None, sample=None):
        inv_temp, seed, keys = sample
        idx = (keys[:, None] * 100 + seed % 100 + torch.arange(k)[None, :]).long()
        return idx, idx.float(), torch.zeros(1, dtype=torch.int32)

    def list_log_probs(hist, hs, lists, inv_temp, user_idx=None, eligible=None):
        asked.append((lists.clone(), inv_temp))
        return -lists.float() / 8, None, None, torch.zeros(1, dtype=torch.int32)

    cache = _stand_in(dot_product_scorer=True)
    cache.recommend, cache.list_log_probs = recommend, list_log_probs
    users = [{"hist": [1, 2]}, {"hist": [3], "user_id": 40}, {"hist": [4, 5, 6]}]
    plain = E.sample_recommendations(cache, users, 2, 3, 4.0, 7, batch_size=2)
    assert isinstance(plain, torch.Tensor) and not asked
    lists, logp = E.sample_recommendations(cache, users, 2, 3, 4.0, 7, batch_size=2, log_probs=True)
    assert torch.equal(lists, plain) and len(asked) == 6 and all(t == 0.25 for _, t in asked)
    assert logp.shape == (3, 3, 2) and logp.dtype == torch.float32 and not logp.is_cuda
    assert torch.equal(logp, -lists.float() / 8)
    lists, logp = E.sample_recommendations(cache, users, 2, 0, 1.0, 1, log_probs=True)
    assert lists.shape == (3, 0, 2) and logp.shape == (3, 0, 2)


# ---- SNIPS ------------------------------------------------------------------------------------------------------------------------------
def test_snips_against_a_hand_computation():
    from newsreclib_amd.metrics import snips_value
    # weights 2, 1/2, 1 on rewards 1, 0, 3: value (2 + 3) / 3.5, effective sample size 3.5^2 / 5.25
    r = [1.0, 0.0, 3.0]
    lt = [math.log(0.2), math.log(0.1), math.log(0.3)]
    ll = [math.log(0.1), math.log(0.2), math.log(0.3)]
    value, ess = snips_value(r, lt, ll)
    assert abs(value - 5.0 / 3.5) <= 1e-14 and abs(ess - 3.5 ** 2 / 5.25) <= 1e-13
    # a common shift of the log-ratios cancels, however large
    v2, e2 = snips_value(torch.tensor(r), torch.tensor(lt, dtype=torch.float64) - 900.0, torch.tensor(ll, dtype=torch.float64))
    assert abs(v2 - value) <= 1e-12 and abs(e2 - ess) <= 1e-12
    # clip = 1: weights 1, 1/2, 1 -> (1 + 3) / 2.5 and 2.5^2 / 2.25
    value, ess = snips_value(r, lt, ll, clip=1.0)
    assert abs(value - 4.0 / 2.5) <= 1e-14 and abs(ess - 2.5 ** 2 / 2.25) <= 1e-13
    # the same policy: the plain mean, n
    value, ess = snips_value(r, ll, ll)
    assert abs(value - 4.0 / 3) <= 1e-15 and abs(ess - 3.0) <= 1e-15
    assert math.isnan(snips_value([], [], [])[0]) and snips_value([], [], [])[1] == 0.0
    with pytest.raises(ValueError, match="per list"):
        snips_value(r, lt, ll[:2])
    with pytest.raises(ValueError, match="not finite"):
        snips_value(r, lt, [0.0, float("nan"), 0.0])
    with pytest.raises(ValueError, match="clip > 0"):
        snips_value(r, lt, ll, clip=0.0)
