"""CPU tier of Gumbel top-k (``nrl_topk_sampled_scores`` / ``nrl_gumbel_noise``): the restatement of the noise
(``tests/topk_sampled_ref.py``) against values computed by hand, the range and the form of ``u``, the ABI (header against
``_lib.SIGNATURES`` and, when the library is built, its exports and the host-side refusals of the native entries), every argument
error of the ``ops`` wrappers and of ``recommend`` before anything looks at a device, the refusals of ``recommend_users(sample=)``
on stand-in caches, and the seeds ``sample_recommendations`` hands down."""
import ctypes
import math
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import topk_sampled_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("nrl_topk_sampled_scores_workspace_size", "nrl_topk_sampled_scores", "nrl_gumbel_noise")
NRL_OK, NRL_E_INVALID, NRL_E_WORKSPACE = 0, -1, -2


def _header():
    return open(os.path.join(ROOT, "include", "newsreclib_amd.h")).read()


def _declared_arguments(header, name):
    m = re.search(r"\b(?:int|size_t) " + name + r"\(([^;]*)\);", header)
    assert m, name + " is not declared in the header"
    return [a.strip().split()[-1].lstrip("*") for a in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")]


# ---- the noise ------------------------------------------------------------------------------------------------------------------------
def test_the_restatement_against_hand_computed_values():
    """Two (seed, key, row) triples worked through the five hash steps with Python integers, outside the reference's numpy code:
    k0, ku, h, m and u; a small seed and key, and a seed above 2^32 with a negative key (all 64 bits of both take part)."""
    from newsreclib_amd import ops
    assert callable(ops.gumbel_noise)
    hand = (((1, 1000, 0), 0xA07C7A97, 0xA7F881A9, 0x266EB84A, 1259356, 0.15012699365615845, -0.6398907598137196),
            ((2 ** 40 + 7, -5, 123456789), 0x70417E41, 0xB575B4E9, 0xF0985AF2, 7883821, 0.9398247599601746, 2.7796238641722995))
    for (seed, key, row), k0, ku, h, m, u, g in hand:
        assert int(R.call_key(seed)) == k0
        assert int(R.user_key(k0, [key])[0]) == ku
        assert int(R.lowbias32((row * 0x9E3779B1 + ku) & R.M32)) == h and h >> 9 == m
        assert int(R.mantissa(seed, [key], [row])[0]) == m
        got = R.uniform(seed, [key], [row])
        assert got.dtype == np.float32 and float(got[0]) == u == (2 * m + 1) * 2.0 ** -24
        assert abs(float(R.gumbel64(got)[0]) - g) <= 1e-15 * max(1.0, abs(g))


def test_u_is_an_odd_multiple_of_2_to_the_minus_24_inside_the_open_interval():
    from newsreclib_amd import ops
    assert callable(ops.gumbel_noise)
    rng = np.random.default_rng(5)
    key = rng.integers(-2 ** 63, 2 ** 63 - 1, 1 << 16, dtype=np.int64)
    row = rng.integers(0, 2 ** 31, 1 << 16, dtype=np.int64)
    for seed in (0, 7, 2 ** 64 - 1):
        m = R.mantissa(seed, key, row)
        u = R.uniform(seed, key, row)
        assert m.max() < 2 ** 23 and u.dtype == np.float32
        assert u.min() >= np.float32(2.0 ** -24) and u.max() <= np.float32(1 - 2.0 ** -24)
        assert np.array_equal(u.astype(np.float64) * 2.0 ** 24, (2 * m + 1).astype(np.float64))
        assert np.isfinite(R.gumbel64(u)).all()
    # the ends of the range: both logs are finite in fp32 as well
    for m in (0, 2 ** 23 - 1):
        u = np.float32((2 * m + 1) * 2.0 ** -24)
        assert 0 < u < 1 and math.isfinite(-math.log(-math.log(float(u))))


def test_the_first_slot_of_the_restatement_follows_the_softmax():
    """The float64 restatement on the distribution case of the GPU tier, one seed: the bound the device must meet is met by the
    statement itself."""
    from newsreclib_amd import ops
    assert callable(ops.topk_sampled_scores)
    s = np.array([2, 1, 0, -1, 0.5, 1.5, -0.5, 0.0])
    u = R.uniform(12345, np.arange(1000, 5096)[:, None], np.arange(8)[None, :]).astype(np.float64)
    order = np.argsort(-(s[None, :] + R.gumbel64(u)), axis=1, kind="stable")
    p1, p2 = R.pl_marginals(s, 1.0)
    assert abs(p1.sum() - 1) < 1e-12 and abs(p2.sum() - 1) < 1e-12
    assert R.chi2(np.bincount(order[:, 0], minlength=8), p1) < R.CHI2_7_1E6
    assert R.chi2(np.bincount(order[:, 1], minlength=8), p2) < R.CHI2_7_1E6


# ---- the ABI --------------------------------------------------------------------------------------------------------------------------
def test_the_three_entries_are_in_the_header_and_in_the_signatures():
    from newsreclib_amd import _lib
    header = _header()
    ws, scores, noise = (_declared_arguments(header, n) for n in NAMES)
    plain = _declared_arguments(header, "nrl_topk_scores")
    assert ws == _declared_arguments(header, "nrl_topk_scores_workspace_bytes")      # (`_size`: the set of *_workspace_bytes names is pinned)
    assert scores[:9] == plain[:6] + ["user_key", "seed", "inv_temp"]
    assert scores[9:] == plain[6:11] + ["out_key"] + plain[11:]
    assert noise == ["user_key", "row", "n", "seed", "out_u", "out_g", "stream"]
    for name, args in zip(NAMES, (ws, scores, noise)):
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == len(args), name
    sig = _lib.SIGNATURES["nrl_topk_sampled_scores"][1]
    assert sig[7] is ctypes.c_uint64 and sig[8] is ctypes.c_float and _lib.SIGNATURES["nrl_gumbel_noise"][1][3] is ctypes.c_uint64
    assert _lib.ABI_VERSION == 19 and re.search(r"#define NRL_ABI_VERSION 19\b", header)


def test_the_built_library_exports_the_entries_and_refuses_on_the_host():
    """With a library built: the exports, the workspace size (the plain entry's: the raw scores read their rows in place) and the
    refusals that come before any launch, none of which needs a device."""
    from newsreclib_amd import _build, _lib, ops
    assert callable(ops.topk_sampled_scores)
    if not os.path.exists(_build.LIB):
        return                                                   # (nothing built here: the GPU tier loads it)
    data = open(_build.LIB, "rb").read()
    for name in NAMES:
        assert name.encode() + b"\0" in data, name
    lib = _lib.load()
    for shape in ((512, 65536, 300, 10, 0), (3, 130, 20, 128, 7), (0, 5, 4, 1, 0)):
        assert lib.nrl_topk_sampled_scores_workspace_size(*shape) == lib.nrl_topk_scores_workspace_bytes(*shape)
    status = ctypes.c_int32(0)
    buf = (ctypes.c_char * 1024)()
    ws = (ctypes.addressof(buf) + 255) & ~255
    st = ctypes.addressof(status)

    def call(B=2, V=10, D=8, k=2, key=st, inv_temp=1.0, out=st, ws_bytes=256):
        return lib.nrl_topk_sampled_scores(st, st, B, V, D, k, key, 3, inv_temp, None, None, None, 0, out, out, out, st, ws, ws_bytes, None)

    for bad in (dict(inv_temp=float("nan")), dict(inv_temp=float("inf")), dict(inv_temp=-0.5), dict(key=None), dict(out=None),
                dict(k=0), dict(k=129), dict(D=6), dict(D=1028), dict(B=2 ** 26, k=64)):
        assert call(**bad) == NRL_E_INVALID, bad
    assert call(ws_bytes=8) == NRL_E_WORKSPACE
    assert call(B=0, key=None, out=None) == NRL_OK          # no users: success without a launch
    assert lib.nrl_gumbel_noise(None, None, 0, 1, None, None, None) == NRL_OK
    assert lib.nrl_gumbel_noise(None, None, 5, 1, None, None, None) == NRL_E_INVALID
    assert lib.nrl_gumbel_noise(st, st, -1, 1, st, st, None) == NRL_E_INVALID


# ---- the wrappers' refusals -------------------------------------------------------------------------------------------------------------
def test_the_wrappers_refuse_before_anything_looks_at_a_device():
    from newsreclib_amd import ops
    U, T = torch.zeros(3, 8), torch.zeros(10, 8)
    key = torch.arange(3)

    def call(key=key, seed=1, inv_temp=1.0):
        return ops.topk_sampled_scores(U, T, 2, key, seed, inv_temp)

    for bad in (key.int(), key.float(), key.tolist(), None):
        with pytest.raises(TypeError, match="`user_key` must be an int64 tensor"):
            call(key=bad)
    for bad in (key[:2], torch.arange(4), key.reshape(3, 1)):
        with pytest.raises(ValueError, match="one entry per user"):
            call(key=bad)
    for bad in (float("nan"), float("inf"), -1.0, -1e-30, 1e39):
        with pytest.raises(ValueError, match="`inv_temp` must be finite"):
            call(inv_temp=bad)
    for bad in (-1, 2 ** 64, 1.5, True, None):
        with pytest.raises(ValueError, match=r"`seed` must be an integer in \[0, 2\^64\)"):
            call(seed=bad)
    for ok in (dict(seed=0), dict(seed=2 ** 64 - 1), dict(inv_temp=0.0), dict(inv_temp=0)):
        with pytest.raises(RuntimeError, match="must live on the GPU"):
            call(**ok)
    row = torch.arange(3)
    with pytest.raises(TypeError, match="`row` must be an int64 tensor"):
        ops.gumbel_noise(key, row.int(), 1)
    with pytest.raises(TypeError, match="`user_key` must be an int64 tensor"):
        ops.gumbel_noise(key.int(), row, 1)
    with pytest.raises(ValueError, match="one entry per user"):
        ops.gumbel_noise(key[:2], row, 1)
    with pytest.raises(ValueError, match="`seed`"):
        ops.gumbel_noise(key, row, -3)
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        ops.gumbel_noise(key, row, 1)


def _stand_in(**markers):
    return SimpleNamespace(module=SimpleNamespace(**markers), table=SimpleNamespace(attrs={}, device="cpu"), _row_time=None)


def test_recommend_refuses_a_window_beside_a_sample_and_bad_triples():
    from newsreclib_amd import evaluation as E
    cache = object.__new__(E.NewsVectorCache)
    hist, hs, key = torch.ones(3, dtype=torch.int64), torch.tensor([1, 2]), torch.arange(2)
    lo = torch.zeros(2, dtype=torch.int32)
    with pytest.raises(NotImplementedError, match="tks_scores_kernel"):
        cache.recommend(hist, hs, 2, sample=(1.0, 1, key), window=(lo, lo))
    with pytest.raises(ValueError, match=r"sample = \(inv_temp, seed, user_key\)"):
        cache.recommend(hist, hs, 2, sample=(1.0, 1))
    with pytest.raises(TypeError, match="int64"):
        cache.recommend(hist, hs, 2, sample=(1.0, 1, key.int()))
    with pytest.raises(ValueError, match="one entry per user"):
        cache.recommend(hist, hs, 2, sample=(1.0, 1, torch.arange(3)))
    with pytest.raises(ValueError, match="`inv_temp`"):
        cache.recommend(hist, hs, 2, sample=(-1.0, 1, key))
    with pytest.raises(ValueError, match="`seed`"):
        cache.recommend(hist, hs, 2, sample=(1.0, 2 ** 64, key))


def test_recommend_users_refuses_before_any_device_work():
    from newsreclib_amd import evaluation as E
    plain = _stand_in(dot_product_scorer=True)
    users = [{"hist": [1], "time": 5}]
    with pytest.raises(NotImplementedError, match="TkSelectCapped"):
        E.recommend_users(plain, users, 3, sample=(1.0, 1), cap=("category", 2))
    with pytest.raises(NotImplementedError, match="tkw_walk"):
        E.recommend_users(plain, users, 3, sample=(1.0, 1), window=(24, 0))
    for other in (dict(diversify=(5, 0.5)), dict(calibrate=dict(pool=5, aspect="category", gamma=0.5)), dict(dpp=dict(pool=5))):
        with pytest.raises(ValueError, match="`sample` excludes"):
            E.recommend_users(plain, users, 3, sample=(1.0, 1), **other)
    for marker in ("multi_interest_scorer", "dnn_predictor_scorer", "personalized_pooling_scorer", "class_biased_scorer"):
        with pytest.raises(NotImplementedError, match="tks_scores_kernel") as info:
            E.recommend_users(_stand_in(**{marker: True}), users, 3, sample=(1.0, 1))
        assert marker in str(info.value) and "tkw_scores_kernel" not in str(info.value)
        with pytest.raises(NotImplementedError, match="tks_scores_kernel"):
            E.sample_recommendations(_stand_in(**{marker: True}), users, 3, 2, 1.0, 1)
    manner = SimpleNamespace(module=SimpleNamespace(), table=plain.table, recommend_ensemble=None, _row_time=None)
    with pytest.raises(NotImplementedError, match="MannerVectorCache"):
        E.recommend_users(manner, users, 3, sample=(1.0, 1))
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="temperature must be finite and > 0"):
            E.recommend_users(plain, users, 3, sample=(bad, 1))
    for bad in (-1, 2 ** 64, 0.5):
        with pytest.raises(ValueError, match="seed must be an integer"):
            E.recommend_users(plain, users, 3, sample=(1.0, bad))
    with pytest.raises(ValueError, match=r"sample = \(temperature, seed\)"):
        E.recommend_users(plain, users, 3, sample=(1.0,))
    with pytest.raises(ValueError, match="draws >= 0"):
        E.sample_recommendations(plain, users, 3, -1, 1.0, 1)


def test_sample_recommendations_hands_down_seed_plus_j_and_the_users_ids():
    """A stand-in cache records what ``recommend`` is asked: draw j carries ``(seed + j) mod 2^64``, the inverse temperature, the
    users' ids as keys (``user_id``, or position + 1), batch by batch; the lists land at (user, draw)."""
    from newsreclib_amd import evaluation as E
    asked = []

    def recommend(hist, hs, k, user_idx=None, eligible=None, sample=None):
        inv_temp, seed, keys = sample
        asked.append((inv_temp, seed, keys.tolist(), hs.tolist()))
        idx = (keys[:, None] * 100 + seed % 100 + torch.arange(k)[None, :]).long()
        return idx, idx.float(), torch.zeros(1, dtype=torch.int32)

    cache = _stand_in(dot_product_scorer=True)
    cache.recommend = recommend
    users = [{"hist": [1, 2]}, {"hist": [3], "user_id": 40}, {"hist": [4, 5, 6]}, {"hist": [7]}, {"hist": [8], "user_id": 2 ** 40}]
    seed = 2 ** 64 - 2
    out = E.sample_recommendations(cache, users, 2, 3, 4.0, seed, batch_size=2)
    assert out.shape == (5, 3, 2) and out.dtype == torch.int64 and not out.is_cuda
    seeds = [2 ** 64 - 2, 2 ** 64 - 1, 0]
    want = [(0.25, s, keys, hs) for keys, hs in (([1, 40], [2, 1]), ([3, 4], [3, 1]), ([2 ** 40], [1])) for s in seeds]
    assert asked == want
    ids = [1, 40, 3, 4, 2 ** 40]
    for b, uid in enumerate(ids):
        for j, s in enumerate(seeds):
            assert out[b, j].tolist() == [uid * 100 + s % 100, uid * 100 + s % 100 + 1], (b, j)
    assert E.sample_recommendations(cache, users, 2, 0, 1.0, 1).shape == (5, 0, 2)


def test_only_recommend_takes_a_sample():
    """A policy argument must never be accepted and ignored: ``sample`` is a parameter of ``NewsVectorCache.recommend`` and of no
    other ``recommend*`` / ``rank_clicks*`` of any cache."""
    import inspect

    from newsreclib_amd import evaluation as E
    takes = {(cls.__name__, name) for cls in (E.NewsVectorCache, E.MannerVectorCache, E.NpaFeatureCache)
             for name, fn in inspect.getmembers(cls, inspect.isfunction)
             if name.startswith(("recommend", "rank_clicks")) and "sample" in inspect.signature(fn).parameters}
    assert takes == {("NewsVectorCache", "recommend")}
