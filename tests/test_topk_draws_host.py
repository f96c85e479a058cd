"""CPU tier of several Gumbel top-k draws per walk and the class exposure of lists (``nrl_topk_sampled_draws`` /
``nrl_list_class_exposure``): the ABI (header against ``_lib.SIGNATURES`` and, when the library is built, its exports, the workspace
equality and the host-side refusals of the native entries), every argument error of the ``ops`` wrappers and of ``recommend_draws``
before anything looks at a device, the restatement of the exposure sum against a hand computation, and the routing of
``sample_recommendations`` on stand-in caches."""
import ctypes
import os
import re
from types import SimpleNamespace

import pytest
import torch

from tests import topk_draws_ref as DR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("nrl_topk_sampled_draws_workspace_size", "nrl_topk_sampled_draws", "nrl_list_class_exposure")
NRL_OK, NRL_E_INVALID, NRL_E_WORKSPACE = 0, -1, -2


def _header():
    return open(os.path.join(ROOT, "include", "newsreclib_amd.h")).read()


def _declared_arguments(header, name):
    m = re.search(r"\b(?:int|size_t) " + name + r"\(([^;]*)\);", header)
    assert m, name + " is not declared in the header"
    return [a.strip().split()[-1].lstrip("*") for a in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")]


# ---- the ABI --------------------------------------------------------------------------------------------------------------------------
def test_the_entries_are_in_the_header_and_in_the_signatures_without_an_abi_bump():
    from newsreclib_amd import _lib, ops
    header = _header()
    ws, draws, exposure = (_declared_arguments(header, n) for n in NAMES)
    single = _declared_arguments(header, "nrl_topk_sampled_scores")
    assert ws == ["B", "V", "D", "k", "R", "slices"]
    assert draws == ["user_vec", "table", "B", "V", "D", "k", "R", "excl_idx", "excl_off", "eligible", "user_key", "seed", "inv_temp",
                     "slices", "out_idx", "out_key", "out_score", "status", "ws", "ws_bytes", "stream"]
    assert sorted(draws) == sorted(single + ["R"])                 # the single entry's arguments and the number of draws
    assert exposure == ["list_idx", "row_class", "pos_weight", "B", "L", "k", "V", "S", "out", "status", "stream"]
    for name, args in zip(NAMES, (ws, draws, exposure)):
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == len(args), name
    sig = _lib.SIGNATURES["nrl_topk_sampled_draws"][1]
    assert sig[6] is ctypes.c_int32 and sig[11] is ctypes.c_uint64 and sig[12] is ctypes.c_float and sig[19] is ctypes.c_size_t
    assert _lib.SIGNATURES["nrl_topk_sampled_draws_workspace_size"][0] is ctypes.c_size_t
    sig = _lib.SIGNATURES["nrl_list_class_exposure"][1]
    assert [sig[i] for i in (3, 4, 5, 6, 7)] == [ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, ctypes.c_int64, ctypes.c_int32]
    assert _lib.ABI_VERSION == 19 and re.search(r"#define NRL_ABI_VERSION 19\b", header)
    assert re.search(r"#define NRL_TOPK_MAX_DRAWS 32\b", header) and ops.TOPK_MAX_DRAWS == 32
    assert set(ops.EXPOSURE_FLAGS) == {DR.E_ROW, DR.E_CLASS}


def test_the_built_library_exports_the_entries_and_refuses_on_the_host():
    """With a library built: the exports, the workspace equality (R lists of k entries are one list of R k) and the refusals that
    come before any launch, none of which needs a device."""
    from newsreclib_amd import _build, _lib, ops
    assert callable(ops.topk_sampled_draws)
    if not os.path.exists(_build.LIB):
        return                                                   # (nothing built here: the GPU tier loads it)
    data = open(_build.LIB, "rb").read()
    for name in NAMES:
        assert name.encode() + b"\0" in data, name
    lib = _lib.load()
    for B, V, D, k, R, slices in ((512, 65536, 300, 10, 8, 0), (65, 129, 4, 4, 32, 7), (3, 0, 4, 1, 1, 0)):
        assert lib.nrl_topk_sampled_draws_workspace_size(B, V, D, k, R, slices) == lib.nrl_topk_scores_workspace_bytes(B, V, D, R * k, slices)
    assert lib.nrl_topk_sampled_draws_workspace_size(512, 65536, 300, 10, 8, 0) > 512 * 80 * 8
    status = ctypes.c_int32(0)
    buf = (ctypes.c_char * 1024)()
    ws = (ctypes.addressof(buf) + 255) & ~255
    st = ctypes.addressof(status)

    def call(B=2, V=10, D=8, k=2, R=3, key=st, inv_temp=1.0, out=st, ws_bytes=256):
        return lib.nrl_topk_sampled_draws(st, st, B, V, D, k, R, None, None, None, key, 3, inv_temp, 0, out, out, out, st, ws, ws_bytes, None)

    for bad in (dict(R=0), dict(R=33), dict(R=-1), dict(k=43, R=3), dict(k=129, R=1), dict(k=1, R=129), dict(B=0, R=0), dict(B=0, R=33),
                dict(B=0, k=43, R=3), dict(B=2 ** 24, k=16, R=8), dict(inv_temp=float("nan")), dict(inv_temp=-0.5), dict(key=None),
                dict(out=None), dict(k=0), dict(D=6)):
        assert call(**bad) == NRL_E_INVALID, bad
    assert call(ws_bytes=8) == NRL_E_WORKSPACE
    assert call(B=0, key=None, out=None) == NRL_OK          # no users: success without a launch

    def expose(B=2, L=2, k=3, V=5, S=4, lists=st, status_=st):
        return lib.nrl_list_class_exposure(lists, st, st, B, L, k, V, S, st, status_, None)

    for bad in (dict(S=0), dict(S=65), dict(k=0), dict(k=129), dict(L=0), dict(B=-1), dict(B=2 ** 31), dict(status_=None), dict(lists=None)):
        assert expose(**bad) == NRL_E_INVALID, bad
    assert expose(B=0, lists=None) == NRL_OK


# ---- the wrappers' refusals -------------------------------------------------------------------------------------------------------------
def test_the_wrappers_refuse_before_anything_looks_at_a_device():
    from newsreclib_amd import ops
    U, T = torch.zeros(3, 8), torch.zeros(10, 8)
    key = torch.arange(3)

    def call(k=2, draws=3, key=key, seed=1, inv_temp=1.0):
        return ops.topk_sampled_draws(U, T, k, draws, key, seed, inv_temp)

    for bad in (0, 33, -1):
        with pytest.raises(ValueError, match=r"`draws` must be in \[1, 32\]"):
            call(draws=bad)
    for bad in (2.0, True, None, "3"):
        with pytest.raises(TypeError, match="`draws` must be an integer"):
            call(draws=bad)
    for k, draws in ((43, 3), (65, 2), (5, 26), (128, 2)):
        with pytest.raises(ValueError, match=r"`draws \* k` must be at most 128"):
            call(k=k, draws=draws)
    with pytest.raises(TypeError, match="`k` must be an integer"):
        call(k=2.0)
    for bad in (key.int(), key.tolist(), None):
        with pytest.raises(TypeError, match="`user_key` must be an int64 tensor"):
            call(key=bad)
    with pytest.raises(ValueError, match="one entry per user"):
        call(key=key[:2])
    with pytest.raises(ValueError, match="`inv_temp` must be finite"):
        call(inv_temp=float("nan"))
    with pytest.raises(ValueError, match=r"`seed` must be an integer in \[0, 2\^64\)"):
        call(seed=2 ** 64)
    for ok in (dict(), dict(draws=1, k=128), dict(draws=32, k=4), dict(seed=2 ** 64 - 1), dict(inv_temp=0)):
        with pytest.raises(RuntimeError, match="must live on the GPU"):
            call(**ok)

    lists, cls, w = torch.zeros(2, 3, 4, dtype=torch.int64), torch.zeros(9, dtype=torch.int32), torch.ones(4)
    with pytest.raises(TypeError, match="`list_idx` must be an int64 tensor"):
        ops.list_class_exposure(lists.int(), cls, w, 3)
    with pytest.raises(TypeError, match="`row_class` must be an int32 tensor"):
        ops.list_class_exposure(lists, cls.float(), w, 3)
    with pytest.raises(TypeError, match="`pos_weight` must be a float32 tensor"):
        ops.list_class_exposure(lists, cls, w.double(), 3)
    for bad in (0, 65):
        with pytest.raises(ValueError, match=r"`S` must be in \[1, 64\]"):
            ops.list_class_exposure(lists, cls, w, bad)
    for bad in (lists[0, 0], lists[:, :0], lists[:, :, :0], torch.zeros(1, 1, 129, dtype=torch.int64), lists.unsqueeze(0)):
        with pytest.raises(ValueError, match="`list_idx` must"):
            ops.list_class_exposure(bad, cls, torch.ones(bad.shape[-1]), 3)
    with pytest.raises(ValueError, match="`pos_weight` must have one entry per slot"):
        ops.list_class_exposure(lists, cls, torch.ones(5), 3)
    with pytest.raises(ValueError, match="`row_class` must be one-dimensional"):
        ops.list_class_exposure(lists, cls.reshape(3, 3), w, 3)
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        ops.list_class_exposure(lists, cls, w, 3)


def test_recommend_draws_and_exposure_report_refuse_before_any_device_work():
    from newsreclib_amd import evaluation as E
    cache = object.__new__(E.NewsVectorCache)
    hist, hs, key = torch.ones(3, dtype=torch.int64), torch.tensor([1, 2]), torch.arange(2)
    with pytest.raises(ValueError, match="draws >= 1"):
        cache.recommend_draws(hist, hs, 2, 0, (1.0, 1, key))
    with pytest.raises(ValueError, match=r"sample = \(inv_temp, seed, user_key\)"):
        cache.recommend_draws(hist, hs, 2, 3, (1.0, 1))
    with pytest.raises(TypeError, match="int64"):
        cache.recommend_draws(hist, hs, 2, 3, (1.0, 1, key.int()))
    with pytest.raises(ValueError, match="one entry per user"):
        cache.recommend_draws(hist, hs, 2, 3, (1.0, 1, torch.arange(3)))
    with pytest.raises(ValueError, match="`inv_temp`"):
        cache.recommend_draws(hist, hs, 2, 3, (-1.0, 1, key))
    with pytest.raises(ValueError, match="`seed`"):
        cache.recommend_draws(hist, hs, 2, 3, (1.0, 2 ** 64, key))
    users = [{"hist": [1]}]
    plain = SimpleNamespace(module=SimpleNamespace(dot_product_scorer=True), table=SimpleNamespace(attrs={}, device="cpu"), _row_class={})
    for marker in ("multi_interest_scorer", "dnn_predictor_scorer", "personalized_pooling_scorer", "class_biased_scorer"):
        other = SimpleNamespace(module=SimpleNamespace(**{marker: True}), table=plain.table)
        with pytest.raises(NotImplementedError, match="tks_scores_kernel"):
            E.exposure_report(other, users, 3, 2, 1.0, 1, "category")
    with pytest.raises(ValueError, match="temperature must be finite and > 0"):
        E.exposure_report(plain, users, 3, 2, 0.0, 1, "category")
    with pytest.raises(ValueError, match="draws >= 1"):
        E.exposure_report(plain, users, 3, 0, 1.0, 1, "category")
    with pytest.raises(ValueError, match="rbp"):
        E.exposure_report(plain, users, 3, 2, 1.0, 1, "category", weights="linear")
    with pytest.raises(ValueError, match="patience"):
        E.exposure_report(plain, users, 3, 2, 1.0, 1, "category", patience=0.0)
    with pytest.raises(ValueError, match="one entry per slot"):
        E.exposure_report(plain, users, 3, 2, 1.0, 1, "category", weights=torch.ones(4))
    with pytest.raises(ValueError, match="no such `category`"):
        E.exposure_report(plain, users, 3, 2, 1.0, 1, "category")


def test_the_position_weights():
    from newsreclib_amd.evaluation import exposure_weights
    rbp, dcg = exposure_weights(4, "rbp", 0.5), exposure_weights(4, "dcg")
    assert rbp.dtype == torch.float32 and rbp.tolist() == [1.0, 0.5, 0.25, 0.125]
    assert torch.equal(dcg, (1.0 / torch.log2(torch.arange(4, dtype=torch.float64) + 2)).float()) and dcg[0] == 1.0 and dcg[2] == 0.5
    assert torch.equal(exposure_weights(3, "rbp"), torch.tensor([1.0, 0.8, 0.8 ** 2], dtype=torch.float64).float())
    given = torch.tensor([3.0, 2.0, 1.0])
    assert torch.equal(exposure_weights(3, given), given)


# ---- the restatement of the exposure sum ----------------------------------------------------------------------------------------------
def test_the_exposure_restatement_against_a_hand_computation():
    """Two users, two lists of three slots, four rows of classes 0, 1, 1, 5 under S = 3: row 3's class is outside [0, S) (flag, no
    mass), row 9 is outside the table (flag, no mass), -1 is an empty slot (no flag)."""
    cls = torch.tensor([0, 1, 1, 5], dtype=torch.int32)
    w = torch.tensor([1.0, 0.5, 0.25])
    lists = torch.tensor([[[0, 1, 2], [2, 0, -1]], [[3, 9, 1], [-1, -1, -1]]])
    out, status = DR.exposure(lists, cls, w, 3)
    assert status == DR.E_ROW | DR.E_CLASS
    assert out.dtype == torch.float32 and out.tolist() == [[(1.0 + 0.5) / 2, (0.5 + 0.25 + 1.0) / 2, 0.0], [0.0, 0.25 / 2, 0.0]]
    assert DR.exposure(lists[:1], cls, w, 3)[1] == 0
    assert DR.draw_seeds(2 ** 64 - 2, 4) == [2 ** 64 - 2, 2 ** 64 - 1, 0, 1]


# ---- the routing of sample_recommendations ----------------------------------------------------------------------------------------------
def test_sample_recommendations_goes_through_recommend_draws_from_two_draws_on():
    """A stand-in cache with both methods: ``draws >= 2`` asks ``recommend_draws`` once per batch with the first seed, the inverse
    temperature and the users' ids, and never ``recommend``; one draw asks ``recommend`` alone.  The lists land at (user, draw)
    either way, and ``log_probs=True`` still asks ``list_log_probs`` once per draw."""
    from newsreclib_amd import evaluation as E
    asked, single, logs = [], [], []

    def lists_of(keys, seed, k):
        return (keys[:, None] * 100 + seed % 100 + torch.arange(k)[None, :]).long()

    def recommend(hist, hs, k, user_idx=None, eligible=None, sample=None):
        inv_temp, seed, keys = sample
        single.append(seed)
        idx = lists_of(keys, seed, k)
        return idx, idx.float(), torch.zeros(1, dtype=torch.int32)

    def recommend_draws(hist, hs, k, draws, policy, user_idx=None, eligible=None):
        inv_temp, seed, keys = policy
        asked.append((inv_temp, seed, draws, keys.tolist(), hs.tolist()))
        idx = torch.stack([lists_of(keys, (seed + r) % 2 ** 64, k) for r in range(draws)], dim=1)
        return idx, idx.float(), torch.zeros(1, dtype=torch.int32)

    def list_log_probs(hist, hs, lists, inv_temp, user_idx=None, eligible=None):
        logs.append(lists.clone())
        return -lists.float() / 8, None, None, torch.zeros(1, dtype=torch.int32)

    cache = SimpleNamespace(module=SimpleNamespace(dot_product_scorer=True), table=SimpleNamespace(attrs={}, device="cpu"),
                            recommend=recommend, recommend_draws=recommend_draws, list_log_probs=list_log_probs)
    users = [{"hist": [1, 2]}, {"hist": [3], "user_id": 40}, {"hist": [4, 5, 6]}]
    seed = 2 ** 64 - 2
    out = E.sample_recommendations(cache, users, 2, 3, 4.0, seed, batch_size=2)
    assert asked == [(0.25, seed, 3, [1, 40], [2, 1]), (0.25, seed, 3, [3], [3])] and not single
    for b, uid in enumerate([1, 40, 3]):
        for j, s in enumerate([seed, seed + 1, 0]):
            assert out[b, j].tolist() == [uid * 100 + s % 100, uid * 100 + s % 100 + 1], (b, j)
    lists, logp = E.sample_recommendations(cache, users, 2, 3, 4.0, seed, batch_size=2, log_probs=True)
    assert torch.equal(lists, out) and len(logs) == 6 and torch.equal(logp, -lists.float() / 8) and not single
    assert torch.equal(torch.stack(logs[:3], dim=1), out[:2])
    one = E.sample_recommendations(cache, users, 2, 1, 4.0, seed, batch_size=2)
    assert single == [seed, seed] and len(asked) == 4 and torch.equal(one, out[:, :1])
