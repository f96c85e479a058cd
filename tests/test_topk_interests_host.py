"""Host tier of the multi-interest full-catalogue top-k (``nrl_topk_interest_scores`` / ``ops.topk_interest_scores`` /
``NewsVectorCache.recommend_interests``): ABI surface, host-side refusals (no device is touched before they return) and the Python
entry points' refusals."""
import ctypes
import json
import os
import re
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "nrl_topk_interest_scores"


def _lib_or_skip():
    from newsreclib_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("library not built")
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in (NAME, "nrl_topk_scores_workspace_bytes", "nrl_last_error", "nrl_abi_version"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    return lib


def test_symbol_is_declared_typed_and_exported_without_an_abi_bump():
    from newsreclib_amd import _lib
    header = open(os.path.join(ROOT, "include", "newsreclib_amd.h")).read()
    assert _lib.ABI_VERSION == 19 and re.search(r"#define NRL_ABI_VERSION 19\b", header)
    assert re.search(r"\bint %s\(" % NAME, header) and NAME in _lib.SIGNATURES
    assert re.search(r"#define NRL_TOPK_MAX_INTERESTS 64\b", header)
    assert len(_lib.SIGNATURES[NAME][1]) == 19
    assert len(_lib.SIGNATURES["nrl_topk_scores"][1]) == 16
    # no size function of its own: the set of *_workspace_bytes names is the committed one
    committed = json.load(open(os.path.join(ROOT, "tests", "data", "workspace_sizes.json")))
    sizers = {n for n in _lib.SIGNATURES if n.endswith("_workspace_bytes")}
    assert sizers == {n for n in committed if n.endswith("_workspace_bytes")}
    assert not re.search(r"\bnrl_topk_interest\w*_workspace_bytes\b", header)
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("library not built")
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert NAME in exported
    assert {n for n in exported if n.endswith("_workspace_bytes")} == sizers
    assert _lib_or_skip().nrl_abi_version() == 19


def test_host_side_refusals_need_no_device():
    lib = _lib_or_skip()
    st = ctypes.c_int32(0)
    ok_gate = 256                                           # a placeholder, never read

    def call(B=4, K=2, V=100, D=8, k=5, mode=0, gate=None, slices=0, ws=256, ws_bytes=1 << 20, status=True):
        # pointers are never dereferenced: every refusal below returns before the first launch
        return lib.nrl_topk_interest_scores(256, gate, 256, B, K, V, D, k, mode, None, None, None, slices, 256, 256,
                                            ctypes.addressof(st) if status else None, ws, ws_bytes, None)

    for kw, word in ((dict(K=0), "K in"), (dict(K=65), "K in"), (dict(mode=3), "mode"), (dict(mode=-1), "mode"),
                     (dict(mode=2, gate=None), "gate"), (dict(k=0), "k in"), (dict(k=129), "k in"), (dict(D=6), "multiple of 4"),
                     (dict(D=1028), "multiple of 4"), (dict(V=1 << 31), "2^31"), (dict(B=-1), "negative")):
        assert call(**kw) == -1, kw
        assert word in lib.nrl_last_error().decode(), (kw, lib.nrl_last_error())
    assert call(B=0) == 0                                   # B == 0: success, nothing launched
    assert call(B=0, mode=2, gate=ok_gate, K=64) == 0
    # a short workspace: NRL_E_WORKSPACE (-2), before any launch, for every K and mode
    need = lib.nrl_topk_scores_workspace_bytes(4, 100, 8, 5, 2)
    for K, mode, gate in ((1, 0, None), (2, 1, None), (64, 2, ok_gate)):
        assert call(K=K, mode=mode, gate=gate, slices=2, ws_bytes=need - 1) == -2, K
        assert "workspace too small" in lib.nrl_last_error().decode()
    # what nrl_topk_scores_workspace_bytes sizes (B in users) is enough whatever K: the size check passes and the next one,
    # the missing status word, is what returns
    need0 = lib.nrl_topk_scores_workspace_bytes(4, 100, 8, 5, 0)
    for K in (1, 64):
        assert call(K=K, ws_bytes=need0, status=False) == -1, K
        assert "status" in lib.nrl_last_error().decode()


def test_existing_workspace_size_covers_every_interest_count():
    """lists(K) = ceil(512 / ceil(B / floor(64 / K))) clamped to [1, tiles] never exceeds the K = 1 count the size function uses:
    checked through the entry itself (the size check precedes the status check) over shapes where the clamp and the ceilings bite."""
    lib = _lib_or_skip()
    for B, V, k, slices in ((1, 100000, 3, 0), (7, 65536, 10, 0), (130, 5000, 128, 0), (513, 1000, 5, 0), (4000, 300, 1, 0),
                            (33, 100000, 7, 9), (64, 129, 2, 0)):
        need = lib.nrl_topk_scores_workspace_bytes(B, V, 8, k, slices)
        for K in (1, 2, 3, 21, 32, 33, 64):
            rc = lib.nrl_topk_interest_scores(256, None, 256, B, K, V, 8, k, 0, None, None, None, slices, 256, 256, None, 256, need,
                                              None)
            assert rc == -1 and "status" in lib.nrl_last_error().decode(), (B, V, k, slices, K)


def test_ops_and_recommend_interests_refusals():
    from newsreclib_amd import ops
    from newsreclib_amd.evaluation import NewsVectorCache
    from newsreclib_amd.miner_module import MINERModule
    from newsreclib_amd.nrms_module import NRMSModule
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.topk_interest_scores(torch.zeros(2, 3, 8), torch.zeros(5, 8), 3, "max")
    cache = NewsVectorCache(object.__new__(NRMSModule), None)
    with pytest.raises(NotImplementedError, match="recommend"):
        cache.recommend_interests(torch.tensor([1, 2, 3]), torch.tensor([2, 1]), 3)
    # before any device work, as `recommend`: host tensors are refused for a MINER cache too
    cache = NewsVectorCache(object.__new__(MINERModule), None)
    with pytest.raises(RuntimeError, match="no CPU path"):
        cache.recommend_interests(torch.tensor([1, 2, 3]), torch.tensor([2, 1]), 3)


def test_miner_is_marked_a_multi_interest_scorer_and_no_dot_product_scorer():
    from newsreclib_amd.miner_module import MINERModule
    from newsreclib_amd.nrms_module import NRMSModule
    assert MINERModule.multi_interest_scorer is True
    assert not getattr(MINERModule, "dot_product_scorer", False)
    assert callable(MINERModule.user_interests)
    assert not getattr(NRMSModule, "multi_interest_scorer", False)
