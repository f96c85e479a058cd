"""Host tier of the full-catalogue top-k by DKN's factored DNN click predictor (``nrl_dkn_user_query`` / ``nrl_dkn_cand_project`` /
``nrl_topk_relu_scores``, ``ops.topk_relu_scores``, ``NewsVectorCache.recommend_dnn``): ABI surface, host-side refusals (no device
is touched before they return), the Python entry points' refusals, and the fp32 evaluation of the factored score emulated on the
CPU against float64 and the derived bound of tests/topk_dnn_ref.py."""
import ctypes
import json
import os
import re
import subprocess

import pytest
import torch

from tests import topk_dnn_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"nrl_topk_relu_scores": 18, "nrl_dkn_user_query": 9, "nrl_dkn_cand_project": 6}       # declared parameters


def _lib_or_skip():
    from newsreclib_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("library not built")
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in (*NAMES, "nrl_topk_scores_workspace_bytes", "nrl_last_error", "nrl_abi_version"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    return lib


def test_symbols_are_declared_typed_and_exported_without_an_abi_bump():
    from newsreclib_amd import _lib, ops
    header = open(os.path.join(ROOT, "include", "newsreclib_amd.h")).read()
    assert _lib.ABI_VERSION == 19 and re.search(r"#define NRL_ABI_VERSION 19\b", header)
    assert re.search(r"#define NRL_TOPK_MAX_HIDDEN 64\b", header) and ops.TOPK_MAX_HIDDEN == 64
    for name, count in NAMES.items():
        decl = re.search(r"\bint %s\((.*?)\);" % name, header, re.S)
        assert decl and name in _lib.SIGNATURES, name
        params = re.sub(r"/\*.*?\*/", "", decl.group(1), flags=re.S).split(",")
        assert len(params) == count and len(_lib.SIGNATURES[name][1]) == count, name
    assert set(ops.TOPK_FLAGS) == {1, 2, 4, 8}
    # no size function of its own: the set of *_workspace_bytes names is the committed one
    committed = json.load(open(os.path.join(ROOT, "tests", "data", "workspace_sizes.json")))
    sizers = {n for n in _lib.SIGNATURES if n.endswith("_workspace_bytes")}
    assert sizers == {n for n in committed if n.endswith("_workspace_bytes")}
    assert not re.search(r"\bnrl_(topk_relu|dkn_user_query|dkn_cand_project)\w*_workspace_bytes\b", header)
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("library not built")
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(NAMES) <= exported
    assert {n for n in exported if n.endswith("_workspace_bytes")} == sizers
    assert _lib_or_skip().nrl_abi_version() == 19


def test_topk_relu_scores_host_side_refusals_need_no_device():
    lib = _lib_or_skip()
    st = ctypes.c_int32(0)

    def call(B=4, V=100, Hd=16, k=5, slices=0, ws_bytes=1 << 20, status=True, w2=256, b2=256):
        # the device pointers are placeholders, never dereferenced: every refusal below returns before the first launch
        return lib.nrl_topk_relu_scores(256, 256, w2, b2, B, V, Hd, k, None, None, None, slices, 256, 256,
                                        ctypes.addressof(st) if status else None, 256, ws_bytes, None)

    for kw, word in ((dict(Hd=0), "Hd in"), (dict(Hd=65), "Hd in"), (dict(k=0), "k in"), (dict(k=129), "k in"),
                     (dict(V=1 << 31), "2^31"), (dict(B=-1), "negative"), (dict(status=False), "status"), (dict(w2=None), "w2"),
                     (dict(b2=None), "b2")):
        assert call(**kw) == -1, kw
        assert word in lib.nrl_last_error().decode(), (kw, lib.nrl_last_error())
    assert call(B=0) == 0                                 # B == 0: success, nothing launched
    # a short workspace: NRL_E_WORKSPACE (-2), before any launch; the size is the one nrl_topk_scores_workspace_bytes gives at
    # D = 4, whatever Hd (a multiple of 4 or not)
    for B, V, k, slices in ((4, 100, 5, 2), (130, 5000, 128, 0), (7, 65536, 10, 9)):
        need = lib.nrl_topk_scores_workspace_bytes(B, V, 4, k, slices)
        assert need >= B * k * 8
        for Hd in (1, 3, 16, 64):
            assert call(B=B, V=V, Hd=Hd, k=k, slices=slices, ws_bytes=need - 1) == -2, (B, V, Hd)
            assert "workspace too small" in lib.nrl_last_error().decode()


def test_dkn_factor_entries_host_side_refusals_need_no_device():
    from newsreclib_amd._lib import NrlDknClickParams
    lib = _lib_or_skip()

    def params(hidden=16, null=False):
        return NrlDknClickParams(*([None if null else 256] * 8), hidden)

    def query(p, max_hist=10, B=4, dim=24, user=256, q=256, off=256):
        return lib.nrl_dkn_user_query(ctypes.byref(p) if p is not None else None, 256, off, max_hist, B, dim, user, q, None)

    def project(p, N=5, dim=24, rows=256, out=256):
        return lib.nrl_dkn_cand_project(ctypes.byref(p) if p is not None else None, rows, N, dim, out, None)

    for fn in (query, project):
        for kw, word in ((dict(p=None), "null parameter"), (dict(p=params(null=True)), "null parameter"),
                         (dict(p=params(0)), "hidden_dim_dnn"), (dict(p=params(65)), "hidden_dim_dnn"), (dict(p=params(), dim=0), "width"),
                         (dict(p=params(), dim=1025), "width")):
            assert fn(**kw) == -1, (fn.__name__, kw)
            assert word in lib.nrl_last_error().decode(), (fn.__name__, kw, lib.nrl_last_error())
    for kw, word in ((dict(max_hist=1025), "history"), (dict(max_hist=-1), "history"), (dict(B=-1), "batch"), (dict(B=1 << 31), "batch"),
                     (dict(user=None), "user"), (dict(q=None), "q"), (dict(off=None), "hist_offsets")):
        assert query(params(), **kw) == -1, kw
        assert word in lib.nrl_last_error().decode(), (kw, lib.nrl_last_error())
    for kw, word in ((dict(N=-1), "N in"), (dict(N=1 << 31), "N in"), (dict(rows=None), "rows"), (dict(out=None), "out")):
        assert project(params(), **kw) == -1, kw
        assert word in lib.nrl_last_error().decode(), (kw, lib.nrl_last_error())
    assert query(params(), B=0) == 0 and project(params(), N=0) == 0      # nothing to do: success, nothing launched


def test_python_refusals_before_any_device_work():
    from newsreclib_amd import evaluation as E
    from newsreclib_amd import ops
    from newsreclib_amd.dkn_module import DKNModule
    from newsreclib_amd.nrms_module import NRMSModule
    q, proj, w2, b2 = torch.zeros(2, 16), torch.zeros(5, 16), torch.zeros(1, 16), torch.zeros(1)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.topk_relu_scores(q, proj, w2, b2, 3)
    for bad in ((q, torch.zeros(5, 12), w2, b2), (q, proj, torch.zeros(1, 12), b2), (torch.zeros(2, 12), proj, w2, b2),
                (q, proj, w2, torch.zeros(2)), (q.reshape(-1), proj, w2, b2)):
        with pytest.raises(ValueError, match="expected"):
            ops.topk_relu_scores(*bad, 3)
    idx, sizes = torch.tensor([1, 2, 3]), torch.tensor([2, 1])
    cache = E.NewsVectorCache(object.__new__(NRMSModule), None)          # uninitialised: refused before any of it is read
    with pytest.raises(NotImplementedError, match="`recommend`.*`recommend_interests`"):
        cache.recommend_dnn(idx, sizes, 3)
    assert DKNModule.dnn_predictor_scorer is True and not getattr(DKNModule, "dot_product_scorer", False)
    assert not getattr(NRMSModule, "dnn_predictor_scorer", False)
    cache = E.NewsVectorCache(object.__new__(DKNModule), None)
    with pytest.raises(NotImplementedError, match="dot product.*recommend_dnn"):
        cache.recommend(idx, sizes, 3)
    with pytest.raises(RuntimeError, match="no CPU path"):
        cache.recommend_dnn(idx, sizes, 3)
    assert cache.projection is None


def test_fp32_factored_score_stays_inside_the_derived_bound_which_is_not_vacuous():
    """The factored score evaluated in fp32 on the CPU over the inputs of the GPU real-value test, against float64: inside the bound
    that test uses, and the bound is below 1 % of the spread of the scores (their standard deviation), so it cannot be vacuous.  It
    can still exceed the gap between a user's k-th and (k + 1)-th score, which is why the GPU test compares by the floor form."""
    c = R.real_case()
    U = R.user_vectors(c["hist"], c["off"], c["att"])
    assert bool((U[3] == 0).all()) and torch.equal(U[4], c["hist"][int(c["off"][4])])      # the empty and a one-row history
    s64, bound = R.scores64(U, c["table"], c["pred"])
    err = (R.emulate_fp32(U, c["table"], c["pred"]).double() - s64).abs()
    spread = float(s64.std())
    top = torch.sort(s64, dim=1, descending=True)[0]
    gap = float((top[:, R.REAL["k"] - 1] - top[:, R.REAL["k"]]).min())
    print(f"max |fp32 - float64| / bound = {float((err / bound).max()):.2e}; max bound / spread = {float(bound.max()) / spread:.2e}; "
          f"smallest gap between place {R.REAL['k']} and {R.REAL['k'] + 1} = {gap:.2e}, bound there >= {float(bound.min()):.2e}")
    assert bool((err <= bound).all())
    assert float(err.max()) > 0.0
    assert float(bound.max()) / spread < 0.01
