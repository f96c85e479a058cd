"""Host tier of the full-catalogue top-k by NPA's personalized-pooling score (``nrl_topk_pooled_scores``,
``ops.topk_pooled_scores``, ``NpaFeatureCache.recommend_pooled``): ABI surface, host-side refusals (no device is touched before they
return), the Python entry points' refusals, and the fp32 online-softmax evaluation of the score emulated on the CPU against float64
and the derived bound of tests/topk_npa_ref.py."""
import ctypes
import json
import os
import re
import subprocess

import pytest
import torch

from tests import topk_npa_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME, COUNT = "nrl_topk_pooled_scores", 18                  # declared parameters


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
    from newsreclib_amd import _lib, ops
    header = open(os.path.join(ROOT, "include", "newsreclib_amd.h")).read()
    assert _lib.ABI_VERSION == 19 and re.search(r"#define NRL_ABI_VERSION 19\b", header)
    assert re.search(r"#define NRL_TOPK_MAX_TOKENS 128\b", header) and ops.TOPK_MAX_TOKENS == 128
    decl = re.search(r"\bint %s\((.*?)\);" % NAME, header, re.S)
    assert decl and NAME in _lib.SIGNATURES
    params = re.sub(r"/\*.*?\*/", "", decl.group(1), flags=re.S).split(",")
    assert len(params) == COUNT and len(_lib.SIGNATURES[NAME][1]) == COUNT
    assert set(ops.TOPK_FLAGS) == {1, 2, 4, 8}
    # no size function of its own: the set of *_workspace_bytes names is the committed one
    committed = json.load(open(os.path.join(ROOT, "tests", "data", "workspace_sizes.json")))
    sizers = {n for n in _lib.SIGNATURES if n.endswith("_workspace_bytes")}
    assert sizers == {n for n in committed if n.endswith("_workspace_bytes")}
    assert not re.search(r"\bnrl_topk_pooled\w*_workspace_bytes\b", header)
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("library not built")
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert NAME in exported
    assert {n for n in exported if n.endswith("_workspace_bytes")} == sizers
    assert _lib_or_skip().nrl_abi_version() == 19


def test_topk_pooled_scores_host_side_refusals_need_no_device():
    lib = _lib_or_skip()
    st = ctypes.c_int32(0)

    def call(B=4, V=100, L=30, F=16, k=5, slices=0, ws_bytes=1 << 20, status=True, q=256, user=256, features=256):
        # the device pointers are placeholders, never dereferenced: every refusal below returns before the first launch
        return lib.nrl_topk_pooled_scores(q, user, features, B, V, L, F, k, None, None, None, slices, 256, 256,
                                          ctypes.addressof(st) if status else None, 256, ws_bytes, None)

    for kw, word in ((dict(L=0), "L in"), (dict(L=129), "L in"), (dict(F=0), "F a multiple"), (dict(F=6), "F a multiple"),
                     (dict(F=1028), "F a multiple"), (dict(k=0), "k in"), (dict(k=129), "k in"), (dict(V=1 << 31), "2^31"),
                     (dict(B=-1), "negative"), (dict(status=False), "status"), (dict(q=None), "null"), (dict(user=None), "null"),
                     (dict(features=None), "null")):
        assert call(**kw) == -1, kw
        assert word in lib.nrl_last_error().decode(), (kw, lib.nrl_last_error())
    assert call(q=260) == -1 and "16-byte aligned" in lib.nrl_last_error().decode()
    assert call(B=0) == 0                                 # B == 0: success, nothing launched
    # a short workspace: NRL_E_WORKSPACE (-2), before any launch; the size is the one nrl_topk_scores_workspace_bytes gives at
    # D = 4, whatever L and F
    for B, V, k, slices in ((4, 100, 5, 2), (130, 5000, 128, 0), (7, 65536, 10, 9)):
        need = lib.nrl_topk_scores_workspace_bytes(B, V, 4, k, slices)
        assert need >= B * k * 8
        for L, F in ((1, 4), (30, 400), (128, 1024)):
            assert call(B=B, V=V, L=L, F=F, k=k, slices=slices, ws_bytes=need - 1) == -2, (B, V, L, F)
            assert "workspace too small" in lib.nrl_last_error().decode()


def test_python_refusals_before_any_device_work():
    from newsreclib_amd import evaluation as E
    from newsreclib_amd import ops
    from newsreclib_amd.caum_module import CAUMModule
    from newsreclib_amd.dkn_module import DKNModule
    from newsreclib_amd.miner_module import MINERModule
    from newsreclib_amd.npa_module import NPAModule
    from newsreclib_amd.nrms_module import NRMSModule
    q, user, feat = torch.zeros(2, 16), torch.zeros(2, 16), torch.zeros(5, 3, 16)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.topk_pooled_scores(q, user, feat, 3)
    for bad in ((q, user, torch.zeros(5, 3, 12)), (q, torch.zeros(2, 12), feat), (q, torch.zeros(3, 16), feat),
                (torch.zeros(2, 12), user, feat), (q, user, torch.zeros(5, 16)), (q.reshape(-1), user, feat)):
        with pytest.raises(ValueError, match="expected"):
            ops.topk_pooled_scores(*bad, 3)
    assert NPAModule.personalized_pooling_scorer is True and not getattr(NPAModule, "dot_product_scorer", False)
    for other in (NRMSModule, DKNModule, MINERModule, CAUMModule):
        assert not getattr(other, "personalized_pooling_scorer", False), other
    idx, sizes = torch.tensor([1, 2, 3]), torch.tensor([2, 1])
    cache = E.NpaFeatureCache(object.__new__(NPAModule), None)           # uninitialised: refused before any of it is read
    with pytest.raises(NotImplementedError, match="depend on the user.*recommend_pooled"):
        cache.recommend(idx, sizes, 3)
    with pytest.raises(ValueError, match="NpaFeatureCache.recommend_pooled needs user_idx: NPA's attention queries come from the "
                                         "user embedding"):
        cache.recommend_pooled(idx, sizes, 3)
    with pytest.raises(RuntimeError, match="no CPU path"):
        cache.recommend_pooled(idx, sizes, 3, user_idx=torch.tensor([0, 1]))
    assert cache.features is None


def test_fp32_online_score_stays_inside_the_derived_bound_which_is_not_vacuous():
    """The online-softmax form evaluated in fp32 on the CPU over the inputs of the GPU real-value test, against float64: inside the
    bound that test uses, and the bound is below 5 % of the spread of the scores (their standard deviation; the construction gives
    about 2 %), so it cannot be vacuous.  It can still exceed the gap between a user's k-th and (k + 1)-th score, which is why the GPU
    test compares by the floor form."""
    c = R.real_case()
    s64, bound = c["raw"], c["bound"]
    err = (R.emulate_fp32(c["q"], c["user"], c["feat"]).double() - s64).abs()
    spread = float(s64.std())
    top = torch.sort(s64, dim=1, descending=True)[0]
    gap = float((top[:, R.REAL["k"] - 1] - top[:, R.REAL["k"]]).min())
    print(f"max |fp32 - float64| / bound = {float((err / bound).max()):.2e}; max bound / spread = {float(bound.max()) / spread:.2e}; "
          f"smallest gap between place {R.REAL['k']} and {R.REAL['k'] + 1} = {gap:.2e}, bound there >= {float(bound.min()):.2e}")
    assert bool((err <= bound).all())
    assert float(err.max()) > 0.0
    assert float(bound.max()) / spread < 0.05


@pytest.mark.parametrize("n", [1, 2, 4, 8])
def test_fp32_online_score_is_exact_on_the_exact_family(n):
    q, user, feat, s64 = R.exact_case(40 + n, 130, 1000, 30, 24, (n,))
    got = R.emulate_fp32(q, user, feat)
    distinct = sum(len(set(row.tolist())) for row in s64) / s64.shape[0]
    print(f"n = {n}: {distinct:.0f} distinct values per user over {s64.shape[1]} rows")
    assert torch.equal(got.double(), s64)
    assert distinct < s64.shape[1] / 2                      # ties
