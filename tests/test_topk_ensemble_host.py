"""Host tier of the z-scored ensemble full-catalogue top-k (``nrl_topk_ensemble_scores`` / ``ops.topk_ensemble_scores`` /
``MannerVectorCache.recommend_ensemble``): ABI surface, host-side refusals (no device is touched before they return), the Python
entry points' refusals, and the fp32 statistics order emulated on the CPU against float64 and the derived bound."""
import ctypes
import json
import os
import re
import subprocess

import pytest
import torch

from tests import catalogue_ref as C
from tests import topk_ensemble_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "nrl_topk_ensemble_scores"


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
    decl = re.search(r"\bint %s\((.*?)\);" % NAME, header, re.S)
    assert decl and NAME in _lib.SIGNATURES
    for define in (r"NRL_TOPK_E_STATS 8", r"NRL_TOPK_MAX_MODELS 3", r"NRL_TOPK_STAT_CHUNKS 64"):
        assert re.search(r"#define %s\b" % define, header), define
    # one argument type per parameter of the declaration (20: the three host arrays, T, the sixteen of nrl_topk_scores less
    # user_vec / table, out_stats and moments)
    params = re.sub(r"/\*.*?\*/", "", decl.group(1), flags=re.S).split(",")
    assert len(params) == 20 and len(_lib.SIGNATURES[NAME][1]) == len(params)
    assert 8 in ops.TOPK_FLAGS and "standardised" in ops.TOPK_FLAGS[8] and set(ops.TOPK_FLAGS) == {1, 2, 4, 8}
    # no size function of its own: the set of *_workspace_bytes names is the committed one
    committed = json.load(open(os.path.join(ROOT, "tests", "data", "workspace_sizes.json")))
    sizers = {n for n in _lib.SIGNATURES if n.endswith("_workspace_bytes")}
    assert sizers == {n for n in committed if n.endswith("_workspace_bytes")}
    assert not re.search(r"\bnrl_topk_ensemble\w*_workspace_bytes\b", header)
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
    wts = (ctypes.c_float * 4)(1.0, 0.2, -0.25, 0.0)

    def call(T=3, B=4, V=100, D=8, k=5, slices=0, ws_bytes=1 << 20, status=True, stats=256, moments=256, null_table=None):
        # the device pointers are placeholders, never dereferenced: every refusal below returns before the first launch.  The two
        # pointer arrays are host arrays and are read
        users = (ctypes.c_void_p * 4)(256, 256, 256, 256)
        tables = (ctypes.c_void_p * 4)(*[None if t == null_table else 256 for t in range(4)])
        return lib.nrl_topk_ensemble_scores(users, tables, wts, T, B, V, D, k, None, None, None, slices, 256, 256, stats, moments,
                                            ctypes.addressof(st) if status else None, 256, ws_bytes, None)

    for kw, word in ((dict(T=0), "T in"), (dict(T=4), "T in"), (dict(null_table=1), "sub-model 1"), (dict(k=0), "k in"),
                     (dict(k=129), "k in"), (dict(D=6), "multiple of 4"), (dict(V=1 << 31), "2^31"), (dict(B=-1), "negative"),
                     (dict(status=False), "status"), (dict(stats=None), "out_stats"), (dict(moments=None), "moments")):
        assert call(**kw) == -1, kw
        assert word in lib.nrl_last_error().decode(), (kw, lib.nrl_last_error())
    assert call(T=2, null_table=2, ws_bytes=0) == -2        # only the first T entries are read: the next refusal is the workspace
    assert call(B=0) == 0                                 # B == 0: success, nothing launched
    # a short workspace: NRL_E_WORKSPACE (-2), before any launch; the size is the one nrl_topk_scores_workspace_bytes gives
    for B, V, D, k, slices in ((4, 100, 8, 5, 2), (130, 5000, 768, 128, 0), (7, 65536, 8, 10, 9)):
        need = lib.nrl_topk_scores_workspace_bytes(B, V, D, k, slices)
        for T in (1, 3):
            assert call(T=T, B=B, V=V, D=D, k=k, slices=slices, ws_bytes=need - 1) == -2, (T, B, V)
            assert "workspace too small" in lib.nrl_last_error().decode()


def test_ops_and_recommend_ensemble_refusals():
    from newsreclib_amd import ops
    from newsreclib_amd.evaluation import MannerVectorCache
    u, t = torch.zeros(2, 8), torch.zeros(5, 8)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.topk_ensemble_scores([u, u], [t, t], [1.0, 0.2], 3)
    with pytest.raises(ValueError, match="one shape"):
        ops.topk_ensemble_scores([u, u], [t, torch.zeros(6, 8)], [1.0, 0.2], 3)
    with pytest.raises(ValueError, match="one shape"):
        ops.topk_ensemble_scores([u, torch.zeros(2, 4)], [t, t], [1.0, 0.2], 3)
    with pytest.raises(ValueError, match="sub-models"):
        ops.topk_ensemble_scores([u] * 4, [t] * 4, [1.0] * 4, 3)
    with pytest.raises(ValueError, match="sub-models"):
        ops.topk_ensemble_scores([u] * 2, [t] * 2, [1.0], 3)
    cache = object.__new__(MannerVectorCache)               # uninitialised: refused before any of it is read
    with pytest.raises(RuntimeError, match="no CPU path"):
        cache.recommend_ensemble(torch.tensor([1, 2, 3]), torch.tensor([2, 1]), 3)
    with pytest.raises(NotImplementedError, match="z-scores"):
        cache.recommend(torch.tensor([1, 2, 3]), torch.tensor([2, 1]), 3)


def test_recommend_users_takes_recommend_ensemble_where_the_cache_has_one():
    from newsreclib_amd.evaluation import MannerVectorCache, NewsVectorCache
    assert callable(MannerVectorCache.recommend_ensemble) and not hasattr(NewsVectorCache, "recommend_ensemble")


@pytest.mark.parametrize("V", R.STATS_V)
@pytest.mark.parametrize("D", R.STATS_D)
def test_fp32_statistics_in_the_prescribed_order_stay_inside_the_derived_bound(V, D):
    """The tile -> chunk -> user order of the kernels, emulated in fp32 on the CPU over the inputs of the GPU statistics test,
    against float64: inside the bound those tests use, and the bound is below 1 % of sd, so it cannot be vacuous."""
    users, tables, eligible, excl = R.stats_case(V, D)
    pop = C.allowed(R.STATS_B, V, excl, eligible)
    worst = 0.0
    for t, (s, bs, n, mean, sd) in enumerate(R.stats64(users, tables, pop)):
        dmu, dsd = R.stat_bounds(s, bs, n, sd, pop, V)
        em, esd = R.emulate_stats(users[t] @ tables[t].T, pop)
        ok = n >= 2
        assert bool(torch.isnan(esd[~ok]).all())
        if not bool(ok.any()):
            continue
        rel = torch.maximum(dmu[ok], dsd[ok]) / sd[ok]
        worst = max(worst, float(rel.max()))
        print(f"V = {V}, D = {D}, t = {t}: |mean - float64| / dmu <= {float(((em.double() - mean).abs() / dmu)[ok].max()):.2e}, "
              f"|sd - float64| / dsd <= {float(((esd.double() - sd).abs() / dsd)[ok].max()):.2e}, bound / sd <= {float(rel.max()):.2e}")
        assert bool(((em.double() - mean).abs() <= dmu)[ok].all())
        assert bool(((esd.double() - sd).abs() <= dsd)[ok].all())
        assert float(rel.max()) < 0.01
    assert V == 2 or worst > 0.0
