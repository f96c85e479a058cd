"""Host tier of the full-catalogue rank of held-out clicks under the MINER, DKN and NPA scorers (``nrl_catalogue_interest_ranks`` /
``nrl_catalogue_relu_ranks`` / ``nrl_catalogue_pooled_ranks``): ABI surface, host-side refusals (no device is touched before they return), the Python entries'
refusals, and the condition the GPU tier's interval check rests on, asserted on the reference alone."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from tests import catalogue_ref as C
from tests import catalogue_rank_scorers_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"nrl_catalogue_interest_ranks": 22, "nrl_catalogue_relu_ranks": 21, "nrl_catalogue_pooled_ranks": 21}      # parameters


def _lib_or_skip():
    from newsreclib_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("library not built")
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in tuple(NAMES) + ("nrl_catalogue_ranks_workspace_size", "nrl_last_error", "nrl_abi_version"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    return lib


def test_symbols_are_declared_typed_and_exported_without_an_abi_bump():
    from newsreclib_amd import _lib, ops
    header = open(os.path.join(ROOT, "include", "newsreclib_amd.h")).read()
    assert _lib.ABI_VERSION == 19 and re.search(r"#define NRL_ABI_VERSION 19\b", header)
    for name, n_args in NAMES.items():
        decl = re.search(r"\bint %s\(([^;]*)\);" % name, header)
        assert decl and name in _lib.SIGNATURES
        args = re.sub(r"/\*.*?\*/", "", decl.group(1), flags=re.S)
        assert len(args.split(",")) == n_args == len(_lib.SIGNATURES[name][1]), name
    assert callable(ops.catalogue_interest_ranks) and callable(ops.catalogue_relu_ranks) and callable(ops.catalogue_pooled_ranks)
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("library not built")
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(NAMES) <= exported
    assert _lib_or_skip().nrl_abi_version() == 19


P = 256                                                      # a placeholder pointer: never read, every refusal is before a launch


def _refusals(lib, call, bad_shapes):
    for kwargs, word in bad_shapes + [(dict(B=-1), "negative"), (dict(V=-2), "negative"), (dict(n=-3), "negative"),
                                      (dict(slices=-1), "negative"), (dict(V=1 << 31), "2^31"), (dict(n=1 << 31), "2^31")]:
        assert call(**kwargs) == -1, kwargs
        assert word in lib.nrl_last_error().decode(), (kwargs, lib.nrl_last_error())
    assert call(status=False) == -1 and "status" in lib.nrl_last_error().decode()
    assert call(tgt_off=None) == -1 and "tgt_idx without tgt_off" in lib.nrl_last_error().decode()
    assert call(n=0, tgt_off=None) == -1 and "tgt_idx without tgt_off" in lib.nrl_last_error().decode()
    assert call(B=0) == 0                                    # B == 0: success, nothing launched
    assert call(ws=None) == -1 and "workspace" in lib.nrl_last_error().decode()


def test_interest_ranks_host_side_refusals_need_no_device():
    lib = _lib_or_skip()
    st = ctypes.c_int32(0)

    def call(B=4, K=3, V=100, D=8, mode=0, n=3, slices=0, gate=None, tgt_idx=P, tgt_off=P, status=True, ws=P, ws_bytes=1 << 20):
        return lib.nrl_catalogue_interest_ranks(P, gate, P, B, K, V, D, mode, tgt_idx, tgt_off, n, None, None, None, slices, P, P, P,
                                                ctypes.addressof(st) if status else None, ws, ws_bytes, None)

    _refusals(lib, call, [(dict(K=0), "K in [1, 64]"), (dict(K=65), "K in [1, 64]"), (dict(mode=3), "mode"), (dict(mode=-1), "mode"),
                          (dict(mode=2), "gate"), (dict(D=6), "multiple of 4"), (dict(D=1028), "multiple of 4")])
    # (one table tile: the plan of 64 / K users per workgroup has the slices of the size function's, so the sizes agree)
    need = lib.nrl_catalogue_ranks_workspace_size(4, 100, 8, 3, 0)
    assert call(ws_bytes=need - 1) == -2 and "workspace too small" in lib.nrl_last_error().decode()


def test_relu_ranks_host_side_refusals_need_no_device():
    lib = _lib_or_skip()
    st = ctypes.c_int32(0)

    def call(B=4, V=100, Hd=6, n=3, slices=0, w2=P, b2=P, tgt_idx=P, tgt_off=P, status=True, ws=P, ws_bytes=1 << 20):
        return lib.nrl_catalogue_relu_ranks(P, P, w2, b2, B, V, Hd, tgt_idx, tgt_off, n, None, None, None, slices, P, P, P,
                                            ctypes.addressof(st) if status else None, ws, ws_bytes, None)

    _refusals(lib, call, [(dict(Hd=0), "Hd in [1, 64]"), (dict(Hd=65), "Hd in [1, 64]"), (dict(w2=None), "w2"),
                          (dict(b2=None), "b2")])
    need = lib.nrl_catalogue_ranks_workspace_size(4, 100, 4, 3, 0)
    assert call(ws_bytes=need - 1) == -2 and "workspace too small" in lib.nrl_last_error().decode()


def test_pooled_ranks_host_side_refusals_need_no_device():
    lib = _lib_or_skip()
    st = ctypes.c_int32(0)

    def call(B=4, V=100, L=5, F=8, n=3, slices=0, q=P, tgt_idx=P, tgt_off=P, status=True, ws=P, ws_bytes=1 << 20):
        return lib.nrl_catalogue_pooled_ranks(q, P, P, B, V, L, F, tgt_idx, tgt_off, n, None, None, None, slices, P, P, P,
                                              ctypes.addressof(st) if status else None, ws, ws_bytes, None)

    _refusals(lib, call, [(dict(L=0), "L in [1, 128]"), (dict(L=129), "L in [1, 128]"), (dict(F=6), "multiple of 4"),
                          (dict(F=0), "multiple of 4"), (dict(F=1028), "multiple of 4"), (dict(q=P + 4), "16-byte aligned")])
    # the workspace does not grow with the feature maps: nothing is gathered
    need = lib.nrl_catalogue_ranks_workspace_size(4, 100, 4, 3, 0)
    assert call(L=128, F=1024, ws_bytes=need - 1) == -2 and "workspace too small" in lib.nrl_last_error().decode()


def test_python_entries_refuse_before_any_device_work():
    from newsreclib_amd import evaluation as E
    from newsreclib_amd import ops
    from newsreclib_amd.dkn_module import DKNModule
    from newsreclib_amd.miner_module import MINERModule
    from newsreclib_amd.nrms_module import NRMSModule
    ti, to = torch.tensor([1]), torch.tensor([0, 1, 1])
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.catalogue_interest_ranks(torch.zeros(2, 3, 8), torch.zeros(5, 8), ti, to, "max")
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.catalogue_relu_ranks(torch.zeros(2, 6), torch.zeros(5, 6), torch.zeros(6), torch.zeros(1), ti, to)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.catalogue_pooled_ranks(torch.zeros(2, 8), torch.zeros(2, 8), torch.zeros(5, 3, 8), ti, to)
    from newsreclib_amd.npa_module import NPAModule
    pooled = E.NpaFeatureCache(object.__new__(NPAModule), None).rank_clicks_pooled
    with pytest.raises(ValueError, match="needs user_idx"):
        pooled(torch.tensor([1, 2, 3]), torch.tensor([2, 1]), torch.tensor([4]), torch.tensor([1, 0]))
    with pytest.raises(ValueError, match="rank_clicks_pooled takes at most 32 clicks"):
        pooled(torch.tensor([1, 2, 3]), torch.tensor([2, 1]), torch.ones(33, dtype=torch.int64), torch.tensor([33, 0]),
               user_idx=torch.tensor([0, 1]))
    with pytest.raises(RuntimeError, match="no CPU path"):
        pooled(torch.tensor([1, 2, 3]), torch.tensor([2, 1]), torch.tensor([4]), torch.tensor([1, 0]), user_idx=torch.tensor([0, 1]))
    # the cache methods: more than 32 clicks a user (from the host sizes), CPU index lists, the wrong family
    hist, hs, many = torch.tensor([1, 2, 3]), torch.tensor([2, 1]), torch.tensor([33, 0])
    for cls, name in ((MINERModule, "rank_clicks_interests"), (DKNModule, "rank_clicks_dnn")):
        method = getattr(E.NewsVectorCache(object.__new__(cls), None), name)
        with pytest.raises(ValueError, match="%s takes at most 32 clicks" % name):
            method(hist, hs, torch.ones(33, dtype=torch.int64), many)
        with pytest.raises(ValueError, match="one entry per user"):
            method(hist, hs, torch.tensor([4]), torch.tensor([1]))
        with pytest.raises(RuntimeError, match="no CPU path"):
            method(hist, hs, torch.tensor([4]), torch.tensor([1, 0]))
        with pytest.raises(NotImplementedError, match="served by `rank_clicks`"):
            getattr(E.NewsVectorCache(object.__new__(NRMSModule), None), name)(hist, hs, torch.tensor([4]), torch.tensor([1, 0]))


def _share_decided(s, bound, targets, excl):
    intervals = C.rank_intervals(s, bound, C.population(s, excl)[0], targets)
    valid = [iv for iv in intervals if iv is not None]
    return sum(lo == hi for lo, hi in valid) / len(valid), len(valid)


def test_the_rank_intervals_of_the_real_cases_are_not_vacuous():
    """The GPU tier asserts ``lo <= rank <= hi``; here, on the reference alone: ``lo == hi`` for at least 90 % of the valid targets
    of every real-valued case, so that check pins the rank itself nearly everywhere."""
    c = R.real_miner()
    for mode in R.MODES:
        s, bound = R.interest_scores64(c["E"], c["T"], mode, c["G"])
        share, n = _share_decided(s, bound, c["targets"], c["excl"])
        print(f"MINER {mode}: lo == hi for {share:.3f} of {n} valid targets")
        assert n >= 20 and share >= 0.9, mode
    d = R.real_dkn()
    share, n = _share_decided(d["s"], d["bound"], d["targets"], d["excl"])
    print(f"DKN: lo == hi for {share:.3f} of {n} valid targets")
    assert n >= 40 and share >= 0.9
    p = R.real_npa()
    share, n = _share_decided(p["s"], p["bound"], p["targets"], p["excl"])
    print(f"NPA: lo == hi for {share:.3f} of {n} valid targets")
    assert n >= 20 and share >= 0.9


def test_the_integer_cases_are_exact_in_fp32():
    """What the GPU tier's ``torch.equal`` comparisons rest on: with entries in [-4, 4] every dot product, every sum over K and every
    relu chain is an integer below 2^24, and a mean over K = 3 is a correctly rounded quotient whose float64 value rounds to the same
    fp32 (n / 3 is never a tie) and orders as the sums do."""
    g = torch.Generator().manual_seed(1)
    E, T = torch.randint(-4, 5, (5, 3, 36), generator=g).float(), torch.randint(-4, 5, (130, 36), generator=g).float()
    s32 = torch.einsum("bkd,vd->bkv", E, T).sum(dim=1)
    assert float(s32.abs().max()) < 2 ** 24 and torch.equal(s32.double(), torch.einsum("bkd,vd->bkv", E.double(), T.double()).sum(dim=1))
    assert torch.equal(s32 / 3.0, (s32.double() / 3).float())
    q, proj = torch.randint(-4, 5, (6, 64), generator=g).float(), torch.randint(-4, 5, (300, 64), generator=g).float()
    w2, b2 = torch.randint(-3, 4, (64,), generator=g).float(), torch.tensor([2.0])
    s = R.DR.relu_scores64(q, proj, w2, b2)
    assert float(s.abs().max()) <= 64 * 3 * 8 + 2 and torch.equal(s, s.round())
