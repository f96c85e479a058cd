"""CPU tier of the device-side streaming metrics (ABI v19): the entry points are declared, bound and exported; the Python layer
refuses host tensors (there is no eager fallback); every opt-in defaults to off."""
import inspect
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("nrl_impression_metrics_workspace_bytes", "nrl_impression_metrics")


def test_metrics_entry_points_are_declared_bound_and_exported():
    from newsreclib_amd import _build, _lib
    _build.build(verbose=False)
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "newsreclib_amd.h")).read()
    declared = set(re.findall(r"\b(nrl_[a-z0-9_]+)\s*\(", header))
    for name in SYMBOLS:
        assert name in declared, f"{name} is not declared in the header"
        assert name in _lib.SIGNATURES, f"{name} has no ctypes signature"
        assert hasattr(lib, name), f"{name} is not exported by the library"
    assert "#define NRL_ABI_VERSION 19" in header
    assert _lib.ABI_VERSION == 19 and lib.nrl_abi_version() == 19
    # the translation unit is picked up by the glob of the build
    assert "nrl_metrics.hip" in _build.sources()


def test_workspace_size_and_host_side_argument_checks_need_no_gpu():
    from newsreclib_amd import _lib
    lib = _lib.load()
    small, big = lib.nrl_impression_metrics_workspace_bytes(100, 8, 0, 2), lib.nrl_impression_metrics_workspace_bytes(100000, 4097, 2, 4)
    assert small >= 100 * 4 + 8 * 3 * 4 and small % 256 == 0
    assert big >= 100000 * 4 + 4097 * 21 * 4 + 4097 * 4 + 2 * 22 * 8 and big > small
    # B == 0 succeeds without touching a device; limits are refused on the host before any launch
    import ctypes
    ks = (ctypes.c_int32 * 2)(5, 10)
    status = 0x1000                      # a non-null stand-in: the call returns before it is read
    assert lib.nrl_impression_metrics(None, None, None, 0, 0, 0, None, None, 0, None, None, 0, None, 0, ks, 2, None, None, None, None,
                                      status, None, 0, None) == 0
    for bad_k in ((0, 5), (5, 1025)):
        ks = (ctypes.c_int32 * 2)(*bad_k)
        assert lib.nrl_impression_metrics(None, None, None, 0, 0, 0, None, None, 0, None, None, 0, None, 0, ks, 2, None, None, None,
                                          None, status, None, 0, None) == -1
        assert b"every k in" in lib.nrl_last_error()
    assert lib.nrl_impression_metrics(None, None, None, 0, 0, 3, None, None, 0, None, None, 0, None, 0, ks, 0, None, None, None, None,
                                      status, None, 0, None) == -1
    assert lib.nrl_impression_metrics(None, None, None, 0, 0, 0, None, None, 0, None, None, 0, None, 0, ks, 5, None, None, None, None,
                                      status, None, 0, None) == -1


def test_python_layer_refuses_host_tensors():
    from newsreclib_amd import metrics, ops
    preds, targets = torch.tensor([0.3, 0.1, 0.7]), torch.tensor([0.0, 1.0, 0.0])
    sizes = torch.tensor([3])
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.impression_metrics(preds, targets, torch.tensor([0, 3]), (5,))
    with pytest.raises(RuntimeError, match="no CPU path"):
        metrics.impression_metrics(preds, targets, sizes, (5,))
    empty = torch.empty(0, dtype=torch.int64)
    step = (torch.tensor(0.0), preds, targets, sizes, torch.tensor([2]), empty, empty, empty, empty, torch.tensor([1]), empty)
    sm = metrics.StreamingMetrics((5, 10), 18, 4)
    with pytest.raises(RuntimeError, match="no CPU path"):
        sm.update(step)
    assert sm.compute() == {}            # nothing was accumulated


def test_streaming_metrics_column_names_are_the_existing_keys():
    from newsreclib_amd import metrics, ops
    preds, targets = torch.tensor([0.9, 0.1, 0.5, 0.2]), torch.tensor([1.0, 0.0, 0.0, 1.0])
    sizes, hsz = torch.tensor([2, 2]), torch.tensor([1, 2])
    ca, ha = torch.tensor([1, 2, 0, 1]), torch.tensor([1, 2, 2])
    want = set(metrics.ranking_metrics(preds, targets, sizes, (5, 10))) - {"auc"}
    want |= set(metrics.aspect_metrics(preds, ca, ha, sizes, hsz, 4, (5, 10), prefix="categ"))
    want |= set(metrics.aspect_metrics(preds, ca, ha, sizes, hsz, 4, (5, 10), prefix="sent"))
    cols = ops.metrics_columns((5, 10), ("categ", "sent"))
    assert set(cols) == want and len(cols) == len(want) == 1 + 2 + 2 * 4


def test_opt_ins_default_to_off():
    from newsreclib_amd.abstract_recommender import AbstractRecommender
    from newsreclib_amd.evaluation import evaluate_impressions
    assert AbstractRecommender.device_metrics is False
    assert inspect.signature(evaluate_impressions).parameters["device_metrics"].default is False
    for cls in AbstractRecommender.__subclasses__():
        assert "device_metrics" not in inspect.signature(cls.__init__).parameters      # a class attribute, not a keyword
