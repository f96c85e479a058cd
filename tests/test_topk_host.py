"""Host tier of the full-catalogue top-k recommendation: ABI surface, workspace sizing, host-side refusals (no device is touched
before they return), the Python entry points' refusals and the recommendation dictionary."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("nrl_topk_scores_workspace_bytes", "nrl_topk_scores")


def _lib_or_skip():
    from newsreclib_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("library not built")
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES + ("nrl_last_error", "nrl_abi_version"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    return lib


def test_symbols_are_declared_typed_and_exported_without_an_abi_bump():
    from newsreclib_amd import _build, _lib
    header = open(os.path.join(ROOT, "include", "newsreclib_amd.h")).read()
    assert "nrl_topk.hip" in _build.sources()
    assert _lib.ABI_VERSION == 19 and re.search(r"#define NRL_ABI_VERSION 19\b", header)
    assert re.search(r"#define NRL_TOPK_MAX_K 128\b", header)
    for name in NAMES:
        assert re.search(r"\b%s\(" % name, header) and name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["nrl_topk_scores"][1]) == 16 and len(_lib.SIGNATURES[NAMES[0]][1]) == 5
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("library not built")
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(NAMES) <= exported
    assert _lib_or_skip().nrl_abi_version() == 19


def test_workspace_bytes():
    ws = _lib_or_skip().nrl_topk_scores_workspace_bytes
    base = ws(512, 65536, 400, 10, 8)
    assert base >= 512 * 8 * 10 * 8 and base % 256 == 0
    assert ws(1024, 65536, 400, 10, 8) > base and ws(512, 65536, 400, 20, 8) > base and ws(512, 65536, 400, 10, 16) > base
    for args in ((1, 1, 4, 1, 0), (3, 1000, 300, 128, 7), (130, 63, 4, 5, 2), (512, 65536, 400, 10, 0)):
        assert ws(*args) % 256 == 0 and ws(*args) >= 256
    # O(B * slices * k): the table length does not enter once the slice count is fixed (and reachable: 8 <= V / 128)
    assert ws(512, 65536, 400, 10, 8) == ws(512, 1 << 20, 400, 10, 8) == ws(512, (1 << 31) - 1, 400, 10, 8)
    # the library's own choice never sizes the workspace by B * V either
    assert ws(512, 1 << 24, 400, 10, 0) == ws(512, 65536, 400, 10, 0) < 512 * 65536 * 4 / 8


def test_host_side_refusals_need_no_device():
    lib = _lib_or_skip()
    st = ctypes.c_int32(0)

    def call(B, V, D, k, ws_bytes=1 << 20):
        # pointers are never dereferenced: every refusal below returns before the first launch
        return lib.nrl_topk_scores(None, None, B, V, D, k, None, None, None, 0, None, None, ctypes.addressof(st), None, ws_bytes, None)

    for B, V, D, k, word in ((4, 100, 8, 0, "k in"), (4, 100, 8, 129, "k in"), (4, 100, 6, 5, "multiple of 4"),
                             (4, 100, 1028, 5, "multiple of 4"), (4, 1 << 31, 8, 5, "2^31"), (-1, 100, 8, 5, "negative"),
                             (4, -2, 8, 5, "negative")):
        assert call(B, V, D, k) == -1, (B, V, D, k)
        assert word in lib.nrl_last_error().decode(), lib.nrl_last_error()
    assert call(0, 100, 8, 5) == 0                          # B == 0: success, nothing launched
    # a short workspace: NRL_E_WORKSPACE (-2), again before any launch (the non-null pointers are placeholders, never read)
    need = lib.nrl_topk_scores_workspace_bytes(4, 100, 8, 5, 0)
    assert lib.nrl_topk_scores(256, 256, 4, 100, 8, 5, None, None, None, 0, 256, 256, ctypes.addressof(st), 256, need - 1, None) == -2
    assert "workspace too small" in lib.nrl_last_error().decode()
    assert lib.nrl_topk_scores(None, None, 4, 100, 8, 5, None, None, None, 0, None, None, None, None, 1 << 20, None) == -1
    assert "status" in lib.nrl_last_error().decode()


def test_ops_and_recommend_refuse_host_tensors():
    from newsreclib_amd import ops
    from newsreclib_amd.evaluation import NewsVectorCache
    from newsreclib_amd.nrms_module import NRMSModule
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.topk_scores(torch.zeros(2, 8), torch.zeros(5, 8), 3)
    cache = NewsVectorCache(object.__new__(NRMSModule), None)
    with pytest.raises(RuntimeError, match="no CPU path"):
        cache.recommend(torch.tensor([1, 2, 3]), torch.tensor([2, 1]), 3)


def test_dot_product_scorers_are_marked():
    from newsreclib_amd.cen_news_rec_module import CenNewsRecModule
    from newsreclib_amd.lstur_module import LSTURModule
    from newsreclib_amd.manner_cr_module import CRModule
    from newsreclib_amd.mins_module import MINSModule
    from newsreclib_amd.naml_module import NAMLModule
    from newsreclib_amd.nrms_module import NRMSModule
    from newsreclib_amd.sentirec_module import SentiRecModule
    from newsreclib_amd.tanr_module import TANRModule
    for cls in (NRMSModule, LSTURModule, NAMLModule, TANRModule, CenNewsRecModule, MINSModule, SentiRecModule, CRModule):
        assert cls.dot_product_scorer is True and callable(cls.user_vectors), cls


def test_dot_product_families_share_one_scoring_skeleton():
    """The eight families take ``user_vectors`` / ``score_news_vectors`` from the one base class, no module file defines either
    name, and the reshape of full rows (``dense_max_is_exact``) stays with NRMS, SentiRec and the CR-Module."""
    import sys

    from newsreclib_amd.cen_news_rec_module import CenNewsRecModule
    from newsreclib_amd.dot_product_recommender import DotProductRecommender
    from newsreclib_amd.lstur_module import LSTURModule
    from newsreclib_amd.manner_cr_module import CRModule
    from newsreclib_amd.mins_module import MINSModule
    from newsreclib_amd.naml_module import NAMLModule
    from newsreclib_amd.nrms_module import NRMSModule, attach_layout, prepare_batch, text_vocab
    from newsreclib_amd.sentirec_module import SentiRecModule
    from newsreclib_amd.tanr_module import TANRModule
    assert callable(attach_layout) and callable(prepare_batch) and callable(text_vocab)
    exact = (NRMSModule, SentiRecModule, CRModule)
    for cls in (NRMSModule, LSTURModule, NAMLModule, TANRModule, CenNewsRecModule, MINSModule, SentiRecModule, CRModule):
        assert issubclass(cls, DotProductRecommender), cls
        assert cls.user_vectors is DotProductRecommender.user_vectors, cls
        assert cls.score_news_vectors is DotProductRecommender.score_news_vectors, cls
        assert cls._encode_user is not DotProductRecommender._encode_user, cls
        assert cls.dense_max_is_exact is (cls in exact), cls
        source = open(sys.modules[cls.__module__].__file__).read()
        assert not re.search(r"def\s+(user_vectors|score_news_vectors)\b", source), cls.__module__


def test_eval_mode_restores_the_mode_when_the_scope_raises():
    from newsreclib_amd.evaluation import eval_mode
    m = torch.nn.Linear(2, 2)
    for training in (True, False):
        m.train(training)
        with pytest.raises(RuntimeError, match="inside"):
            with eval_mode(m):
                assert m.training is False
                raise RuntimeError("inside")
        assert m.training is training
        with eval_mode(m):
            assert m.training is False
        assert m.training is training


def test_the_three_caches_share_one_model_step():
    from newsreclib_amd import evaluation as E
    from newsreclib_amd.npa_module import NPAModule
    caches = (E.NewsVectorCache, E.MannerVectorCache, E.NpaFeatureCache)
    base = [c for c in E.NewsVectorCache.__mro__ if "model_step" in vars(c)]
    assert len(base) == 1 and base[0] not in caches
    for cls in caches:
        assert issubclass(cls, base[0]) and cls.model_step is base[0].model_step and cls._meta is base[0]._meta, cls
    # before any device work: the module is not initialised, there is no table and the arguments are host tensors
    cache = E.NpaFeatureCache(object.__new__(NPAModule), None)
    idx, sizes = torch.tensor([1, 2, 3]), torch.tensor([2, 1])
    with pytest.raises(ValueError, match="NpaFeatureCache.model_step needs user_idx: NPA's attention queries come from the user embedding"):
        cache.model_step(idx, sizes, idx, sizes, torch.zeros(3), user_idx=None)


@pytest.mark.parametrize("family", ["miner", "caum", "dkn", "sentidebias", "npa", "manner"])
def test_recommend_is_refused_where_the_score_is_no_single_dot_product(family):
    """Before any device work: the modules are not even initialised and the arguments are host tensors."""
    from newsreclib_amd import evaluation as E
    if family == "npa":
        from newsreclib_amd.npa_module import NPAModule
        cache = E.NpaFeatureCache(object.__new__(NPAModule), None)
    elif family == "manner":
        cache = object.__new__(E.MannerVectorCache)
    else:
        from newsreclib_amd.caum_module import CAUMModule
        from newsreclib_amd.dkn_module import DKNModule
        from newsreclib_amd.miner_module import MINERModule
        from newsreclib_amd.senti_debias_module import SentiDebiasModule
        cls = {"miner": MINERModule, "caum": CAUMModule, "dkn": DKNModule, "sentidebias": SentiDebiasModule}[family]
        assert not getattr(cls, "dot_product_scorer", False)
        cache = E.NewsVectorCache(object.__new__(cls), None)
    with pytest.raises(NotImplementedError, match="dot product|depend on the user|z-scores"):
        cache.recommend(torch.tensor([1, 2, 3]), torch.tensor([2, 1]), 3)


def test_recommendation_dictionary_format():
    from newsreclib_amd.evaluation import format_recommendations
    idx = torch.tensor([[4, 2, -1], [0, -1, -1], [-1, -1, -1]])
    score = torch.tensor([[1.5, 0.25, float("-inf")], [-2.0, float("-inf"), float("-inf")], [float("-inf")] * 3])
    assert format_recommendations([7, 8, 9], idx, score) == {"U7": {"N4": 1.5, "N2": 0.25}, "U8": {"N0": -2.0}, "U9": {}}
    news_ids = torch.tensor([100, 101, 102, 103, 104])
    got = format_recommendations([7, 8, 9], idx, score, news_ids)
    assert got == {"U7": {"N104": 1.5, "N102": 0.25}, "U8": {"N100": -2.0}, "U9": {}}
    assert list(got["U7"]) == ["N104", "N102"]              # best first, as ranked
