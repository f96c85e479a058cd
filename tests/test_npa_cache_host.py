"""``evaluation.NpaFeatureCache`` on the host: what it refuses, before any device work."""
import pytest
import torch

from tests import builders


def _table():
    from newsreclib_amd.evaluation import DeviceNewsTable
    return DeviceNewsTable({"title": torch.ones(4, 6, dtype=torch.int64)}, device="cpu")


def test_npa_feature_cache_refuses_other_modules():
    from newsreclib_amd.evaluation import NpaFeatureCache
    with pytest.raises(TypeError):
        NpaFeatureCache(torch.nn.Linear(2, 2), _table())


def test_npa_feature_cache_requires_user_idx():
    """raised before the table is encoded: the CPU table would fail the kernels' device check with a RuntimeError"""
    cache = builders.npa_contract_module().feature_cache(_table())
    sizes = torch.tensor([1, 1])
    with pytest.raises(ValueError):
        cache.scores(torch.tensor([0, 1]), sizes, torch.tensor([2, 3]), sizes, None)
    with pytest.raises(ValueError):
        cache.model_step(torch.tensor([0, 1]), sizes, torch.tensor([2, 3]), sizes, torch.tensor([1.0, 0.0]))
    assert cache.features is None


def test_news_vector_cache_still_refuses_npa_and_names_the_feature_cache():
    from newsreclib_amd.evaluation import NewsVectorCache
    with pytest.raises(NotImplementedError, match="NpaFeatureCache"):
        NewsVectorCache(builders.npa_contract_module(), _table()).build()
