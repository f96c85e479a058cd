"""Drop-in for ``newsreclib.models.fair_rec.manner_cr_module.CRModule`` (MANNeR's content-based recommendation module) on MI355X
HIP kernels::

    model._target_: newsreclib_amd.manner_cr_module.CRModule          # configs/model/manner_cr_module.yaml:1

Same 22 constructor keyword arguments (manner_cr_module.py:73-97), sub-module attributes and ``state_dict`` keys: ``news_encoder``
(``NewsEncoder(concatenate_inputs=True, combine_type="linear")`` over one ``PLM(use_mhsa=False, apply_reduce_dim=False)`` -- the CLS
row of the concatenated title + abstract text -- and, with ``use_entities``, one ``MHSAAddAtt`` over the concatenated entity ids),
``user_encoder`` (NRMS ``UserEncoder``, early fusion only) and ``click_predictor``.  An optional in-memory
``pretrained_entity_embeddings`` tensor replaces the ``.npy`` path.  This is composition of existing kernels.

``temperature`` is accepted and IGNORED, as in the reference: its constructor builds the criterion through
``_get_loss(self.hparams.loss)`` (manner_cr_module.py:111), which instantiates ``SupConLoss()`` without arguments
(abstract_recommender.py:117-118), so the temperature of the score-matrix SupCon is the loss's default 0.1 whatever the config says.

The CLS head encodes every news on its own (``PLM.news_independent``), so ``evaluation.NewsVectorCache`` applies
(``score_news_vectors``); the transformer body runs once over history and candidate texts (``PLM.share_body``).

``load_from_checkpoint(path, **overrides)`` reads the ``hyper_parameters`` and ``state_dict`` of a Lightning checkpoint file;
``plm_model=`` (a local model directory) is the usual override, since a hub name cannot be resolved offline."""
from __future__ import annotations

from typing import Any, Dict, List, Optional

import torch

from .batch_layout import prepare_batch
from .click_predictor import DotProduct
from .dot_product_recommender import DotProductRecommender
from .news_encoder import PLM, MHSAAddAtt, NewsEncoder, _draw_seed
from .user_encoder import UserEncoder


def build_manner_news_encoder(owner, hp, pretrained_entity_embeddings: Optional[torch.Tensor]) -> NewsEncoder:
    """The news encoder CRModule and AModule share (manner_cr_module.py:113-162 == manner_a_module.py:88-137)."""
    assert isinstance(hp.plm_model, str)
    text_encoder = PLM(plm_model=hp.plm_model, frozen_layers=hp.frozen_layers, embed_dim=hp.text_embed_dim, use_mhsa=False,
                       apply_reduce_dim=False, reduced_embed_dim=None, num_heads=hp.num_heads, query_dim=hp.query_dim,
                       dropout_probability=hp.dropout_probability)
    entity_encoder = None
    if hp.use_entities:
        if pretrained_entity_embeddings is None:
            assert isinstance(hp.pretrained_entity_embeddings_path, str)
            pretrained_entity_embeddings = owner._init_embedding(filepath=hp.pretrained_entity_embeddings_path)
        entity_encoder = MHSAAddAtt(pretrained_embeddings=pretrained_entity_embeddings, embed_dim=hp.entity_embed_dim,
                                    num_heads=hp.num_heads, query_dim=hp.query_dim, dropout_probability=hp.dropout_probability)
    input_dim = hp.text_embed_dim + hp.entity_embed_dim if hp.use_entities else hp.text_embed_dim
    return NewsEncoder(dataset_attributes=hp.dataset_attributes, attributes2encode=hp.attributes2encode, concatenate_inputs=True,
                       text_encoder=text_encoder, category_encoder=None, entity_encoder=entity_encoder, combine_vectors=True,
                       combine_type="linear", input_dim=input_dim, query_dim=None, output_dim=hp.text_embed_dim)


def load_module_from_checkpoint(cls, checkpoint_path: str, map_location="cpu", strict: bool = True, **overrides):
    """``LightningModule.load_from_checkpoint`` for the stand-in base: ``cls(**hyper_parameters, **overrides)`` then
    ``load_state_dict(state_dict)``."""
    ckpt = torch.load(checkpoint_path, map_location=map_location, weights_only=False)
    if "state_dict" not in ckpt or "hyper_parameters" not in ckpt:
        raise KeyError(f"{checkpoint_path}: a Lightning checkpoint holds `state_dict` and `hyper_parameters`")
    kwargs = dict(ckpt["hyper_parameters"])
    kwargs.update(overrides)
    module = cls(**kwargs)
    module.load_state_dict(ckpt["state_dict"], strict=strict)
    return module


class CRModule(DotProductRecommender):
    dense_max_is_exact = True

    def __init__(
        self,
        dataset_attributes: List[str],
        attributes2encode: List[str],
        outputs: Dict[str, List[str]],
        loss: str,
        late_fusion: bool,
        temperature: Optional[float],
        plm_model: Optional[str],
        frozen_layers: Optional[List[int]],
        text_embed_dim: int,
        num_heads: int,
        query_dim: int,
        dropout_probability: float,
        use_entities: bool,
        pretrained_entity_embeddings_path: str,
        entity_embed_dim: int,
        top_k_list: List[int],
        num_categ_classes: int,
        num_sent_classes: int,
        save_recs: bool,
        recs_fpath: Optional[str],
        optimizer: Any,
        scheduler: Any,
        pretrained_entity_embeddings: Optional[torch.Tensor] = None,
    ) -> None:
        super().__init__()
        self.save_hyperparameters(logger=False, ignore=["pretrained_entity_embeddings"])
        self.num_categ_classes = num_categ_classes + 1          # manner_cr_module.py:104-105
        self.num_sent_classes = num_sent_classes + 1
        if save_recs:
            assert isinstance(recs_fpath, str)
        self.criterion = self._get_loss(loss)                   # :111 -- `temperature` never reaches it
        if isinstance(self.criterion, tuple):
            raise ValueError("CRModule trains with `cross_entropy_loss` or `sup_con_loss` (manner_cr_module.py:286-314)")
        self.news_encoder = build_manner_news_encoder(self, self.hparams, pretrained_entity_embeddings)
        if not late_fusion:
            self.user_encoder = UserEncoder(news_embed_dim=text_embed_dim, num_heads=num_heads, query_dim=query_dim)
        self.click_predictor = DotProduct()
        self._init_step_outputs(outputs)

    load_from_checkpoint = classmethod(load_module_from_checkpoint)

    def _prepare(self, batch: Dict) -> Dict:
        return prepare_batch(batch, None, need_order=False)

    def _loss(self, scores: torch.Tensor, y_true: torch.Tensor, batch: Dict) -> torch.Tensor:
        if self.hparams.loss == "cross_entropy_loss":           # manner_cr_module.py:286-314
            return self.criterion(scores, y_true)
        return self.criterion(scores, y_true, batch["cand_sizes"])

    # -- reference: manner_cr_module.py:229-254 -----------------------------------------------------------
    def forward(self, batch: Dict, seed: Optional[int] = None) -> torch.Tensor:
        batch = self._prepare(batch)
        if seed is None and self.training and self.hparams.dropout_probability > 0.0:
            seed = _draw_seed()
        self.news_encoder.share_plm_bodies(batch["x_hist"], batch["x_cand"])
        hist_vec = self.news_encoder(batch["x_hist"], seed=seed)
        cand_vec = self.news_encoder(batch["x_cand"], seed=seed, stream_base=4)
        return self.score_news_vectors(hist_vec, cand_vec, batch)

    def _encode_user(self, hist_dense: torch.Tensor, batch: Dict, seed: Optional[int]) -> torch.Tensor:
        return self.user_encoder(hist_dense)
