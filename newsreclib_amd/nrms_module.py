"""Drop-in for ``newsreclib.models.general_rec.nrms_module.NRMSModule`` on MI355X HIP kernels.

Select it from the reference's Hydra configs by overriding one key::

    model._target_: newsreclib_amd.nrms_module.NRMSModule        # configs/model/nrms.yaml:1

Same 23 constructor keyword arguments (nrms_module.py:75-100), same sub-module attributes
(``news_encoder`` / ``user_encoder`` / ``click_predictor``) and ``state_dict`` keys, same
``forward`` / ``model_step`` / ``training_step`` / ``configure_optimizers`` contracts.  What
differs is underneath: the encoders and the scorer call the C-ABI HIP library, history and
candidate news are encoded in ONE encoder call (row-independent, so identical results), and
``model_step`` builds its outputs without per-user Python loops or device->host syncs
(the reference pays ~2B syncs + 6B tiny kernels per step, nrms_module.py:331-345).
"""
from __future__ import annotations

from typing import Any, Dict, List, Optional

import torch

from . import ops
from .batch_layout import attach_layout, prepare_batch, text_vocab  # noqa: F401  (their import path of record)
from .click_predictor import DotProduct
from .dot_product_recommender import DotProductRecommender
from .news_encoder import PLM, MHSAAddAtt, NewsEncoder
from .user_encoder import UserEncoder


class NRMSModule(DotProductRecommender):
    dense_max_is_exact = True

    def __init__(
        self,
        dataset_attributes: List[str],
        attributes2encode: List[str],
        outputs: Dict[str, List[str]],
        dual_loss_training: bool,
        dual_loss_coef: Optional[float],
        loss: str,
        late_fusion: bool,
        temperature: Optional[float],
        use_plm: bool,
        pretrained_embeddings_path: Optional[str],
        plm_model: Optional[str],
        frozen_layers: Optional[List[int]],
        embed_dim: int,
        num_heads: int,
        query_dim: int,
        dropout_probability: float,
        top_k_list: List[int],
        num_categ_classes: int,
        num_sent_classes: int,
        save_recs: bool,
        recs_fpath: Optional[str],
        optimizer: Any,
        scheduler: Any,
        pretrained_embeddings: Optional[torch.Tensor] = None,
    ) -> None:
        super().__init__()
        self.save_hyperparameters(logger=False, ignore=["pretrained_embeddings"])
        hp = self.hparams
        self.num_categ_classes = num_categ_classes + 1
        self.num_sent_classes = num_sent_classes + 1
        if save_recs:
            assert isinstance(recs_fpath, str)
        self._init_loss(loss, dual_loss_training, dual_loss_coef)      # CE / SupCon / dual

        if not use_plm:
            # pretrained embeddings + contextualisation (nrms_module.py:122-135)
            if pretrained_embeddings is None:
                assert isinstance(pretrained_embeddings_path, str)
                pretrained_embeddings = self._init_embedding(pretrained_embeddings_path)
            text_encoder = MHSAAddAtt(pretrained_embeddings=pretrained_embeddings, embed_dim=embed_dim,
                                      num_heads=num_heads, query_dim=query_dim,
                                      dropout_probability=dropout_probability)
        else:
            # PLM news encoder (nrms_module.py:136-149)
            assert isinstance(plm_model, str)
            text_encoder = PLM(plm_model=plm_model, frozen_layers=frozen_layers, embed_dim=embed_dim,
                               use_mhsa=True, apply_reduce_dim=False, reduced_embed_dim=None,
                               num_heads=num_heads, query_dim=query_dim, dropout_probability=dropout_probability)
        self.news_encoder = NewsEncoder(
            dataset_attributes=dataset_attributes, attributes2encode=attributes2encode,
            concatenate_inputs=False, text_encoder=text_encoder, category_encoder=None,
            entity_encoder=None, combine_vectors=False, combine_type=None, input_dim=None,
            query_dim=None, output_dim=None)
        if not late_fusion:                                     # nrms_module.py:165-171
            self.user_encoder = UserEncoder(news_embed_dim=embed_dim, num_heads=num_heads, query_dim=query_dim)
        self.click_predictor = DotProduct()
        self._text_attr = next(iter(self.news_encoder.text_encoders.keys()))

        self._init_step_outputs(outputs)
        assert hp is not None

    def _prepare(self, batch: Dict) -> Dict:
        te = self.news_encoder.text_encoders[self._text_attr]
        emb = getattr(te, "embedding_layer", None)
        return prepare_batch(batch, emb.weight.shape[0] if emb is not None else None)

    # -- reference: nrms_module.py:230-255 ---------------------------------------------------------
    def forward(self, batch: Dict) -> torch.Tensor:
        batch = self._prepare(batch)
        B = batch["batch_size"]
        hist_text = batch["x_hist"][self._text_attr]
        n_hist = (hist_text if torch.is_tensor(hist_text) else next(iter(hist_text.values()))).shape[0]
        if self.hparams.use_plm:
            # the PLM encoder's seq-first attention runs ACROSS THE NEWS OF ONE CALL (text.py:92-96), so the two
            # calls of the reference (:232,236) are NOT interchangeable with one call over [history; candidates]
            # (the transformer BODY treats every news on its own: it runs once over both calls' news, news_encoder.PLM.share_body)
            self.news_encoder.share_plm_bodies(batch["x_hist"], batch["x_cand"])
            hist_vec = self.news_encoder(batch["x_hist"])
            cand_vec = self.news_encoder(batch["x_cand"])
            return self.score_news_vectors(hist_vec, cand_vec, batch)
        # rows of the MHSAAddAtt encoder are independent: one call for history + candidate news gives the same
        # vectors as the reference's two (:232,236)
        news_vector = self.news_encoder(batch["x_all"])
        return self.score_news_vectors(*ops.split_rows(news_vector, n_hist), batch)

    def _encode_user(self, hist_dense: torch.Tensor, batch: Dict, seed=None) -> torch.Tensor:
        return self.user_encoder(hist_dense)
