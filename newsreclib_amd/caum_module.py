"""Drop-in for ``newsreclib.models.general_rec.caum_module.CAUMModule`` on MI355X HIP kernels::

    model._target_: newsreclib_amd.caum_module.CAUMModule          # configs/model/caum.yaml:1

Same 33 constructor keyword arguments (caum_module.py:95-130), sub-module attributes and ``state_dict`` keys:
``news_encoder`` (``NewsEncoder``: ``MHSAAddAtt`` over the title, ``LinearEncoder`` with dropout and ReLU-linear over the
category, a second ``MHSAAddAtt`` over ``title_entities``, ``combine_type="linear"``), ``user_encoder`` (CAUM
``UserEncoder``, early fusion only) and ``click_predictor`` (``DotProduct``).  Optional in-memory tables
(``pretrained_word_embeddings``, ``pretrained_entity_embeddings``) replace the ``.npy`` paths.  ``use_plm=True`` is not built.

Differences from the reference: history and candidates are encoded in one news-encoder call (dropout streams:
``ops_caum``); the user encoder runs every candidate slot in one pass instead of a Python loop over the slots
(``user_encoder_caum``), reassociating its first layers (equal within rounding).  A news vector depends on the news alone,
so ``evaluation.NewsVectorCache`` applies (``score_news_vectors``).  ``factored_eval = True`` (class or instance attribute)
switches the evaluation-mode user encoder to its factored form, whose cost follows the real candidate lists instead of the
padded (B, max_cand) block; inference only, and the status word of its last call is kept in ``factored_status``."""
from __future__ import annotations

from typing import Any, Dict, List, Optional

import numpy as np
import torch

from . import ops
from .abstract_recommender import AbstractRecommender
from .click_predictor import DotProduct
from .dense_batch import dense_rows
from .news_encoder import LinearEncoder, MHSAAddAtt, NewsEncoder, _draw_seed
from .nrms_module import prepare_batch
from .user_encoder_caum import UserEncoder


class CAUMModule(AbstractRecommender):
    # True: in evaluation mode with early fusion, ``score_news_vectors`` scores the real (user, candidate) pairs only
    # (``UserEncoder.score_ragged``: same dense (B, max_cand) result within rounding, no work on padded slots).  Training mode
    # and late fusion ignore it.  False (default): the path below, unchanged.
    factored_eval = False

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
        pretrained_word_embeddings_path: Optional[str],
        plm_model: Optional[str],
        frozen_layers: Optional[List[int]],
        text_embed_dim: int,
        categ_embed_dim: int,
        use_entities: float,
        pretrained_entity_embeddings_path: Optional[str],
        entity_embed_dim: Optional[int],
        entity_num_heads: Optional[int],
        text_num_heads: int,
        news_embed_dim: int,
        query_dim: int,
        dropout_probability: float,
        user_vector_dim: int,
        num_filters: int,
        dense_att_hidden_dim1: int,
        dense_att_hidden_dim2: int,
        top_k_list: List[int],
        num_categ_classes: int,
        num_sent_classes: int,
        save_recs: bool,
        recs_fpath: Optional[str],
        optimizer: Any,
        scheduler: Any,
        pretrained_word_embeddings: Optional[torch.Tensor] = None,
        pretrained_entity_embeddings: Optional[torch.Tensor] = None,
    ) -> None:
        super().__init__()
        self.save_hyperparameters(logger=False, ignore=["pretrained_word_embeddings", "pretrained_entity_embeddings"])
        if use_plm:
            raise NotImplementedError("newsreclib_amd.CAUMModule: use_plm=True (the PLM text encoder) is not built")
        self.num_categ_classes = num_categ_classes + 1          # caum_module.py:132-133
        self.num_sent_classes = num_sent_classes + 1
        if save_recs:
            assert isinstance(recs_fpath, str)
        if not late_fusion and news_embed_dim != user_vector_dim:
            raise ValueError("CAUM needs news_embed_dim == user_vector_dim (the reference's DenseAttention takes "
                             "2 * user_vector_dim features but receives user_vector_dim + news_embed_dim)")
        self._init_loss(loss, dual_loss_training, dual_loss_coef)      # CE / SupCon / dual
        if pretrained_word_embeddings is None:
            assert isinstance(pretrained_word_embeddings_path, str)
            pretrained_word_embeddings = self._init_embedding(pretrained_word_embeddings_path)
        text_encoder = MHSAAddAtt(pretrained_embeddings=pretrained_word_embeddings, embed_dim=text_embed_dim,
                                  num_heads=text_num_heads, query_dim=query_dim, dropout_probability=dropout_probability)
        category_encoder = LinearEncoder(pretrained_embeddings=None, from_pretrained=False, freeze_pretrained_emb=False,
                                         num_categories=self.num_categ_classes, embed_dim=categ_embed_dim,
                                         use_dropout=True, dropout_probability=dropout_probability,
                                         linear_transform=True, output_dim=categ_embed_dim)
        entity_encoder = None
        if use_entities:
            assert isinstance(entity_embed_dim, int) and isinstance(entity_num_heads, int)
            if pretrained_entity_embeddings is None:
                assert isinstance(pretrained_entity_embeddings_path, str)
                pretrained_entity_embeddings = torch.from_numpy(np.load(pretrained_entity_embeddings_path)).float()
            entity_encoder = MHSAAddAtt(pretrained_embeddings=pretrained_entity_embeddings, embed_dim=entity_embed_dim,
                                        num_heads=entity_num_heads, query_dim=query_dim,
                                        dropout_probability=dropout_probability)
        # caum_module.py:233-259: the combine layer's input width
        news_text_dim = text_embed_dim * (2 if "title" in attributes2encode and "abstract" in attributes2encode else 1)
        news_categ_dim = categ_embed_dim * (2 if "category" in attributes2encode and "subcategory" in attributes2encode
                                            else 1)
        news_entity_dim = 0
        if use_entities:
            news_entity_dim = entity_embed_dim * (2 if "title_entities" in attributes2encode and
                                                  "abstract_entities" in attributes2encode else 1)
        self.news_encoder = NewsEncoder(dataset_attributes=dataset_attributes, attributes2encode=attributes2encode,
                                        concatenate_inputs=False, text_encoder=text_encoder,
                                        category_encoder=category_encoder, entity_encoder=entity_encoder,
                                        combine_vectors=True, combine_type="linear",
                                        input_dim=news_text_dim + news_categ_dim + news_entity_dim, query_dim=None,
                                        output_dim=news_embed_dim)
        if not late_fusion:
            self.user_encoder = UserEncoder(news_embed_dim=news_embed_dim, num_filters=num_filters,
                                            dense_att_hidden_dim1=dense_att_hidden_dim1,
                                            dense_att_hidden_dim2=dense_att_hidden_dim2, user_vector_dim=user_vector_dim,
                                            num_heads=text_num_heads, dropout_probability=dropout_probability)
        self.click_predictor = DotProduct()
        self._init_step_outputs(outputs)

    def _prepare(self, batch: Dict) -> Dict:
        out = prepare_batch(batch, self.news_encoder.text_encoders[next(iter(self.news_encoder.text_encoders))]
                            .embedding_layer.weight.shape[0])
        ents = [a for a in self.news_encoder.entity_attrs if a not in out["x_all"]]
        if ents:
            out = dict(out)
            out["x_all"] = dict(out["x_all"])
            for a in ents:
                out["x_all"][a] = torch.cat([batch["x_hist"][a], batch["x_cand"][a]], dim=0)
        return out

    # -- reference: caum_module.py:326-360 ------------------------------------------------------------
    def forward(self, batch: Dict, seed: Optional[int] = None) -> torch.Tensor:
        """``seed``: the dropout seed of the step (drawn from torch's CPU generator when None); the news encoder and the
        user encoder take their masks from it under the streams of ``ops_caum``."""
        batch = self._prepare(batch)
        if seed is None and self.training and self.hparams.dropout_probability > 0.0:
            seed = _draw_seed()
        news_vector = self.news_encoder(batch["x_all"], seed=seed)
        hist_vec, cand_vec = ops.split_rows(news_vector, batch["batch_hist"].shape[0])
        return self.score_news_vectors(hist_vec, cand_vec, batch, seed=seed)

    def score_news_vectors(self, hist_news_vector: torch.Tensor, cand_news_vector: torch.Tensor, batch: Dict,
                           seed: Optional[int] = None) -> torch.Tensor:
        """caum_module.py:333-358 from already-encoded news rows (see ``evaluation.NewsVectorCache``)."""
        B = batch["batch_size"]
        hist_agg = dense_rows(hist_news_vector, batch["batch_hist"], B, batch["max_hist"], batch["hist_offsets"])
        if self.factored_eval and not self.training and not self.hparams.late_fusion:
            flat, self.factored_status = self.user_encoder.score_ragged(hist_agg, cand_news_vector, batch["cand_offsets"])
            dense = flat.new_zeros(B * batch["max_cand"])
            dense[batch["cand_flat_idx"]] = flat            # padded slots stay exactly 0
            return dense.view(B, batch["max_cand"])
        cand_agg = dense_rows(cand_news_vector, batch["batch_cand"], B, batch["max_cand"], batch["cand_offsets"])
        if not self.hparams.late_fusion:
            return self.user_encoder(hist_agg, cand_agg, batch["cand_offsets"], seed=seed or 0)
        user_vector = ops.HistMeanFn.apply(hist_agg, batch["hist_offsets"])          # :347-352, the true history size
        return self.click_predictor(user_vector.unsqueeze(dim=1), cand_agg.permute(0, 2, 1))
