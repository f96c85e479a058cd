"""Drop-in for ``newsreclib.models.general_rec.npa_module.NPAModule`` on MI355X HIP kernels::

    model._target_: newsreclib_amd.npa_module.NPAModule          # configs/model/npa.yaml:1

Same 22 constructor keyword arguments (npa_module.py:77-100), sub-module attributes and ``state_dict`` keys:
``user_projection`` (``UserProjection``), ``news_encoder`` (``CNNPersAtt`` itself, no ``NewsEncoder`` wrapper),
``user_encoder`` (NPA ``UserEncoder``, early fusion only), ``click_predictor`` (``DotProduct``).

A news vector depends on the user it is encoded for (the text query is personalized), so there is no
``score_news_vectors`` and ``evaluation.NewsVectorCache`` refuses this module.  In eval mode only the pooling is
personalized, though: the conv feature maps ``relu(cnn(embedding(title)))`` depend on the news alone, and
``evaluation.NpaFeatureCache`` (``feature_cache(table)``) keeps them for the whole corpus and scores impressions from them
with one fused kernel pair -- the encode-once evaluation path.  The forward under ``torch.no_grad()`` computes the same
scores from token ids.  Differences from the reference: history and candidate rows are encoded in one call (their two text
queries keep two dropout draws); at batch size 1 the reference's ``.squeeze()`` (attention.py:257) drops the batch axis and
its ``bmm`` fails, while this module returns the (1, C) scores."""
from __future__ import annotations

from typing import Any, Dict, List, Optional

import torch

from . import ops, ops_npa
from .abstract_recommender import AbstractRecommender
from .click_predictor import DotProduct
from .dense_batch import dense_rows
from .news_encoder import CNNPersAtt, _draw_seed
from .npa_layers import UserProjection, query_head
from .nrms_module import prepare_batch
from .user_encoder_npa import UserEncoder


class NPAModule(AbstractRecommender):
    user_dependent_news_vectors = True       # (evaluation.NewsVectorCache refuses to cache them: NpaFeatureCache)
    # in eval mode the news vector depends on the user only through the attention pooling of the cached conv feature maps, and the
    # score is a dot product with a candidate-independent user vector: ``evaluation.NpaFeatureCache.recommend_pooled`` ranks the
    # whole table by it.  There is still no (V, D) table, so there is no ``dot_product_scorer``
    personalized_pooling_scorer = True

    def __init__(
        self,
        outputs: Dict[str, List[str]],
        dual_loss_training: bool,
        dual_loss_coef: Optional[float],
        loss: str,
        late_fusion: bool,
        temperature: Optional[float],
        pretrained_embeddings_path: str,
        text_embed_dim: int,
        user_embed_dim: int,
        num_users: int,
        num_filters: int,
        window_size: int,
        word_pref_query_dim: int,
        news_pref_query_dim: int,
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
        self.num_categ_classes = num_categ_classes + 1          # npa_module.py:104-105
        self.num_sent_classes = num_sent_classes + 1
        if save_recs:
            assert isinstance(recs_fpath, str)
        self._init_loss(loss, dual_loss_training, dual_loss_coef)      # CE / SupCon / dual
        if pretrained_embeddings is None:
            assert isinstance(pretrained_embeddings_path, str)
            pretrained_embeddings = self._init_embedding(pretrained_embeddings_path)
        self.user_projection = UserProjection(num_users=num_users + 1, user_embed_dim=user_embed_dim,
                                              dropout_probability=dropout_probability)
        self.news_encoder = CNNPersAtt(pretrained_embeddings=pretrained_embeddings, text_embed_dim=text_embed_dim,
                                       user_embed_dim=user_embed_dim, num_filters=num_filters, window_size=window_size,
                                       query_dim=word_pref_query_dim, dropout_probability=dropout_probability)
        if not late_fusion:
            self.user_encoder = UserEncoder(user_embed_dim=user_embed_dim, num_filters=num_filters,
                                            preference_query_dim=news_pref_query_dim,
                                            dropout_probability=dropout_probability)
        self.click_predictor = DotProduct()
        self._init_step_outputs(outputs)

    def feature_cache(self, table, chunk: int = 16384):
        """The encode-once evaluation cache of this module over a ``evaluation.DeviceNewsTable`` (a snapshot of the present
        weights: call its ``build()`` again after they change)."""
        from .evaluation import NpaFeatureCache
        return NpaFeatureCache(self, table, chunk)

    def _prepare(self, batch: Dict) -> Dict:
        return prepare_batch(batch, self.news_encoder.embedding_layer.weight.shape[0])

    def user_queries(self, user_idx: torch.Tensor, p: float = 0.0, seed: Optional[int] = None):
        """Projected users (once), the text query of both encoder calls and the user encoder's news query in one launch:
        -> (text queries (2B, F): rows [history; candidates], news queries (B, F) or None under late fusion)."""
        enc = self.news_encoder
        news_head = None if self.hparams.late_fusion else query_head(self.user_encoder.news_query_projection,
                                                                      self.user_encoder.personalized_attention)
        params = (self.user_projection.user_embed,) + query_head(enc.text_query_projection, enc.personalized_attention) \
            + (news_head or (None,) * 4)
        bufs = tuple(getattr(t, "main_grad", None) if t is not None else None for t in params)
        queries = ops_npa.NpaUserQueriesFn.apply(user_idx, *params, p, seed or 0, ops_npa.QUERY_STREAM0,
                                                 bufs if any(b is not None for b in bufs) else None)
        return (queries, None) if news_head is None else queries

    # -- reference: npa_module.py:208-252 -------------------------------------------------------------
    def forward(self, batch: Dict, seed: Optional[int] = None) -> torch.Tensor:
        batch = self._prepare(batch)
        B = batch["batch_size"]
        if self.training and seed is None:
            seed = _draw_seed()                       # one draw per step; streams separate the dropouts
        p = float(self.news_encoder.dropout.p) if self.training else 0.0
        enc = self.news_encoder
        text_q, news_q = self.user_queries(batch["user_idx"], p, seed)
        # history rows attend with query row batch_hist[n], candidate rows with B + batch_cand[n]
        n_hist = batch["batch_hist"].shape[0]
        owner = torch.cat([batch["batch_hist"], batch["batch_cand"] + B]).to(torch.int32)
        offsets = torch.cat([batch["hist_offsets"][:-1], batch["cand_offsets"] + n_hist])
        news_vector = enc(batch["x_all"]["title"], text_q, owner, offsets, seed=seed,
                          order=batch["x_all"].get("title_order"), stream0=ops_npa.ENCODER_STREAM0)
        hist_vec, cand_vec = ops.split_rows(news_vector, n_hist)
        cand_news_vector_agg = dense_rows(cand_vec, batch["batch_cand"], B, batch["max_cand"], batch["cand_offsets"])
        if not self.hparams.late_fusion:
            user_vector = self.user_encoder(hist_vec, batch["hist_offsets"], batch["max_hist"], news_q)
        else:                                         # npa_module.py:234-240
            hist_news_vector_agg = dense_rows(hist_vec, batch["batch_hist"], B, batch["max_hist"],
                                              batch["hist_offsets"])
            user_vector = ops.HistMeanFn.apply(hist_news_vector_agg, batch["hist_offsets"])
        return self.click_predictor(user_vector.unsqueeze(dim=1), cand_news_vector_agg.permute(0, 2, 1))
