"""Drop-in for ``newsreclib.models.general_rec.dkn_module.DKNModule`` on MI355X HIP kernels::

    model._target_: newsreclib_amd.dkn_module.DKNModule          # configs/model/dkn.yaml:1

Same 21 constructor keyword arguments (dkn_module.py:72-94), sub-module attributes and ``state_dict`` keys:
``news_encoder`` (``KCNN`` itself), ``user_encoder`` (DKN ``UserEncoder``, early fusion only), ``click_predictor``
(``DNNPredictor`` under early fusion, ``DotProduct`` under late fusion).  Optional in-memory tables
(``pretrained_word_embeddings``, ``pretrained_entity_embeddings``) replace the ``.npy`` paths; the context table is
initialised from the entity table, as the reference loads both from one file (:117-122), but is a parameter of its own.

DKN has no dropout, and a news vector depends on the news alone, so ``evaluation.NewsVectorCache`` applies
(``score_news_vectors``).  Differences from the reference: history and candidates are encoded in one call; the user
encoder's attention is computed once per impression instead of once per candidate -- its DNN is affine, so the candidate's
share of the attention score is constant over the history and cancels in the softmax (exactly equal weights; the
reference's gradients of ``user_encoder.dnn.0.weight[:, :dim]``, ``dnn.0.bias`` and ``dnn.1.bias`` are round-off, ours
are zero)."""
from __future__ import annotations

from typing import Any, Dict, List, Optional

import numpy as np
import torch

from . import ops, ops_dkn
from .abstract_recommender import AbstractRecommender
from .click_predictor import DNNPredictor, DotProduct
from .dense_batch import dense_rows
from .news_encoder import KCNN
from .nrms_module import prepare_batch
from .user_encoder_dkn import UserEncoder


class DKNModule(AbstractRecommender):
    # the DNN click predictor's first layer splits by columns into a news half and a user half, and the user vector does not depend
    # on the candidate (the affine attention DNN): ``evaluation.NewsVectorCache.recommend_dnn`` ranks the whole table by it.  The
    # score is still no single dot product, so there is no ``dot_product_scorer`` and ``recommend`` refuses
    dnn_predictor_scorer = True

    def __init__(
        self,
        outputs: Dict[str, List[str]],
        dual_loss_training: bool,
        dual_loss_coef: Optional[float],
        loss: str,
        late_fusion: bool,
        temperature: Optional[float],
        pretrained_word_embeddings_path: str,
        text_embed_dim: int,
        use_context: bool,
        pretrained_entity_embeddings_path: str,
        entity_embed_dim: int,
        num_filters: int,
        window_sizes: List[int],
        hidden_dim_dnn: int,
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
        self.num_categ_classes = num_categ_classes + 1          # dkn_module.py:102-103
        self.num_sent_classes = num_sent_classes + 1
        if save_recs:
            assert isinstance(recs_fpath, str)
        if not late_fusion and not 1 <= hidden_dim_dnn <= 64:
            raise NotImplementedError("the fused DKN user encoder / click predictor takes hidden_dim_dnn in [1, 64]")
        if not late_fusion and len(window_sizes) * num_filters > 1024:
            raise NotImplementedError("the fused DKN user encoder takes news vectors of at most 1024 features")
        self._init_loss(loss, dual_loss_training, dual_loss_coef)      # CE / SupCon / dual
        if pretrained_word_embeddings is None:
            assert isinstance(pretrained_word_embeddings_path, str)
            pretrained_word_embeddings = self._init_embedding(pretrained_word_embeddings_path)
        if pretrained_entity_embeddings is None:
            assert isinstance(pretrained_entity_embeddings_path, str)
            pretrained_entity_embeddings = torch.from_numpy(np.load(pretrained_entity_embeddings_path)).float()
        ent = torch.as_tensor(pretrained_entity_embeddings, dtype=torch.float32)
        self.news_encoder = KCNN(pretrained_text_embeddings=pretrained_word_embeddings,
                                 pretrained_entity_embeddings=ent.clone(), pretrained_context_embeddings=ent.clone(),
                                 use_context=use_context, text_embed_dim=text_embed_dim, entity_embed_dim=entity_embed_dim,
                                 num_filters=num_filters, window_sizes=window_sizes)
        dim = len(window_sizes) * num_filters
        if not late_fusion:
            self.user_encoder = UserEncoder(input_dim=dim, hidden_dim=hidden_dim_dnn)
            self.click_predictor = DNNPredictor(input_dim=2 * dim, hidden_dim=hidden_dim_dnn)
        else:
            self.click_predictor = DotProduct()
        self._init_step_outputs(outputs)

    def _prepare(self, batch: Dict) -> Dict:
        out = prepare_batch(batch, self.news_encoder.text_embedding_layer.weight.shape[0])
        if "title_entities" not in out["x_all"]:
            out = dict(out)
            out["x_all"] = dict(out["x_all"])
            out["x_all"]["title_entities"] = torch.cat([batch["x_hist"]["title_entities"],
                                                        batch["x_cand"]["title_entities"]], dim=0)
        return out

    # -- reference: dkn_module.py:207-240 -------------------------------------------------------------
    def forward(self, batch: Dict, seed: Optional[int] = None) -> torch.Tensor:
        batch = self._prepare(batch)
        x = batch["x_all"]
        news_vector = self.news_encoder({"title": x["title"], "title_entities": x["title_entities"]},
                                        order=x.get("title_order"))
        hist_vec, cand_vec = ops.split_rows(news_vector, batch["batch_hist"].shape[0])
        return self.score_news_vectors(hist_vec, cand_vec, batch)

    def score_news_vectors(self, hist_news_vector: torch.Tensor, cand_news_vector: torch.Tensor, batch: Dict,
                           seed: Optional[int] = None) -> torch.Tensor:
        """dkn_module.py:212-240 from already-encoded news rows (see ``evaluation.NewsVectorCache``)."""
        B = batch["batch_size"]
        if not self.hparams.late_fusion:
            # user encoder + DNN predictor + the padded-candidate mask in one HIP call on the ragged rows
            return ops_dkn.DknClickFn.apply(hist_news_vector, batch["hist_offsets"], batch["max_hist"], cand_news_vector,
                                            batch["cand_offsets"], batch["max_cand"], *self.user_encoder.params(),
                                            *self.click_predictor.params())
        hist_agg = dense_rows(hist_news_vector, batch["batch_hist"], B, batch["max_hist"], batch["hist_offsets"])
        cand_agg = dense_rows(cand_news_vector, batch["batch_cand"], B, batch["max_cand"], batch["cand_offsets"])
        user_vector = ops.HistMeanFn.apply(hist_agg, batch["hist_offsets"])          # :226-232, the true history size
        return self.click_predictor(user_vector.unsqueeze(dim=1), cand_agg.permute(0, 2, 1))

    def user_queries(self, hist_news_vector: torch.Tensor, meta: Dict):
        """Early fusion, from the gathered history rows and the history half of the batch metadata (``hist_offsets``,
        ``max_hist``) -> (user (B, dim), q (B, Hd)): the candidate-independent user vector -- the one ``score_news_vectors``
        computes -- and ``q = user Wu^T + b1``, the user's share of the click predictor's first layer
        (``click_predictor.dnn.0.weight = [Wc | Wu]``).  The score of a news vector ``c`` is then
        ``b2 + w2 . relu(c Wc^T + q)``.  DKN has no dropout: eval and train semantics are the same.  No gradient."""
        if self.hparams.late_fusion:
            raise NotImplementedError("DKN under late fusion has no DNN predictor: its score is the dot product with the history mean")
        return ops_dkn.dkn_user_query(hist_news_vector, meta["hist_offsets"], meta["max_hist"], self.user_encoder.params(),
                                      self.click_predictor.params())
