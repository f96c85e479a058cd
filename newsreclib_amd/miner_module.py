"""Drop-in for ``newsreclib.models.general_rec.miner_module.MINERModule`` on MI355X HIP kernels::

    model._target_: newsreclib_amd.miner_module.MINERModule          # configs/model/miner.yaml:1

Same 27 constructor keyword arguments (miner_module.py:91-120), sub-module attributes and ``state_dict`` keys:
``news_encoder`` (``NewsEncoder`` over one ``PLM(use_mhsa=False)``: CLS row -> ``reduce_dim`` -> dropout), ``categ_encoder``
(``LinearEncoder``: pretrained embedding + dropout, with ``use_categ_bias``), ``user_encoder`` (``PolyAttention``, early fusion
only), ``target_aware_attn`` (``score_type="weighted"``) and ``click_predictor``.  An optional in-memory
``pretrained_categ_embeddings`` tensor replaces the ``.npy`` path.  ``use_plm=False`` is not built: the reference constructs a
``PLM`` unconditionally.

Differences from the reference (results equal within rounding):
  * the history stays ragged.  The reference's ``masked_fill_(~mask, 1e-30)`` lets the ``max_hist - n`` padded rows of a user
    take part in the softmax with logit ~0; their embeddings are zero, so they are a closed-form term of the denominator
    (``ops_miner.PolyFn``).  A user's weights still depend on the batch's ``max_hist``, as in the reference.
  * the category bias is REASSOCIATED.  The reference forms the (n_hist, n_cand) cosine matrix of ALL history and candidate
    category rows of the batch, zeroes user i's own candidates and takes the mean over the whole candidate axis, zeros
    included (miner_module.py:275-285, attention.py:113).  With hh / ch the unit rows that is
    ``hh_t . (S_all - S_own[user(t)]) / n_cand`` where S are sums of ch -- built in that form (``ops_miner.CategBiasFn``), which
    never forms the matrix; checked against the masked-matrix form in fp64 (difference 3e-17).  The bias couples the users of a
    batch, as in the reference.
  * the transformer body runs once over history and candidate titles (``PLM.share_body``); the CLS head is per news, so
    ``evaluation.NewsVectorCache`` applies (``score_news_vectors``).
The disagreement loss goes through the ``forward -> (scores, aux)`` / ``_aux_loss`` hook with ``aux = user_vector``."""
from __future__ import annotations

from typing import Any, Dict, List, Optional

import numpy as np
import torch

from . import ops, ops_miner
from .abstract_recommender import AbstractRecommender
from .click_predictor import DotProduct
from .dense_batch import dense_rows
from .news_encoder import PLM, LinearEncoder, NewsEncoder, _draw_seed
from .nrms_module import prepare_batch
from .user_encoder_miner import PolyAttention as UserEncoder
from .user_encoder_miner import TargetAwareAttention


class MINERModule(AbstractRecommender):
    # score = an aggregate over K candidate-independent interest vectors (``user_interests``): no single dot product, so not a
    # ``dot_product_scorer``; ``evaluation.NewsVectorCache.recommend_interests`` ranks the whole table by it
    multi_interest_scorer = True

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
        plm_model: Optional[str],
        frozen_layers: Optional[List[int]],
        apply_reduce_dim: bool,
        text_embed_dim: int,
        news_embed_dim: int,
        use_categ_bias: bool,
        pretrained_categ_embeddings_path: Optional[str],
        num_context_codes: int,
        context_code_dim: int,
        score_type: str,
        dropout_probability: float,
        top_k_list: List[int],
        num_categ_classes: int,
        num_sent_classes: int,
        save_recs: bool,
        recs_fpath: Optional[str],
        optimizer: Any,
        scheduler: Any,
        pretrained_categ_embeddings: Optional[torch.Tensor] = None,
    ) -> None:
        super().__init__()
        self.save_hyperparameters(logger=False, ignore=["pretrained_categ_embeddings"])
        if not use_plm:
            raise NotImplementedError("newsreclib_amd.MINERModule: use_plm=False is not built (the reference builds a PLM text "
                                      "encoder unconditionally, miner_module.py:146-156)")
        if score_type not in ops_miner.SCORE_MODES:
            raise ValueError("Invalid method of aggregating scores.")          # miner_module.py:308
        self.num_categ_classes = num_categ_classes + 1          # miner_module.py:127-128
        self.num_sent_classes = num_sent_classes + 1
        if save_recs:
            assert isinstance(recs_fpath, str)
        self._init_loss(loss, dual_loss_training, dual_loss_coef)      # CE / SupCon / dual
        width = news_embed_dim if apply_reduce_dim else text_embed_dim          # :141-144
        assert isinstance(plm_model, str)
        text_encoder = PLM(plm_model=plm_model, frozen_layers=frozen_layers, embed_dim=text_embed_dim, use_mhsa=False,
                           apply_reduce_dim=apply_reduce_dim, reduced_embed_dim=width, num_heads=None, query_dim=None,
                           dropout_probability=dropout_probability)
        if use_categ_bias:                                      # :159-174 (built under late fusion too, never called there)
            if pretrained_categ_embeddings is None:
                assert isinstance(pretrained_categ_embeddings_path, str)
                pretrained_categ_embeddings = torch.from_numpy(np.load(pretrained_categ_embeddings_path)).float()
            self.categ_encoder = LinearEncoder(pretrained_embeddings=pretrained_categ_embeddings, from_pretrained=True,
                                               freeze_pretrained_emb=False, num_categories=self.num_categ_classes,
                                               embed_dim=None, use_dropout=True, dropout_probability=dropout_probability,
                                               linear_transform=False, output_dim=None)
        self.news_encoder = NewsEncoder(dataset_attributes=dataset_attributes, attributes2encode=attributes2encode,
                                        concatenate_inputs=False, text_encoder=text_encoder, category_encoder=None,
                                        entity_encoder=None, combine_vectors=False, combine_type=None, input_dim=None,
                                        query_dim=None, output_dim=None)
        if not late_fusion:
            self.user_encoder = UserEncoder(input_dim=width, num_context_codes=num_context_codes,
                                            context_code_dim=context_code_dim)
        self.click_predictor = DotProduct()
        if score_type == "weighted":                            # :201-202 (built under late fusion too)
            self.target_aware_attn = TargetAwareAttention(input_dim=width)
        self._init_step_outputs(outputs)

    @property
    def score_news_attrs(self):
        """News attributes ``score_news_vectors`` reads beside the vectors (``evaluation.NewsVectorCache`` gathers them)."""
        return ("category",) if self.hparams.use_categ_bias and not self.hparams.late_fusion else ()

    def _prepare(self, batch: Dict) -> Dict:
        return prepare_batch(batch, None, need_order=False)

    # -- reference: miner_module.py:258-323 -----------------------------------------------------------
    def forward(self, batch: Dict, seed: Optional[int] = None):
        """-> (scores, user_vector).  ``seed``: the dropout seed of the step (drawn from torch's CPU generator when None); the
        four masks of the model take their streams from ``ops_miner``."""
        batch = self._prepare(batch)
        if seed is None and self.training and self.hparams.dropout_probability > 0.0:
            seed = _draw_seed()
        # one body pass over both calls' titles; the CLS heads stay two calls with their own dropout streams
        self.news_encoder.share_plm_bodies(batch["x_hist"], batch["x_cand"])
        hist_vec = self.news_encoder(batch["x_hist"], seed=seed, stream_base=ops_miner.REDUCE_HIST)
        cand_vec = self.news_encoder(batch["x_cand"], seed=seed, stream_base=ops_miner.REDUCE_CAND)
        return self.score_news_vectors(hist_vec, cand_vec, batch, seed=seed, with_aux=True)

    def score_news_vectors(self, hist_news_vector: torch.Tensor, cand_news_vector: torch.Tensor, batch: Dict,
                           seed: Optional[int] = None, with_aux: bool = False):
        """miner_module.py:261-323 from already-encoded news rows (see ``evaluation.NewsVectorCache``).  With the category bias,
        ``batch["x_hist"]["category"]`` / ``batch["x_cand"]["category"]`` are read.  -> scores, or (scores, user_vector)."""
        hp = self.hparams
        B = batch["batch_size"]
        if hp.late_fusion:
            hist_agg = dense_rows(hist_news_vector, batch["batch_hist"], B, batch["max_hist"], batch["hist_offsets"])
            cand_agg = dense_rows(cand_news_vector, batch["batch_cand"], B, batch["max_cand"], batch["cand_offsets"])
            user_vector = ops.HistMeanFn.apply(hist_agg, batch["hist_offsets"])          # :312-316, the true history size
            scores = self.click_predictor(user_vector.unsqueeze(dim=1), cand_agg.permute(0, 2, 1))
            return (scores, user_vector) if with_aux else scores
        bias = None
        if hp.use_categ_bias:
            hc = self.categ_encoder(batch["x_hist"]["category"], seed=seed, stream=ops_miner.CATEG_HIST)
            cc = self.categ_encoder(batch["x_cand"]["category"], seed=seed, stream=ops_miner.CATEG_CAND)
            bias = ops_miner.CategBiasFn.apply(hc, cc, batch["batch_hist"], batch["batch_cand"], batch["hist_offsets"],
                                               batch["cand_offsets"], B)
        user_vector = self.user_encoder(hist_news_vector, batch["hist_offsets"], B, batch["max_hist"], bias=bias)
        if hp.score_type == "weighted":
            scores = self.target_aware_attn(user_vector, cand_news_vector, batch["cand_offsets"], batch["max_cand"])
        else:
            scores = ops_miner.ScoreFn.apply(cand_news_vector, user_vector, None, batch["cand_offsets"], B,
                                             batch["max_cand"], hp.score_type)
        return (scores, user_vector) if with_aux else scores

    @property
    def interest_score_mode(self) -> str:
        """The aggregate over the interest vectors of ``user_interests`` (``ops_miner.SCORE_MODES``): ``score_type``, or "mean"
        over the one history mean under late fusion."""
        return "mean" if self.hparams.late_fusion else self.hparams.score_type

    def user_interests(self, hist_news_vector: torch.Tensor, batch: Dict, bias: Optional[torch.Tensor] = None):
        """The candidate-independent half of ``score_news_vectors`` -> (interests (B, K, D), gate (B, K, D) or None); the score
        of any news is their aggregate ``interest_score_mode`` (``ops.topk_interest_scores``).  Early fusion: the
        poly-attention user vectors and, for ``score_type="weighted"``, ``gate = gelu(user_vector Wt^T)`` with the projection
        formed as ``TargetAwareAttention.forward`` forms it.  Late fusion: the history mean as the one interest (K = 1), no gate.

        The category bias of the reference is a mean over the candidate rows OF THE BATCH, each user's own candidates counted
        as 0 (miner_module.py:275-285, ``ops_miner.CategBiasFn``): a function of the batch's candidate lists, and 0 for a user
        whose candidates are all their own.  There are no candidate lists here, so the poly attention runs with ``bias=None``
        whatever ``use_categ_bias`` says; ``bias`` (n_hist) takes a per-history-row bias from a caller who has one."""
        hp = self.hparams
        B = batch["batch_size"]
        if hp.late_fusion:
            hist_agg = dense_rows(hist_news_vector, batch["batch_hist"], B, batch["max_hist"], batch["hist_offsets"])
            return ops.HistMeanFn.apply(hist_agg, batch["hist_offsets"]).unsqueeze(dim=1), None
        user_vector = self.user_encoder(hist_news_vector, batch["hist_offsets"], B, batch["max_hist"], bias=bias)
        gate = None
        if hp.score_type == "weighted":
            K, D = user_vector.shape[1], user_vector.shape[2]
            z = ops_miner.BiasFreeLinearFn.apply(user_vector.reshape(B * K, D), self.target_aware_attn.linear.weight, None)
            gate = torch.nn.functional.gelu(z).view(B, K, D)
        return user_vector, gate

    # -- reference: miner_module.py:398-406 -----------------------------------------------------------
    def _aux_loss(self, batch: Dict, user_vector: torch.Tensor) -> torch.Tensor:
        return ops_miner.disagreement_loss(user_vector, bool(self.hparams.late_fusion))
