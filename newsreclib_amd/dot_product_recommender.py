"""What the recommenders that score a news by ONE dot product with a candidate-independent user vector share (NRMS, SentiRec,
LSTUR, NAML, TANR, CenNewsRec, MINS, MANNeR's CR-Module): the forward and the scoring from already-encoded news rows.  A family
writes its constructor and ``_encode_user``; DESIGN.md section 7h."""
from __future__ import annotations

from typing import Dict, Optional

import torch

from . import ops
from .abstract_recommender import AbstractRecommender
from .batch_layout import prepare_batch, text_vocab
from .dense_batch import dense_rows
from .news_encoder import _draw_seed


class DotProductRecommender(AbstractRecommender):
    dot_product_scorer = True                # score = user_vectors(...) . news vector (evaluation.NewsVectorCache.recommend)
    # True where a longest list always fills ``max_hist`` / ``max_cand`` exactly, so that a batch of full rows is a reshape and
    # no kernel runs (``dense_rows``).  Part of a family's bits: not to be harmonised across families.
    dense_max_is_exact = False

    def _prepare(self, batch: Dict) -> Dict:
        return prepare_batch(batch, text_vocab(self))

    def _encode_user(self, hist_dense: torch.Tensor, batch: Dict, seed: Optional[int]) -> torch.Tensor:
        """(B, max_hist, D) zero-padded history vectors -> (B, D): the family's user encoder (early fusion only)."""
        raise NotImplementedError

    def _encode_and_score(self, batch: Dict, seed: Optional[int]):
        """-> (scores, history news vectors, candidate news vectors): the whole forward, for families that return more than
        the scores (TANR's topic scores over the same news vectors)."""
        batch = self._prepare(batch)
        if self.training and seed is None:
            seed = _draw_seed()                       # one draw per step; streams separate the dropouts
        hist_vec, cand_vec = self._encode_news(batch, seed)
        return self.score_news_vectors(hist_vec, cand_vec, batch, seed=seed), hist_vec, cand_vec

    def forward(self, batch: Dict, seed: Optional[int] = None) -> torch.Tensor:
        return self._encode_and_score(batch, seed)[0]

    def score_news_vectors(self, hist_news_vector: torch.Tensor, cand_news_vector: torch.Tensor, batch: Dict,
                           seed: Optional[int] = None) -> torch.Tensor:
        """The reference's forward after its two encoder calls (e.g. nrms_module.py:233-253), from already-encoded news rows:
        also the entry of the evaluation path that encodes every unique news once (``evaluation.NewsVectorCache``)."""
        user_vector = self.user_vectors(hist_news_vector, batch, seed=seed)
        cand_news_vector_agg = dense_rows(cand_news_vector, batch["batch_cand"], batch["batch_size"], batch["max_cand"],
                                          batch["cand_offsets"], max_is_exact=self.dense_max_is_exact)
        return self.click_predictor(user_vector.unsqueeze(dim=1), cand_news_vector_agg.permute(0, 2, 1))

    def user_vectors(self, hist_news_vector: torch.Tensor, batch: Dict, seed: Optional[int] = None) -> torch.Tensor:
        """The candidate-independent half of ``score_news_vectors``: dense history rows, then the user encoder (or the history
        mean under late fusion) -> (B, D).  The score of any news is one dot product with it (``dot_product_scorer``), which is
        what ``evaluation.NewsVectorCache.recommend`` ranks the whole table by."""
        hist_news_vector_agg = dense_rows(hist_news_vector, batch["batch_hist"], batch["batch_size"], batch["max_hist"],
                                          batch["hist_offsets"], max_is_exact=self.dense_max_is_exact)
        if not self.hparams.late_fusion:
            return self._encode_user(hist_news_vector_agg, batch, seed)
        # aggregate embeddings of clicked news (nrms_module.py:243-248)
        return ops.HistMeanFn.apply(hist_news_vector_agg, batch["hist_offsets"])
