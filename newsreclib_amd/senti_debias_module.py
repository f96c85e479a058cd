"""Drop-in for ``newsreclib.models.fair_rec.senti_debias_module`` (SentiDebias: adversarial sentiment debiasing) on HIP kernels::

    model._target_:                               newsreclib_amd.senti_debias_module.SentiDebiasModule   # configs/model/senti_debias.yaml:1
    model.generator._target_:                     newsreclib_amd.senti_debias_module.Generator           # :12
    model.discriminator._target_:                 newsreclib_amd.senti_debias_module.Discriminator       # :5
    model.generator.sentiment_encoder._target_:   newsreclib_amd.senti_debias_module.SentimentEncoder    # :28

Same constructor keyword arguments (14 / 12 / 3 / 3), sub-module attribute names and ``state_dict`` keys.  The generator is the NRMS
path (``MHSAAddAtt`` / ``NewsEncoder`` / ``UserEncoder`` / ``DotProduct`` unchanged, history and candidates in one encoder call); the
head never builds a per-news sentiment vector: with ``S = num_sent_classes + 1`` ids every such vector is a row of the (S, D) table
``T = tanh(E W^T + b)``, and the kernels of ``ops_sentidebias`` read ``T[id]``.

The model trains with TWO optimizers and manual optimization (senti_debias_module.py:475-530): ``training_step`` runs a generator
phase and a discriminator phase through ``optimizers()`` / ``toggle_optimizer`` / ``manual_backward`` -- Lightning's when it is
installed, the stand-in's of ``_lightning`` otherwise; ``trainer.SentiDebiasTrainer`` drives it with the library's flat Adam.

Reproduced as they are in the reference (each cited where it is implemented): the adversarial target column ``id - 1`` with id 0
wrapping to the last column, the scalar news terms of ``loss_orth`` broadcast onto the (B, 1) user term, zero vectors (not the vector
of id 0) at padded sentiment slots, one shared ``UserEncoder`` for the news history and the sentiment history, and late fusion as
history sums divided by the history size."""
from __future__ import annotations

from typing import Any, Dict, List, Optional, Tuple

import torch
import torch.nn as nn

from . import ops, ops_sentidebias as SD
from .abstract_recommender import AbstractRecommender
from .click_predictor import DotProduct
from .dense_batch import dense_rows
from .news_encoder import MHSAAddAtt, NewsEncoder
from .nrms_module import prepare_batch
from .ops_blocks import LinearActFn
from .user_encoder import UserEncoder

COS_EPS = 1e-8          # senti_debias_module.py:212,223,235


class SentimentEncoder(nn.Module):
    """``newsreclib.models.components.encoders.news.aspect.SentimentEncoder``: embedding (padding_idx 0) -> linear -> tanh.
    The generator evaluates it once per step on its ``num_sent_classes + 1`` ids (``table``); ``forward`` keeps the reference's
    per-id interface by gathering the table's rows."""

    def __init__(self, num_sent_classes: int, sent_embed_dim: int, sent_output_dim: int) -> None:
        super().__init__()
        self.embedding_layer = nn.Embedding(num_embeddings=num_sent_classes + 1, embedding_dim=sent_embed_dim, padding_idx=0)
        self.linear = nn.Linear(in_features=sent_embed_dim, out_features=sent_output_dim)

    def table(self) -> torch.Tensor:
        return SD.sentiment_table(self)          # (the padding row of the embedding is detached there, as padding_idx = 0 asks)

    def forward(self, sentiment: torch.Tensor) -> torch.Tensor:
        return self.table().index_select(0, sentiment.reshape(-1)).reshape(*sentiment.shape, -1)


class Discriminator(nn.Module):
    """senti_debias_module.py:23-51.  ``forward`` keeps the reference's interface (two logit matrices, on the GEMM engine);
    the train step uses ``losses``, which never writes the logits out."""

    def __init__(self, input_dim: int, hidden_dim: int, output_dim: int) -> None:
        super().__init__()
        self.linear1 = nn.Linear(input_dim, hidden_dim)
        self.linear2 = nn.Linear(hidden_dim, output_dim)

    def _logits(self, x: torch.Tensor) -> torch.Tensor:
        h = LinearActFn.apply(x.contiguous(), self.linear1.weight, self.linear1.bias, "tanh", None)
        w, b = self.linear2.weight, self.linear2.bias
        n_out = w.shape[0]
        pad = (-n_out) % 4                                                 # the GEMM wants 4-column multiples
        wp = torch.cat([w, w.new_zeros(pad, w.shape[1])]) if pad else w
        bp = torch.cat([b, b.new_zeros(pad)]) if pad else b
        return LinearActFn.apply(h, wp, bp, "none", None)[:, :n_out]

    def forward(self, hist_news_vector: torch.Tensor, cand_news_vector: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        return self._logits(hist_news_vector), self._logits(cand_news_vector)

    def losses(self, news_vector: torch.Tensor, sentiment: torch.Tensor, n_hist: int) -> torch.Tensor:
        """-> (2): ``adversarial_loss`` of the history rows and of the candidate rows of ``news_vector`` (history first)."""
        return SD.DiscriminatorLossFn.apply(news_vector, self.linear1.weight, self.linear1.bias, self.linear2.weight,
                                            self.linear2.bias, sentiment, n_hist)


class Generator(nn.Module):
    def __init__(
        self,
        dataset_attributes: List[str],
        attributes2encode: List[str],
        late_fusion: bool,
        use_plm: bool,
        pretrained_embeddings_path: Optional[str],
        plm_model: Optional[str],
        frozen_layers: Optional[List[int]],
        embed_dim: int,
        num_heads: int,
        query_dim: int,
        dropout_probability: float,
        sentiment_encoder: nn.Module,
        pretrained_embeddings: Optional[torch.Tensor] = None,
    ) -> None:
        super().__init__()
        self.late_fusion = late_fusion
        if use_plm:
            raise NotImplementedError("newsreclib_amd: SentiDebias with use_plm=True is not built (the PLM encoder couples the "
                                      "news of one call; only the MHSAAddAtt generator is)")
        if pretrained_embeddings is None:
            import numpy as np
            assert isinstance(pretrained_embeddings_path, str)
            pretrained_embeddings = torch.from_numpy(np.load(pretrained_embeddings_path)).float()      # :110-111
        text_encoder = MHSAAddAtt(pretrained_embeddings=pretrained_embeddings, embed_dim=embed_dim, num_heads=num_heads,
                                  query_dim=query_dim, dropout_probability=dropout_probability)
        self.news_encoder = NewsEncoder(
            dataset_attributes=dataset_attributes, attributes2encode=attributes2encode, concatenate_inputs=False,
            text_encoder=text_encoder, category_encoder=None, entity_encoder=None, combine_vectors=False, combine_type=None,
            input_dim=None, query_dim=None, output_dim=None)
        if not self.late_fusion:
            # ONE user encoder (:150-155): the same weights encode the news history and the sentiment history (:186,189)
            self.user_encoder = UserEncoder(news_embed_dim=embed_dim, num_heads=num_heads, query_dim=query_dim)
        self.sentiment_encoder = sentiment_encoder
        self.click_predictor_bias_free = DotProduct()
        self.click_predictor_bias_aware = DotProduct()
        self._text_attr = next(iter(self.news_encoder.text_encoders.keys()))

    # -- batch layout ------------------------------------------------------------------------------------------------------
    def prepare(self, batch: Dict, max_id: Optional[int] = None) -> Dict:
        """``nrms_module.prepare_batch`` + the sentiment ids of history and candidates as the one-call kernels read them.

        The ids are validated here, once per UNPREPARED batch: two scalar read-backs, i.e. host syncs, like the layout metadata
        of ``attach_layout``.  A prepared batch passes through untouched, so a loader that prepares its batches (or a loop
        that reuses one) pays them outside the step; a collate function that already knows its ids are in range says so with
        ``batch["sentiment_ids_checked"] = True`` and no read-back happens.  The upper limit is the smaller of the table's
        last row and ``max_id`` (the module passes the discriminator's ``output_dim``: the reference raises from its Python
        loop, :408-409, for an id above it; the kernels would drop such a row from the loss)."""
        if "x_all" in batch and "sentiment" in batch["x_all"]:
            return batch
        ids = torch.cat([batch["x_hist"]["sentiment"].reshape(-1), batch["x_cand"]["sentiment"].reshape(-1)]).long()
        top = self.sentiment_encoder.embedding_layer.weight.shape[0] - 1
        if max_id is not None:
            top = min(top, int(max_id))
        if ids.numel() and not batch.get("sentiment_ids_checked", False) and (int(ids.min()) < 0 or int(ids.max()) > top):
            raise IndexError(f"newsreclib_amd: sentiment ids must lie in [0, {top}] (the sentiment table's rows and the "
                             "discriminator's outputs)")
        emb = getattr(self.news_encoder.text_encoders[self._text_attr], "embedding_layer", None)
        out = dict(prepare_batch(batch, emb.weight.shape[0] if emb is not None else None))
        out["x_all"] = dict(out.get("x_all", {}))
        out["x_all"]["sentiment"] = ids
        return out

    def encode_news(self, batch: Dict) -> torch.Tensor:
        """(n_hist + n_cand, D): history and candidate news in ONE encoder call (rows are independent: the reference's two
        calls, :168,172, give the same vectors)."""
        return self.news_encoder(batch["x_all"])

    def user_vectors(self, hist_news_vector: torch.Tensor, batch: Dict, table: Optional[torch.Tensor]):
        """-> (bias-free user vector, bias-aware user vector or None without ``table``)."""
        B = batch["batch_size"]
        hist_dense = dense_rows(hist_news_vector, batch["batch_hist"], B, batch["max_hist"], batch["hist_offsets"],
                                max_is_exact=True)
        n_hist = hist_news_vector.shape[0]
        sent_hist = batch["x_all"]["sentiment"][:n_hist] if table is not None else None
        if not self.late_fusion:
            free = self.user_encoder(hist_dense)
            if table is None:
                return free, None
            # padded slots are ZERO vectors (to_dense_batch, :177), a real row of id 0 is T[0] = tanh(linear.bias)
            aware = self.user_encoder(SD.SentHistFn.apply(table, sent_hist, batch["hist_offsets"], B, batch["max_hist"]))
            return free, aware
        free = ops.HistMeanFn.apply(hist_dense, batch["hist_offsets"])                                   # :198-200
        aware = SD.LateUserFn.apply(table, sent_hist, batch["hist_offsets"], B) if table is not None else None   # :203-205
        return free, aware

    def bias_free_scores(self, hist_news_vector: torch.Tensor, cand_news_vector: torch.Tensor, batch: Dict) -> torch.Tensor:
        free, _ = self.user_vectors(hist_news_vector, batch, None)
        cand_dense = dense_rows(cand_news_vector, batch["batch_cand"], batch["batch_size"], batch["max_cand"],
                                batch["cand_offsets"], max_is_exact=True)
        return self.click_predictor_bias_free(free.unsqueeze(dim=1), cand_dense.permute(0, 2, 1))

    # -- reference: senti_debias_module.py:164-263 ----------------------------------------------------------------------------
    def forward_full(self, batch: Dict):
        """``forward`` plus the unsplit (n_hist + n_cand, D) news vectors the discriminator's fused loss reads."""
        batch = self.prepare(batch)
        B = batch["batch_size"]
        n_hist = batch["batch_hist"].shape[0]
        sent = batch["x_all"]["sentiment"]
        news_vector = self.encode_news(batch)
        hist_news_vector, cand_news_vector = ops.split_rows(news_vector, n_hist)
        table = SD.sentiment_table(self.sentiment_encoder)      # (any encoder with `embedding_layer` and `linear`)
        user_free, user_aware = self.user_vectors(hist_news_vector, batch, table)
        # orthogonality regulariser (:208-246).  The two news terms are SCALARS (means over all history / candidate rows of the
        # batch, :208-229) and are broadcast onto the (B, 1) user term before the final mean (:241-246).
        news_cos = SD.RowCosFn.apply(news_vector, table, sent, n_hist)
        # the user term is B rows of dense against dense: six elementwise / row-reduction torch launches over (B, D), no kernel
        dot = (user_free * user_aware).sum(dim=1, keepdim=True)
        den = COS_EPS + torch.linalg.norm(user_free, dim=1, ord=2) * torch.linalg.norm(user_aware, dim=1, ord=2)
        loss_orth_user = dot / den.unsqueeze(dim=1)                                                    # (B, 1), :230-239
        loss_orth = torch.mean(torch.abs(news_cos[0]) + torch.abs(news_cos[1]) + torch.abs(loss_orth_user))
        cand_dense = dense_rows(cand_news_vector, batch["batch_cand"], B, batch["max_cand"], batch["cand_offsets"],
                                max_is_exact=True)
        bias_free_scores = self.click_predictor_bias_free(user_free.unsqueeze(dim=1), cand_dense.permute(0, 2, 1))
        combined_scores = SD.CombinedScoresFn.apply(bias_free_scores, user_aware, table, sent[n_hist:], batch["cand_offsets"])
        return (combined_scores, bias_free_scores, loss_orth, hist_news_vector, cand_news_vector), news_vector, batch

    def forward(self, batch: Dict):
        return self.forward_full(batch)[0]


class SentiDebiasModule(AbstractRecommender):
    def __init__(
        self,
        outputs: Dict[str, List[str]],
        generator: nn.Module,
        discriminator: nn.Module,
        top_k_list: List[int],
        num_categ_classes: int,
        num_sent_classes: int,
        save_recs: bool,
        recs_fpath: Optional[str],
        optimizer: Any,
        alpha_coefficient: float,
        beta_coefficient: float,
        optimizer_generator: Any,
        optimizer_discriminator: Any,
        scheduler: Any,
    ) -> None:
        super().__init__()
        self.save_hyperparameters(logger=False, ignore=["generator", "discriminator"])
        self.automatic_optimization = False                      # :327: two optimizers, stepped by training_step itself
        self.num_categ_classes = num_categ_classes + 1
        self.num_sent_classes = num_sent_classes + 1
        if save_recs:
            assert isinstance(recs_fpath, str)
        self.rec_loss = self._get_loss("cross_entropy_loss")     # :336
        self.generator = generator
        self.discriminator = discriminator
        self._init_step_outputs(outputs)
        self.last_losses = None

    # (what the shared epoch / evaluation machinery looks for on a recommender)
    @property
    def news_encoder(self):
        return self.generator.news_encoder

    def _prepare(self, batch: Dict) -> Dict:
        return self.generator.prepare(batch, max_id=self.discriminator.linear2.out_features)

    def _loss(self, scores: torch.Tensor, y_true: torch.Tensor, batch: Dict) -> torch.Tensor:
        return self.rec_loss(scores, y_true)

    def score_news_vectors(self, hist_news_vector: torch.Tensor, cand_news_vector: torch.Tensor, batch: Dict) -> torch.Tensor:
        """The bias-free scores from already-encoded news rows: what ``model_step`` ranks by (:431,443), and the entry of the
        encode-once evaluation (``evaluation.NewsVectorCache``; the news vectors do not depend on the user)."""
        return self.generator.bias_free_scores(hist_news_vector, cand_news_vector, batch)

    # Ranking the whole news table (``evaluation.NewsVectorCache.recommend_biased`` / ``rank_clicks_biased``).  The module has no
    # ``dot_product_scorer``: its trained score is a dot product PLUS a term per (user, sentiment class), which the class-biased
    # top-k entries of ``ops`` rank by; the classes are the table's ``class_bias_aspect`` column.
    class_biased_scorer = True
    class_bias_aspect = "sentiment"

    def user_vectors_and_bias(self, hist_news_vector: torch.Tensor, meta: Dict, hist_classes: Optional[torch.Tensor],
                              combined: bool) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
        """-> (u_free (B, D), bias (B, S) or None) from already-encoded history rows and the history meta of the cache
        (``Generator.user_vectors``).  ``combined=False``: the bias-free score ``u_free . n_v`` alone, what ``model_step`` ranks
        by; the sentiment half is not evaluated.  ``combined=True``: ``bias = u_aware T^T``, so that ``u_free . n_v + bias[u,
        sentiment(v)]`` is the combined score ``Generator.forward_full`` trains on; ``hist_classes`` (n_hist) are the history
        rows' sentiment ids.  The bias is ``CombinedScoresFn`` over a candidate list of the S classes per user and zero bias-free
        scores: the very values the training-time score adds, each a function of its user and its class alone."""
        gen = self.generator
        if not combined:
            return gen.user_vectors(hist_news_vector, meta, None)[0], None
        batch = dict(meta)
        batch["x_all"] = {"sentiment": hist_classes.reshape(-1).long()}
        table = SD.sentiment_table(gen.sentiment_encoder)
        free, aware = gen.user_vectors(hist_news_vector, batch, table)
        B, S = free.shape[0], table.shape[0]
        ids = torch.arange(S, device=free.device).repeat(B)
        off = torch.arange(B + 1, device=free.device) * S
        return free, SD.CombinedScoresFn.apply(free.new_zeros((B, S)), aware, table, ids, off)

    def forward(self, batch: Dict):
        return self.generator(batch)

    # -- reference: senti_debias_module.py:406-411 ------------------------------------------------------------------------------
    def adversarial_loss(self, preds: torch.Tensor, targets: torch.Tensor) -> torch.Tensor:
        """The reference's interface over logits: the one-hot sits at column ``targets[i] - 1`` (:409), so sentiment id 0 --
        news without a known sentiment -- wraps to the LAST column; CrossEntropyLoss with probability targets is the mean
        over rows of ``-log_softmax`` at that column.  (The train step computes the same value inside the discriminator's
        fused tail, ``Discriminator.losses``, without the logits.)"""
        n_out = preds.shape[1]
        if targets.numel() and int(targets.max()) > n_out:
            raise IndexError(f"index {int(targets.max()) - 1} is out of bounds for dimension 1 with size {n_out}")
        col = torch.where(targets == 0, torch.full_like(targets, n_out - 1), targets - 1)
        return -torch.log_softmax(preds, dim=1).gather(1, col.reshape(-1, 1)).mean()

    # -- reference: senti_debias_module.py:417-473 ------------------------------------------------------------------------------
    def model_step(self, batch: Dict) -> Tuple:
        batch = self._prepare(batch)
        n_hist = batch["batch_hist"].shape[0]
        if torch.is_grad_enabled():
            _, scores, _, _, _ = self.forward(batch)
        else:                       # only the bias-free scores are used (:431): the sentiment half is not evaluated
            hist_vec, cand_vec = ops.split_rows(self.generator.encode_news(batch), n_hist)
            scores = self.score_news_vectors(hist_vec, cand_vec, batch)
        # gathering the valid slots in row-major order == the reference's per-user concatenation; no loops, no syncs
        if batch["labels"].shape[0] == scores.numel():
            preds = scores.detach().reshape(-1)
        else:
            preds = scores.detach().reshape(-1)[batch["cand_flat_idx"]]

        def attr(side, name):
            v = batch["x_" + side].get(name)
            return v if v is not None else torch.empty(0, dtype=torch.int64, device=scores.device)

        return (preds, batch["labels"], batch["cand_sizes"], batch["hist_sizes"], attr("cand", "category"),
                attr("cand", "sentiment"), attr("hist", "category"), attr("hist", "sentiment"), batch["user_ids"],
                attr("cand", "news_ids"))

    # -- reference: senti_debias_module.py:475-530 ------------------------------------------------------------------------------
    def adversarial_step(self, batch: Dict):
        """Both phases of one train step -> (g_loss, d_loss, phase G's bias-free scores, the prepared batch)."""
        hp = self.hparams
        optimizer_g, optimizer_d = self.optimizers()
        batch = self._prepare(batch)
        n_hist = batch["batch_hist"].shape[0]
        sent = batch["x_all"]["sentiment"]
        y_true = dense_rows(batch["labels"], batch["batch_cand"], batch["batch_size"], batch["max_cand"],
                            batch["cand_offsets"], batch["cand_flat_idx"], max_is_exact=True).float()

        # train generator (:479-504)
        self.toggle_optimizer(optimizer_g)
        (combined_scores, bias_free_scores, loss_orth, _, _), news_vector, _ = self.generator.forward_full(batch)
        adv = self.discriminator.losses(news_vector, sent, n_hist)
        g_loss = self.rec_loss(combined_scores, y_true) + hp.beta_coefficient * loss_orth \
            - hp.alpha_coefficient * (adv[0] + adv[1])
        self.log("g_loss", g_loss, prog_bar=True)
        self.manual_backward(g_loss)
        optimizer_g.step()
        optimizer_g.zero_grad()
        self.untoggle_optimizer(optimizer_g)

        # train discriminator (:507-518).  The reference runs the whole generator again and keeps the news vectors only: a news
        # encoder forward in train mode with its own dropout draw over the weights phase G just wrote (the generator's flags
        # are off, so nothing is saved for a backward)
        self.toggle_optimizer(optimizer_d)
        adv = self.discriminator.losses(self.generator.encode_news(batch), sent, n_hist)
        d_loss = adv[0] + adv[1]
        self.log("d_loss", d_loss, prog_bar=True)
        self.manual_backward(d_loss)
        optimizer_d.step()
        optimizer_d.zero_grad()
        self.untoggle_optimizer(optimizer_d)
        self.last_losses = (g_loss.detach(), d_loss.detach())
        return g_loss.detach(), d_loss.detach(), bias_free_scores.detach(), batch

    def training_step(self, batch: Dict, batch_idx: int):
        _, _, scores, batch = self.adversarial_step(batch)
        preds = scores.reshape(-1) if batch["labels"].shape[0] == scores.numel() else scores.reshape(-1)[batch["cand_flat_idx"]]
        targets, cand_news_size = batch["labels"], batch["cand_sizes"]
        self.training_step_outputs = self._collect_step_outputs(self.training_step_outputs, locals())

    def validation_step(self, batch: Dict, batch_idx: int):
        preds, targets, cand_news_size, *_ = self.model_step(batch)
        self.val_step_outputs = self._collect_step_outputs(self.val_step_outputs, locals())

    def test_step(self, batch: Dict, batch_idx: int):
        (preds, targets, cand_news_size, hist_news_size, target_categories, target_sentiments, hist_categories,
         hist_sentiments, user_ids, cand_news_ids) = self.model_step(batch)
        self.test_step_outputs = self._collect_step_outputs(self.test_step_outputs, locals())

    # -- reference: senti_debias_module.py:672-679 ------------------------------------------------------------------------------
    def configure_optimizers(self):
        optimizer_generator = self.hparams.optimizer_generator(params=self.generator.parameters())
        optimizer_discriminator = self.hparams.optimizer_discriminator(params=self.discriminator.parameters())
        return [optimizer_generator, optimizer_discriminator]
