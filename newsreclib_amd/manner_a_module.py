"""Drop-in for ``newsreclib.models.fair_rec.manner_a_module.AModule`` (MANNeR's aspect module) on MI355X HIP kernels::

    model._target_: newsreclib_amd.manner_a_module.AModule          # configs/model/manner_a_module.yaml:1

Same 16 constructor keyword arguments (manner_a_module.py:63-81) and ``state_dict`` keys: one ``news_encoder`` built exactly as
``CRModule``'s.  ``forward(batch) = news_encoder(batch["news"])``; ``model_step`` -> ``(loss, embeddings, labels)`` with
pytorch-metric-learning's ``SupConLoss(temperature, DotProductSimilarity(normalize_embeddings=False))`` over the batch's embeddings
and integer aspect labels -- one fused forward + backward call (``ops_manner.SupConEmbedLoss`` -> ``nrl_supcon_embed_fwd_bwd``).

NOT built: the t-SNE scatter plots the reference draws in ``on_validation_epoch_end`` (every 10th epoch) and
``on_test_epoch_end`` (manner_a_module.py:220-245,270-291).  MulticoreTSNE, seaborn and colorcet are not dependencies of this
package; the hooks log the losses and clear the collected ``embeddings`` / ``labels``, nothing else.  ``labels_path`` is accepted and
``index2label`` is loaded when the file exists (tab-separated ``label<TAB>index`` lines, as the reference's
``load_idx_map_as_dict`` reads them); it only ever served the plot legends."""
from __future__ import annotations

import os
from typing import Any, Dict, List, Optional

import torch

from .abstract_recommender import AbstractRecommender
from .manner_cr_module import build_manner_news_encoder, load_module_from_checkpoint
from .news_encoder import _draw_seed
from .ops_manner import SupConEmbedLoss


def load_idx_map_as_dict(filepath: str) -> Dict[str, int]:
    out: Dict[str, int] = {}
    with open(filepath, encoding="utf-8") as f:
        for line in f:
            if line.strip():
                key, value = line.rstrip("\n").split("\t")
                out[key] = int(value)
    return out


class AModule(AbstractRecommender):
    def __init__(
        self,
        dataset_attributes: List[str],
        attributes2encode: List[str],
        outputs: Dict[str, List[str]],
        temperature: float,
        labels_path: str,
        plm_model: Optional[str],
        frozen_layers: Optional[List[int]],
        text_embed_dim: int,
        num_heads: int,
        query_dim: int,
        dropout_probability: float,
        use_entities: bool,
        pretrained_entity_embeddings_path: str,
        entity_embed_dim: int,
        optimizer: Any,
        scheduler: Any,
        pretrained_entity_embeddings: Optional[torch.Tensor] = None,
    ) -> None:
        super().__init__()
        self.save_hyperparameters(logger=False, ignore=["pretrained_entity_embeddings"])
        self.news_encoder = build_manner_news_encoder(self, self.hparams, pretrained_entity_embeddings)
        self.index2label: Dict[int, str] = {}
        if isinstance(labels_path, str) and os.path.isfile(labels_path):
            self.index2label = {v: k for k, v in load_idx_map_as_dict(labels_path).items()}
        self.criterion = SupConEmbedLoss(temperature=temperature)          # manner_a_module.py:151-153
        self._init_step_outputs(outputs)

    load_from_checkpoint = classmethod(load_module_from_checkpoint)

    def forward(self, batch: Dict, seed: Optional[int] = None) -> torch.Tensor:
        if seed is None and self.training and self.hparams.dropout_probability > 0.0:
            seed = _draw_seed()
        return self.news_encoder(batch["news"], seed=seed)

    def model_step(self, batch: Dict):
        embeddings = self.forward(batch)
        labels = batch["labels"]
        loss = self.criterion(embeddings, labels.long())
        return loss, embeddings, labels

    def training_step(self, batch: Dict, batch_idx: int):
        loss, embeddings, labels = self.model_step(batch)
        self._track("train", loss)
        return loss

    def validation_step(self, batch: Dict, batch_idx: int):
        loss, embeddings, labels = self.model_step(batch)
        self._track("val", loss)
        self.val_step_outputs = self._collect_step_outputs(self.val_step_outputs, locals())

    def test_step(self, batch: Dict, batch_idx: int):
        loss, embeddings, labels = self.model_step(batch)
        self._track("test", loss)
        self.test_step_outputs = self._collect_step_outputs(self.test_step_outputs, locals())

    def on_train_epoch_end(self) -> None:
        self._epoch_end("train", {})

    def on_validation_epoch_start(self) -> None:
        pass

    def on_test_epoch_start(self) -> None:
        pass

    def on_validation_epoch_end(self) -> None:
        logs = self._epoch_end("val", self.val_step_outputs)          # logs the loss, clears the collected outputs; no plot
        if "val/loss" in logs:
            self.val_loss_best = min(self.val_loss_best, logs["val/loss"])
            self.log("val/loss_best", self.val_loss_best, prog_bar=True, logger=True, sync_dist=True)

    def on_test_epoch_end(self) -> None:
        self._epoch_end("test", self.test_step_outputs)
