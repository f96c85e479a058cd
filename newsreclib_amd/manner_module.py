"""Drop-in for ``newsreclib.models.fair_rec.manner_module.MANNERModule`` (MANNeR's inference-time ensemble) on MI355X HIP kernels::

    model._target_: newsreclib_amd.manner_module.MANNERModule          # configs/model/manner.yaml:1

Same 13 constructor keyword arguments (manner_module.py:54-69).  ``cr_module`` is always loaded, ``a_module_categ`` /
``a_module_sent`` only when their weight is != 0 (:83-96), each through its class's ``load_from_checkpoint``; ``plm_model=`` given
here is handed to all of them as an override (a hub name cannot be resolved offline).  ``MANNERModule.from_modules(cr_module,
a_module_categ=None, a_module_sent=None, **kw)`` builds the ensemble around modules the caller already holds.

``forward`` (manner_module.py:152-204): every loaded sub-model encodes the history and the candidate news with its own news encoder;
the per-impression mean of the history vectors, the dot product with every candidate, the z-score over the impression's own
candidates (unbiased standard deviation) and the weighted sum ``cr + categ_weight * categ + sent_weight * sent`` are ONE launch
(``ops_manner.manner_scores`` -> ``nrl_manner_scores``) that reads the encoded rows through identity index lists.
``evaluation.MannerVectorCache`` is the encode-once form over cached tables.

Reference quirks kept: an impression with a single candidate has ``torch.std = NaN`` and so a NaN row; zero score variance gives
inf / NaN; no epsilon is added.  The module has no loss; ``training_step`` / ``validation_step`` do nothing, as in the reference."""
from __future__ import annotations

from typing import Any, Dict, List, Optional

import torch

from .abstract_recommender import AbstractRecommender
from .click_predictor import DotProduct
from .manner_a_module import AModule
from .manner_cr_module import CRModule
from .nrms_module import prepare_batch
from .ops_manner import manner_scores


class MANNERModule(AbstractRecommender):
    def __init__(
        self,
        outputs: Dict[str, List[str]],
        cr_module_module_ckpt: str,
        a_module_categ_ckpt: Optional[str],
        a_module_sent_ckpt: Optional[str],
        categ_weight: Optional[float],
        sent_weight: Optional[float],
        top_k_list: List[int],
        num_categ_classes: int,
        num_sent_classes: int,
        save_recs: bool,
        recs_fpath: Optional[str],
        optimizer: Any,
        scheduler: Any,
        plm_model: Optional[str] = None,
        _modules_given: Optional[Dict[str, Any]] = None,
    ) -> None:
        super().__init__()
        self.save_hyperparameters(logger=False, ignore=["plm_model", "_modules_given"])
        self.num_categ_classes = num_categ_classes + 1          # manner_module.py:76-77
        self.num_sent_classes = num_sent_classes + 1
        if save_recs:
            assert isinstance(recs_fpath, str)
        over = {} if plm_model is None else {"plm_model": plm_model}
        given = _modules_given or {}
        if "cr_module" in given:
            self.cr_module = given["cr_module"]
        else:
            self.cr_module = CRModule.load_from_checkpoint(checkpoint_path=cr_module_module_ckpt, **over)
        if categ_weight != 0:                                    # :87-96
            if given.get("a_module_categ") is not None:
                self.a_module_categ = given["a_module_categ"]
            else:
                assert isinstance(a_module_categ_ckpt, str)
                self.a_module_categ = AModule.load_from_checkpoint(checkpoint_path=a_module_categ_ckpt, **over)
        if sent_weight != 0:
            if given.get("a_module_sent") is not None:
                self.a_module_sent = given["a_module_sent"]
            else:
                assert isinstance(a_module_sent_ckpt, str)
                self.a_module_sent = AModule.load_from_checkpoint(checkpoint_path=a_module_sent_ckpt, **over)
        self.click_predictor = DotProduct()
        self._init_step_outputs(outputs)

    @classmethod
    def from_modules(cls, cr_module, a_module_categ=None, a_module_sent=None, **kw):
        """The ensemble around modules the caller holds; ``kw``: the remaining constructor arguments (``outputs``,
        ``categ_weight``, ``sent_weight``, ``top_k_list``, ``num_categ_classes``, ``num_sent_classes``, ...).  A weight != 0 needs
        its module."""
        kw.setdefault("cr_module_module_ckpt", None)
        kw.setdefault("a_module_categ_ckpt", None)
        kw.setdefault("a_module_sent_ckpt", None)
        for name in ("save_recs", "recs_fpath", "optimizer", "scheduler"):
            kw.setdefault(name, False if name == "save_recs" else None)
        if kw.get("categ_weight") and a_module_categ is None:
            raise ValueError("categ_weight != 0 needs a_module_categ")
        if kw.get("sent_weight") and a_module_sent is None:
            raise ValueError("sent_weight != 0 needs a_module_sent")
        return cls(_modules_given={"cr_module": cr_module, "a_module_categ": a_module_categ, "a_module_sent": a_module_sent}, **kw)

    def submodels(self):
        """[(sub-model, weight)] in the order of the weighted sum: the CR-Module with weight 1 first."""
        out = [(self.cr_module, 1.0)]
        if self.hparams.categ_weight != 0:
            out.append((self.a_module_categ, float(self.hparams.categ_weight)))
        if self.hparams.sent_weight != 0:
            out.append((self.a_module_sent, float(self.hparams.sent_weight)))
        return out

    def _prepare(self, batch: Dict) -> Dict:
        return prepare_batch(batch, None, need_order=False)

    # -- reference: manner_module.py:152-204 -----------------------------------------------------------
    def forward(self, batch: Dict) -> torch.Tensor:
        batch = self._prepare(batch)
        n_hist, n_cand = int(batch["batch_hist"].shape[0]), int(batch["batch_cand"].shape[0])
        tables, weights = [], []
        for model, weight in self.submodels():
            enc = model.news_encoder
            enc.share_plm_bodies(batch["x_hist"], batch["x_cand"])
            tables.append(torch.cat([enc(batch["x_hist"]), enc(batch["x_cand"])], dim=0))      # rows: history, then candidates
            weights.append(weight)
        dev = tables[0].device
        hist_idx = torch.arange(n_hist, device=dev)
        cand_idx = torch.arange(n_hist, n_hist + n_cand, device=dev)
        return manner_scores(tables, weights, hist_idx, batch["hist_offsets"], cand_idx, batch["cand_offsets"], batch["max_cand"])

    def model_step(self, batch: Dict):
        """The reference's 10-tuple (manner_module.py:254-265): no loss."""
        return AbstractRecommender.model_step(self, batch)[1:]

    def _loss(self, scores, y_true, batch):
        return scores.new_zeros(())

    def training_step(self, batch: Dict, batch_idx: int):
        pass

    def validation_step(self, batch: Dict, batch_idx: int):
        pass

    def test_step(self, batch: Dict, batch_idx: int):
        (preds, targets, cand_news_size, hist_news_size, target_categories, target_sentiments, hist_categories, hist_sentiments,
         user_ids, cand_news_ids) = self.model_step(batch)
        self.test_step_outputs = self._collect_step_outputs(self.test_step_outputs, locals())

    def on_test_epoch_start(self) -> None:
        pass
