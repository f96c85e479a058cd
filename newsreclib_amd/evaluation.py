"""Evaluation path: device-resident news table, batches built by index, and
scoring of full impressions with every unique news encoded ONCE.

The reference re-tokenises and re-encodes every history and candidate news of every impression in every
validation / test batch (``rec_dataset.py:98-121,148-293`` -> ``nrms_module.py:230-255``): with ~37 candidates
and up to 50 clicks per impression over a pool of ~65k news that is ~50x redundant work, and the collate does
pandas ``.loc`` + per-row ``F.pad`` on the host.  Here

* ``DeviceNewsTable`` keeps the pre-tokenised attributes of all news in HBM (one row per unique news) and
  builds a ``RecommendationBatch`` from per-impression news-index lists with index gathers on the device --
  the same layout ``DatasetCollate`` produces (concatenated rows + sorted assignment vectors);
* ``NewsVectorCache`` runs the module's news encoder over the table once (eval mode: no dropout, rows are
  independent, so the cached vector of a news is BIT-IDENTICAL to what any batch would compute for it) and
  then scores impressions from gathered vectors through the module's own user encoder and click predictor
  (``score_news_vectors``).  The seq-first user-attention quirk still couples the users of a batch, exactly
  as in the uncached forward, so scores match the uncached path for the same batch composition.

* ``NpaFeatureCache`` is the NPA form: its news vectors depend on the user, so it caches the conv feature maps (the part that
  does not) and scores from them with ``nrl_npa_cached_scores``.

Everything runs through the same C-ABI kernels; nothing here is a second implementation of the model.
"""
from __future__ import annotations

import contextlib
import math
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from . import ops
from .dense_batch import dense_rows
from .news_encoder import token_tables
from .nrms_module import prepare_batch

TEXT_ATTRS = ("title", "abstract")
ASPECT_ATTRS = ("category", "subcategory", "sentiment")


@contextlib.contextmanager
def eval_mode(module):
    """``module`` in eval mode for the scope, back in the mode it was in afterwards -- also when the scope raises (a module left
    in eval mode trains on without dropout and nothing reports it)."""
    was_training = module.training
    module.eval()
    try:
        yield module
    finally:
        module.train(was_training)


def ragged_offsets(sizes: torch.Tensor, device) -> torch.Tensor:
    """(B) list lengths -> (B + 1) int64 start offsets on ``device``."""
    sizes = sizes.to(device).long()
    return torch.cat([sizes.new_zeros(1), torch.cumsum(sizes, 0)])


def _map_rows(v, fn):
    """fn over a news attribute: a tensor, or the dict of tensors of a PLM's tokenised text."""
    return {k: fn(t) for k, t in v.items()} if isinstance(v, dict) else fn(v)


class DeviceNewsTable:
    """attrs: name -> (num_news, ...) tensor (token ids (num_news, L) int64 for text attributes, (num_news,)
    int64 for category / sentiment ...) or, for a PLM's tokenised text, a dict of such tensors (``input_ids``,
    ``attention_mask``).  Row 0 may be a padding news; indices are plain row numbers."""

    def __init__(self, attrs: Dict[str, torch.Tensor], device="cuda"):
        if not attrs:
            raise ValueError("DeviceNewsTable needs at least one news attribute")
        n = {int(t.shape[0]) for v in attrs.values() for t in (v.values() if isinstance(v, dict) else (v,))}
        if len(n) != 1:
            raise ValueError(f"all news attributes must have the same number of rows, got {sorted(n)}")
        self.num_news = n.pop()
        self.attrs = {k: _map_rows(v, lambda t: t.to(device).contiguous()) for k, v in attrs.items()}
        self.device = torch.device(device)

    def gather(self, idx: torch.Tensor) -> Dict[str, torch.Tensor]:
        return {k: _map_rows(v, lambda t: t.index_select(0, idx)) for k, v in self.attrs.items()}

    def build_batch(self, hist_idx: torch.Tensor, hist_sizes: torch.Tensor, cand_idx: torch.Tensor,
                    cand_sizes: torch.Tensor, labels: torch.Tensor, user_idx: Optional[torch.Tensor] = None,
                    user_ids: Optional[torch.Tensor] = None) -> Dict:
        """The collated batch of ``rec_dataset.py:289-293`` from index lists: ``x_hist`` / ``x_cand`` hold the
        rows of the clicked / candidate news (concatenated over impressions), ``batch_hist`` / ``batch_cand``
        the sorted impression number of every row."""
        dev = self.device
        hist_idx, cand_idx = hist_idx.to(dev), cand_idx.to(dev)
        hist_sizes, cand_sizes = hist_sizes.to(dev).long(), cand_sizes.to(dev).long()
        B = int(hist_sizes.numel())
        if int(cand_sizes.numel()) != B:
            raise ValueError("hist_sizes and cand_sizes must have one entry per impression")
        ar = torch.arange(B, device=dev)
        batch = {
            "x_hist": self.gather(hist_idx), "x_cand": self.gather(cand_idx),
            "batch_hist": torch.repeat_interleave(ar, hist_sizes), "batch_cand": torch.repeat_interleave(ar, cand_sizes),
            "labels": labels.to(dev).float(),
            "user_idx": user_idx.to(dev) if user_idx is not None else ar.clone(),
            "user_ids": user_ids.to(dev) if user_ids is not None else ar + 1,
            "batch_size": B,
        }
        if "news_ids" not in self.attrs:            # no id column in the table: the row number stands in
            batch["x_cand"]["news_ids"] = cand_idx
        return batch


class _ImpressionCache:
    """What the encode-once caches share: the batch metadata of a list of impressions given by news indices, and the
    ``model_step`` tuple over the cache's own ``scores`` (``self.module`` / ``self.table`` are the subclass's)."""
    user_idx_reason: Optional[str] = None       # why ``model_step`` cannot do without ``user_idx``, where it cannot (NPA)

    def _meta(self, hist_sizes, cand_sizes, labels, user_idx, user_ids) -> Dict:
        dev = self.table.device
        hist_sizes, cand_sizes = hist_sizes.to(dev).long(), cand_sizes.to(dev).long()
        B = int(hist_sizes.numel())
        ar = torch.arange(B, device=dev)
        meta = {
            "x_hist": {}, "x_cand": {},
            "batch_hist": torch.repeat_interleave(ar, hist_sizes), "batch_cand": torch.repeat_interleave(ar, cand_sizes),
            "labels": labels.to(dev).float() if labels is not None else None,
            "user_idx": user_idx.to(dev) if user_idx is not None else ar.clone(),
            "user_ids": user_ids.to(dev) if user_ids is not None else ar + 1,
            "batch_size": B,
        }
        return prepare_batch(meta)

    def _step_loss(self, scores: torch.Tensor, meta: Dict) -> torch.Tensor:
        y_true = dense_rows(meta["labels"], meta["batch_cand"], meta["batch_size"], meta["max_cand"], meta["cand_offsets"],
                            meta["cand_flat_idx"])
        return self.module._loss(scores, y_true.float(), meta)

    @torch.no_grad()
    def model_step(self, hist_idx, hist_sizes, cand_idx, cand_sizes, labels, user_idx=None, user_ids=None):
        """The tuple ``model_step`` returns (loss, preds, targets, cand_news_size, hist_news_size, aspects ...)
        for a batch given by index lists; feeds ``test_step`` / the epoch-end metrics unchanged."""
        if user_idx is None and self.user_idx_reason:
            raise ValueError(f"{type(self).__name__}.model_step needs user_idx: {self.user_idx_reason}")
        dev = self.table.device
        scores = self.scores(hist_idx, hist_sizes, cand_idx, cand_sizes, user_idx)      # (builds the cache at its first use)
        meta = self._meta(hist_sizes, cand_sizes, labels, user_idx, user_ids)
        loss = self._step_loss(scores, meta)
        preds = scores.reshape(-1)[meta["cand_flat_idx"]]
        empty = torch.empty(0, dtype=torch.int64, device=dev)

        def attr(idx, name):
            return self.table.attrs[name].index_select(0, idx.to(dev)) if name in self.table.attrs else empty

        return (loss, preds, meta["labels"], meta["cand_sizes"], meta["hist_sizes"], attr(cand_idx, "category"),
                attr(cand_idx, "sentiment"), attr(hist_idx, "category"), attr(hist_idx, "sentiment"),
                meta["user_ids"], cand_idx.to(dev))


def _click_sizes(who: str, hist_idx, hist_sizes, click_idx, click_sizes) -> torch.Tensor:
    """The checks ``rank_clicks`` makes on the click side, for ``who``: the limit from the HOST sizes (``ValueError``) and both
    index lists on the GPU -> the sizes as a host int64 tensor; nothing is read back."""
    cs = click_sizes.detach().cpu().long()                  # host sizes: the limit and the offsets cost no read-back
    if cs.numel() != int(hist_sizes.numel()):
        raise ValueError("newsreclib_amd: hist_sizes and click_sizes must have one entry per user")
    if cs.numel() and int(cs.max()) > ops.RANK_MAX_TARGETS:
        raise ValueError(f"newsreclib_amd: {who} takes at most {ops.RANK_MAX_TARGETS} clicks per user (got {int(cs.max())})")
    if not hist_idx.is_cuda or not click_idx.is_cuda:
        raise RuntimeError(f"newsreclib_amd: `hist_idx` and `click_idx` must live on the GPU (got {hist_idx.device} and "
                           f"{click_idx.device}); there is no CPU path")
    return cs


def _click_offsets(cs: torch.Tensor, dev) -> torch.Tensor:
    return torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(cs, 0)]).pin_memory().to(dev, non_blocking=True)


def _catalogue_side(who: str, cache, hist_idx, hist_sizes, eligible, clicks):
    """The caller's side of a whole-table method ``who``, checked and moved to the device of ``cache``'s table (which is not
    touched before every check has passed).  ``clicks`` None (a ``recommend*``): ``hist_idx`` must live on the GPU; ``clicks``
    (click_idx, click_sizes) (a ``rank_clicks*``): the checks of ``_click_sizes`` -> (hist_idx int64, eligible or None, the click
    lists as ``ops.catalogue_*ranks`` take them: (click_idx, click_off), or ())."""
    if clicks is None:
        if not hist_idx.is_cuda:
            raise RuntimeError(f"newsreclib_amd: `hist_idx` must live on the GPU (got {hist_idx.device}); there is no CPU path")
    else:
        cs = _click_sizes(who, hist_idx, hist_sizes, *clicks)
    dev = cache.table.device
    targets = () if clicks is None else (clicks[0].to(dev).long(), _click_offsets(cs, dev))
    return hist_idx.to(dev).long(), eligible.to(dev) if eligible is not None else None, targets


def _aspect_classes(cache, aspect: str) -> torch.Tensor:
    """The class of every news under ``aspect`` as the capped top-k entries take it: ``cache.table.attrs[aspect]`` (one integer
    per news: ``category``, ``subcategory``, ``sentiment``) as int32, converted once per aspect and kept on the cache."""
    got = cache._row_class.get(aspect)
    if got is None:
        col = cache.table.attrs.get(aspect)
        if not isinstance(col, torch.Tensor) or col.dim() != 1 or col.is_floating_point():
            raise ValueError(f"newsreclib_amd: a class cap needs an integer news attribute with one value per news; the table has "
                             f"no such `{aspect}`")
        got = cache._row_class[aspect] = col.to(torch.int32)
    return got


def _row_times(cache) -> torch.Tensor:
    """The time of every news as the windowed entries take it: ``cache.table.attrs["time"]`` (one integer per news, in any unit)
    as int32, converted once and kept on the cache.  The values must already fit int32: the conversion is one device op and
    checking the range would cost a read-back, so a wider value (epoch milliseconds in int64) wraps silently -- rebase or rescale
    such a column on the host first."""
    if cache._row_time is None:
        col = cache.table.attrs.get("time")
        if not isinstance(col, torch.Tensor) or col.dim() != 1 or col.is_floating_point():
            raise ValueError("newsreclib_amd: a time window needs an integer news attribute `time` with one value per news (or the "
                             "times as the window's third member); the table has none")
        cache._row_time = col.to(torch.int32)
    return cache._row_time


def _window_arrays(cache, window):
    """``window`` = (win_lo, win_hi[, row_time]) of ``recommend`` / ``rank_clicks`` as ``ops.topk_window_scores`` takes it ->
    (row_time, win_lo, win_hi), int32 on the table's device.  Host bounds go through pinned memory; nothing is read back."""
    if not isinstance(window, (tuple, list)) or len(window) not in (2, 3):
        raise ValueError("newsreclib_amd: window = (win_lo, win_hi) or (win_lo, win_hi, row_time)")
    dev = cache.table.device
    row_time = _row_times(cache) if len(window) == 2 else window[2]

    def up(t, name):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int32:
            raise TypeError(f"newsreclib_amd: the window's `{name}` must be an int32 tensor")
        return t if t.is_cuda else t.pin_memory().to(dev, non_blocking=True)

    return up(row_time, "row_time"), up(window[0], "win_lo"), up(window[1], "win_hi")


def user_windows(users: Sequence[Dict], before, after):
    """The window of each user dictionary around its request: ``[time - before, time + after]`` in Python integers, clamped to
    int32 (``None`` for a side: unbounded) -> (win_lo, win_hi) host int32 tensors.  ``ValueError`` when a user has no ``"time"``."""
    lo, hi = [], []
    for j, u in enumerate(users):
        if "time" not in u:
            raise ValueError(f"newsreclib_amd: a time window needs every user's request time: user {j} of the list has no \"time\"")
        t = int(u["time"])
        lo.append(ops.INT32_MIN if before is None else min(max(t - int(before), ops.INT32_MIN), ops.INT32_MAX))
        hi.append(ops.INT32_MAX if after is None else min(max(t + int(after), ops.INT32_MIN), ops.INT32_MAX))
    return torch.tensor(lo, dtype=torch.int32), torch.tensor(hi, dtype=torch.int32)


def _window_refusal(who: str, cache) -> None:
    """``NotImplementedError`` where the windowed walk has no kernel: only the plain dot-product producer runs under it."""
    module = getattr(cache, "module", None)
    kind = [a for a in ("multi_interest_scorer", "dnn_predictor_scorer", "personalized_pooling_scorer", "class_biased_scorer")
            if getattr(module, a, False)]
    if hasattr(cache, "recommend_ensemble"):
        kind.append("z-scored ensemble (MannerVectorCache)")
    if kind:
        raise NotImplementedError(f"{who} serves the plain dot-product caches: {type(cache).__name__} over {type(module).__name__} "
                                  f"is a `{kind[0]}`, and "
                                  "the windowed walk (tkw_scores_kernel / tkwc_count_kernel) runs under the dot-product producer "
                                  "alone; a windowed kernel for that scorer does not exist yet")


def _sample_triple(sample, n_users: int):
    """``sample`` = (inv_temp, seed, user_key) of ``recommend`` checked before any device work (``ops._sample_args``: the key
    tensor int64 with one entry per user, the seed in [0, 2^64), ``inv_temp`` finite and >= 0) -> (inv_temp, seed, user_key)."""
    if not isinstance(sample, (tuple, list)) or len(sample) != 3:
        raise ValueError("newsreclib_amd: sample = (inv_temp, seed, user_key)")
    seed, inv_temp = ops._sample_args(sample[2], n_users, sample[1], sample[0])
    return inv_temp, seed, sample[2]


def _sample_policy(who: str, cache, sample, cap=None, window=None, rerankers=()):
    """``sample`` = (temperature, seed) of ``recommend_users`` / ``sample_recommendations`` -> (inv_temp, seed), after the refusals:
    ``NotImplementedError`` where the sampled walk has no kernel (under a cap, under a window, under every producer but the plain
    dot product), ``ValueError`` beside a re-ranker and for a temperature that is not positive or a seed outside [0, 2^64)."""
    if not isinstance(sample, (tuple, list)) or len(sample) != 2:
        raise ValueError(f"{who}: sample = (temperature, seed)")
    if cap is not None:
        raise NotImplementedError(f"{who} with cap=...: the sampled producer (tks_scores_kernel) feeds the plain selecting consumer; "
                                  "a sampled kernel with the class-capped consumer (TkSelectCapped) does not exist yet")
    if window is not None:
        raise NotImplementedError(f"{who} with window=...: the sampled producer (tks_scores_kernel) runs under the plain walk; a "
                                  "sampled kernel under the windowed walk (tkw_walk) does not exist yet")
    if any(r is not None for r in rerankers):
        raise ValueError(f"{who}: `sample` excludes `diversify`, `calibrate` and `dpp`: each of those picks the listed news from a "
                         "pool by an objective of its own, a sampled list is a draw from the policy and stays as drawn")
    module = getattr(cache, "module", None)
    kind = [a for a in ("multi_interest_scorer", "dnn_predictor_scorer", "personalized_pooling_scorer", "class_biased_scorer")
            if getattr(module, a, False)]
    if hasattr(cache, "recommend_ensemble"):
        kind.append("z-scored ensemble (MannerVectorCache)")
    if kind:
        raise NotImplementedError(f"{who} draws from the Plackett-Luce policy over plain dot-product scores: {type(cache).__name__} "
                                  f"over {type(module).__name__} is a `{kind[0]}`, and the Gumbel perturbation (tks_scores_kernel) "
                                  "sits behind the dot-product producer alone; a sampled kernel for that scorer does not exist yet")
    temperature, seed = float(sample[0]), sample[1]
    if not math.isfinite(temperature) or temperature <= 0:
        raise ValueError(f"{who}: the temperature must be finite and > 0, got {sample[0]!r}")
    if isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed < 2 ** 64:
        raise ValueError(f"{who}: the seed must be an integer in [0, 2^64), got {seed!r}")
    return 1.0 / temperature, seed


def _policy_refusal(who: str, cache, window=None) -> None:
    """``NotImplementedError`` where the log-partition has no kernel: the summing consumer (``TkLogZ``) is instantiated under the
    plain dot-product producer and the plain walk alone."""
    if window is not None:
        raise NotImplementedError(f"{who} with window=...: the summing consumer (tkz_sum_kernel) runs under the plain walk; a "
                                  "log-partition kernel under the windowed walk (tkw_walk) does not exist yet")
    module = getattr(cache, "module", None)
    kind = [a for a in ("multi_interest_scorer", "dnn_predictor_scorer", "personalized_pooling_scorer", "class_biased_scorer")
            if getattr(module, a, False)]
    if hasattr(cache, "recommend_ensemble"):
        kind.append("z-scored ensemble (MannerVectorCache)")
    if hasattr(cache, "recommend_pooled"):
        kind.append("personalized_pooling_scorer (NpaFeatureCache)")
    if kind:
        raise NotImplementedError(f"{who} is the log-partition of the Plackett-Luce policy over plain dot-product scores: "
                                  f"{type(cache).__name__} over {type(module).__name__} is a `{kind[0]}`, and the summing consumer "
                                  "(tkz_sum_kernel: TkLogZ under TkDot) is instantiated under the dot-product producer alone; a "
                                  "log-partition kernel for that scorer does not exist yet")


def _policy_lists(lists, n_users: int) -> torch.Tensor:
    """``lists`` of ``list_log_probs`` checked before any device work: int64 (``TypeError``), (n_users, k <= ops.TOPK_MAX_K)
    (``ValueError``)."""
    if not isinstance(lists, torch.Tensor) or lists.dtype != torch.int64:
        raise TypeError(f"newsreclib_amd: `lists` must be an int64 tensor, got "
                        f"{lists.dtype if isinstance(lists, torch.Tensor) else type(lists).__name__}")
    if lists.dim() != 2 or lists.shape[0] != n_users or not 1 <= lists.shape[1] <= ops.TOPK_MAX_K:
        raise ValueError(f"newsreclib_amd: `lists` must be (B, k) with one list per user ({n_users}) and 1 <= k <= "
                         f"{ops.TOPK_MAX_K}, got {tuple(lists.shape)}")
    return lists


def _policy_inv_temp(inv_temp) -> float:
    inv_temp = float(inv_temp)
    if not math.isfinite(inv_temp) or inv_temp < 0:
        raise ValueError(f"newsreclib_amd: `inv_temp` must be finite and >= 0, got {inv_temp!r}")
    return inv_temp


def _user_ids(chunk: Sequence[Dict], lo: int) -> List[int]:
    """The id of each user dictionary of a batch that starts at position ``lo`` of the list: its ``user_id``, or position + 1."""
    return [int(u["user_id"]) if "user_id" in u else lo + j + 1 for j, u in enumerate(chunk)]


class NewsVectorCache(_ImpressionCache):
    """Encode-once evaluation of a drop-in recommender (any of the module mirrors: NRMS, LSTUR, NAML, TANR,
    CenNewsRec, MINS -- whatever exposes ``news_encoder`` and ``score_news_vectors``)."""

    def __init__(self, module, table: DeviceNewsTable, chunk: int = 16384):
        self.module, self.table, self.chunk = module, table, int(chunk)
        self.vectors: Optional[torch.Tensor] = None
        self.projection: Optional[torch.Tensor] = None      # (num_news, Hd): ``recommend_dnn``'s share of the table, built lazily
        self._row_class: Dict[str, torch.Tensor] = {}       # aspect -> (num_news) int32: ``recommend_capped``'s classes
        self._row_time: Optional[torch.Tensor] = None       # (num_news) int32: the ``time`` column, for ``window=``

    @torch.no_grad()
    def build(self) -> torch.Tensor:
        """news vectors (num_news, D) of the whole table, in chunks (the encoder workspace is O(rows))."""
        self.projection = None
        if getattr(self.module, "user_dependent_news_vectors", False):
            raise NotImplementedError("this recommender's news vectors depend on the user (NPA's personalized attention, "
                                      "text.py:385-390): they cannot be cached; NpaFeatureCache caches what does not "
                                      "(the conv feature maps) and scores from it")
        enc = self.module.news_encoder
        text_encoders = list((getattr(enc, "text_encoders", {}) or {}).values())
        # (a PLM text encoder with the CLS head -- use_mhsa == False, MINER -- encodes every news on its own and says so)
        if getattr(getattr(self.module, "hparams", None), "use_plm", False) and \
                not (text_encoders and all(getattr(t, "news_independent", False) for t in text_encoders)):
            raise NotImplementedError("the PLM text encoder attends across the news of one call (text.py:92-96): "
                                      "a news vector is not a function of the news alone and cannot be cached")
        names = [k for k in self.table.attrs if k in TEXT_ATTRS or k in ("category", "subcategory")]
        # encoders that read entity ids (DKN's KCNN) declare them; every other encoder's call stays as it was
        names += [k for k in getattr(enc, "entity_attrs", ()) if k in self.table.attrs and k not in names]
        out = []
        # one pass over the whole corpus under frozen weights: MHSAAddAtt text encoders run their in-projection once per
        # VOCABULARY id instead of once per token position (news_encoder.MHSAAddAtt.token_table; same bits)
        with eval_mode(self.module), token_tables(enc):
            for lo in range(0, self.table.num_news, self.chunk):
                hi = min(lo + self.chunk, self.table.num_news)
                out.append(enc({k: _map_rows(self.table.attrs[k], lambda t: t[lo:hi]) for k in names}))
        self.vectors = torch.cat(out, dim=0)
        return self.vectors

    @torch.no_grad()
    def scores(self, hist_idx: torch.Tensor, hist_sizes: torch.Tensor, cand_idx: torch.Tensor,
               cand_sizes: torch.Tensor, user_idx: Optional[torch.Tensor] = None) -> torch.Tensor:
        """(B, max_cand) click scores of a batch of impressions given by news-index lists."""
        if self.vectors is None:
            self.build()
        meta = self._meta(hist_sizes, cand_sizes, None, user_idx, None)
        dev = self.table.device
        hv = ops.embedding_gather(self.vectors, hist_idx.to(dev).reshape(-1, 1)).reshape(-1, self.vectors.shape[1])
        cv = ops.embedding_gather(self.vectors, cand_idx.to(dev).reshape(-1, 1)).reshape(-1, self.vectors.shape[1])
        # a scorer that reads news attributes beside the vectors (MINER's category bias) declares them
        for name in getattr(self.module, "score_news_attrs", ()):
            meta["x_hist"][name] = self.table.attrs[name].index_select(0, hist_idx.to(dev))
            meta["x_cand"][name] = self.table.attrs[name].index_select(0, cand_idx.to(dev))
        with eval_mode(self.module):
            return self.module.score_news_vectors(hv, cv, meta)

    def _user_meta(self, hist_sizes: torch.Tensor, user_idx: Optional[torch.Tensor]) -> Dict:
        """The history half of ``_meta`` from HOST sizes: maxima and offsets are computed on the host and copied over, so nothing
        is read back from the device (``_meta`` reads the longest list back)."""
        dev = self.table.device
        hs = hist_sizes.detach().cpu().long()               # (a device tensor here costs the one read-back this avoids)
        B = int(hs.numel())
        ar = torch.arange(B, device=dev)

        def up(t):                                          # host -> device through pinned memory: the host does not wait
            return t if t.is_cuda else t.pin_memory().to(dev, non_blocking=True)

        both = up(torch.cat([hs, torch.zeros(1, dtype=torch.int64), torch.cumsum(hs, 0)]))
        return {
            "batch_size": B, "hist_sizes": both[:B], "batch_hist": torch.repeat_interleave(ar, both[:B], output_size=int(hs.sum())),
            "hist_offsets": both[B:], "max_hist": int(hs.max()) if B else 0, "min_hist": int(hs.min()) if B else 0,
            "user_idx": up(user_idx) if user_idx is not None else ar.clone(),
        }

    # ---- ranking the whole table: each scorer's user side, written once for its `recommend*` and its `rank_clicks*` ----
    def _history(self, who: str, hist_idx, hist_sizes, user_idx, exclude_history: bool, eligible, clicks):
        """What every whole-table method ``who`` does before its scorer's own user side: the caller's side of the call checked
        and on the device (``_catalogue_side``), the table built when it is missing -> (the gathered history vectors, the
        history meta, the click lists ``_catalogue_side`` returns, the (excl_idx, excl_off, eligible) every ``ops`` entry ends
        with)."""
        hist_idx, eligible, targets = _catalogue_side(who, self, hist_idx, hist_sizes, eligible, clicks)
        if self.vectors is None:
            self.build()
        meta = self._user_meta(hist_sizes, user_idx)
        hv = ops.embedding_gather(self.vectors, hist_idx.reshape(-1, 1)).reshape(-1, self.vectors.shape[1])
        excl = (hist_idx, meta["hist_offsets"]) if exclude_history else (None, None)
        return hv, meta, targets, (*excl, eligible)

    def _dot_users(self, verb: str, *side):
        """The user side of ``recommend`` / ``rank_clicks`` (``verb``): the refusal, then the module's ``user_vectors`` (eval mode)
        -> (user (B, D), click lists, (excl_idx, excl_off, eligible))."""
        if not getattr(self.module, "dot_product_scorer", False):
            raise NotImplementedError(
                f"{type(self.module).__name__} does not score a news by one dot product with a candidate-independent user vector "
                "(no `dot_product_scorer`): " + {
                    "recommend":
                        "its user representation or its predictor depends on the candidate (MINER's "
                        "poly-attention scores, CAUM's candidate-aware encoder, DKN's DNN predictor, SentiDebias' generator), so "
                        "the whole table cannot be ranked by one GEMM + top-k; MINER is served by `recommend_interests`, DKN (whose "
                        "user vector does not depend on the candidate and whose DNN factors) by `recommend_dnn`",
                    "rank_clicks":
                        "only the dot-product families are served by `rank_clicks`; MINER is served by `rank_clicks_interests`, "
                        "DKN (whose user vector does not depend on the candidate and whose DNN factors) by `rank_clicks_dnn`",
                }[verb])
        hv, meta, targets, tail = self._history(verb, *side)
        with eval_mode(self.module):
            user = self.module.user_vectors(hv, meta)
        return user, targets, tail

    def _biased_users(self, verb: str, combined: bool, aspect, bias, *side):
        """The user side of ``recommend_biased`` / ``rank_clicks_biased``: the refusal, then either the module's
        ``user_vectors_and_bias`` (a ``class_biased_scorer``: SentiDebias; the classes are its ``class_bias_aspect`` column of the
        table, the history's classes gathered from the same column) or the module's ``user_vectors`` with the caller's ``aspect``
        and ``bias`` (a ``dot_product_scorer``) -> (user (B, D), bias (B, S) or None: rank by the dot product alone, the classes
        (num_news) int32 or None, click lists, (excl_idx, excl_off, eligible))."""
        own = getattr(self.module, "class_biased_scorer", False)
        if not own and not getattr(self.module, "dot_product_scorer", False):
            raise NotImplementedError(
                f"{type(self.module).__name__} scores a news neither by a dot product plus a per-class term of its own "
                f"(`class_biased_scorer`: SentiDebias) nor by one dot product with a candidate-independent user vector "
                f"(`dot_product_scorer`), to which `{verb}_biased` could add the caller's per-class `bias`")
        if own and (aspect is not None or bias is not None):
            raise ValueError(f"newsreclib_amd: {type(self.module).__name__} brings its own class bias (`combined=True`); `aspect` and "
                             "`bias` are for a `dot_product_scorer` module")
        if not own and (aspect is None or bias is None or combined):
            raise ValueError(f"newsreclib_amd: {verb}_biased over a `dot_product_scorer` module needs `aspect` and `bias` (B, S), and "
                             "has no `combined` score")
        hv, meta, targets, tail = self._history(verb + "_biased", *side)
        with eval_mode(self.module):
            if not own:
                return self.module.user_vectors(hv, meta), bias.to(self.table.device), _aspect_classes(self, aspect), targets, tail
            if not combined:
                return self.module.user_vectors_and_bias(hv, meta, None, False)[0], None, None, targets, tail
            classes = _aspect_classes(self, self.module.class_bias_aspect)
            hist_classes = self.table.attrs[self.module.class_bias_aspect].index_select(0, side[0].to(self.table.device).long())
            user, own_bias = self.module.user_vectors_and_bias(hv, meta, hist_classes, True)
        return user, own_bias, classes, targets, tail

    @torch.no_grad()
    def recommend_biased(self, hist_idx: torch.Tensor, hist_sizes: torch.Tensor, k: int, user_idx: Optional[torch.Tensor] = None,
                         exclude_history: bool = True, eligible: Optional[torch.Tensor] = None, combined: bool = False,
                         aspect: Optional[str] = None, bias: Optional[torch.Tensor] = None, cap: Optional[Tuple[str, int]] = None):
        """``recommend`` by a dot product plus a per-(user, class) additive term -> (news_idx (B, k) int64, scores (B, k) fp32,
        status).  Two uses.  A ``class_biased_scorer`` module (SentiDebias): ``combined=False`` (the default) ranks by the
        bias-free score ``u_free . n_v`` through ``ops.topk_scores`` -- what the reference's test step ranks by; ``combined=True``
        ranks by the score the generator is trained on, ``u_free . n_v + (u_aware T^T)[u, sentiment(v)]``, through
        ``ops.topk_bias_scores`` with the table's ``class_bias_aspect`` column as the classes.  A ``dot_product_scorer`` module:
        the caller passes ``aspect`` (an integer news attribute of the table) and ``bias`` (B, S), a boost or penalty per user
        and class of its own (a category-affinity prior, a sentiment penalty); the user vectors are ``recommend``'s.
        ``cap`` = (aspect, max_per_class) selects under ``recommend_capped``'s class cap as well (``k`` at most
        ``ops.TOPK_CAP_MAX_K``); its aspect need not be the bias's.  Same contract as ``recommend``: ``hist_idx`` on the GPU,
        ``hist_sizes`` on the host, nothing read back; ``status``: ``ops.TOPK_BIAS_FLAGS``."""
        user, bias, classes, _, tail = self._biased_users("recommend", combined, aspect, bias,
                                                          hist_idx, hist_sizes, user_idx, exclude_history, eligible, None)
        capped = () if cap is None else (_aspect_classes(self, cap[0]), cap[1])
        if bias is None:
            return (ops.topk_scores_capped if capped else ops.topk_scores)(user, self.vectors, k, *capped, *tail)
        return (ops.topk_bias_scores_capped if capped else ops.topk_bias_scores)(user, self.vectors, bias, classes, k, *capped, *tail)

    @torch.no_grad()
    def rank_clicks_biased(self, hist_idx: torch.Tensor, hist_sizes: torch.Tensor, click_idx: torch.Tensor,
                           click_sizes: torch.Tensor, user_idx: Optional[torch.Tensor] = None, exclude_history: bool = True,
                           eligible: Optional[torch.Tensor] = None, combined: bool = False, aspect: Optional[str] = None,
                           bias: Optional[torch.Tensor] = None):
        """``rank_clicks`` by ``recommend_biased``'s scores -> (rank int32 (n_clicks), score fp32 (n_clicks), ranked int32 (B),
        status): its user side, ``combined`` / ``aspect`` / ``bias``, scores, order, exclusion of the history and ``eligible``,
        with ``ops.catalogue_bias_ranks`` (the bias-free score: ``ops.catalogue_ranks``) counting where ``recommend_biased``
        selects: ``rank <= k`` exactly when the click is slot ``rank - 1`` of ``recommend_biased(k)``.  The click side is that of
        ``rank_clicks`` (host ``click_sizes``, at most ``ops.RANK_MAX_TARGETS`` a user, nothing read back); ``status``:
        ``ops.RANK_BIAS_FLAGS``."""
        user, bias, classes, targets, tail = self._biased_users(
            "rank_clicks", combined, aspect, bias, hist_idx, hist_sizes, user_idx, exclude_history, eligible, (click_idx, click_sizes))
        if bias is None:
            return ops.catalogue_ranks(user, self.vectors, *targets, *tail)
        return ops.catalogue_bias_ranks(user, self.vectors, bias, classes, *targets, *tail)

    def _interest_users(self, verb: str, bias, *side):
        """The user side of ``recommend_interests`` / ``rank_clicks_interests``: the refusal, then the module's ``user_interests``
        (eval mode) -> (interests, gate, click lists, (excl_idx, excl_off, eligible))."""
        if not getattr(self.module, "multi_interest_scorer", False):
            raise NotImplementedError(
                f"{type(self.module).__name__} has no candidate-independent interest vectors (no `multi_interest_scorer`); a "
                f"module that scores by one dot product with a user vector (`dot_product_scorer`) is served by `{verb}`")
        hv, meta, targets, tail = self._history(verb + "_interests", *side)
        with eval_mode(self.module):
            interests, gate = self.module.user_interests(hv, meta, bias=bias.to(self.table.device) if bias is not None else None)
        return interests, gate, targets, tail

    def _dnn_users(self, verb: str, *side):
        """The user side of ``recommend_dnn`` / ``rank_clicks_dnn``: the refusal, then under late fusion the history mean against
        ``vectors``, under early fusion the module's ``user_queries`` (eval mode) against ``projection``, built when it is missing
        -> (late fusion?, the scorer's leading ``ops`` arguments: (user, vectors) or (q, projection, w2, b2), click lists,
        (excl_idx, excl_off, eligible))."""
        if not getattr(self.module, "dnn_predictor_scorer", False):
            raise NotImplementedError(
                f"{type(self.module).__name__} has no DNN click predictor over a candidate-independent user vector (no "
                "`dnn_predictor_scorer`); a module that scores by one dot product with a user vector (`dot_product_scorer`) is "
                f"served by `{verb}`, one with interest vectors (`multi_interest_scorer`) by `{verb}_interests`")
        hv, meta, targets, tail = self._history(verb + "_dnn", *side)
        if self.module.hparams.late_fusion:
            dense = dense_rows(hv, meta["batch_hist"], meta["batch_size"], meta["max_hist"], meta["hist_offsets"])
            return True, (ops.HistMeanFn.apply(dense, meta["hist_offsets"]), self.vectors), targets, tail
        from . import ops_dkn
        pred = self.module.click_predictor.params()
        if self.projection is None:
            self.projection = ops_dkn.dkn_cand_project(self.vectors, pred)
        with eval_mode(self.module):
            _, q = self.module.user_queries(hv, meta)
        return False, (q, self.projection, pred[2], pred[3]), targets, tail

    @torch.no_grad()
    def recommend(self, hist_idx: torch.Tensor, hist_sizes: torch.Tensor, k: int, user_idx: Optional[torch.Tensor] = None,
                  exclude_history: bool = True, eligible: Optional[torch.Tensor] = None, window=None, sample=None):
        """The ``k`` news of the WHOLE table each user scores highest -> (news_idx (B, k) int64, scores (B, k) fp32, status):
        the module's ``user_vectors`` over the gathered history vectors (eval mode, restored afterwards), then
        ``ops.topk_scores`` against the cached table with the history as the exclusion list (``exclude_history``) and
        ``eligible`` (num_news, uint8 / bool: 0 = never recommended, e.g. the padding row 0).  Slots beyond the rows that
        qualify hold ``-1`` / ``-inf``; ``status`` (``ops.TOPK_FLAGS``) stays on the device.  ``hist_idx`` is a GPU tensor (the
        library has no CPU path), ``hist_sizes`` a HOST tensor as ``evaluate_impressions`` builds it: nothing is read back.

        ``window`` = (win_lo, win_hi) or (win_lo, win_hi, row_time), int32, host or device: user ``b`` is recommended only news
        with ``win_lo[b] <= time <= win_hi[b]`` (``ops.topk_window_scores``); without the third member the times are the table's
        ``time`` column (``ValueError`` when it has none).  ``None`` is the call without it, launch for launch.

        ``sample`` = (inv_temp, seed, user_key): instead of the ``k`` best news, ONE draw without replacement from the
        Plackett-Luce policy over ``softmax(score * inv_temp)`` (``ops.topk_sampled_scores``: Gumbel top-k); ``user_key`` is one
        int64 key per user, host (through pinned memory) or device, and a user's list depends on ``(seed, its key)`` and its own
        inputs alone.  The returned scores are the raw scores of the drawn news, in the order drawn.  ``NotImplementedError``
        together with ``window``.  ``None`` is the call without it, launch for launch."""
        if sample is not None:
            if window is not None:
                raise NotImplementedError("recommend(sample=..., window=...): the sampled producer (tks_scores_kernel) runs under the "
                                          "plain walk; a sampled kernel under the windowed walk (tkw_walk) does not exist yet")
            inv_temp, seed, user_key = _sample_triple(sample, int(hist_sizes.numel()))
        times = None if window is None else _window_arrays(self, window)
        user, _, tail = self._dot_users("recommend", hist_idx, hist_sizes, user_idx, exclude_history, eligible, None)
        if sample is not None:
            if not user_key.is_cuda:
                user_key = user_key.pin_memory().to(user.device, non_blocking=True)
            idx, _, score, status = ops.topk_sampled_scores(user, self.vectors, k, user_key, seed, inv_temp, *tail)
            return idx, score, status
        if times is not None:
            return ops.topk_window_scores(user, self.vectors, k, *times, *tail)
        return ops.topk_scores(user, self.vectors, k, *tail)

    @torch.no_grad()
    def recommend_draws(self, hist_idx: torch.Tensor, hist_sizes: torch.Tensor, k: int, draws: int, policy,
                        user_idx: Optional[torch.Tensor] = None, exclude_history: bool = True,
                        eligible: Optional[torch.Tensor] = None):
        """``draws`` lists per user from the policy of ``recommend(sample=...)`` -> (news_idx (B, draws, k) int64, raw scores
        (B, draws, k) fp32, status).  ``policy`` = (inv_temp, seed, user_key) is ``recommend``'s ``sample`` triple (the argument has
        a name of its own because ``recommend`` alone takes a ``sample``: here it is the first of ``draws`` seeds), and draw ``r``
        is, bit for bit, ``recommend(..., sample=(inv_temp, (seed + r) mod 2^64, user_key))``.  The user encoder runs once;
        ``ops.topk_sampled_draws`` (tkd_scores_kernel) computes every dot product once per group of at most
        ``min(ops.TOPK_MAX_DRAWS, ops.TOPK_MAX_K // k)`` draws, group ``g`` starting at seed ``seed + r0``; the groups' status words
        are ORed on the device and nothing is read back.  The caller's side and the refusals are ``recommend``'s."""
        draws = int(draws)
        if draws < 1:
            raise ValueError(f"recommend_draws: draws >= 1, got {draws}")
        inv_temp, seed, user_key = _sample_triple(policy, int(hist_sizes.numel()))
        k = int(k)
        group = max(1, min(ops.TOPK_MAX_DRAWS, ops.TOPK_MAX_K // max(k, 1)))
        user, _, tail = self._dot_users("recommend", hist_idx, hist_sizes, user_idx, exclude_history, eligible, None)
        if not user_key.is_cuda:
            user_key = user_key.pin_memory().to(user.device, non_blocking=True)
        idx, score, status = [], [], None
        for r0 in range(0, draws, group):
            i, _, s, st = ops.topk_sampled_draws(user, self.vectors, k, min(group, draws - r0), user_key, (seed + r0) % 2 ** 64,
                                                 inv_temp, *tail)
            idx.append(i)
            score.append(s)
            status = st if status is None else status | st
        if len(idx) == 1:
            return idx[0], score[0], status
        return torch.cat(idx, dim=1), torch.cat(score, dim=1), status

    @torch.no_grad()
    def policy_stats(self, hist_idx: torch.Tensor, hist_sizes: torch.Tensor, inv_temp: float, user_idx: Optional[torch.Tensor] = None,
                     exclude_history: bool = True, eligible: Optional[torch.Tensor] = None, window=None) -> Dict[str, torch.Tensor]:
        """What the sampled policy of ``recommend(sample=(inv_temp, ...))`` looks like per user, over the population ``recommend``
        selects from: {"max", "log_sum" (``log sum exp(t - max)``), "log_z" (= max + log_sum, fp32), "entropy" (nats),
        "population" (int32), "status" (``ops.POLICY_FLAGS``)}, all on the device (``ops.catalogue_logz``).  ``exp(entropy)`` is the
        effective catalogue size, ``exp(-log_sum)`` the probability of the user's best news.  The caller's side is ``recommend``'s
        (``hist_idx`` on the GPU, ``hist_sizes`` on the host); nothing is read back.  ``NotImplementedError`` with ``window`` and
        for every scorer but the plain dot product: their log-partition kernels do not exist yet."""
        _policy_refusal("policy_stats", self, window)
        inv_temp = _policy_inv_temp(inv_temp)
        user, _, tail = self._dot_users("recommend", hist_idx, hist_sizes, user_idx, exclude_history, eligible, None)
        mx, ls, ent, pop, _, status = ops.catalogue_logz(user, self.vectors, inv_temp, *tail)
        return {"max": mx, "log_sum": ls, "log_z": mx + ls, "entropy": ent, "population": pop, "status": status}

    @torch.no_grad()
    def list_log_probs(self, hist_idx: torch.Tensor, hist_sizes: torch.Tensor, lists: torch.Tensor, inv_temp: float,
                       user_idx: Optional[torch.Tensor] = None, exclude_history: bool = True,
                       eligible: Optional[torch.Tensor] = None, window=None):
        """The log-probability of ``lists`` ((B, k) int64 news rows, host or device, ``-1`` in trailing empty slots) under the
        policy ``recommend(sample=(inv_temp, ...))`` draws from -> (logp (B, k) fp32, total (B) fp32, score (B, k) fp32, status):
        ``ops.list_logprob`` against the cached table with ``recommend``'s user side, exclusion of the history and ``eligible``.
        A list the policy could not have drawn (a news of the history, an ineligible one, one listed twice) is NaN for that user
        and sets bit 128 of ``status`` (``ops.POLICY_FLAGS``).  Nothing is read back.  Refusals as ``policy_stats``."""
        _policy_refusal("list_log_probs", self, window)
        inv_temp = _policy_inv_temp(inv_temp)
        lists = _policy_lists(lists, int(hist_sizes.numel()))
        user, _, tail = self._dot_users("recommend", hist_idx, hist_sizes, user_idx, exclude_history, eligible, None)
        if not lists.is_cuda:
            lists = lists.pin_memory().to(user.device, non_blocking=True)
        return ops.list_logprob(user, self.vectors, lists, inv_temp, *tail)

    @torch.no_grad()
    def recommend_capped(self, hist_idx: torch.Tensor, hist_sizes: torch.Tensor, k: int, aspect: str, max_per_class: int,
                         user_idx: Optional[torch.Tensor] = None, exclude_history: bool = True,
                         eligible: Optional[torch.Tensor] = None):
        """``recommend`` with a diversity constraint on the list itself: the ``k`` (at most ``ops.TOPK_CAP_MAX_K``) best news of
        each user with at most ``max_per_class`` of any one class of ``aspect``, a news attribute of the table with one integer
        per news (``category``, ``subcategory``, ``sentiment``) -> (news_idx (B, k) int64, scores (B, k) fp32, status).  The user
        side, the scores, the order, the exclusion of the history, ``eligible`` and the refusals are ``recommend``'s;
        ``ops.topk_scores_capped`` selects.  Slots beyond the rows that qualify hold ``-1`` / ``-inf``, which also happens when
        the classes together admit fewer than ``k`` rows.  Nothing is read back."""
        user, _, tail = self._dot_users("recommend", hist_idx, hist_sizes, user_idx, exclude_history, eligible, None)
        return ops.topk_scores_capped(user, self.vectors, k, _aspect_classes(self, aspect), max_per_class, *tail)

    @torch.no_grad()
    def rerank_diverse(self, pool_idx: torch.Tensor, pool_score: torch.Tensor, k: int, lam: float, similarity: str = "cosine",
                       normalize: bool = True):
        """Greedy MMR over a pool any ``recommend*`` of this cache returned (``pool_idx`` / ``pool_score`` (B, N), N at most
        ``ops.MMR_MAX_POOL``) -> (news_idx (B, k) int64, scores (B, k) fp32: the pool's own, mmr (B, k) fp32, status:
        ``ops.MMR_FLAGS``): ``ops.mmr_rerank`` against the cached news vectors, built when they are missing.  The similarity is
        between news vectors, whatever scorer produced the pool.  Nothing is read back."""
        if self.vectors is None:
            self.build()
        return ops.mmr_rerank(pool_idx, pool_score, self.vectors, k, lam, similarity, normalize)

    @torch.no_grad()
    def rerank_dpp(self, pool_idx: torch.Tensor, pool_score: torch.Tensor, k: int, alpha: float = 1.0, similarity: str = "cosine",
                   normalize: bool = True, quality: Optional[torch.Tensor] = None, eps: float = 1e-4):
        """Greedy DPP re-ranking of a pool any ``recommend*`` of this cache returned (``pool_idx`` / ``pool_score`` (B, N), N at
        most ``ops.MMR_MAX_POOL``, ``k`` at most ``ops.DPP_MAX_K``) -> (news_idx (B, k) int64, scores (B, k) fp32: the pool's own,
        gain (B, k) fp32, status: ``ops.DPP_FLAGS``): ``ops.dpp_rerank`` against the cached news vectors, built when they are
        missing.  Where ``rerank_diverse`` penalises a news by its one nearest neighbour in the list, this penalises what the
        listed news span together.  Nothing is read back."""
        if self.vectors is None:
            self.build()
        return ops.dpp_rerank(pool_idx, pool_score, self.vectors, k, alpha, similarity, normalize, quality, eps)

    @torch.no_grad()
    def rerank_calibrated(self, pool_idx: torch.Tensor, pool_score: torch.Tensor, k: int, aspect: str, target: torch.Tensor,
                          lam: float, mu: float, gamma: float, similarity: str = "cosine", normalize: bool = True):
        """Calibrated greedy re-ranking of a pool any ``recommend*`` of this cache returned -> (news_idx (B, k) int64, scores
        (B, k) fp32: the pool's own, obj (B, k) fp32, cal (B, k) fp32, status: ``ops.CAL_FLAGS``): ``ops.calibrated_rerank`` with
        the table's ``aspect`` column as the classes and ``target`` (B, S) fp32 (``ops.class_targets``) as the class mix to pull
        the list towards.  ``mu != 0`` adds MMR's penalty by the cached news vectors, built when they are missing; ``mu == 0``
        touches no vectors.  Nothing is read back."""
        table = None
        if float(mu) != 0.0:
            if self.vectors is None:
                self.build()
            table = self.vectors
        return ops.calibrated_rerank(pool_idx, pool_score, table, _aspect_classes(self, aspect), target, k, lam, mu, gamma, similarity,
                                     normalize)

    @torch.no_grad()
    def rank_clicks(self, hist_idx: torch.Tensor, hist_sizes: torch.Tensor, click_idx: torch.Tensor, click_sizes: torch.Tensor,
                    user_idx: Optional[torch.Tensor] = None, exclude_history: bool = True,
                    eligible: Optional[torch.Tensor] = None, window=None):
        """Where each user's held-out clicks land when the user is ranked against the WHOLE table -> (rank int32 (n_clicks),
        score fp32 (n_clicks), ranked int32 (B), status): ``recommend``'s user vectors, scores, order, exclusion of the history
        and ``eligible``, with ``ops.catalogue_ranks`` counting where ``recommend`` selects.  ``rank`` is the click's 1-based
        place among the ``ranked[b]`` news the user could be recommended, 0 when the click is not one of them (in the history,
        ineligible, outside the table); ``rank <= k`` exactly when the click is slot ``rank - 1`` of ``recommend(k)``.  At most
        ``ops.RANK_MAX_TARGETS`` clicks per user (``ValueError`` otherwise, from the host sizes).  Same contract as ``recommend``:
        ``hist_idx`` and ``click_idx`` on the GPU, ``hist_sizes`` and ``click_sizes`` on the host, nothing read back; ``status``
        (``ops.RANK_FLAGS``) stays on the device.  ``metrics.full_rank_metrics`` turns the result into MRR / nDCG@k / recall@k.

        ``window``: as for ``recommend`` (``ops.catalogue_window_ranks``): the population is the news inside the user's window,
        and a click outside it has rank 0."""
        times = None if window is None else _window_arrays(self, window)
        user, targets, tail = self._dot_users("rank_clicks",
                                              hist_idx, hist_sizes, user_idx, exclude_history, eligible, (click_idx, click_sizes))
        if times is not None:
            return ops.catalogue_window_ranks(user, self.vectors, *targets, *times, *tail)
        return ops.catalogue_ranks(user, self.vectors, *targets, *tail)

    @torch.no_grad()
    def recommend_interests(self, hist_idx: torch.Tensor, hist_sizes: torch.Tensor, k: int, user_idx: Optional[torch.Tensor] = None,
                            exclude_history: bool = True, eligible: Optional[torch.Tensor] = None,
                            bias: Optional[torch.Tensor] = None):
        """``recommend`` for a module whose score is an aggregate over K candidate-independent interest vectors
        (``multi_interest_scorer``: MINER) -> (news_idx (B, k) int64, scores (B, k) fp32, status): the module's
        ``user_interests`` over the gathered history vectors (eval mode, restored afterwards; ``max_hist`` is the batch's longest
        history, as ``scores`` uses), then ``ops.topk_interest_scores`` with the module's ``interest_score_mode`` against the
        cached table.  Same contract as ``recommend``: ``hist_idx`` on the GPU, ``hist_sizes`` on the host, nothing read back.
        MINER's category bias needs the batch's candidate lists and is left out (``MINERModule.user_interests``); ``bias``
        (n_hist) passes a per-history-row bias of the caller's own."""
        interests, gate, _, tail = self._interest_users("recommend", bias,
                                                        hist_idx, hist_sizes, user_idx, exclude_history, eligible, None)
        return ops.topk_interest_scores(interests, self.vectors, k, self.module.interest_score_mode, gate, *tail)

    @torch.no_grad()
    def recommend_dnn(self, hist_idx: torch.Tensor, hist_sizes: torch.Tensor, k: int, user_idx: Optional[torch.Tensor] = None,
                      exclude_history: bool = True, eligible: Optional[torch.Tensor] = None):
        """``recommend`` for a module that scores ``[news; user]`` with a DNN whose first layer splits by columns and whose user
        vector does not depend on the candidate (``dnn_predictor_scorer``: DKN) -> (news_idx (B, k) int64, scores (B, k) fp32,
        status).  Early fusion: the module's ``user_queries`` over the gathered history vectors gives every user's share ``q`` of
        the first layer, and ``ops.topk_relu_scores`` ranks ``b2 + w2 . relu(P[v] + q[u])`` against ``projection``
        ``P = vectors Wc^T`` (num_news, Hd).  ``P`` is built from ``vectors`` at the first call and dropped by ``build()``; like
        ``vectors`` it is a SNAPSHOT of the weights at that moment: after they change, call ``build()`` again (nothing is keyed on
        them).  ``w2``, ``b2`` and the user half are read from the module at every call.  Late fusion (a dot product with the
        history mean): ``ops.topk_scores`` against ``vectors``.  Same contract as ``recommend``: ``hist_idx`` on the GPU,
        ``hist_sizes`` on the host, nothing read back."""
        late, scorer, _, tail = self._dnn_users("recommend", hist_idx, hist_sizes, user_idx, exclude_history, eligible, None)
        return (ops.topk_scores if late else ops.topk_relu_scores)(*scorer, k, *tail)

    @torch.no_grad()
    def rank_clicks_interests(self, hist_idx: torch.Tensor, hist_sizes: torch.Tensor, click_idx: torch.Tensor,
                              click_sizes: torch.Tensor, user_idx: Optional[torch.Tensor] = None, exclude_history: bool = True,
                              eligible: Optional[torch.Tensor] = None, bias: Optional[torch.Tensor] = None):
        """``rank_clicks`` for a ``multi_interest_scorer`` module (MINER) -> (rank int32 (n_clicks), score fp32 (n_clicks), ranked
        int32 (B), status): ``recommend_interests``' interests, gate, ``interest_score_mode``, scores, order, exclusion of the
        history and ``eligible``, with ``ops.catalogue_interest_ranks`` counting where ``recommend_interests`` selects: ``rank <=
        k`` exactly when the click is slot ``rank - 1`` of ``recommend_interests(k)``.  The click side is that of ``rank_clicks``
        (host ``click_sizes``, at most ``ops.RANK_MAX_TARGETS`` a user, nothing read back)."""
        interests, gate, targets, tail = self._interest_users(
            "rank_clicks", bias, hist_idx, hist_sizes, user_idx, exclude_history, eligible, (click_idx, click_sizes))
        return ops.catalogue_interest_ranks(interests, self.vectors, *targets, self.module.interest_score_mode, gate, *tail)

    @torch.no_grad()
    def rank_clicks_dnn(self, hist_idx: torch.Tensor, hist_sizes: torch.Tensor, click_idx: torch.Tensor, click_sizes: torch.Tensor,
                        user_idx: Optional[torch.Tensor] = None, exclude_history: bool = True,
                        eligible: Optional[torch.Tensor] = None):
        """``rank_clicks`` for a ``dnn_predictor_scorer`` module (DKN) -> (rank int32 (n_clicks), score fp32 (n_clicks), ranked
        int32 (B), status): ``recommend_dnn``'s user side (``user_queries`` and the cached ``projection`` under early fusion, the
        history mean under late fusion), scores, order, exclusion of the history and ``eligible``, with
        ``ops.catalogue_relu_ranks`` (late fusion: ``ops.catalogue_ranks``) counting where ``recommend_dnn`` selects: ``rank <= k``
        exactly when the click is slot ``rank - 1`` of ``recommend_dnn(k)``.  The click side is that of ``rank_clicks`` (host
        ``click_sizes``, at most ``ops.RANK_MAX_TARGETS`` a user, nothing read back)."""
        late, scorer, targets, tail = self._dnn_users("rank_clicks",
                                                      hist_idx, hist_sizes, user_idx, exclude_history, eligible, (click_idx, click_sizes))
        return (ops.catalogue_ranks if late else ops.catalogue_relu_ranks)(*scorer, *targets, *tail)


class MannerVectorCache(_ImpressionCache):
    """Encode-once evaluation of ``manner_module.MANNERModule``: one ``NewsVectorCache`` per loaded sub-model over the same
    ``DeviceNewsTable``; ``scores`` is one ``nrl_manner_scores`` launch that gathers straight from the (up to three) tables.
    ``model_step`` returns the 11-tuple ``evaluate_impressions`` consumes, with a zero tensor in the loss slot (MANNeR has no
    loss).  ``recommend_ensemble`` / ``rank_clicks_ensemble`` rank the whole table by the ensemble z-scored over the user's
    population (top-k and the rank of held-out clicks; ``recommend`` / ``rank_clicks`` refuse and say why).  The sub-models' encoders read the concatenated ``text`` input, which ``NewsVectorCache.build`` passes through because
    ``NewsEncoder.entity_attrs`` lists it beside ``entities`` under ``concatenate_inputs`` (that property is the cache's list of
    inputs to hand over besides title / abstract / category, entity ids or not).

    ``hist_sizes`` / ``cand_sizes`` are HOST tensors, as ``evaluate_impressions`` builds them: the width of the score matrix is
    their maximum, read on the host (a device tensor there costs one read-back per batch), so it covers every impression."""

    def __init__(self, module, table: DeviceNewsTable, chunk: int = 16384):
        self.module, self.table = module, table
        pairs = module.submodels()
        self.weights = [w for _, w in pairs]
        self.caches = [NewsVectorCache(m, table, chunk) for m, _ in pairs]
        self.vectors = None
        self._row_class: Dict[str, torch.Tensor] = {}       # aspect -> (num_news) int32: ``recommend_ensemble_capped``'s classes

    @torch.no_grad()
    def build(self):
        self.vectors = [c.build() for c in self.caches]
        return self.vectors

    @torch.no_grad()
    def scores(self, hist_idx: torch.Tensor, hist_sizes: torch.Tensor, cand_idx: torch.Tensor, cand_sizes: torch.Tensor,
               user_idx: Optional[torch.Tensor] = None) -> torch.Tensor:
        from .ops_manner import manner_scores
        if self.vectors is None:
            self.build()
        dev = self.table.device
        max_cand = int(cand_sizes.max())                       # the true largest count: no impression is truncated
        hist_off, cand_off = ragged_offsets(hist_sizes, dev), ragged_offsets(cand_sizes, dev)
        return manner_scores(self.vectors, self.weights, hist_idx.to(dev).long(), hist_off, cand_idx.to(dev).long(), cand_off,
                             max_cand)

    @torch.no_grad()
    def zscores(self, hist_idx: torch.Tensor, hist_sizes: torch.Tensor, cand_idx: torch.Tensor, cand_sizes: torch.Tensor) -> torch.Tensor:
        """(T, N) standardised scores of every loaded sub-model, flat in candidate order: what ``scores`` combines with
        ``self.weights``, uncombined (``ops_manner.manner_zscores``, one launch).  The components ``evaluate_weight_grid`` hands
        to ``metrics.GridStreamingMetrics``; sizes on the host as in ``scores``."""
        from .ops_manner import manner_zscores
        if self.vectors is None:
            self.build()
        dev = self.table.device
        max_cand = int(cand_sizes.max())                       # the true largest count: no impression is truncated
        hist_off, cand_off = ragged_offsets(hist_sizes, dev), ragged_offsets(cand_sizes, dev)
        return manner_zscores(self.vectors, hist_idx.to(dev).long(), hist_off, cand_idx.to(dev).long(), cand_off, max_cand)

    def _step_loss(self, scores: torch.Tensor, meta: Dict) -> torch.Tensor:
        return scores.new_zeros(())                            # MANNeR has no loss

    def recommend(self, *args, **kwargs):
        raise NotImplementedError("MANNeR z-scores every sub-model's scores within an impression's own candidate list "
                                  "(manner_module.py: the ensemble of standardised scores): without a candidate list there is no "
                                  "score to rank the whole table by; recommend from one sub-model's NewsVectorCache instead, or "
                                  "name the population: `recommend_ensemble` z-scores over every row a user may be recommended")

    def rank_clicks(self, *args, **kwargs):
        raise NotImplementedError("only the dot-product families are served by `rank_clicks` so far (NewsVectorCache over a "
                                  "`dot_product_scorer` module): MANNeR z-scores every sub-model's scores within a candidate list, "
                                  "and without a named population there is no z-score to rank a click by; rank the clicks with "
                                  "one sub-model's NewsVectorCache instead, or name the population: `rank_clicks_ensemble` "
                                  "z-scores over every row a user may be recommended, as `recommend_ensemble` does")

    def policy_stats(self, *args, **kwargs):
        _policy_refusal("policy_stats", self)

    def list_log_probs(self, *args, **kwargs):
        _policy_refusal("list_log_probs", self)

    @torch.no_grad()
    def recommend_ensemble(self, hist_idx: torch.Tensor, hist_sizes: torch.Tensor, k: int, user_idx: Optional[torch.Tensor] = None,
                           exclude_history: bool = True, eligible: Optional[torch.Tensor] = None, return_stats: bool = False):
        """The ``k`` news of the WHOLE table each user's ensemble score ranks highest -> (news_idx (B, k) int64, scores (B, k)
        fp32, status[, stats (B, T, 2): mean, sd]).  The candidate list of a user is its population: every eligible row that is
        not in its history (``exclude_history``); each sub-model's scores are z-scored over it and the weighted sum is what
        ``scores`` returns for that candidate list (``ops.topk_ensemble_scores``).  Per sub-model the user vector is the mean of
        the gathered history rows of that sub-model's table, as in ``scores``; an empty history gives a NaN vector and that user
        is refused through ``status`` (``ops.TOPK_FLAGS``), as is any user whose scores cannot be standardised.  Same contract as
        ``NewsVectorCache.recommend``: ``hist_idx`` on the GPU, ``hist_sizes`` on the host, nothing read back."""
        users, _, tail = self._ensemble_users("recommend_ensemble", hist_idx, hist_sizes, user_idx, exclude_history, eligible, None)
        idx, score, status, stats = ops.topk_ensemble_scores(users, self.vectors, self.weights, k, *tail)
        return (idx, score, status, stats) if return_stats else (idx, score, status)

    @torch.no_grad()
    def recommend_ensemble_capped(self, hist_idx: torch.Tensor, hist_sizes: torch.Tensor, k: int, aspect: str, max_per_class: int,
                                  user_idx: Optional[torch.Tensor] = None, exclude_history: bool = True,
                                  eligible: Optional[torch.Tensor] = None, return_stats: bool = False):
        """``recommend_ensemble`` with at most ``max_per_class`` news of any one class of ``aspect`` in a user's list, as
        ``NewsVectorCache.recommend_capped`` caps ``recommend``: the users, the population, the statistics and the scores are
        ``recommend_ensemble``'s (the z-scores do not know the cap), ``ops.topk_ensemble_scores_capped`` selects."""
        users, _, tail = self._ensemble_users("recommend_ensemble_capped", hist_idx, hist_sizes, user_idx, exclude_history, eligible,
                                              None)
        idx, score, status, stats = ops.topk_ensemble_scores_capped(users, self.vectors, self.weights, k,
                                                                    _aspect_classes(self, aspect), max_per_class, *tail)
        return (idx, score, status, stats) if return_stats else (idx, score, status)

    @torch.no_grad()
    def rerank_diverse(self, pool_idx: torch.Tensor, pool_score: torch.Tensor, k: int, lam: float, similarity: str = "cosine",
                       normalize: bool = True, submodel: int = 0):
        """``NewsVectorCache.rerank_diverse`` of a pool ``recommend_ensemble*`` returned, against the table of sub-model
        ``submodel`` (the similarity between two news needs one vector space; the ensemble has one per sub-model)."""
        if self.vectors is None:
            self.build()
        return ops.mmr_rerank(pool_idx, pool_score, self.vectors[submodel], k, lam, similarity, normalize)

    @torch.no_grad()
    def rerank_dpp(self, pool_idx: torch.Tensor, pool_score: torch.Tensor, k: int, alpha: float = 1.0, similarity: str = "cosine",
                   normalize: bool = True, quality: Optional[torch.Tensor] = None, eps: float = 1e-4, submodel: int = 0):
        """``NewsVectorCache.rerank_dpp`` of a pool ``recommend_ensemble*`` returned, against the table of sub-model ``submodel``,
        as ``rerank_diverse`` takes its similarity there."""
        if self.vectors is None:
            self.build()
        return ops.dpp_rerank(pool_idx, pool_score, self.vectors[submodel], k, alpha, similarity, normalize, quality, eps)

    @torch.no_grad()
    def rerank_calibrated(self, pool_idx: torch.Tensor, pool_score: torch.Tensor, k: int, aspect: str, target: torch.Tensor,
                          lam: float, mu: float, gamma: float, similarity: str = "cosine", normalize: bool = True, which: int = 0):
        """``NewsVectorCache.rerank_calibrated`` of a pool ``recommend_ensemble*`` returned; with ``mu != 0`` the similarity is
        taken in the table of sub-model ``which``, as ``rerank_diverse`` takes it in that of ``submodel``."""
        table = None
        if float(mu) != 0.0:
            if self.vectors is None:
                self.build()
            table = self.vectors[which]
        return ops.calibrated_rerank(pool_idx, pool_score, table, _aspect_classes(self, aspect), target, k, lam, mu, gamma, similarity,
                                     normalize)

    def _ensemble_users(self, who: str, hist_idx, hist_sizes, user_idx, exclude_history: bool, eligible, clicks):
        """The user side of ``recommend_ensemble`` and ``rank_clicks_ensemble`` (``who``): the caller's side of the call checked and
        on the device (``_catalogue_side``) -> (the user matrix of every sub-model: the mean of the gathered history rows of its
        table, the click lists, (excl_idx, excl_off, eligible)).  Builds the tables when they are missing; nothing is read
        back."""
        from .dense_batch import dense_rows
        hist_idx, eligible, targets = _catalogue_side(who, self, hist_idx, hist_sizes, eligible, clicks)
        if self.vectors is None:
            self.build()
        meta = self.caches[0]._user_meta(hist_sizes, user_idx)
        users = []
        for vec in self.vectors:
            hv = ops.embedding_gather(vec, hist_idx.reshape(-1, 1)).reshape(-1, vec.shape[1])
            dense = dense_rows(hv, meta["batch_hist"], meta["batch_size"], meta["max_hist"], meta["hist_offsets"])
            users.append(ops.HistMeanFn.apply(dense, meta["hist_offsets"]))
        excl = (hist_idx, meta["hist_offsets"]) if exclude_history else (None, None)
        return users, targets, (*excl, eligible)

    @torch.no_grad()
    def rank_clicks_ensemble(self, hist_idx: torch.Tensor, hist_sizes: torch.Tensor, click_idx: torch.Tensor,
                             click_sizes: torch.Tensor, user_idx: Optional[torch.Tensor] = None, exclude_history: bool = True,
                             eligible: Optional[torch.Tensor] = None, return_stats: bool = False):
        """Where each user's held-out clicks land when the user's ensemble score ranks the WHOLE table -> (rank int32 (n_clicks),
        score fp32 (n_clicks), ranked int32 (B), status[, stats (B, T, 2): mean, sd]): ``recommend_ensemble``'s user vectors,
        population, statistics, scores, order, exclusion of the history and ``eligible``, with ``ops.catalogue_ensemble_ranks``
        counting where ``recommend_ensemble`` selects: ``rank <= k`` exactly when the click is slot ``rank - 1`` of
        ``recommend_ensemble(k)``.  ``rank`` is 0 when the click is not in the user's population, and for every click of a user
        ``recommend_ensemble`` refuses (``status``: ``ops.ENSEMBLE_RANK_FLAGS``; its ``ranked`` is 0 too).  The z-score is taken
        over the user's whole population, not over an impression's candidates: it is the number ``recommend_ensemble`` ranks
        by, not the one ``scores`` returns for an impression.  Same contract as ``NewsVectorCache.rank_clicks``: ``hist_idx``
        and ``click_idx`` on the GPU, ``hist_sizes`` and ``click_sizes`` on the host, at most ``ops.RANK_MAX_TARGETS`` clicks a
        user (``ValueError`` otherwise), nothing read back."""
        users, targets, tail = self._ensemble_users("rank_clicks_ensemble",
                                                    hist_idx, hist_sizes, user_idx, exclude_history, eligible, (click_idx, click_sizes))
        rank, score, ranked, status, stats = ops.catalogue_ensemble_ranks(users, self.vectors, self.weights, *targets, *tail)
        return (rank, score, ranked, status, stats) if return_stats else (rank, score, ranked, status)


class NpaFeatureCache(_ImpressionCache):
    """Encode-once evaluation of ``npa_module.NPAModule``.  An NPA news vector depends on the user, but in eval mode only through the
    pooling: the conv feature maps ``c = relu(cnn(embedding(title)))`` (L, F) depend on the news alone.  ``build`` runs the lookup and
    the convolution over the table once into ``features`` (num_news, L, F) fp32 (65 k news x 30 x 400: 3.1 GB); ``scores`` is the
    per-user queries (``NpaUserQueriesFn`` at p = 0, as the forward) plus ``nrl_npa_cached_scores``, which pools the history and
    candidate maps straight from the table with each user's queries, attends over the pooled history (counting the zero rows up to
    the batch's longest history, as the forward) and takes the dot products.

    A SNAPSHOT of the weights at ``build()``: after they change, call ``build()`` again (nothing is keyed on them).  The feature maps
    carry the bits of the GEMM engine they were built under (``engine``); the scorer itself is engine-independent.
    ``hist_sizes`` / ``cand_sizes`` are HOST tensors, as ``evaluate_impressions`` builds them: their maxima are read on the host."""
    user_idx_reason = "NPA's attention queries come from the user embedding"

    def __init__(self, module, table: DeviceNewsTable, chunk: int = 16384):
        from .npa_module import NPAModule
        if not isinstance(module, NPAModule):
            raise TypeError(f"NpaFeatureCache caches the conv feature maps of an NPAModule, got {type(module).__name__}; "
                            "every other recommender is served by NewsVectorCache")
        self.module, self.table, self.chunk = module, table, int(chunk)
        self.features: Optional[torch.Tensor] = None
        self.engine: Optional[str] = None
        self._row_class: Dict[str, torch.Tensor] = {}       # aspect -> (num_news) int32: ``rerank_calibrated``'s classes

    @torch.no_grad()
    def build(self) -> torch.Tensor:
        """conv feature maps (num_news, L, F) of the whole table: one allocation, filled chunk by chunk in place."""
        from . import _lib
        enc = self.module.news_encoder
        title = self.table.attrs["title"]
        with eval_mode(self.module):
            feats = torch.empty((self.table.num_news, title.shape[1], enc.cnn.out_channels), dtype=torch.float32,
                                device=self.table.device)
            for lo in range(0, self.table.num_news, self.chunk):
                hi = min(lo + self.chunk, self.table.num_news)
                enc.conv_features(title[lo:hi], out=feats[lo:hi])
        self.features, self.engine = feats, _lib.get_gemm_engine()
        return feats

    @torch.no_grad()
    def scores(self, hist_idx: torch.Tensor, hist_sizes: torch.Tensor, cand_idx: torch.Tensor, cand_sizes: torch.Tensor,
               user_idx: Optional[torch.Tensor] = None) -> torch.Tensor:
        """(B, max_cand) click scores of a batch of impressions given by news-index lists; ``user_idx`` (B) is required."""
        from .ops_npa import npa_cached_scores
        if user_idx is None:
            raise ValueError(f"NpaFeatureCache.scores needs user_idx: {self.user_idx_reason}")
        if self.features is None:
            self.build()
        dev = self.table.device
        max_hist = int(hist_sizes.max()) if hist_sizes.numel() else 0      # host tensors: no read-back
        max_cand = int(cand_sizes.max()) if cand_sizes.numel() else 0
        hist_off, cand_off = ragged_offsets(hist_sizes, dev), ragged_offsets(cand_sizes, dev)
        B = int(hist_sizes.numel())
        text_q, q_news = self.module.user_queries(user_idx.to(dev).long())      # p = 0: the forward's eval-mode queries
        q_hist, q_cand = text_q[:B], text_q[B:]
        return npa_cached_scores(self.features, hist_idx.to(dev).long(), hist_off, cand_idx.to(dev).long(), cand_off, q_hist,
                                 q_cand, q_news, max_hist, max_cand)

    def recommend(self, *args, **kwargs):
        raise NotImplementedError("NPA's news vectors depend on the user (personalized attention pooling, text.py:385-390): there "
                                  "is no (V, D) table to rank with one user vector, so the whole catalogue cannot be scored by "
                                  "one GEMM + top-k; `recommend_pooled` ranks it from the cached feature maps (two GEMMs and a "
                                  "softmax over the tokens per user and news, fused)")

    def rank_clicks(self, *args, **kwargs):
        raise NotImplementedError("only the dot-product families are served by `rank_clicks` so far (NewsVectorCache over a "
                                  "`dot_product_scorer` module): NPA's personalized-pooling score is counted by "
                                  "`rank_clicks_pooled`")

    def policy_stats(self, *args, **kwargs):
        _policy_refusal("policy_stats", self)

    def list_log_probs(self, *args, **kwargs):
        _policy_refusal("list_log_probs", self)

    def rerank_diverse(self, *args, **kwargs):
        raise NotImplementedError("MMR trades relevance against the similarity of two news vectors, and an NPA news vector depends "
                                  "on the user (personalized attention pooling, text.py:385-390): the cache holds feature maps, not "
                                  "a (V, D) table of news vectors to take that similarity in")

    def rerank_dpp(self, *args, **kwargs):
        raise NotImplementedError("a DPP's kernel matrix is built from the similarity of two news vectors, and an NPA news vector "
                                  "depends on the user (personalized attention pooling, text.py:385-390): the cache holds feature "
                                  "maps, not a (V, D) table of news vectors to take that similarity in")

    @torch.no_grad()
    def rerank_calibrated(self, pool_idx: torch.Tensor, pool_score: torch.Tensor, k: int, aspect: str, target: torch.Tensor,
                          lam: float, mu: float, gamma: float, similarity: str = "cosine", normalize: bool = True):
        """``NewsVectorCache.rerank_calibrated`` of a pool ``recommend_pooled`` returned, without a table: calibration needs the
        classes of the news, not their vectors.  ``ValueError`` unless ``mu == 0``: the redundancy penalty is what
        ``rerank_diverse`` refuses."""
        if float(mu) != 0.0:
            raise ValueError("NpaFeatureCache.rerank_calibrated serves mu == 0 only: the penalty mu weighs is a similarity of news "
                             "vectors, and an NPA news vector depends on the user (`rerank_diverse` says why)")
        return ops.calibrated_rerank(pool_idx, pool_score, None, _aspect_classes(self, aspect), target, k, lam, 0.0, gamma, similarity,
                                     normalize)

    @torch.no_grad()
    def recommend_pooled(self, hist_idx: torch.Tensor, hist_sizes: torch.Tensor, k: int, user_idx: Optional[torch.Tensor] = None,
                         exclude_history: bool = True, eligible: Optional[torch.Tensor] = None):
        """The ``k`` news of the WHOLE table each user scores highest -> (news_idx (B, k) int64, scores (B, k) fp32, status), by
        the score ``scores`` gives a candidate: the user vector dotted with the news' feature map pooled by the user's
        candidate-side text query (``ops.topk_pooled_scores``: neither the pooled vectors nor a (B, V, L) array is formed).  The
        queries come from ``module.user_queries(user_idx)`` (required: ``user_idx_reason``); the user vectors are the ones
        ``scores`` computes for the same batch, bit for bit -- ``npa_cached_scores`` over the history with an empty candidate
        list: history rows pooled with the history-side query, then the personalized attention, or the mean under late fusion
        (the same ranking kernel either way).  Under early fusion that attention counts ``max_hist - n`` virtual zero rows,
        ``max_hist`` the longest history OF THE BATCH (the model's own ``to_dense_batch`` quirk): a user's vector, hence its
        ranking, depends on the batch it is in exactly as in ``scores``.  Same contract as ``NewsVectorCache.recommend``:
        ``hist_idx`` on the GPU, ``hist_sizes`` on the host, nothing read back; the features are built at the first use."""
        scorer, _, tail = self._pooled_user_side("recommend_pooled",
                                                 hist_idx, hist_sizes, user_idx, exclude_history, eligible, None)
        return ops.topk_pooled_scores(*scorer, self.features, k, *tail)

    def _pooled_user_side(self, who: str, hist_idx, hist_sizes, user_idx, exclude_history: bool, eligible, clicks):
        """The user side ``recommend_pooled`` documents, for it and for ``rank_clicks_pooled`` (``who``): ``user_idx`` required, the
        caller's side of the call checked and on the device (``_catalogue_side``) -> ((q_cand, user), the click lists,
        (excl_idx, excl_off, eligible)); nothing read back."""
        from .ops_npa import npa_cached_scores
        if user_idx is None:
            raise ValueError(f"NpaFeatureCache.{who} needs user_idx: {self.user_idx_reason}")
        hist_idx, eligible, targets = _catalogue_side(who, self, hist_idx, hist_sizes, eligible, clicks)
        if self.features is None:
            self.build()
        dev = self.table.device
        hs = hist_sizes.detach().cpu().long()               # host sizes: the maximum and the offsets cost no read-back
        B = int(hs.numel())
        max_hist = int(hs.max()) if B else 0
        hist_off = _click_offsets(hs, dev)
        user_idx = user_idx if user_idx.is_cuda else user_idx.pin_memory().to(dev, non_blocking=True)
        with eval_mode(self.module):
            text_q, q_news = self.module.user_queries(user_idx.to(dev).long())      # p = 0, as ``scores``
        q_hist, q_cand = text_q[:B], text_q[B:]
        no_cand = torch.empty(0, dtype=torch.int64, device=dev)
        # (the scorer wants a score buffer: one padded slot per user, no candidate rows)
        _, user = npa_cached_scores(self.features, hist_idx, hist_off, no_cand, torch.zeros(B + 1, dtype=torch.int64, device=dev),
                                    q_hist, q_cand, q_news, max_hist, 1, return_user_vectors=True)
        excl = (hist_idx, hist_off) if exclude_history else (None, None)
        return (q_cand, user), targets, (*excl, eligible)

    @torch.no_grad()
    def rank_clicks_pooled(self, hist_idx: torch.Tensor, hist_sizes: torch.Tensor, click_idx: torch.Tensor, click_sizes: torch.Tensor,
                           user_idx: Optional[torch.Tensor] = None, exclude_history: bool = True,
                           eligible: Optional[torch.Tensor] = None):
        """``NewsVectorCache.rank_clicks`` by the score of ``recommend_pooled`` -> (rank int32 (n_clicks), score fp32 (n_clicks),
        ranked int32 (B), status): ``recommend_pooled``'s queries and user vectors (``user_idx`` required; the ``max_hist`` quirk
        included), scores, order, exclusion of the history and ``eligible``, with ``ops.catalogue_pooled_ranks`` counting where
        ``recommend_pooled`` selects: ``rank <= k`` exactly when the click is slot ``rank - 1`` of ``recommend_pooled(k)``.  The
        click side is that of ``rank_clicks`` (host ``click_sizes``, at most ``ops.RANK_MAX_TARGETS`` a user, nothing read back)."""
        scorer, targets, tail = self._pooled_user_side("rank_clicks_pooled",
                                                       hist_idx, hist_sizes, user_idx, exclude_history, eligible, (click_idx, click_sizes))
        return ops.catalogue_pooled_ranks(*scorer, self.features, *targets, *tail)


def evaluate_impressions(cache: NewsVectorCache, impressions: Sequence[Dict], batch_size: int = 512,
                         top_k_list: Sequence[int] = (5, 10), num_categ_classes: Optional[int] = None,
                         num_sent_classes: Optional[int] = None, device_metrics: bool = False) -> Dict[str, float]:
    """Scores a list of impressions ({"hist": idx tensor, "cand": idx tensor, "labels": tensor[, "user_idx"]})
    in batches and returns the epoch-end metrics of ``on_test_epoch_end`` (nrms_module.py:456-493).
    ``device_metrics=True`` feeds every batch to a ``metrics.StreamingMetrics`` (``nrl_impression_metrics`` into an epoch
    accumulator) instead of keeping the step outputs for the torch metrics; the returned dict has the same keys."""
    from .metrics import StreamingMetrics, aspect_metrics, ranking_metrics
    outs = []
    stream = StreamingMetrics(top_k_list, num_categ_classes, num_sent_classes) if device_metrics else None
    loss_sum, steps = 0.0, 0
    for lo in range(0, len(impressions), batch_size):
        chunk = impressions[lo:lo + batch_size]
        hs = torch.tensor([len(i["hist"]) for i in chunk])
        cs = torch.tensor([len(i["cand"]) for i in chunk])
        uidx = torch.stack([torch.as_tensor(i["user_idx"]) for i in chunk]) if "user_idx" in chunk[0] else None
        out = cache.model_step(torch.cat([torch.as_tensor(i["hist"]) for i in chunk]), hs,
                               torch.cat([torch.as_tensor(i["cand"]) for i in chunk]), cs,
                               torch.cat([torch.as_tensor(i["labels"]).float() for i in chunk]), uidx)
        if stream is not None:
            stream.update(out)
            loss_sum, steps = loss_sum + out[0].detach().double(), steps + 1      # stays on the device until the end
        else:
            outs.append(out)
    if stream is not None:
        logs = {"loss": float(loss_sum) / max(1, steps)}
        logs.update(stream.compute() or {"mrr": 0.0, **{f"ndcg@{k}": 0.0 for k in top_k_list}, "auc": 0.0})
        return logs
    cat = lambda j: torch.cat([o[j] for o in outs])  # noqa: E731
    logs = {"loss": float(sum(float(o[0]) for o in outs) / max(1, len(outs)))}
    logs.update(ranking_metrics(cat(1), cat(2), cat(3), top_k_list))
    for name, tj, hj, ncls in (("categ", 5, 7, num_categ_classes), ("sent", 6, 8, num_sent_classes)):
        if ncls and cat(tj).numel() and cat(hj).numel():
            logs.update(aspect_metrics(cat(1), cat(tj), cat(hj), cat(3), cat(4), ncls, top_k_list, prefix=name))
    return logs


def evaluate_weight_grid(cache, impressions: Sequence[Dict], weights, batch_size: int = 512, top_k_list: Sequence[int] = (5, 10),
                         num_categ_classes: Optional[int] = None, num_sent_classes: Optional[int] = None) -> Dict:
    """``evaluate_impressions(..., device_metrics=True)`` for a whole grid of ensemble weights in one pass over the impressions
    -> ``metrics.GridStreamingMetrics.compute()``: {"weights", "columns", "values" (G, columns)}, row g being, to the bit, the
    means ``evaluate_impressions`` returns for an ensemble whose sub-model weights are ``weights[g]`` (no "auc", no "loss").
    ``weights`` (G, T): one entry per LOADED sub-model of ``cache.module``, in ``module.submodels()`` order (the CR-Module
    first, where the reference's weight is 1) -- so the module must be built with every sub-model the grid is to cover, at any
    non-zero weight; a weight of 0 in a row leaves that sub-model out of the row, as the reference's ``if categ_weight != 0``.
    Batches exactly as ``evaluate_impressions``; per batch one ``cache.zscores``, one ``GridStreamingMetrics.update`` and no
    device-to-host copy; one read at the end."""
    from .metrics import GridStreamingMetrics
    if not hasattr(cache, "zscores"):
        raise TypeError(f"evaluate_weight_grid needs a cache with `zscores` (MannerVectorCache): the grid combines the standardised "
                        f"scores of an ensemble's sub-models, and {type(cache).__name__} has none")
    n_sub = len(cache.weights)
    w = torch.as_tensor(weights, dtype=torch.float32)
    if w.dim() != 2 or w.shape[1] != n_sub:
        raise ValueError(f"evaluate_weight_grid: every weight row needs one entry per loaded sub-model, in module.submodels() order: "
                         f"{n_sub} here, got weights of shape {tuple(w.shape)}; build the module with every sub-model the grid is "
                         "to cover (any non-zero weight loads it)")
    grid = GridStreamingMetrics(w, top_k_list, num_categ_classes, num_sent_classes)
    dev = cache.table.device
    empty = torch.empty(0, dtype=torch.int64, device=dev)

    def attr(idx, name):
        return cache.table.attrs[name].index_select(0, idx) if name in cache.table.attrs else empty

    for lo in range(0, len(impressions), batch_size):
        chunk = impressions[lo:lo + batch_size]
        hs = torch.tensor([len(i["hist"]) for i in chunk])
        cs = torch.tensor([len(i["cand"]) for i in chunk])
        hist_idx = torch.cat([torch.as_tensor(i["hist"]) for i in chunk]).to(dev).long()
        cand_idx = torch.cat([torch.as_tensor(i["cand"]) for i in chunk]).to(dev).long()
        labels = torch.cat([torch.as_tensor(i["labels"]).float() for i in chunk]).to(dev)
        comp = cache.zscores(hist_idx, hs, cand_idx, cs)
        grid.update(comp, (None, None, labels, cs, hs, attr(cand_idx, "category"), attr(cand_idx, "sentiment"),
                           attr(hist_idx, "category"), attr(hist_idx, "sentiment")))
    return grid.compute() or {"weights": w.tolist(), "columns": [], "values": [[] for _ in range(w.shape[0])]}


def format_recommendations(user_ids: Sequence, news_idx: torch.Tensor, scores: torch.Tensor,
                           news_ids: Optional[torch.Tensor] = None) -> Dict[str, Dict[str, float]]:
    """Host tensors (B, k) of ``recommend`` -> the reference's recommendation dictionary ``{"U<user id>": {"N<news id>": score}}``
    (``AbstractRecommender._get_recommendations``; ``_save_recommendations`` writes it unchanged).  ``news_ids`` (num_news) maps
    a table row to its news id, the row number stands in without it; slots with index ``-1`` are left out."""
    out: Dict[str, Dict[str, float]] = {}
    for uid, rows, vals in zip(user_ids, news_idx.tolist(), scores.tolist()):
        out["U" + str(int(uid))] = {"N" + str(int(news_ids[r]) if news_ids is not None else r): float(v)
                                    for r, v in zip(rows, vals) if r >= 0}
    return out


def recommend_users(cache: NewsVectorCache, users: Sequence[Dict], k: int, batch_size: int = 512,
                    eligible: Optional[torch.Tensor] = None, cap: Optional[Tuple[str, int]] = None,
                    diversify: Optional[Tuple[int, float]] = None, calibrate: Optional[Dict] = None,
                    dpp: Optional[Dict] = None, window: Optional[Tuple[int, int]] = None,
                    sample: Optional[Tuple[float, int]] = None) -> Dict[str, Dict[str, float]]:
    """``cache.recommend`` (``cache.recommend_interests`` where the cache's module is a ``multi_interest_scorer``,
    ``cache.recommend_dnn`` where it is a ``dnn_predictor_scorer``, ``cache.recommend_pooled`` where it is a
    ``personalized_pooling_scorer``: ``NpaFeatureCache``, whose users need ``user_idx``,
    ``cache.recommend_biased`` -- the bias-free score, its default -- where it is a ``class_biased_scorer``: SentiDebias, to which
    ``cap`` is routed as well, ``cache.recommend_ensemble`` where the cache has one: ``MannerVectorCache``) over a list of
    users ({"hist": idx tensor[, "user_idx", "user_id"]}) in batches -> the recommendation dictionary of ``format_recommendations``.  ``user_id`` defaults to the user's position in the list + 1 (as ``build_batch``);
    news ids come from the table's ``news_ids`` column when it has one.  One device-to-host copy per batch, at its end; a status
    flag of the batch (``ops.TOPK_FLAGS``: each is handled by the kernel) is passed on as a warning.

    ``cap`` = (aspect, max_per_class): at most that many news of any one class of the table's ``aspect`` column in a user's list
    (``cache.recommend_ensemble_capped`` where the cache has one, else ``cache.recommend_capped``).  ``NotImplementedError`` for
    the caches of the other scorers (MINER, DKN, NPA): their capped kernels do not exist yet.

    ``diversify`` = (pool, lam): the method picked above returns each user's ``pool`` best news (``k <= pool <=
    ops.MMR_MAX_POOL``; under ``cap`` at most ``ops.TOPK_CAP_MAX_K``) and ``cache.rerank_diverse(idx, score, k, lam)`` -- greedy
    MMR by the cosine of the cached news vectors, the relevance min-max scaled -- picks the ``k`` that are listed, in its order,
    with the scores the scorer gave them.  Its status word (``ops.MMR_FLAGS``) is OR-ed into the batch's on the device, 16 bits
    up, so there is still one device-to-host copy per batch.  ``None`` is the path without it, launch for launch.

    ``calibrate`` = dict(pool=, aspect=, gamma=, lam=1.0, mu=0.0, target="history" | "proportional"): the method picked above
    returns each user's ``pool`` best news and ``cache.rerank_calibrated`` picks the ``k`` that are listed, pulling the list's
    mix of the classes of the table's ``aspect`` column towards the user's own with weight ``gamma``.  The target is
    ``ops.class_targets`` of the batch's histories over ``ops.CAL_MAX_CLASSES`` classes (no read-back is needed to count them;
    a class id beyond is flagged): the integer class counts (``"history"``, the default: the term is the list's
    Personalization@k) or the class proportions times ``k`` (``"proportional"``).  ``mu`` adds MMR's penalty, so ``calibrate``
    together with ``diversify`` is a ``ValueError``; an ``NpaFeatureCache`` is served with ``mu == 0``.  The status word
    (``ops.CAL_FLAGS``) is OR-ed in 16 bits up like ``diversify``'s.  ``None`` is the path without it, launch for launch.

    ``dpp`` = dict(pool=, alpha=1.0, eps=1e-4): the method picked above returns each user's ``pool`` best news (``k <= pool``,
    ``k <= ops.DPP_MAX_K``) and ``cache.rerank_dpp(idx, score, k, alpha, eps=eps)`` -- greedy DPP inference by the cosine of the
    cached news vectors with quality ``exp(alpha * rel)``, the relevance min-max scaled -- picks the ``k`` that are listed.  It is
    a diversifier of its own, so together with ``diversify`` or ``calibrate`` it is a ``ValueError``.  The status word
    (``ops.DPP_FLAGS``) is OR-ed in 16 bits up like theirs.  ``None`` is the path without it, launch for launch.

    ``window`` = (before, after), in the unit of the table's ``time`` column: every user dictionary carries ``"time"`` (the time of
    the request; ``ValueError`` otherwise) and is recommended only news published in ``[time - before, time + after]`` (``None``
    for a side: unbounded), computed on the host and clamped to int32 (``user_windows``): ``cache.recommend(..., window=...)``.
    The pool of ``diversify`` / ``calibrate`` / ``dpp`` comes from the windowed call.  ``NotImplementedError`` together with
    ``cap`` and for every cache but a plain dot-product one: the windowed walk has no capped consumer and no other producer yet.

    ``sample`` = (temperature, seed): every user's list is ONE draw without replacement from the Plackett-Luce policy over
    ``softmax(score / temperature)`` instead of the ``k`` best news (``cache.recommend(..., sample=...)``: Gumbel top-k), in the
    order drawn, with the raw scores.  ``temperature > 0``; its inverse is taken on the host.  The key of a user is its
    ``user_id``, so a user's draw is a function of ``(seed, user_id)`` and its own history: it does not depend on ``batch_size`` or
    on the other users of the list (given a user encoder that does not couple the users of a batch; NRMS' seq-first user attention
    does).  ``NotImplementedError`` together with ``cap`` or ``window`` and for every cache but a plain
    dot-product one (the sampled kernels do not exist yet), ``ValueError`` together with ``diversify`` / ``calibrate`` / ``dpp``."""
    if sample is not None:
        inv_temp, sample_seed = _sample_policy("recommend_users(sample=...)", cache, sample, cap, window, (diversify, calibrate, dpp))
    if window is not None:
        if cap is not None:
            raise NotImplementedError("recommend_users(window=..., cap=...): the windowed walk runs the plain selecting consumer; a "
                                      "windowed class-capped kernel (tkcap_scores_kernel under a window) does not exist yet")
        _window_refusal("recommend_users(window=...)", cache)
        win_lo, win_hi = user_windows(users, *window)
        _row_times(cache)
    if dpp is not None:
        if diversify is not None or calibrate is not None:
            raise ValueError("recommend_users: `dpp` excludes `diversify` and `calibrate`: each of the three picks the k listed "
                             "news from the pool by an objective of its own")
        unknown = set(dpp) - {"pool", "alpha", "eps"}
        if unknown or "pool" not in dpp:
            raise ValueError(f"recommend_users(dpp=dict(pool=, alpha=1.0, eps=1e-4)): got {sorted(dpp)}")
        pool, dpp_alpha, dpp_eps = int(dpp["pool"]), float(dpp.get("alpha", 1.0)), float(dpp.get("eps", 1e-4))
        if pool < k:
            raise ValueError(f"recommend_users(dpp=dict(pool=...)): the pool ({pool}) must hold at least k = {k} news")
        if getattr(cache.module, "personalized_pooling_scorer", False):
            cache.rerank_dpp()                              # (NpaFeatureCache: refuses and says why, before any device work)
    if calibrate is not None:
        if diversify is not None:
            raise ValueError("recommend_users: `calibrate` and `diversify` exclude each other; calibrate=dict(..., mu=...) is MMR's "
                             "penalty beside the calibration term")
        unknown = set(calibrate) - {"pool", "aspect", "gamma", "lam", "mu", "target"}
        if unknown or not {"pool", "aspect", "gamma"} <= set(calibrate):
            raise ValueError("recommend_users(calibrate=dict(pool=, aspect=, gamma=, lam=1.0, mu=0.0, target=\"history\")): got "
                             f"{sorted(calibrate)}")
        pool, cal_aspect, cal_how = int(calibrate["pool"]), calibrate["aspect"], calibrate.get("target", "history")
        cal_weights = (float(calibrate.get("lam", 1.0)), float(calibrate.get("mu", 0.0)), float(calibrate["gamma"]))
        if pool < k:
            raise ValueError(f"recommend_users(calibrate=dict(pool=...)): the pool ({pool}) must hold at least k = {k} news")
        if cal_how not in ("history", "proportional"):
            raise ValueError(f"recommend_users(calibrate=dict(target=...)): \"history\" or \"proportional\", got {cal_how!r}")
        if getattr(cache.module, "personalized_pooling_scorer", False) and cal_weights[1] != 0.0:
            cache.rerank_calibrated(None, None, k, cal_aspect, None, *cal_weights)      # (NpaFeatureCache: refuses and says why)
    if diversify is not None:
        pool, lam = int(diversify[0]), float(diversify[1])
        if pool < k:
            raise ValueError(f"recommend_users(diversify=(pool, lam)): the pool ({pool}) must hold at least k = {k} news")
        if getattr(cache.module, "personalized_pooling_scorer", False):
            cache.rerank_diverse()                          # (NpaFeatureCache: refuses and says why, before any device work)
    if cap is not None:
        other = [a for a in ("multi_interest_scorer", "dnn_predictor_scorer", "personalized_pooling_scorer")
                 if getattr(cache.module, a, False)]
        if other:
            raise NotImplementedError(f"recommend_users(cap=...) serves the dot-product families and MANNeR's ensemble; "
                                      f"{type(cache.module).__name__} is a `{other[0]}`, whose capped top-k kernel does not exist yet")
        aspect, max_per_class = cap
    dev = cache.table.device
    news_ids = cache.table.attrs["news_ids"].cpu() if "news_ids" in cache.table.attrs else None
    out: Dict[str, Dict[str, float]] = {}
    for lo in range(0, len(users), batch_size):
        chunk = users[lo:lo + batch_size]
        hs = torch.tensor([len(u["hist"]) for u in chunk])
        hist = torch.cat([torch.as_tensor(u["hist"]).long() for u in chunk]).to(dev)
        uidx = torch.stack([torch.as_tensor(u["user_idx"]) for u in chunk]) if "user_idx" in chunk[0] else None
        rank = cache.recommend_interests if getattr(cache.module, "multi_interest_scorer", False) else \
            cache.recommend_dnn if getattr(cache.module, "dnn_predictor_scorer", False) else \
            cache.recommend_pooled if getattr(cache.module, "personalized_pooling_scorer", False) else cache.recommend
        rank = getattr(cache, "recommend_ensemble", rank)
        biased = getattr(cache.module, "class_biased_scorer", False)
        if biased:
            rank = cache.recommend_biased
        if cap is not None and biased:
            rank = lambda hist, hs, k, **kw: cache.recommend_biased(hist, hs, k, cap=(aspect, max_per_class), **kw)  # noqa: E731
        elif cap is not None:
            capped = getattr(cache, "recommend_ensemble_capped", None) or cache.recommend_capped
            rank = lambda hist, hs, k, **kw: capped(hist, hs, k, aspect, max_per_class, **kw)  # noqa: E731
        reranked = diversify is not None or calibrate is not None or dpp is not None
        if sample is not None:
            idx, score, status = cache.recommend(hist, hs, k, user_idx=uidx, eligible=eligible,
                                                 sample=(inv_temp, sample_seed, torch.tensor(_user_ids(chunk, lo), dtype=torch.int64)))
        elif window is not None:
            idx, score, status = cache.recommend(hist, hs, pool if reranked else k, user_idx=uidx, eligible=eligible,
                                                 window=(win_lo[lo:lo + batch_size], win_hi[lo:lo + batch_size]))
        else:
            idx, score, status = rank(hist, hs, pool if reranked else k, user_idx=uidx, eligible=eligible)
        if dpp is not None:
            idx, score, _, dpp_status = cache.rerank_dpp(idx, score, k, dpp_alpha, eps=dpp_eps)
            status = status | (dpp_status << 16)
        if diversify is not None:
            idx, score, _, mmr_status = cache.rerank_diverse(idx, score, k, lam)
            status = status | (mmr_status << 16)
        if calibrate is not None:
            target = ops.class_targets(hist, _click_offsets(hs.long(), dev), _aspect_classes(cache, cal_aspect), ops.CAL_MAX_CLASSES,
                                       k if cal_how == "proportional" else None)
            idx, score, _, _, cal_status = cache.rerank_calibrated(idx, score, k, cal_aspect, target, *cal_weights)
            status = status | (cal_status << 16)
        packed = torch.cat([idx.double(), score.double(), status.double().expand(idx.shape[0], 1)], dim=1).cpu()      # the one copy
        word = int(packed[0, -1]) if packed.shape[0] else 0
        if word:                                            # the kernel has dealt with each of these; the caller should know
            import warnings
            flags = ops.TOPK_BIAS_FLAGS if biased else ops.TOPK_FLAGS
            second = ops.DPP_FLAGS if dpp is not None else ops.CAL_FLAGS if calibrate is not None else ops.MMR_FLAGS
            said = [msg for bit, msg in flags.items() if word & bit] + [msg for bit, msg in second.items() if (word >> 16) & bit]
            warnings.warn("recommend_users: " + "; ".join(said))
        out.update(format_recommendations(_user_ids(chunk, lo), packed[:, :k].long(), packed[:, k:2 * k].float(), news_ids))
    return out


def sample_recommendations(cache: NewsVectorCache, users: Sequence[Dict], k: int, draws: int, temperature: float, seed: int,
                           batch_size: int = 512, eligible: Optional[torch.Tensor] = None, log_probs: bool = False):
    """``draws`` independent lists per user from the Plackett-Luce policy over ``softmax(score / temperature)`` -> news rows
    (n_users, draws, k) int64 on the host, ``-1`` beyond a user's population.  Draw ``j`` is the list
    ``recommend_users(..., sample=(temperature, (seed + j) mod 2^64))`` gives the user -- the same keys (``user_id``, or position
    + 1), the same refusals -- so it is reproducible user by user whatever the batching.  A batch's histories are uploaded once and
    serve all its draws; a status flag (``ops.TOPK_FLAGS``) is passed on as a warning.  With ``draws >= 2`` a batch goes through
    ``cache.recommend_draws`` (where the cache has one): one pass of the user encoder, every dot product computed once per group of
    draws (``ops.topk_sampled_draws``) and one device-to-host copy per batch.  A single draw, and a cache without
    ``recommend_draws``, is one ``cache.recommend(sample=...)`` and one copy per draw; the lists are the same bits either way.

    ``log_probs=True`` returns ``(lists, logp)``: ``logp`` (n_users, draws, k) float32 on the host, slot by slot the log-probability
    ``cache.list_log_probs`` gives the drawn list under the same temperature (``+0`` in an empty slot; a list's propensity is the
    sum over its slots).  The histories are still uploaded once per batch; every draw costs one ``cache.list_log_probs`` call, one
    more pass over the table (the tail of its list), and the batch's copy carries the log-probabilities as well.  The default
    returns exactly what it returned without the argument."""
    who = "sample_recommendations"
    inv_temp, seed = _sample_policy(who, cache, (temperature, seed))
    draws = int(draws)
    if draws < 0:
        raise ValueError(f"{who}: draws >= 0, got {draws}")
    dev = cache.table.device
    out = torch.full((len(users), draws, max(int(k), 0)), -1, dtype=torch.int64)
    logp = torch.zeros((len(users), draws, max(int(k), 0)), dtype=torch.float32) if log_probs else None
    word = 0
    for lo in range(0, len(users), batch_size):
        chunk = users[lo:lo + batch_size]
        hs = torch.tensor([len(u["hist"]) for u in chunk])
        hist = torch.cat([torch.as_tensor(u["hist"]).long() for u in chunk]).to(dev)
        uidx = torch.stack([torch.as_tensor(u["user_idx"]) for u in chunk]) if "user_idx" in chunk[0] else None
        keys = torch.tensor(_user_ids(chunk, lo), dtype=torch.int64).to(dev)
        together = getattr(cache, "recommend_draws", None) if draws >= 2 else None
        if together is not None:
            idx, _, status = together(hist, hs, k, draws, (inv_temp, seed, keys), user_idx=uidx, eligible=eligible)
            n, flat = idx.shape[0], [idx.reshape(idx.shape[0], -1).double()]
            if log_probs:
                for j in range(draws):
                    lp, _, _, lp_status = cache.list_log_probs(hist, hs, idx[:, j].contiguous(), inv_temp, user_idx=uidx, eligible=eligible)
                    flat.append(lp.double())
                    status = status | lp_status
            packed = torch.cat(flat + [status.double().expand(n, 1)], dim=1).cpu()                        # the one copy
            cells = draws * idx.shape[2]
            out[lo:lo + len(chunk)] = packed[:, :cells].long().reshape(n, draws, -1)
            if log_probs:
                logp[lo:lo + len(chunk)] = packed[:, cells:-1].float().reshape(n, draws, -1)
            word |= int(packed[0, -1]) if packed.shape[0] else 0
            continue
        for j in range(draws):
            idx, _, status = cache.recommend(hist, hs, k, user_idx=uidx, eligible=eligible,
                                             sample=(inv_temp, (seed + j) % 2 ** 64, keys))
            if log_probs:
                lp, _, _, lp_status = cache.list_log_probs(hist, hs, idx, inv_temp, user_idx=uidx, eligible=eligible)
                packed = torch.cat([idx.double(), lp.double(), (status | lp_status).double().expand(idx.shape[0], 1)], dim=1).cpu()
                logp[lo:lo + len(chunk), j] = packed[:, idx.shape[1]:-1].float()
                packed = torch.cat([packed[:, :idx.shape[1]], packed[:, -1:]], dim=1).long()
            else:
                packed = torch.cat([idx, status.long().expand(idx.shape[0], 1)], dim=1).cpu()             # the one copy
            out[lo:lo + len(chunk), j] = packed[:, :-1]
            word |= int(packed[0, -1]) if packed.shape[0] else 0
    if word:                                                # the kernel has dealt with each of these; the caller should know
        import warnings
        flags = ops.POLICY_FLAGS if log_probs else ops.TOPK_FLAGS
        warnings.warn(f"{who}: " + "; ".join(msg for bit, msg in flags.items() if word & bit))
    return (out, logp) if log_probs else out


def exposure_weights(k: int, weights="rbp", patience: float = 0.8) -> torch.Tensor:
    """The position weights of ``exposure_report`` -> (k) float32 on the host: ``"rbp"``: ``patience ** j`` (rank-biased precision's
    browsing model), ``"dcg"``: ``1 / log2(j + 2)``, or a given tensor of ``k`` weights.  Computed in float64 and rounded once."""
    k = int(k)
    if isinstance(weights, torch.Tensor):
        if weights.dim() != 1 or weights.numel() != k:
            raise ValueError(f"exposure_report: `weights` must have one entry per slot ({k}), got {tuple(weights.shape)}")
        return weights.detach().to("cpu", torch.float32)
    j = torch.arange(max(k, 0), dtype=torch.float64)
    if weights == "rbp":
        patience = float(patience)
        if not 0.0 < patience <= 1.0:
            raise ValueError(f"exposure_report: the patience must be in (0, 1], got {patience!r}")
        return (patience ** j).float()
    if weights == "dcg":
        return (1.0 / torch.log2(j + 2.0)).float()
    raise ValueError(f"exposure_report: weights = \"rbp\", \"dcg\" or a tensor of k weights, got {weights!r}")


def exposure_report(cache: NewsVectorCache, users: Sequence[Dict], k: int, draws: int, temperature: float, seed: int, aspect: str,
                    weights="rbp", patience: float = 0.8, batch_size: int = 512, eligible: Optional[torch.Tensor] = None):
    """How much position-weighted exposure the Plackett-Luce policy over ``softmax(score / temperature)`` gives each class of the
    table's ``aspect`` column (``category``, ``sentiment``, ...; class ids in ``[0, ops.TOPK_MAX_BIAS_CLASSES)``), estimated from
    ``draws`` lists of ``k`` per user -> {"per_user": (n_users, S) float32 -- user by user the mean over its draws of the summed
    weights of the slots that show class ``s`` --, "mean": (S) its mean over the users, "share": mean / mean.sum()}, on the host;
    ``S`` is 1 + the largest class id of the column (a class id outside the range is flagged and counts for no class).  The draws are ``sample_recommendations``' (the same seeds, keys and refusals:
    ``cache.recommend_draws``) and never leave the device: ``ops.list_class_exposure`` reduces a batch's lists to its (B, S) rows,
    which stay on the device until one copy at the end.  Position weights: ``exposure_weights(k, weights, patience)``.  A status
    flag of the draws (``ops.TOPK_FLAGS``) or of the reduction (``ops.EXPOSURE_FLAGS``, 16 bits up) is passed on as one warning."""
    who = "exposure_report"
    inv_temp, seed = _sample_policy(who, cache, (temperature, seed))
    draws = int(draws)
    if draws < 1:
        raise ValueError(f"{who}: draws >= 1, got {draws}")
    w = exposure_weights(k, weights, patience)
    classes = _aspect_classes(cache, aspect)
    dev = cache.table.device
    S = ops.TOPK_MAX_BIAS_CLASSES                           # (reduced over every class a lane can own; cut to the column's on the host)
    w = w.to(dev)
    rows, status = [], torch.zeros(1, dtype=torch.int32, device=dev)
    for lo in range(0, len(users), batch_size):
        chunk = users[lo:lo + batch_size]
        hs = torch.tensor([len(u["hist"]) for u in chunk])
        hist = torch.cat([torch.as_tensor(u["hist"]).long() for u in chunk]).to(dev)
        uidx = torch.stack([torch.as_tensor(u["user_idx"]) for u in chunk]) if "user_idx" in chunk[0] else None
        keys = torch.tensor(_user_ids(chunk, lo), dtype=torch.int64).to(dev)
        idx, _, st = cache.recommend_draws(hist, hs, k, draws, (inv_temp, seed, keys), user_idx=uidx, eligible=eligible)
        exposure, est = ops.list_class_exposure(idx, classes, w, S)
        rows.append(exposure)
        status = status | st | (est << 16)
    top = classes.max().reshape(1) if classes.numel() else torch.zeros(1, dtype=torch.int32, device=dev)
    if not rows:
        S = min(max(int(top), 0) + 1, S)
        empty = torch.zeros((0, S), dtype=torch.float32)
        return {"per_user": empty, "mean": torch.full((S,), float("nan")), "share": torch.full((S,), float("nan"))}
    packed = torch.cat([torch.cat(rows).double().reshape(-1), top.double(), status.double()]).cpu()       # the one copy
    word, S = int(packed[-1]), min(max(int(packed[-2]), 0) + 1, S)
    per_user = packed[:-2].float().reshape(-1, ops.TOPK_MAX_BIAS_CLASSES)[:, :S].contiguous()
    if word:                                                # the kernels have dealt with each of these; the caller should know
        import warnings
        said = [msg for bit, msg in ops.TOPK_FLAGS.items() if word & bit] + \
               [msg for bit, msg in ops.EXPOSURE_FLAGS.items() if (word >> 16) & bit]
        warnings.warn(f"{who}: " + "; ".join(said))
    mean = per_user.double().mean(dim=0)
    return {"per_user": per_user, "mean": mean.float(), "share": (mean / mean.sum()).float()}


def policy_report(cache: NewsVectorCache, users: Sequence[Dict], temperatures: Sequence[float], batch_size: int = 512,
                  eligible: Optional[torch.Tensor] = None) -> Dict[float, Dict[str, float]]:
    """How peaked the sampled policy is at each of ``temperatures`` (each finite and > 0), averaged over ``users`` ({"hist": idx
    tensor[, "user_idx"]}) -> {temperature: {"entropy": mean entropy in nats, "perplexity": mean ``exp(entropy)`` -- the effective
    catalogue size --, "top1": mean probability of the user's best news, ``exp(-log_sum)``}}: ``cache.policy_stats`` per batch and
    temperature, the histories of a batch uploaded once.  The per-user values of all batches stay on the device; one
    device-to-host copy per temperature, at the end.  Users with an empty population count with entropy 0, perplexity 1 and
    top1 0.  A status flag (``ops.POLICY_FLAGS``) is passed on as one warning.  Refusals as ``policy_stats``."""
    _policy_refusal("policy_report", cache)
    temps = [float(t) for t in temperatures]
    for t in temps:
        if not math.isfinite(t) or t <= 0:
            raise ValueError(f"policy_report: every temperature must be finite and > 0, got {t!r}")
    dev = cache.table.device
    kept = {t: [] for t in temps}
    for lo in range(0, len(users), batch_size):
        chunk = users[lo:lo + batch_size]
        hs = torch.tensor([len(u["hist"]) for u in chunk])
        hist = torch.cat([torch.as_tensor(u["hist"]).long() for u in chunk]).to(dev)
        uidx = torch.stack([torch.as_tensor(u["user_idx"]) for u in chunk]) if "user_idx" in chunk[0] else None
        for t in temps:
            st = cache.policy_stats(hist, hs, 1.0 / t, user_idx=uidx, eligible=eligible)
            ent, ls = st["entropy"].double(), st["log_sum"].double()
            top1 = torch.where(st["population"] > 0, torch.exp(-ls), torch.zeros_like(ls))
            kept[t].append(torch.cat([ent, torch.exp(ent), top1, st["status"].double()]))
    out, word = {}, 0
    for t in temps:
        if not kept[t]:
            out[t] = {"entropy": float("nan"), "perplexity": float("nan"), "top1": float("nan")}
            continue
        ent, ppl, top1 = [], [], []
        for part in torch.cat(kept[t]).cpu().split([p.numel() for p in kept[t]]):                      # the one copy
            n = (part.numel() - 1) // 3
            ent.append(part[:n])
            ppl.append(part[n:2 * n])
            top1.append(part[2 * n:3 * n])
            word |= int(part[-1])
        out[t] = {"entropy": float(torch.cat(ent).mean()), "perplexity": float(torch.cat(ppl).mean()),
                  "top1": float(torch.cat(top1).mean())}
    if word:                                                # the kernel has dealt with each of these; the caller should know
        import warnings
        warnings.warn("policy_report: " + "; ".join(msg for bit, msg in ops.POLICY_FLAGS.items() if word & bit))
    return out


def evaluate_full_rank(cache: NewsVectorCache, users: Sequence[Dict], top_k_list: Sequence[int] = (5, 10), batch_size: int = 512,
                       eligible: Optional[torch.Tensor] = None, ensemble: bool = False,
                       until_request: bool = False) -> Dict[str, float]:
    """Full-catalogue ranking metrics of held-out clicks: ``cache.rank_clicks`` (``cache.rank_clicks_interests`` where the cache's
    module is a ``multi_interest_scorer``, ``cache.rank_clicks_dnn`` where it is a ``dnn_predictor_scorer``,
    ``cache.rank_clicks_pooled`` where it is a ``personalized_pooling_scorer``, ``cache.rank_clicks_biased`` -- the bias-free score --
    where it is a ``class_biased_scorer``, as ``recommend_users`` picks ``recommend_*``)
    over a list of users ({"hist": idx tensor,
    "clicks": idx tensor[, "user_idx"]}), batched as ``recommend_users`` batches them, then ``metrics.full_rank_metrics``
    (``mrr``, ``ndcg@k``, ``recall@k``, ``hit@k``, ``auc_user``; every click is ranked against every news the user could be
    recommended, not against an impression's candidates).  The ranks, the click counts and the populations of all batches stay
    on the device; one device-to-host copy at the end.  The OR of the batches' status words (``ops.RANK_FLAGS``: each flag is
    handled by the kernel) is passed on as one warning.

    ``ensemble=True`` ranks by MANNeR's ensemble instead: ``cache.rank_clicks_ensemble`` (``MannerVectorCache``; ``TypeError`` for
    a cache without one), the warning worded from ``ops.ENSEMBLE_RANK_FLAGS``.  It is opt-in, where ``recommend_users`` picks
    ``recommend_ensemble`` by itself, because the z-score over the whole catalogue is a different number from the z-score over an
    impression's candidates that MANNeR's ``scores`` returns: the default must not silently change what ``rank_clicks`` means for
    MANNeR, so without the flag ``MannerVectorCache.rank_clicks`` keeps refusing and says where to go.

    ``until_request=True`` is the temporal protocol: every user dictionary carries ``"time"`` (``ValueError`` otherwise) and its
    clicks are ranked against the news of the table's ``time`` column up to that time -- the window ``[INT32_MIN, time]`` of
    ``cache.rank_clicks(..., window=...)`` -- not against news that did not exist yet.  Served and refused as
    ``recommend_users(window=...)``."""
    from .metrics import full_rank_metrics
    if until_request:
        if ensemble:
            raise NotImplementedError("evaluate_full_rank(until_request=True, ensemble=True): a window changes the population the "
                                      "ensemble's statistics pass standardises over; a windowed tkec_count_kernel does not exist yet")
        _window_refusal("evaluate_full_rank(until_request=True)", cache)
        win_lo, win_hi = user_windows(users, None, 0)
        _row_times(cache)
    if ensemble and not callable(getattr(cache, "rank_clicks_ensemble", None)):
        raise TypeError(f"evaluate_full_rank(ensemble=True) needs a cache with `rank_clicks_ensemble` (MannerVectorCache), got "
                        f"{type(cache).__name__}")
    flags = ops.ENSEMBLE_RANK_FLAGS if ensemble else ops.RANK_FLAGS
    dev = cache.table.device
    ranks, sizes, pops, words = [], [], [], []
    for lo in range(0, len(users), batch_size):
        chunk = users[lo:lo + batch_size]
        hs = torch.tensor([len(u["hist"]) for u in chunk])
        cs = torch.tensor([len(u["clicks"]) for u in chunk])
        hist = torch.cat([torch.as_tensor(u["hist"]).long() for u in chunk]).to(dev)
        clicks = torch.cat([torch.as_tensor(u["clicks"]).long() for u in chunk]).to(dev)
        uidx = torch.stack([torch.as_tensor(u["user_idx"]) for u in chunk]) if "user_idx" in chunk[0] else None
        rank_clicks = cache.rank_clicks_interests if getattr(cache.module, "multi_interest_scorer", False) else \
            cache.rank_clicks_dnn if getattr(cache.module, "dnn_predictor_scorer", False) else \
            cache.rank_clicks_pooled if getattr(cache.module, "personalized_pooling_scorer", False) else \
            cache.rank_clicks_biased if getattr(cache.module, "class_biased_scorer", False) else cache.rank_clicks
        if ensemble:
            rank_clicks = cache.rank_clicks_ensemble
        if until_request:
            rank, _, ranked, status = cache.rank_clicks(hist, hs, clicks, cs, user_idx=uidx, eligible=eligible,
                                                        window=(win_lo[lo:lo + batch_size], win_hi[lo:lo + batch_size]))
        else:
            rank, _, ranked, status = rank_clicks(hist, hs, clicks, cs, user_idx=uidx, eligible=eligible)
        ranks.append(rank)
        sizes.append(cs.pin_memory().to(dev, non_blocking=True))
        pops.append(ranked)
        words.append(status)
    if not ranks:
        return full_rank_metrics(torch.zeros(0, dtype=torch.int32), torch.zeros(0, dtype=torch.int64),
                                 torch.zeros(0, dtype=torch.int32), top_k_list)
    word = words[0]
    for w in words[1:]:
        word = torch.bitwise_or(word, w)
    n, B = sum(int(r.numel()) for r in ranks), sum(int(p.numel()) for p in pops)
    packed = torch.cat([torch.cat(ranks).long(), torch.cat(sizes).long(), torch.cat(pops).long(), word.reshape(1).long()]).cpu()
    word = int(packed[-1])
    if word:                                                # the kernel has dealt with each of these; the caller should know
        import warnings
        warnings.warn("evaluate_full_rank: " + "; ".join(msg for bit, msg in flags.items() if word & bit))
    return full_rank_metrics(packed[:n], packed[n:n + B], packed[n + B:n + 2 * B], top_k_list)
