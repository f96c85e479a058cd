"""Epoch-end ranking metrics (AUC, MRR, nDCG@k) over concatenated per-impression scores.

The reference wires torchmetrics ``AUROC``/``RetrievalMRR``/``RetrievalNormalizedDCG`` grouped by an
``indexes`` vector (nrms_module.py:182-195,380-396).  These run once per epoch, outside the timed
step, on small vectors; they are host-side bookkeeping in plain torch, vectorised over queries.

``impression_metrics`` / ``StreamingMetrics`` are the opt-in device-side form (``nrl_impression_metrics``): one small kernel
per batch computes the per-impression values from the ragged outputs and adds them into an O(1) epoch accumulator, so the
epoch end needs neither the concatenated step outputs (beyond the two flat vectors of the global AUC) nor the dense
(impressions, longest impression) tensors and their sorts.  ``ranking_metrics`` / ``aspect_metrics`` stay the default."""
from typing import Dict, Optional, Sequence, Tuple

import torch


def _dense(preds, targets, sizes):
    B, C = sizes.numel(), int(sizes.max()) if sizes.numel() else 0
    mask = torch.arange(C, device=preds.device)[None, :] < sizes[:, None]
    p = preds.new_full((B, C), float("-inf"))
    t = targets.new_zeros((B, C))
    p[mask], t[mask] = preds, targets
    return p, t, mask


def _global_auc(preds: torch.Tensor, targets: torch.Tensor) -> float:
    """global AUROC over all (score, label) pairs, as torchmetrics' binary AUROC without indexes"""
    pos, neg = preds[targets > 0], preds[targets <= 0]
    if pos.numel() and neg.numel():
        allv = torch.cat([pos, neg])
        r = torch.empty(allv.shape, dtype=torch.float64, device=allv.device)
        srt, idx = torch.sort(allv)
        # average ranks for ties; rank sums in float64 (an epoch holds millions of pairs: float32 ranks stop being integers at 2^24)
        uniq, inv, cnt = torch.unique_consecutive(srt, return_inverse=True, return_counts=True)
        ends = torch.cumsum(cnt, 0).double()
        avg_rank = ends - (cnt.double() - 1) / 2
        r[idx] = avg_rank[inv]
        auc = (r[: pos.numel()].sum() - pos.numel() * (pos.numel() + 1) / 2) / (float(pos.numel()) * neg.numel())
        return float(auc)
    return 0.0


def ranking_metrics(preds: torch.Tensor, targets: torch.Tensor, cand_news_size: torch.Tensor,
                    top_k_list: Sequence[int] = (5, 10)) -> Dict[str, float]:
    sizes = cand_news_size.to(preds.device)
    p, t, mask = _dense(preds.float(), targets.float(), sizes)
    order = torch.argsort(p, dim=1, descending=True, stable=True)
    t_sorted = torch.gather(t, 1, order)
    ranks = torch.arange(1, p.shape[1] + 1, device=p.device, dtype=torch.float32)[None, :]
    has_pos = t.sum(1) > 0
    # MRR: reciprocal rank of the first relevant item.  torchmetrics' retrieval metrics default to
    # empty_target_action="neg": an impression WITHOUT a positive counts as 0 and stays in the mean
    # (RetrievalMRR() / RetrievalNormalizedDCG(top_k=k) at nrms_module.py:186,190 take that default).
    first = torch.where(t_sorted > 0, ranks, torch.full_like(ranks, float("inf"))).min(1).values
    rr = torch.where(has_pos, 1.0 / first, torch.zeros_like(first))
    mrr = rr.mean() if rr.numel() else preds.new_tensor(0.0)
    out = {"mrr": float(mrr)}
    disc = 1.0 / torch.log2(ranks + 1.0)
    ideal = torch.sort(t, dim=1, descending=True).values
    for k in top_k_list:
        dcg = (t_sorted[:, :k] * disc[:, :k]).sum(1)
        idcg = (ideal[:, :k] * disc[:, :k]).sum(1)
        ndcg = torch.where(idcg > 0, dcg / idcg.clamp_min(1e-12), torch.zeros_like(dcg))
        out[f"ndcg@{k}"] = float(ndcg.mean()) if ndcg.numel() else 0.0      # 0 for impressions without a positive
    out["auc"] = _global_auc(preds, targets)
    return out


def full_rank_metrics(rank: torch.Tensor, click_sizes: torch.Tensor, ranked: torch.Tensor,
                      top_k_list: Sequence[int] = (5, 10)) -> Dict[str, float]:
    """Full-catalogue ranking metrics from ranks alone (``ops.catalogue_ranks`` / ``NewsVectorCache.rank_clicks``): ``rank``
    (n_clicks) the 1-based place of every held-out click among the news its user could be recommended, 0 = the click is not one
    of them and does not count; ``click_sizes`` (B) the clicks per user, in order; ``ranked`` (B) the size N of each user's
    population.  Plain torch on whatever device the inputs share, in float64.  With r_1 < ... < r_P a user's valid ranks:

    * ``mrr``       1 / r_1;
    * ``ndcg@k``    sum_{r_j <= k} 1 / log2(r_j + 1)  /  sum_{j <= min(P, k)} 1 / log2(j + 1);
    * ``recall@k``  #{r_j <= k} / P;   ``hit@k``  [r_1 <= k];
    * ``auc_user``  1 - sum_j (r_j - j) / (P (N - P)): the share of (click, other news) pairs ranked the right way round.  The
      ranks come with ties already BROKEN by row (equal scores rank by ascending row), not averaged as ``_global_auc`` does.

    Each is the mean over users; a user without a valid click counts 0 and stays in the mean (``ranking_metrics``' convention,
    torchmetrics' ``empty_target_action="neg"``), and so does, for ``auc_user``, a user with N = P.  ``mrr`` and ``ndcg@k`` equal
    ``ranking_metrics`` run on one impression per user whose candidate list is the user's whole population in ascending row
    order."""
    dev = rank.device
    sizes, N = click_sizes.to(dev).long(), ranked.to(dev).double()
    B = int(sizes.numel())
    keys = ["mrr"] + [f"{m}@{k}" for k in top_k_list for m in ("ndcg", "recall", "hit")] + ["auc_user"]
    if B == 0:
        return {k: 0.0 for k in keys}
    C = max(int(sizes.max()), 1)
    off = torch.cumsum(sizes, 0) - sizes
    user = torch.repeat_interleave(torch.arange(B, device=dev), sizes, output_size=int(rank.numel()))
    col = torch.arange(rank.numel(), device=dev) - off[user]
    big = torch.iinfo(torch.int64).max
    dense = torch.full((B, C), big, dtype=torch.int64, device=dev)
    r = rank.long()
    dense[user, col] = torch.where(r > 0, r, torch.full_like(r, big))
    dense = torch.sort(dense, dim=1).values                 # r_1 <= r_2 <= ..., the clicks that do not count at the end
    valid = dense < big
    P = valid.sum(1).double()
    has = P > 0
    rd = torch.where(valid, dense, torch.ones_like(dense)).double()
    zero = torch.zeros(B, dtype=torch.float64, device=dev)
    out = {"mrr": float(torch.where(has, 1.0 / rd[:, 0], zero).mean())}
    gain = torch.where(valid, 1.0 / torch.log2(rd + 1.0), torch.zeros_like(rd))
    ideal = torch.cumsum(1.0 / torch.log2(torch.arange(1, C + 1, device=dev, dtype=torch.float64) + 1.0), 0)
    for k in top_k_list:
        inside = valid & (dense <= k)
        dcg = (gain * inside).sum(1)
        idcg = ideal[(torch.minimum(P, torch.full_like(P, min(int(k), C))).long() - 1).clamp_min(0)]
        out[f"ndcg@{k}"] = float(torch.where(has, dcg / idcg, zero).mean())
        out[f"recall@{k}"] = float(torch.where(has, inside.sum(1).double() / P.clamp_min(1.0), zero).mean())
        out[f"hit@{k}"] = float((has & (dense[:, 0] <= k)).double().mean())
    j = torch.arange(1, C + 1, device=dev, dtype=torch.float64)[None, :]
    wrong = torch.where(valid, rd - j, torch.zeros_like(rd)).sum(1)
    pairs = P * (N - P)
    out["auc_user"] = float(torch.where(has & (pairs > 0), 1.0 - wrong / pairs.clamp_min(1.0), zero).mean())
    return out


def aspect_metrics(preds: torch.Tensor, cand_aspects: torch.Tensor, hist_aspects: torch.Tensor,
                   cand_news_size: torch.Tensor, hist_news_size: torch.Tensor, num_classes: int,
                   top_k_list: Sequence[int] = (5, 10), prefix: str = "categ") -> Dict[str, float]:
    """Aspect-based diversity and personalization of the top-k recommendations, mean over impressions --
    the reference's ``Diversity`` / ``Personalization`` (metrics/diversity.py, metrics/personalization.py,
    metrics/base.py:137-182 on top of metrics/functional.py:8-127), vectorised over impressions instead of
    a Python loop per impression:

    * diversity@k: entropy of the aspect distribution of the k highest-scored candidates / log(num_classes)
      (``functional.py:36-46``: the counts are divided by num_classes and re-normalised by ``Categorical``);
    * personalization@k: generalised Jaccard sum(min) / sum(max) between the aspect counts of those k
      candidates and the aspect counts of the clicked history (``functional.py:85-127``);
    * an impression whose candidate aspects sum to 0 scores 0 (``empty_target_action="neg"``).
    Flat inputs in impression order (as ``model_step`` returns them) + the per-impression sizes."""
    dev = preds.device
    csz, hsz = cand_news_size.to(dev).long(), hist_news_size.to(dev).long()
    B = csz.numel()
    C = int(csz.max()) if B else 0
    cmask = torch.arange(C, device=dev)[None, :] < csz[:, None]
    p = preds.new_full((B, C), float("-inf")).float()
    a = torch.zeros((B, C), dtype=torch.long, device=dev)
    p[cmask], a[cmask] = preds.float(), cand_aspects.to(dev).long()
    order = torch.argsort(p, dim=1, descending=True, stable=True)
    a_sorted = torch.gather(a, 1, order)
    valid_sorted = torch.gather(cmask, 1, order)
    nonempty = (a * cmask).sum(1) > 0
    hist_q = torch.repeat_interleave(torch.arange(B, device=dev), hsz)
    hist_cnt = torch.zeros((B, num_classes), device=dev)
    hist_cnt.index_put_((hist_q, hist_aspects.to(dev).long()), torch.ones(hist_q.numel(), device=dev), accumulate=True)
    out = {}
    log_nc = float(torch.log(torch.tensor(float(num_classes))))
    for k in top_k_list:
        take = valid_sorted & (torch.arange(C, device=dev)[None, :] < k)
        cnt = torch.zeros((B, num_classes), device=dev)
        cnt.scatter_add_(1, a_sorted, take.float())
        prob = cnt / cnt.sum(1, keepdim=True).clamp_min(1.0)
        ent = -(torch.where(prob > 0, prob * torch.log(prob.clamp_min(1e-38)), torch.zeros_like(prob))).sum(1)
        div = torch.where(nonempty, ent / log_nc, torch.zeros_like(ent))
        jac = torch.minimum(cnt, hist_cnt).sum(1) / torch.maximum(cnt, hist_cnt).sum(1).clamp_min(1e-38)
        pers = torch.where(nonempty, jac, torch.zeros_like(jac))
        out[f"{prefix}_div@{k}"] = float(div.mean()) if B else 0.0
        out[f"{prefix}_pers@{k}"] = float(pers.mean()) if B else 0.0
    return out


# ---- device-side streaming form ------------------------------------------------------------------
def _offsets(sizes: torch.Tensor, device) -> torch.Tensor:
    """(B + 1) int64 prefix sums of the per-impression sizes, on the device, without a read-back."""
    sizes = sizes.to(device).long()
    off = torch.zeros(sizes.numel() + 1, dtype=torch.int64, device=device)
    torch.cumsum(sizes, 0, out=off[1:])
    return off


def impression_metrics(preds: torch.Tensor, targets: torch.Tensor, cand_news_size: torch.Tensor,
                       top_k_list: Sequence[int] = (5, 10), aspects: Optional[Dict[str, Tuple]] = None,
                       hist_news_size: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
    """Per-impression values of ``ranking_metrics`` / ``aspect_metrics`` as (B,) device tensors under the same key names (the
    reciprocal rank under "mrr"), plus "rank": the 0-based position of every candidate in its impression's stable descending
    ranking, and "status": the kernel's one-word error mask (``ops.METRICS_FLAGS``; 0 = every impression was taken), which the
    caller reads when it wants to.  ``aspects``: prefix -> (cand_aspects, hist_aspects, num_classes), at most two, with
    ``hist_news_size``.  GPU tensors only; nothing here synchronises with the host."""
    from . import ops
    aspects = aspects or {}
    dev = preds.device
    if aspects and hist_news_size is None:
        raise ValueError("impression_metrics: aspects need hist_news_size")
    rank, rows, status = ops.impression_metrics(
        preds.float(), targets.float(), _offsets(cand_news_size, dev), top_k_list,
        [(ca.to(dev).long(), ha.to(dev).long(), ncls) for ca, ha, ncls in aspects.values()],
        _offsets(hist_news_size, dev) if aspects else None)
    out = {name: rows[:, j] for j, name in enumerate(ops.metrics_columns(top_k_list, list(aspects)))}
    out["rank"], out["status"] = rank, status
    return out


def recommendation_aspect_metrics(idx: torch.Tensor, scores: torch.Tensor, row_class: torch.Tensor, hist_idx: torch.Tensor,
                                  hist_off: torch.Tensor, num_classes: int, top_k_list: Sequence[int] = (5, 10),
                                  prefix: str = "categ") -> Dict[str, float]:
    """``{prefix}_div@k`` / ``{prefix}_pers@k`` of recommendation LISTS, mean over users: what a class cap
    (``ops.topk_scores_capped``, ``NewsVectorCache.recommend_capped``) buys, in the terms of ``aspect_metrics``.  ``idx`` /
    ``scores`` (B, k): the lists as ``ops.topk_*`` return them (a slot with ``idx < 0`` is empty and left out); ``row_class``
    (V): the class of every news, in [0, num_classes); ``hist_idx`` / ``hist_off`` (B + 1): the ragged histories the
    personalization compares with.  Each user's valid slots are ONE impression of ``impression_metrics`` (candidates: the list,
    scores: its scores), so the values are those ``aspect_metrics`` gives the same lists.  GPU tensors; Python only: no kernel
    of its own.  One read of the status word and of the means at the end (``ValueError`` when the kernel refused a list)."""
    from . import ops
    dev = idx.device
    valid = idx >= 0
    rows = idx[valid]
    preds = scores.float()[valid]
    row_class, hist_off = row_class.to(dev).long(), hist_off.to(dev).long()
    out = impression_metrics(preds, torch.zeros_like(preds), valid.sum(1), top_k_list,
                             {prefix: (row_class[rows], row_class[hist_idx.to(dev).long()], int(num_classes))},
                             hist_off[1:] - hist_off[:-1])
    flags = int(out["status"])
    if flags:
        raise ValueError("recommendation_aspect_metrics: the metrics kernel refused input: " +
                         "; ".join(msg for bit, msg in ops.METRICS_FLAGS.items() if flags & bit))
    keys = [f"{prefix}_{m}@{k}" for k in top_k_list for m in ("div", "pers")]
    B = int(idx.shape[0])
    return {key: float(out[key].double().mean()) if B else 0.0 for key in keys}


def intra_list_similarity(idx: torch.Tensor, table: torch.Tensor) -> float:
    """The intra-list similarity of recommendation LISTS: per user the mean cosine over the pairs of distinct valid slots of its
    list (``idx`` (B, k): rows of ``table`` (V, D); a slot with ``idx < 0`` is empty and left out; a zero vector has cosine 0 with
    everything), then the mean over the users with at least two valid slots (0.0 when there is none).  Lower is more diverse: it
    is what ``ops.mmr_rerank`` buys, as ``recommendation_aspect_metrics`` shows what a class cap buys.  Torch ops on the
    tensors' device (a (B, k, D) gather and a (B, k, k) product); a metric, not a hot path; one read at the end."""
    valid = idx >= 0
    rows = table.float()[idx.clamp(min=0).long()]                               # (B, k, D)
    norm = rows.norm(dim=2, keepdim=True)
    unit = torch.where(norm > 0, rows / norm.clamp(min=torch.finfo(torch.float32).tiny), torch.zeros_like(rows))
    unit = unit * valid.unsqueeze(2)
    n = valid.sum(1).double()
    gram = torch.bmm(unit, unit.transpose(1, 2)).double()
    off_diagonal = gram.sum((1, 2)) - torch.diagonal(gram, dim1=1, dim2=2).sum(1)
    users = n >= 2
    if not bool(users.any()):
        return 0.0
    return float((off_diagonal[users] / (n[users] * (n[users] - 1))).mean())


class StreamingMetrics:
    """Epoch metrics without the epoch's step outputs: ``update`` takes the tuple ``model_step`` / ``*Cache.model_step`` returns
    and launches ``nrl_impression_metrics`` into a float64 accumulator (one sum per metric column, an impression count and a status
    word, all on the device); ``compute`` returns the dict of ``ranking_metrics`` + ``aspect_metrics(prefix="categ")`` +
    ``aspect_metrics(prefix="sent")``.  Only the flat ``preds`` / ``targets`` are kept, for the global AUC (a sort over all pairs).
    ``update`` performs no device-to-host transfer; ``compute`` reads the status word first and raises ``ValueError`` when the
    kernel refused an impression.  An aspect is computed when its class count was given and the step outputs carry its ids; the
    set of aspects is fixed by the first ``update``."""

    def __init__(self, top_k_list: Sequence[int] = (5, 10), num_categ_classes: Optional[int] = None,
                 num_sent_classes: Optional[int] = None):
        self.top_k_list = tuple(int(k) for k in top_k_list)
        self.num_classes = {"categ": num_categ_classes, "sent": num_sent_classes}
        self.reset()

    def reset(self) -> None:
        self.prefixes: Optional[Tuple[str, ...]] = None
        self.sums = self.count = self.status = None
        self._preds, self._targets = [], []
        self._hist_ids = 0                        # history aspect ids seen (a shape, known on the host)

    def _alloc(self, prefixes, device) -> None:
        from . import ops
        self.prefixes = tuple(prefixes)
        self.columns = ops.metrics_columns(self.top_k_list, self.prefixes)
        self.sums = torch.zeros(len(self.columns), dtype=torch.float64, device=device)
        self.count = torch.zeros(1, dtype=torch.int64, device=device)
        self.status = torch.zeros(1, dtype=torch.int32, device=device)

    def update(self, step_output: Sequence) -> None:
        from . import ops
        (_, preds, targets, cand_news_size, hist_news_size, target_categories, target_sentiments, hist_categories,
         hist_sentiments, *_) = step_output
        if not preds.is_cuda:
            raise RuntimeError(f"newsreclib_amd: StreamingMetrics.update needs GPU step outputs (got {preds.device}); there is no "
                               "CPU path -- metrics.ranking_metrics / aspect_metrics serve host tensors")
        dev = preds.device
        given = {"categ": (target_categories, hist_categories), "sent": (target_sentiments, hist_sentiments)}
        prefixes = tuple(p for p in ("categ", "sent") if self.num_classes[p] and given[p][0].numel())
        if self.prefixes is None:
            self._alloc(prefixes, dev)
        elif prefixes != self.prefixes:
            raise ValueError(f"StreamingMetrics.update: this step carries the aspects {prefixes}, the accumulator was started with "
                             f"{self.prefixes}")
        preds, targets = preds.detach(), targets.detach()
        aspects = [(given[p][0].to(dev).long(), given[p][1].to(dev).long(), self.num_classes[p]) for p in prefixes]
        ops.impression_metrics(preds.float(), targets.float(), _offsets(cand_news_size, dev), self.top_k_list, aspects,
                               _offsets(hist_news_size, dev) if aspects else None, status=self.status, sums=self.sums,
                               count=self.count, want_rank=False, want_rows=False)
        self._preds.append(preds)
        self._targets.append(targets)
        if aspects:
            self._hist_ids += int(aspects[0][1].numel())

    def merge(self, other: "StreamingMetrics") -> "StreamingMetrics":
        """Adds another accumulator of the same configuration (say, a second evaluation stream over other impressions)."""
        if other.top_k_list != self.top_k_list or other.num_classes != self.num_classes:
            raise ValueError("StreamingMetrics.merge: the two accumulators were configured differently")
        if other.prefixes is None:
            return self
        if self.prefixes is None:
            self._alloc(other.prefixes, other.sums.device)
        elif other.prefixes != self.prefixes:
            raise ValueError(f"StreamingMetrics.merge: aspects {other.prefixes} against {self.prefixes}")
        self.sums += other.sums.to(self.sums.device)
        self.count += other.count.to(self.sums.device)
        self.status |= other.status.to(self.sums.device)
        self._preds += other._preds
        self._targets += other._targets
        self._hist_ids += other._hist_ids
        return self

    def compute(self) -> Dict[str, float]:
        from . import ops
        if self.prefixes is None:
            return {}
        flags = int(self.status)                   # the one read of the status word
        if flags:
            raise ValueError("StreamingMetrics: the metrics kernel refused input: " +
                             "; ".join(msg for bit, msg in ops.METRICS_FLAGS.items() if flags & bit))
        n = int(self.count)
        mean = (self.sums / max(n, 1)).tolist()
        vals = dict(zip(self.columns, mean))
        out = {"mrr": vals["mrr"]}
        out.update({f"ndcg@{k}": vals[f"ndcg@{k}"] for k in self.top_k_list})
        out["auc"] = _global_auc(torch.cat(self._preds), torch.cat(self._targets)) if self._preds else 0.0
        for p in self.prefixes:
            if self._hist_ids:                     # (an epoch without any history id has no aspect metrics, as the torch path)
                for k in self.top_k_list:
                    out[f"{p}_div@{k}"] = vals[f"{p}_div@{k}"]
                    out[f"{p}_pers@{k}"] = vals[f"{p}_pers@{k}"]
        return out


class GridStreamingMetrics:
    """``StreamingMetrics`` for a grid of ensemble weights: G weight rows over T score components are ranked and scored in ONE
    ``nrl_grid_metrics`` launch per batch, into a (G, columns) float64 accumulator.  ``update(comp, step_output)`` takes the
    batch's (T, N) components (``MannerVectorCache.zscores``) and the tuple ``model_step`` returns (its ``preds`` slot is not
    read: every row of the grid has its own); ``compute()`` returns ``{"weights": (G, T) list, "columns": [...], "values":
    (G, columns) float64 list}`` with ``values = sums / count``, row g being to the bit what a ``StreamingMetrics`` fed row g's
    scores accumulates.  The weights are checked on the host once, here (``ops.grid_weights``).  ``update`` performs no
    device-to-host transfer; ``compute`` reads the status word first and raises ``ValueError`` when the kernel refused an
    impression.  There is no AUC: the global AUC is a sort over every (score, target) pair of the epoch PER ROW, so it needs all G
    flat score vectors kept -- G x 2.7 M floats on a MIND-small-dev epoch, 4.8 GB at G = 441; evaluate the rows that matter with
    ``evaluate_impressions`` for it."""

    def __init__(self, weights, top_k_list: Sequence[int] = (5, 10), num_categ_classes: Optional[int] = None,
                 num_sent_classes: Optional[int] = None):
        from . import ops
        self.weights = ops.grid_weights(weights)
        self.top_k_list = tuple(int(k) for k in top_k_list)
        self.num_classes = {"categ": num_categ_classes, "sent": num_sent_classes}
        self.reset()

    def reset(self) -> None:
        self.prefixes: Optional[Tuple[str, ...]] = None
        self.sums = self.count = self.status = self._dev_weights = None

    def _alloc(self, prefixes, device) -> None:
        from . import ops
        self.prefixes = tuple(prefixes)
        self.columns = ops.metrics_columns(self.top_k_list, self.prefixes)
        self.sums = torch.zeros((self.weights.shape[0], len(self.columns)), dtype=torch.float64, device=device)
        self.count = torch.zeros(1, dtype=torch.int64, device=device)
        self.status = torch.zeros(1, dtype=torch.int32, device=device)
        self._dev_weights = self.weights.pin_memory().to(device, non_blocking=True)      # (a pageable copy would synchronise)

    def update(self, comp: torch.Tensor, step_output: Sequence) -> None:
        from . import ops
        (_, _, targets, cand_news_size, hist_news_size, target_categories, target_sentiments, hist_categories,
         hist_sentiments, *_) = step_output
        if not comp.is_cuda:
            raise RuntimeError(f"newsreclib_amd: GridStreamingMetrics.update needs GPU components (got {comp.device}); there is no "
                               "CPU path")
        if comp.dim() != 2 or comp.shape[0] != self.weights.shape[1]:
            raise ValueError(f"GridStreamingMetrics.update: the weight rows have {self.weights.shape[1]} entries, the batch "
                             f"carries components of shape {tuple(comp.shape)}")
        dev = comp.device
        given = {"categ": (target_categories, hist_categories), "sent": (target_sentiments, hist_sentiments)}
        prefixes = tuple(p for p in ("categ", "sent") if self.num_classes[p] and given[p][0].numel())
        if self.prefixes is None:
            self._alloc(prefixes, dev)
        elif prefixes != self.prefixes:
            raise ValueError(f"GridStreamingMetrics.update: this step carries the aspects {prefixes}, the accumulator was started "
                             f"with {self.prefixes}")
        aspects = [(given[p][0].to(dev).long(), given[p][1].to(dev).long(), self.num_classes[p]) for p in prefixes]
        ops.grid_metrics(comp.detach().float(), self._dev_weights, targets.detach().to(dev).float(), _offsets(cand_news_size, dev),
                         self.top_k_list, aspects, _offsets(hist_news_size, dev) if aspects else None, status=self.status,
                         sums=self.sums, count=self.count)

    def merge(self, other: "GridStreamingMetrics") -> "GridStreamingMetrics":
        """Adds another accumulator of the same grid and configuration (a second evaluation stream over other impressions)."""
        if (other.top_k_list != self.top_k_list or other.num_classes != self.num_classes
                or not torch.equal(other.weights, self.weights)):
            raise ValueError("GridStreamingMetrics.merge: the two accumulators were configured differently")
        if other.prefixes is None:
            return self
        if self.prefixes is None:
            self._alloc(other.prefixes, other.sums.device)
        elif other.prefixes != self.prefixes:
            raise ValueError(f"GridStreamingMetrics.merge: aspects {other.prefixes} against {self.prefixes}")
        self.sums += other.sums.to(self.sums.device)
        self.count += other.count.to(self.sums.device)
        self.status |= other.status.to(self.sums.device)
        return self

    def compute(self) -> Dict:
        from . import ops
        if self.prefixes is None:
            return {}
        flags = int(self.status)                   # the one read of the status word
        if flags:
            raise ValueError("GridStreamingMetrics: the metrics kernel refused input: " +
                             "; ".join(msg for bit, msg in ops.METRICS_FLAGS.items() if flags & bit))
        n = int(self.count)
        return {"weights": self.weights.tolist(), "columns": list(self.columns), "values": (self.sums / max(n, 1)).tolist()}


def snips_value(reward, logp_target, logp_logging, clip: Optional[float] = None) -> Tuple[float, float]:
    """Self-normalised importance sampling (SNIPS) over logged lists -> (value, effective sample size), on the host in float64.
    ``reward`` (n): the reward each logged list earned; ``logp_target`` / ``logp_logging`` (n): the list's log-probability under
    the policy being evaluated and under the policy that drew it (``list_log_probs``' totals, or the sum of
    ``sample_recommendations(log_probs=True)``'s slots).  The weights are ``w = exp(logp_target - logp_logging)``, computed after
    subtracting the largest log-ratio (self-normalisation cancels the shift, and no weight overflows); ``clip`` caps ``w``, in
    its own units, before it is normalised.  ``value = sum w r / sum w``; ``effective sample size = (sum w)^2 / sum w^2``, between
    1 and n.  No lists: ``(nan, 0.0)``.  ``ValueError`` for lengths that differ, a non-finite log-probability or ``clip <= 0``."""
    r = torch.as_tensor(reward, dtype=torch.float64).reshape(-1).cpu()
    lt = torch.as_tensor(logp_target, dtype=torch.float64).reshape(-1).cpu()
    ll = torch.as_tensor(logp_logging, dtype=torch.float64).reshape(-1).cpu()
    if not (r.numel() == lt.numel() == ll.numel()):
        raise ValueError(f"snips_value: one reward and two log-probabilities per list, got {r.numel()}, {lt.numel()} and {ll.numel()}")
    if clip is not None and not float(clip) > 0:
        raise ValueError(f"snips_value: clip > 0, got {clip!r}")
    if r.numel() == 0:
        return float("nan"), 0.0
    if not bool(torch.isfinite(lt).all() and torch.isfinite(ll).all()):
        raise ValueError("snips_value: a log-probability is not finite (an invalid list, or one the logging policy could not draw)")
    ratio = lt - ll
    shift = ratio.max()
    w = torch.exp(ratio - shift)
    if clip is not None:
        w = torch.minimum(w, torch.exp(torch.log(torch.tensor(float(clip), dtype=torch.float64)) - shift))
    total = w.sum()
    return float((w * r).sum() / total), float(total * total / (w * w).sum())
