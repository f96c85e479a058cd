"""Synthetic MIND-shaped ``RecommendationBatch`` generator.

Reproduces the *layout* of the reference's collated batch (``data/components/batch.py:6-32``,
``rec_dataset.py:148-168,289-293``): ragged, concatenated news rows plus sorted assignment vectors.
There is no network, so MIND itself is unavailable; shapes and distributions follow the reference
configs (``configs/data/mind_rec.yaml:55-58``: title 30 tokens, history <= 50, 4 negatives per
positive).
"""
from __future__ import annotations

from typing import Dict

import numpy as np
import torch


def _zipf_ids(rng: np.random.Generator, n: int, vocab: int, a: float = 1.1) -> np.ndarray:
    """n token ids in [1, vocab) with P(k) ~ k**-a (bounded Zipf; id 0 is the pad token)."""
    ranks = np.arange(1, vocab, dtype=np.float64)
    cdf = np.cumsum(ranks ** (-a))
    cdf /= cdf[-1]
    return (np.searchsorted(cdf, rng.random(n), side="left") + 1).astype(np.int64)


def _titles(rng: np.random.Generator, n_news: int, vocab: int, L: int) -> np.ndarray:
    """(n_news, L) int64: ``len ~ clip(round(N(11.5, 3.5)), 3, L)`` real tokens, then 0-padding
    (right padding as ``rec_dataset.py:170-178``)."""
    lens = np.clip(np.rint(rng.normal(11.5, 3.5, n_news)), 3, L).astype(np.int64)
    ids = _zipf_ids(rng, n_news * L, vocab).reshape(n_news, L)
    ids[np.arange(L)[None, :] >= lens[:, None]] = 0
    return ids


def make_batch(batch_size: int, vocab: int = 70_000, mode: str = "fixed", seed: int = 1234,
               L: int = 30, H: int = 50, neg_ratio: int = 4, device="cpu") -> Dict:
    """One synthetic training batch.

    mode="fixed":  every user has H clicks and (1 + neg_ratio) candidates, one positive at a
                   random slot (the headline shape the FLOP/byte math in DESIGN.md uses).
    mode="ragged": hist_i ~ clip(round(lognormal(3.0, 0.8)), 1, H); npos_i ~ 1 + Poisson(0.35);
                   C_i = (1 + neg_ratio) * npos_i with shuffled labels (``rec_dataset.py:60-95``).
    """
    rng = np.random.default_rng(seed)
    B = batch_size
    if mode == "fixed":
        hist_sizes = np.full(B, H, dtype=np.int64)
        npos = np.ones(B, dtype=np.int64)
    elif mode == "ragged":
        hist_sizes = np.clip(np.rint(rng.lognormal(3.0, 0.8, B)), 1, H).astype(np.int64)
        npos = 1 + rng.poisson(0.35, B).astype(np.int64)
    else:
        raise ValueError(f"unknown mode {mode!r}")
    cand_sizes = npos * (1 + neg_ratio)
    labels = []
    for b in range(B):
        lab = np.zeros(cand_sizes[b], dtype=np.float32)
        lab[: npos[b]] = 1.0
        rng.shuffle(lab)
        labels.append(lab)
    n_hist, n_cand = int(hist_sizes.sum()), int(cand_sizes.sum())
    batch = {
        "batch_hist": np.repeat(np.arange(B, dtype=np.int64), hist_sizes),
        "batch_cand": np.repeat(np.arange(B, dtype=np.int64), cand_sizes),
        "x_hist": {"title": _titles(rng, n_hist, vocab, L)},
        "x_cand": {"title": _titles(rng, n_cand, vocab, L)},
        "labels": np.concatenate(labels),
        "user_ids": np.arange(B, dtype=np.int64) + 1,
        "user_idx": np.arange(B, dtype=np.int64),
    }
    return batch_to_torch(batch, B, device)


def batch_to_torch(batch: Dict, batch_size: int, device="cpu") -> Dict:
    def cv(a):
        return torch.as_tensor(a).to(device)

    out = {}
    for k, v in batch.items():
        out[k] = {kk: cv(vv) for kk, vv in v.items()} if isinstance(v, dict) else cv(v)
    out["batch_size"] = int(batch_size)
    return out


def batch_from_sizes(hist_sizes, cand_sizes, labels, vocab: int, seed: int, L: int = 30) -> Dict:
    """Explicit ragged batch (used for the hand-made golden cases)."""
    rng = np.random.default_rng(seed)
    hist_sizes = np.asarray(hist_sizes, dtype=np.int64)
    cand_sizes = np.asarray(cand_sizes, dtype=np.int64)
    B = len(hist_sizes)
    batch = {
        "batch_hist": np.repeat(np.arange(B, dtype=np.int64), hist_sizes),
        "batch_cand": np.repeat(np.arange(B, dtype=np.int64), cand_sizes),
        "x_hist": {"title": _titles(rng, int(hist_sizes.sum()), vocab, L)},
        "x_cand": {"title": _titles(rng, int(cand_sizes.sum()), vocab, L)},
        "labels": np.asarray(labels, dtype=np.float32),
        "user_ids": np.arange(B, dtype=np.int64) + 1,
        "user_idx": np.arange(B, dtype=np.int64),
    }
    return batch_to_torch(batch, B)


def add_lstur_fields(batch: Dict, vocab: int, n_categ: int = 19, n_users: int = 1000, L_abstract: int = 50,
                     seed: int = 4321) -> Dict:
    """Adds what ``LSTURModule.forward`` reads on top of the NRMS batch (``lstur_module.py:278-303``):
    abstract token ids and category ids per news row (``rec_dataset.py:148-168``), and ``user_idx``
    drawn from [0, n_users) -- 0 is the reference's "unknown user" / padding row."""
    rng = np.random.default_rng(seed)
    dev = batch["labels"].device
    for part in ("x_hist", "x_cand"):
        n = batch[part]["title"].shape[0]
        lens = np.clip(np.rint(rng.normal(32.0, 12.0, n)), 5, L_abstract).astype(np.int64)
        ids = _zipf_ids(rng, n * L_abstract, vocab).reshape(n, L_abstract)
        ids[np.arange(L_abstract)[None, :] >= lens[:, None]] = 0
        batch[part]["abstract"] = torch.as_tensor(ids).to(dev)
        batch[part]["category"] = torch.as_tensor(rng.integers(1, n_categ, n)).to(dev)
    B = batch["batch_size"]
    uidx = rng.integers(1, n_users, B)
    uidx[rng.random(B) < 0.15] = 0
    batch["user_idx"] = torch.as_tensor(uidx).to(dev)
    return batch


def add_dkn_fields(batch: Dict, n_entities: int = 30_000, seed: int = 7, max_per_title: int = 3) -> Dict:
    """DKN inputs (dkn_module.py, news.py:262-266): ``title_entities`` (n_news, L) beside every ``title``, as
    ``input_pipeline`` pads them.  Each title carries 0..max_per_title linked entities in its leading real-token slots
    (uniform over [1, n_entities)), the rest 0 -- the padding / no-entity id.  n_entities = 30,000 stands for the order of
    magnitude of MIND's small entity vocabulary (no dataset is on hand to count it exactly)."""
    rng = np.random.default_rng(seed)
    out = dict(batch)
    for side in ("x_hist", "x_cand"):
        title = batch[side]["title"]
        ids = title.cpu().numpy() if torch.is_tensor(title) else np.asarray(title)
        n, L = ids.shape
        real = (ids != 0).sum(axis=1)
        k = np.minimum(rng.integers(0, max_per_title + 1, n), real)
        ents = rng.integers(1, n_entities, size=(n, L)).astype(np.int64)
        ents[np.arange(L)[None, :] >= k[:, None]] = 0
        t = torch.from_numpy(ents)
        out[side] = dict(batch[side])
        out[side]["title_entities"] = t.to(title.device) if torch.is_tensor(title) else t
    return out


def add_plm_fields(batch: Dict, vocab_size: int = 50265, pad_id: int = 1, seed: int = 11, L: int = 30) -> Dict:
    """PLM-style ``title`` inputs (``rec_dataset.py:180-190``: the tokenizer's ``input_ids`` / ``attention_mask`` dict) on both
    sides of a batch whose ``title`` is a plain id tensor (or absent); a ``title`` that already is a dict is kept.  Every news
    gets 3..L real tokens (ids uniform over [3, vocab_size): 0-2 are roberta's special tokens), the rest ``pad_id`` under
    mask 0."""
    rng = np.random.default_rng(seed)
    out = dict(batch)
    for side, key in (("x_hist", "batch_hist"), ("x_cand", "batch_cand")):
        if isinstance(batch[side].get("title"), dict):
            continue
        n, dev = int(batch[key].shape[0]), batch[key].device
        ids = rng.integers(3, vocab_size, (n, L))
        lens = rng.integers(3, L + 1, n)
        m = (np.arange(L)[None, :] < lens[:, None]).astype(np.int64)
        out[side] = dict(batch[side])
        out[side]["title"] = {"input_ids": torch.from_numpy(np.where(m == 1, ids, pad_id)).to(dev),
                              "attention_mask": torch.from_numpy(m).to(dev)}
    return out


def make_news_batch(n_classes: int, samples_per_class: int, vocab_size: int = 50265, n_entities: int = 30_000, L: int = 96,
                    L_entities: int = 10, pad_id: int = 1, seed: int = 21, use_entities: bool = True) -> Dict:
    """A ``NewsBatch`` as the A-Module reads it (manner_a_module.py:159-176): ``news["text"]`` = the tokenised concatenation of title
    and abstract (``input_ids`` / ``attention_mask``, 3..L real tokens per news), ``news["entities"]`` = the concatenated title +
    abstract entity ids (0 = none), and int64 aspect ``labels`` with ``samples_per_class`` news of each of ``n_classes`` classes in
    shuffled order (the reference's MPerClassSampler batch: 17 x 5 = 85 at the configured shape)."""
    rng = np.random.default_rng(seed)
    n = int(n_classes) * int(samples_per_class)
    ids = rng.integers(3, vocab_size, (n, L))
    lens = rng.integers(3, L + 1, n)
    m = (np.arange(L)[None, :] < lens[:, None]).astype(np.int64)
    news = {"text": {"input_ids": torch.from_numpy(np.where(m == 1, ids, pad_id)), "attention_mask": torch.from_numpy(m)}}
    if use_entities:
        k = rng.integers(0, L_entities + 1, n)
        ents = rng.integers(1, n_entities, (n, L_entities)).astype(np.int64)
        ents[np.arange(L_entities)[None, :] >= k[:, None]] = 0
        news["entities"] = torch.from_numpy(ents)
    labels = np.repeat(np.arange(n_classes, dtype=np.int64), samples_per_class)
    return {"news": news, "labels": torch.from_numpy(rng.permutation(labels))}


def news_times(n_news: int, span: int = 28 * 24, seed: int = 31) -> torch.Tensor:
    """A non-decreasing int64 ``time`` column for a table of ``n_news`` news: publication times uniform over ``[0, span)`` (the
    default unit: hours over 28 days), sorted, as a news table that grows by appending is stored (the behaviours' ``time`` column,
    ``mind_dataframe.py:528-581``, is what a split goes by)."""
    rng = np.random.default_rng(seed)
    return torch.from_numpy(np.sort(rng.integers(0, max(int(span), 1), int(n_news))).astype(np.int64))


def add_request_times(users, span: int = 28 * 24, last: int = 7 * 24, seed: int = 37):
    """The user dictionaries of ``recommend_users`` / ``evaluate_full_rank`` with a ``"time"`` each: a request time drawn from the
    last ``last`` units of ``[0, span)`` (in the unit of ``news_times``) -> a new list; the dictionaries are copied."""
    rng = np.random.default_rng(seed)
    t = rng.integers(max(int(span) - int(last), 0), max(int(span), 1), len(users))
    return [{**u, "time": int(t[j])} for j, u in enumerate(users)]
