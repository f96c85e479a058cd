"""What a collated batch needs before any recommender's forward: the ragged-layout metadata (``attach_layout``) and the per-step
device work on the token ids (``prepare_batch``).  ``nrms_module`` re-exports the three names."""
from __future__ import annotations

import os
from typing import Dict, Optional

import torch

from . import ops
from .dense_batch import dense_slot_index


def attach_layout(batch: Dict) -> Dict:
    """Attach the ragged-layout metadata the forward needs (offsets, max lengths, batch size).

    A collate function has these on the host for free (it builds ``batch_hist`` from the per-user
    list lengths, rec_dataset.py:289-293; ``input_pipeline.build_batch`` supplies them); computing
    them from the device vectors costs two syncs, so a loader does it once per batch, outside the step."""
    if "cand_flat_idx" in batch:
        return batch
    B = int(batch["batch_size"]) if "batch_size" in batch else (
        int(batch["user_idx"].shape[0]) if "user_idx" in batch else int(batch["batch_hist"].max()) + 1)
    out = dict(batch)
    out["batch_size"] = B
    for key in ("hist", "cand"):
        if key + "_offsets" in batch:       # a loader that knows the row lengths on the host supplies these
            continue                        # (input_pipeline.build_batch): no device read-back at all
        off = ops.offsets_from_sorted_batch(batch["batch_" + key], B)
        out[key + "_offsets"] = off
        sizes = off[1:] - off[:-1]
        out["max_" + key] = int(sizes.max())
        out[key + "_sizes"] = sizes
    if "min_hist" not in out:
        out["min_hist"] = int(out["hist_sizes"].min())
    out["cand_flat_idx"] = dense_slot_index(batch["batch_cand"], out["cand_offsets"], out["max_cand"])
    return out


def text_vocab(module) -> Optional[int]:
    """Rows of the word-embedding table the module's text encoders share (None: no embedding table, e.g. a PLM): the
    exclusive upper bound of the token ids, which lets ``prepare_batch`` group them with the counting sort."""
    enc = getattr(module, "news_encoder", None)
    for te in getattr(enc, "text_encoders", {}).values() if enc is not None else ():
        emb = getattr(te, "embedding_layer", None)
        if emb is not None:
            return int(emb.weight.shape[0])
    return None


def prepare_batch(batch: Dict, vocab: Optional[int] = None, need_order: Optional[bool] = None) -> Dict:
    """``attach_layout`` + the per-step device work on the token ids: history and candidate ids as the single
    encoder call sees them, and their id-sorted visiting order for the embedding gradient (the sort the reference
    pays inside ``embedding_dense_backward``).  No host sync; part of the train step (bench.py times it).
    ``need_order`` (default: whether gradients are enabled): the visiting order serves the backward only, so a forward
    under ``torch.no_grad()`` does not sort."""
    if need_order is None:
        need_order = torch.is_grad_enabled()
    out = attach_layout(batch)
    if "x_all" in out:
        return out
    out = dict(out)
    for attr in ("title", "abstract"):
        if attr in batch["x_hist"] and attr in batch["x_cand"]:
            h, c = batch["x_hist"][attr], batch["x_cand"][attr]
            if torch.is_tensor(h):
                ids = torch.cat([h, c], dim=0)
                out.setdefault("x_all", {})[attr] = ids
                # counting sort over the vocabulary on a side stream: the order is needed by the backward only, so its four
                # small launches (~50 us at B = 128) run beside the fused forward instead of in front of it.  Measured slower
                # mid-round (3.30 vs 3.26 ms: the sort was 80 us of atomics then); with the current sort, two alternating pairs
                # of 100 steps: 2.98 / 3.00 vs 3.03 / 3.02 ms.  NRL_SORT_ASYNC=0 keeps it on the launch stream.
                # NRL_SORT_ASYNC=2: not here at all -- the news encoder's forward issues it on the side stream AFTER its own launches,
                # so it runs beside the user encoder's few-row launches instead of beside the fused forward
                mode = os.environ.get("NRL_SORT_ASYNC", "1")
                if mode != "2" and need_order:
                    sort = ops.sort_positions_async if mode == "1" else ops.sort_positions
                    out["x_all"][attr + "_order"] = sort(ids, vocab)
            # (PLM tokenizer output -- a dict of (N, L) tensors, rec_dataset.py:180-190 -- is NOT merged: the
            #  two sides are padded to their own longest text and the PLM encoder must see them in separate calls)
    for attr in ("category", "subcategory"):
        if attr in batch["x_hist"] and attr in batch["x_cand"]:
            out.setdefault("x_all", {})[attr] = torch.cat([batch["x_hist"][attr], batch["x_cand"][attr]], dim=0)
    return out
