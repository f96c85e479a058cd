#!/usr/bin/env python3
"""Generate tests/golden/manner_*.npz and manner_contract.json by running the REFERENCE's own components (same rules as
make_golden_miner.py).  Imported at generation time only: ``PLM``, ``MHSAAddAtt`` (text.py), ``NewsEncoder`` (news.py), the NRMS
``UserEncoder`` and ``DotProduct``.  RESTATED, not imported (tests/manner_oracle.py): the wiring of ``CRModule`` / ``AModule`` /
``MANNERModule`` (the modules need lightning / torch_geometric / plotting libraries), ``to_dense_batch`` (loops) and
pytorch-metric-learning's SupCon (not installed: the score-matrix form of oracle/losses_oracle.py, the labels form of
manner_oracle.supcon_embed).  The entity encoder's ``nn.Dropout`` is replaced by an injector that hands out the library's
counter-based masks in call order (history call: streams 6, 7; candidate call: 10, 11).  The body is tests/manner_oracle.make_body.

Seeds are picked first-hit counting up from 1 under conditions only the reference's numbers enter: every SupCon row loss is
exactly 0 or >= 1e-3 (the reducer's `> 0` cannot flip within tolerance); every multi-candidate impression of the ensemble has
std >= 1e-2 max|score| in every sub-model.  Only data and name lists are written.

Usage:  python tests/golden/make_golden_manner.py   (from the repo root)
"""
import ast
import importlib.util
import json
import os
import sys
import tempfile

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REF = "/root/reference"
sys.path.insert(0, REPO)
from tests import manner_oracle as MO  # noqa: E402

sys.path.insert(0, REF)
from newsreclib.models.components.encoders.news.news import NewsEncoder  # noqa: E402
from newsreclib.models.components.encoders.news.text import PLM, MHSAAddAtt  # noqa: E402
from newsreclib.models.components.encoders.user.nrms import UserEncoder  # noqa: E402
from newsreclib.models.components.layers.click_predictor import DotProduct  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
MAX_BYTES = 654 * 1024
CFG = MO.TINY
ATTRS = ["title", "abstract", "title_entities", "abstract_entities"]


class Injected(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.mults, self.k = [], 0

    def arm(self, mults):
        self.mults, self.k = list(mults), 0

    def forward(self, x):
        if not self.mults:
            return x
        m = self.mults[self.k]
        self.k += 1
        assert m.shape == x.shape, (m.shape, x.shape)
        return x * m


class RefModel(torch.nn.Module):
    """The components of CRModule (manner_cr_module.py:113-173) / AModule (manner_a_module.py:88-137) with seeded parameters."""

    def __init__(self, plm_path, param_seed, use_entities=True, user_encoder=False, p=0.2):
        super().__init__()
        T, De, H, Q = CFG["T"], CFG["De"], CFG["H"], CFG["Q"]
        params = MO.make_manner_params(param_seed, use_entities, user_encoder)
        text = PLM(plm_model=plm_path, frozen_layers=list(CFG["frozen"]), embed_dim=T, use_mhsa=False, apply_reduce_dim=False,
                   reduced_embed_dim=None, num_heads=H, query_dim=Q, dropout_probability=p)
        self.inj = Injected()
        ent = None
        if use_entities:
            ent = MHSAAddAtt(pretrained_embeddings=params[MO.ENT + "embedding_layer.weight"].clone(), embed_dim=De, num_heads=H,
                             query_dim=Q, dropout_probability=p)
            ent.dropout = self.inj
        self.news_encoder = NewsEncoder(dataset_attributes=ATTRS, attributes2encode=ATTRS if use_entities else ATTRS[:2],
                                        concatenate_inputs=True, text_encoder=text, category_encoder=None, entity_encoder=ent,
                                        combine_vectors=True, combine_type="linear", input_dim=T + De if use_entities else T,
                                        query_dim=None, output_dim=T)
        if user_encoder:
            self.user_encoder = UserEncoder(news_embed_dim=T, num_heads=H, query_dim=Q)
        self.click_predictor = DotProduct()
        self.use_entities = use_entities
        res = self.load_state_dict(params, strict=False)
        assert not res.unexpected_keys and all(".plm_model." in k for k in res.missing_keys), res

    def arm(self, calls, p, seed):
        """calls: [(rows, entity length, stream_base)] in call order."""
        seq = []
        if p > 0.0 and self.use_entities:
            for n, L, base in calls:
                seq += MO.entity_masks(seed, p, n, L, CFG["De"], base)
        self.inj.arm(seq)


def toks(rng, n, L):
    ids = rng.integers(3, 200, (n, L))
    lens = rng.integers(3, L + 1, n)
    m = (np.arange(L)[None, :] < lens[:, None]).astype(np.int64)
    return {"input_ids": torch.from_numpy(np.where(m == 1, ids, 1)), "attention_mask": torch.from_numpy(m)}


def news(rng, n, L, Le):
    k = rng.integers(1, Le + 1, n)                       # (at least one entity: an all-padding row is not a case of these fixtures)
    ents = rng.integers(1, CFG["n_ent"], (n, Le)).astype(np.int64)
    ents[np.arange(Le)[None, :] >= k[:, None]] = 0
    return {"text": toks(rng, n, L), "entities": torch.from_numpy(ents)}


def rec_batch(seed, hist_sizes, cand_sizes):
    rng = np.random.default_rng(seed)
    nh, nc, B = sum(hist_sizes), sum(cand_sizes), len(hist_sizes)
    labels = torch.zeros(nc)
    start = 0
    for c in cand_sizes:
        labels[start + int(rng.integers(0, c))] = 1.0
        start += c
    return {"x_hist": news(rng, nh, 9, 5), "x_cand": news(rng, nc, 11, 4),
            "batch_hist": torch.repeat_interleave(torch.arange(B), torch.tensor(hist_sizes)),
            "batch_cand": torch.repeat_interleave(torch.arange(B), torch.tensor(cand_sizes)),
            "labels": labels, "batch_size": B}


def store_news(arrays, tag, nd):
    for k, v in nd["text"].items():
        arrays[f"in_{tag}_text_{k}"] = v.numpy()
    arrays[f"in_{tag}_entities"] = nd["entities"].numpy()


def store_grads(arrays, model):
    for k, prm in model.named_parameters():
        g = prm.grad if prm.grad is not None else torch.zeros_like(prm)
        arrays["gnorm/" + k] = np.float64(g.detach().reshape(-1).double().norm())
        if k.endswith("embedding_layer.weight"):          # (padding_idx = 0: helpers.check_grads_against_golden checks row 0)
            arrays["gfull/" + k] = g.detach().numpy()
        else:
            arrays["gsample/" + k] = g.detach().reshape(-1)[::MO.SAMPLE_STRIDE].numpy().copy()


def save(name, arrays):
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **arrays)
    size = os.path.getsize(path)
    assert size <= MAX_BYTES, (name, size)
    return size


def rows_ok(rows):
    return rows is None or bool(((rows == 0) | (rows >= 1e-3)).all())


def run_cr(name, plm, loss, late_fusion, p, seed, batch_seed=5):
    batch = rec_batch(batch_seed, [2, 5, 1, 4], [5, 4, 3, 5])
    nh, nc = batch["batch_hist"].shape[0], batch["batch_cand"].shape[0]
    for param_seed in range(1, 50):
        model = RefModel(plm, param_seed, True, not late_fusion)
        model.train(p > 0.0)
        model.arm([(nh, 5, 0), (nc, 4, MO.CAND_STREAM_BASE)], p, seed)
        scores, hist_vec, cand_vec, mask_cand = MO.cr_forward(model.news_encoder, getattr(model, "user_encoder", None),
                                                              model.click_predictor, batch)
        assert model.inj.k == len(model.inj.mults)
        loss_v, y_true = MO.cr_loss(scores, batch, mask_cand, loss)
        if loss == "cross_entropy_loss" or rows_ok(MO.score_supcon_rows(scores.detach().double(), y_true.double(), mask_cand)):
            break
    else:
        raise AssertionError("no parameter seed satisfies the row-loss condition")
    loss_v.backward()
    arrays = {"in_batch_hist": batch["batch_hist"].numpy(), "in_batch_cand": batch["batch_cand"].numpy(),
              "in_labels": batch["labels"].numpy(), "in_batch_size": np.int64(batch["batch_size"]),
              "cfg_param_seed": np.int64(param_seed), "cfg_p_drop": np.float64(p), "cfg_seed": np.int64(seed),
              "cfg_sample_stride": np.int64(MO.SAMPLE_STRIDE), "cfg_late_fusion": np.int64(late_fusion),
              "cfg_sup_con": np.int64(loss == "sup_con_loss")}
    store_news(arrays, "hist", batch["x_hist"])
    store_news(arrays, "cand", batch["x_cand"])
    for k, v in (("scores", scores), ("loss", loss_v), ("hist_vec", hist_vec), ("cand_vec", cand_vec)):
        arrays["out_" + k] = v.detach().numpy()
    store_grads(arrays, model)
    print(f"{name}: param seed {param_seed} loss={float(loss_v.detach()):.6f} max|score|={float(scores.detach().abs().max()):.3f} "
          f"-> {save(name, arrays) / 1024:.1f} KiB")


def run_a(name, plm, labels, temperature=0.9, p=0.2, seed=3, batch_seed=8, expect_zero=False):
    labels = torch.tensor(labels)
    n = labels.shape[0]
    nd = news(np.random.default_rng(batch_seed), n, 10, 4)
    for param_seed in range(1, 50):
        model = RefModel(plm, param_seed, True, False)
        model.train()
        model.arm([(n, 4, 0)], p, seed)
        emb = model.news_encoder(nd)
        assert model.inj.k == len(model.inj.mults)
        if rows_ok(MO.supcon_rows(emb.detach().double(), labels, temperature)):
            break
    else:
        raise AssertionError("no parameter seed satisfies the row-loss condition")
    loss = MO.supcon_embed(emb, labels, temperature)
    loss.backward()
    if expect_zero:
        assert float(loss.detach()) == 0.0 and all(p.grad is None or float(p.grad.abs().max()) == 0.0 for p in model.parameters())
    arrays = {"in_labels": labels.numpy(), "cfg_param_seed": np.int64(param_seed), "cfg_p_drop": np.float64(p),
              "cfg_seed": np.int64(seed), "cfg_sample_stride": np.int64(MO.SAMPLE_STRIDE),
              "cfg_temperature": np.float64(temperature), "out_embeddings": emb.detach().numpy(), "out_loss": loss.detach().numpy()}
    rows = MO.supcon_rows(emb.detach().double(), labels, temperature)
    arrays["out_rows"] = (rows if rows is not None else torch.zeros(n, dtype=torch.float64)).numpy()
    store_news(arrays, "news", nd)
    store_grads(arrays, model)
    print(f"{name}: param seed {param_seed} loss={float(loss.detach()):.6f} -> {save(name, arrays) / 1024:.1f} KiB")


def run_ens(name, plm, batch_seed=12):
    batch = rec_batch(batch_seed, [3, 1, 4, 2, 5], [4, 1, 6, 2, 5])          # impression 1: ONE candidate, a NaN row
    for base in range(1, 50):
        seeds = [base, base + 100, base + 200]
        models = [RefModel(plm, s, True, False).eval() for s in seeds]
        with torch.no_grad():
            subs = [MO.submodel_forward(m.news_encoder, m.click_predictor, batch) for m in models]
        ok = True
        for z, raw, mask in subs:
            for b in range(batch["batch_size"]):
                s = raw[b][mask[b]].double()
                if len(s) > 1 and float(torch.std(s)) < 1e-2 * float(s.abs().max()):
                    ok = False
        if ok:
            break
    else:
        raise AssertionError("no parameter seeds satisfy the std condition")
    arrays = {"in_batch_hist": batch["batch_hist"].numpy(), "in_batch_cand": batch["batch_cand"].numpy(),
              "in_labels": batch["labels"].numpy(), "in_batch_size": np.int64(batch["batch_size"]),
              "cfg_param_seeds": np.asarray(seeds, dtype=np.int64), "cfg_weights": np.asarray(MO.ENS_WEIGHTS, dtype=np.float64)}
    store_news(arrays, "hist", batch["x_hist"])
    store_news(arrays, "cand", batch["x_cand"])
    for i, (cw, sw) in enumerate(MO.ENS_WEIGHTS):          # manner_module.py:190-204
        scores = subs[0][0].clone()
        if cw != 0:
            scores += cw * subs[1][0]
        if sw != 0:
            scores += sw * subs[2][0]
        assert bool(torch.isnan(scores[1]).all()) and bool(torch.isfinite(scores[0][subs[0][2][0]]).all())
        arrays[f"out_scores_{i}"] = scores.numpy()
    arrays["out_mask_cand"] = subs[0][2].numpy()
    print(f"{name}: param seeds {seeds} -> {save(name, arrays) / 1024:.1f} KiB")


def init_kwargs(path, cls_name):
    tree = ast.parse(open(path).read())
    cls = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == cls_name)
    init = next(n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name == "__init__")
    return [a.arg for a in init.args.args if a.arg != "self"]


def contract(plm):
    fair = os.path.join(REF, "newsreclib", "models", "fair_rec")
    out = {name: {"init_kwargs": init_kwargs(os.path.join(fair, f), name)}
           for f, name in (("manner_cr_module.py", "CRModule"), ("manner_a_module.py", "AModule"),
                           ("manner_module.py", "MANNERModule"))}

    def head(model):
        return sorted(k for k in model.state_dict() if ".plm_model." not in k)

    out["CRModule"]["head_keys"] = head(RefModel(plm, 1, True, True))
    out["CRModule"]["head_keys_late_fusion"] = head(RefModel(plm, 1, True, False))
    out["AModule"]["head_keys"] = head(RefModel(plm, 1, True, False))
    with open(os.path.join(OUT, "manner_contract.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("manner_contract:", {k: len(v["init_kwargs"]) for k, v in out.items()})


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    plm = MO.make_body(tempfile.mkdtemp())
    with torch.backends.mkldnn.flags(enabled=False):
        run_cr("manner_cr_tiny_train", plm, "sup_con_loss", late_fusion=False, p=0.2, seed=5)
        run_cr("manner_cr_tiny_late_fusion", plm, "cross_entropy_loss", late_fusion=True, p=0.2, seed=6)
        run_cr("manner_cr_tiny_eval", plm, "cross_entropy_loss", late_fusion=False, p=0.0, seed=0)
        run_a("manner_a_tiny_categ", plm, [0, 1, 2, 3, 2, 0, 1, 3, 3, 1, 0, 2])
        run_a("manner_a_tiny_sent", plm, [0, 1, 1, 0, 2, 1, 0, 1], seed=4)          # class 2 is a singleton: its row is dropped
        run_a("manner_a_one_class", plm, [4, 4, 4, 4, 4], seed=5, expect_zero=True)
        run_a("manner_a_all_distinct", plm, [0, 1, 2, 3, 4], seed=6, expect_zero=True)
        run_ens("manner_ens_tiny", plm)
        contract(plm)


if __name__ == "__main__":
    main()
