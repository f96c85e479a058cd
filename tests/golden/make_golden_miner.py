#!/usr/bin/env python3
"""Generate tests/golden/miner_*.npz and miner_contract.json by running the REFERENCE's own MINER components (same rules as
make_golden_caum.py / make_golden_naml_plm.py).  Imported: ``PLM`` (text.py:15-109), ``LinearEncoder`` (category.py),
``NewsEncoder`` (news.py), ``PolyAttention`` / ``TargetAwareAttention`` (layers/attention.py:45-166), ``DotProduct`` and
``components.utils.pairwise_cosine_similarity``.  RESTATED here, not imported: the ``MINERModule`` wiring and forward
(miner_module.py:141-202, 258-323, 398-406 -- the module itself needs lightning / torch_geometric / torchmetrics),
``to_dense_batch`` (loops) and torchmetrics' 2-D ``pairwise_cosine_similarity`` (``cosine_2d``: rows divided by the plain L2
norm, no epsilon -- as recalled; torchmetrics is not installed here).  Every ``nn.Dropout`` of the model is replaced by one
injector that hands out the library's counter-based masks in call order: ``reduce_dim`` dropout of the history call, of the
candidate call, category dropout of the history call, of the candidate call (streams: tests/miner_oracle.py).  The body comes
from tests/miner_oracle.make_body (tests/helpers.make_tiny_roberta; its own dropouts are 0).

Usage:  python tests/golden/make_golden_miner.py   (from the repo root)
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
from tests import miner_oracle as MO  # noqa: E402

spec = importlib.util.spec_from_file_location("nrl_test_helpers", os.path.join(REPO, "tests", "helpers.py"))
th = importlib.util.module_from_spec(spec)          # (the reference ships its own tests/helpers package)
spec.loader.exec_module(th)
sys.path.insert(0, REF)

from newsreclib.models.components.encoders.news.category import LinearEncoder  # noqa: E402
from newsreclib.models.components.encoders.news.news import NewsEncoder  # noqa: E402
from newsreclib.models.components.encoders.news.text import PLM  # noqa: E402
from newsreclib.models.components.layers.attention import PolyAttention, TargetAwareAttention  # noqa: E402
from newsreclib.models.components.layers.click_predictor import DotProduct  # noqa: E402
from newsreclib.models.components.utils import pairwise_cosine_similarity as pairwise_cosine_similarity_3d  # noqa: E402

from oracle.nrms_oracle import dropout_multiplier  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
SAMPLE_STRIDE = 13
MAX_BYTES = 654 * 1024          # plm_full.npz, the largest fixture committed before this one


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


def cosine_2d(x, y, zero_diagonal=False):
    """torchmetrics.functional.pairwise_cosine_similarity, RESTATED (not imported: torchmetrics is not installed)."""
    x = x / torch.linalg.norm(x, ord=2, dim=1, keepdim=True)
    y = y / torch.linalg.norm(y, ord=2, dim=1, keepdim=True)
    d = x @ y.t()
    if zero_diagonal:
        d.fill_diagonal_(0)
    return d


def dense_batch_loops(x, batch, B):
    counts = [int((batch == b).sum()) for b in range(B)]
    mx = max(counts)
    rows, masks, start = [], [], 0
    for b in range(B):
        r = x.new_zeros((mx,) + tuple(x.shape[1:]))
        m = torch.zeros(mx, dtype=torch.bool)
        if counts[b]:
            r[: counts[b]] = x[start:start + counts[b]]
            m[: counts[b]] = True
        rows.append(r)
        masks.append(m)
        start += counts[b]
    return torch.stack(rows), torch.stack(masks)


class RefHead(torch.nn.Module):
    """miner_module.py:159-202 without the news encoder."""

    def __init__(self, cfg, params, p=0.2):
        super().__init__()
        D = cfg["Dn"] if cfg["apply_reduce_dim"] else cfg["T"]
        self.cfg = cfg
        self.inj = Injected()
        if cfg["use_categ_bias"]:
            self.categ_encoder = LinearEncoder(pretrained_embeddings=params["categ_encoder.embedding_layer.weight"].clone(),
                                               from_pretrained=True, freeze_pretrained_emb=False,
                                               num_categories=cfg["n_categ"], embed_dim=None, use_dropout=True,
                                               dropout_probability=p, linear_transform=False, output_dim=None)
            self.categ_encoder.dropout = self.inj
        if not cfg["late_fusion"]:
            self.user_encoder = PolyAttention(input_dim=D, num_context_codes=cfg["K"], context_code_dim=cfg["Cd"])
        self.click_predictor = DotProduct()
        if cfg["score_type"] == "weighted":
            self.target_aware_attn = TargetAwareAttention(input_dim=D)
        self.criterion = torch.nn.CrossEntropyLoss()

    def head(self, hist_news_vector, cand_news_vector, batch):
        """miner_module.py:261-323 and :398-406 after the two news-encoder calls."""
        cfg, B = self.cfg, batch["batch_size"]
        hist_agg, mask_hist = dense_batch_loops(hist_news_vector, batch["batch_hist"], B)
        cand_agg, _ = dense_batch_loops(cand_news_vector, batch["batch_cand"], B)
        extra = {}
        if not cfg["late_fusion"]:
            if cfg["use_categ_bias"]:
                hist_categ_vector = self.categ_encoder(batch["x_hist"]["category"])
                cand_categ_vector = self.categ_encoder(batch["x_cand"]["category"])
                assert float(hist_categ_vector.abs().sum(1).min()) > 0 and float(cand_categ_vector.abs().sum(1).min()) > 0, \
                    "a category row is all-zero after dropout: choose another seed"
                categ_bias = cosine_2d(hist_categ_vector, cand_categ_vector)
                categ_bias_agg, _ = dense_batch_loops(categ_bias, batch["batch_hist"], B)
                mask_cand = batch["batch_cand"].unsqueeze(dim=0).repeat(categ_bias_agg.shape[0], 1)
                cand_idx = [torch.where(mask_cand[i] == i)[0] for i in range(mask_cand.shape[0])]
                mask = torch.zeros(mask_cand.shape, dtype=torch.bool)
                for i in range(mask.shape[0]):
                    mask[i, cand_idx[i]] = True
                mask = mask.unsqueeze(dim=1).repeat(1, categ_bias_agg.shape[1], 1)
                categ_bias_agg = categ_bias_agg.masked_fill(mask, 0)
                user_vector = self.user_encoder(embeddings=hist_agg, attn_mask=mask_hist, bias=categ_bias_agg)
            else:
                user_vector = self.user_encoder(embeddings=hist_agg, attn_mask=mask_hist, bias=None)
            scores = self.click_predictor(cand_agg, user_vector.permute(0, 2, 1))
            extra["matching"] = scores
            if cfg["score_type"] == "max":
                scores = scores.max(dim=2)[0]
            elif cfg["score_type"] == "mean":
                scores = scores.mean(dim=2)
            else:
                scores = self.target_aware_attn(query=user_vector, key=cand_agg, value=scores)
            disagreement = pairwise_cosine_similarity_3d(user_vector, user_vector, zero_diagonal=True).mean()
        else:
            hist_size = torch.tensor([torch.where(mask_hist[i])[0].shape[0] for i in range(mask_hist.shape[0])])
            user_vector = torch.div(hist_agg.sum(dim=1), hist_size.unsqueeze(dim=-1))
            scores = self.click_predictor(user_vector.unsqueeze(dim=1), cand_agg.permute(0, 2, 1))
            disagreement = cosine_2d(user_vector, user_vector, zero_diagonal=True).mean()
        y_true, mask_c = dense_batch_loops(batch["labels"], batch["batch_cand"], B)
        loss = self.criterion(scores, y_true) + disagreement
        return dict(scores=scores, user_vector=user_vector, y_true=y_true, loss=loss, disagreement=disagreement,
                    mask_cand=mask_c, **extra)


class RefMINER(RefHead):
    def __init__(self, cfg, params, plm_path, p=0.2):
        super().__init__(cfg, params, p)
        width = cfg["Dn"] if cfg["apply_reduce_dim"] else cfg["T"]
        text_encoder = PLM(plm_model=plm_path, frozen_layers=list(MO.BODY_FROZEN), embed_dim=cfg["T"], use_mhsa=False,
                           apply_reduce_dim=cfg["apply_reduce_dim"], reduced_embed_dim=width, num_heads=None, query_dim=None,
                           dropout_probability=p)
        if cfg["apply_reduce_dim"]:
            text_encoder.dropout = self.inj
        self.news_encoder = NewsEncoder(dataset_attributes=["title", "abstract", "category"], attributes2encode=["title"],
                                        concatenate_inputs=False, text_encoder=text_encoder, category_encoder=None,
                                        entity_encoder=None, combine_vectors=False, combine_type=None, input_dim=None,
                                        query_dim=None, output_dim=None)
        res = self.load_state_dict(params, strict=False)
        assert not res.unexpected_keys and all(".plm_model." in k for k in res.missing_keys), res

    def forward(self, batch, p, seed):
        cfg = self.cfg
        nh, nc = batch["batch_hist"].shape[0], batch["batch_cand"].shape[0]
        D = cfg["Dn"] if cfg["apply_reduce_dim"] else cfg["T"]
        seq = []
        if p > 0.0:
            if cfg["apply_reduce_dim"]:
                seq += [dropout_multiplier(seed, MO.REDUCE_HIST, p, (nh, D)), dropout_multiplier(seed, MO.REDUCE_CAND, p, (nc, D))]
            if cfg["use_categ_bias"] and not cfg["late_fusion"]:
                seq += [dropout_multiplier(seed, MO.CATEG_HIST, p, (nh, cfg["Dc"])),
                        dropout_multiplier(seed, MO.CATEG_CAND, p, (nc, cfg["Dc"]))]
        self.inj.arm(seq)
        hist_vec = self.news_encoder({"title": batch["x_hist"]["title"]})
        cand_vec = self.news_encoder({"title": batch["x_cand"]["title"]})
        out = self.head(hist_vec, cand_vec, batch)
        assert self.inj.k == len(self.inj.mults), "every injected mask is used"
        out.update(hist_vec=hist_vec, cand_vec=cand_vec)
        return out


def assert_max_gap(out):
    """The largest and second-largest matching score differ by >= 1e-3 in every valid slot (ten times the loosest score
    tolerance), so the argmax is not a matter of rounding and no slot has to be left out of the comparison."""
    top = out["matching"].detach().topk(2, dim=2)[0]
    gap = (top[..., 0] - top[..., 1])[out["mask_cand"]]
    assert float(gap.min()) >= 1e-3, float(gap.min())
    return float(gap.min())


def store_grads(arrays, named, full):
    for k, prm in named.items():
        g = prm.grad if prm.grad is not None else torch.zeros_like(prm)
        flat = g.detach().reshape(-1).double()
        arrays["gnorm/" + k] = np.float64(flat.norm())
        if full(k):
            arrays["gfull/" + k] = g.detach().numpy()
        else:
            arrays["gsample/" + k] = g.detach().reshape(-1)[::SAMPLE_STRIDE].numpy().copy()


def save(name, arrays):
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **arrays)
    size = os.path.getsize(path)
    assert size <= MAX_BYTES, (name, size)
    return size


def cfg_arrays(cfg, param_seed, p, seed):
    a = {"cfg_" + k: np.int64(cfg[k]) for k in MO.CFG_KEYS}
    a.update(cfg_param_seed=np.int64(param_seed), cfg_p_drop=np.float64(p), cfg_seed=np.int64(seed),
             cfg_sample_stride=np.int64(SAMPLE_STRIDE), cfg_score_type=np.int64(MO.SCORE_TYPES.index(cfg["score_type"])),
             cfg_use_categ_bias=np.int64(cfg["use_categ_bias"]), cfg_late_fusion=np.int64(cfg["late_fusion"]),
             cfg_apply_reduce_dim=np.int64(cfg["apply_reduce_dim"]))
    return a


def toks(rng, n, L):
    ids = rng.integers(3, 200, (n, L))
    lens = rng.integers(3, L + 1, n)
    m = (np.arange(L)[None, :] < lens[:, None]).astype(np.int64)
    return {"input_ids": torch.from_numpy(np.where(m == 1, ids, 1)), "attention_mask": torch.from_numpy(m)}


def tiny_batch(cfg, seed):
    """Ragged histories (one user with a single click, one with the longest history) and ragged candidates."""
    hist_sizes, cand_sizes = [2, 5, 1, 4], [5, 7, 3, 5]
    rng = np.random.default_rng(seed)
    nh, nc, B = sum(hist_sizes), sum(cand_sizes), len(hist_sizes)
    labels = torch.zeros(nc)
    start = 0
    for c in cand_sizes:
        labels[start + int(rng.integers(0, c))] = 1.0
        start += c
    return {"x_hist": {"title": toks(rng, nh, 9), "category": torch.from_numpy(rng.integers(1, cfg["n_categ"], nh))},
            "x_cand": {"title": toks(rng, nc, 11), "category": torch.from_numpy(rng.integers(1, cfg["n_categ"], nc))},
            "batch_hist": torch.repeat_interleave(torch.arange(B), torch.tensor(hist_sizes)),
            "batch_cand": torch.repeat_interleave(torch.arange(B), torch.tensor(cand_sizes)),
            "labels": labels, "batch_size": B}


def run_tiny(name, cfg, param_seed, p=0.0, seed=0, batch_seed=5):
    params = MO.make_miner_params(cfg, seed=param_seed)
    model = RefMINER(cfg, params, MO.make_body(tempfile.mkdtemp(), cfg))
    model.train()
    batch = tiny_batch(cfg, batch_seed)
    out = model(batch, p, seed)
    out["loss"].backward()
    gap = assert_max_gap(out) if cfg["score_type"] == "max" and not cfg["late_fusion"] else None
    arrays = {"in_batch_hist": batch["batch_hist"].numpy(), "in_batch_cand": batch["batch_cand"].numpy(),
              "in_labels": batch["labels"].numpy(), "in_batch_size": np.int64(batch["batch_size"])}
    for side in ("hist", "cand"):
        arrays[f"in_category_{side}"] = batch["x_" + side]["category"].numpy()
        for k, v in batch["x_" + side]["title"].items():
            arrays[f"in_title_{side}_{k}"] = v.numpy()
    arrays.update(cfg_arrays(cfg, param_seed, p, seed))
    if gap is not None:
        arrays["out_matching"] = out["matching"].detach().numpy()
    for k in ("scores", "y_true", "loss", "disagreement", "user_vector", "hist_vec", "cand_vec"):
        arrays["out_" + k] = out[k].detach().numpy()
    store_grads(arrays, dict(model.named_parameters()), full=lambda k: ".plm_model." not in k)
    size = save(name, arrays)
    print(f"{name}: loss={float(out['loss'].detach()):.6f} disagreement={float(out['disagreement'].detach()):.6f}"
          + (f" max-gap={gap:.2e}" if gap is not None else "") + f" -> {size / 1024:.1f} KiB")


# configs/model/miner.yaml widths: news vector 256, 32 context codes of 200 features; 200 candidates; histories up to 50
FULL = dict(T=768, Dn=256, K=32, Cd=200, Dc=100, n_categ=19, score_type="weighted", use_categ_bias=True, late_fusion=False,
            apply_reduce_dim=True)
FULL_HIST, FULL_CAND = [50, 23, 1, 37], [200, 150, 5, 80]


def head_full_inputs(cfg, seed):
    """Seeded news vectors and categories of the head-only fixture (re-created by the tests from the seed)."""
    g = torch.Generator().manual_seed(seed)
    nh, nc, B = sum(FULL_HIST), sum(FULL_CAND), len(FULL_HIST)
    hist_vec = (torch.randn(nh, cfg["Dn"], generator=g) * 0.25).float()
    cand_vec = (torch.randn(nc, cfg["Dn"], generator=g) * 0.25).float()
    rng = np.random.default_rng(seed)
    labels = torch.zeros(nc)
    start = 0
    for c in FULL_CAND:
        labels[start + int(rng.integers(0, c))] = 1.0
        start += c
    batch = {"x_hist": {"category": torch.from_numpy(rng.integers(1, cfg["n_categ"], nh))},
             "x_cand": {"category": torch.from_numpy(rng.integers(1, cfg["n_categ"], nc))},
             "batch_hist": torch.repeat_interleave(torch.arange(B), torch.tensor(FULL_HIST)),
             "batch_cand": torch.repeat_interleave(torch.arange(B), torch.tensor(FULL_CAND)),
             "labels": labels, "batch_size": B}
    return hist_vec, cand_vec, batch


def run_head_full(name="miner_head_full", param_seed=11, p=0.2, seed=21, input_seed=31):
    cfg = FULL
    params = MO.make_miner_params(cfg, seed=param_seed)
    params = {k: v for k, v in params.items() if not k.startswith(MO.TXT)}
    model = RefHead(cfg, params)
    res = model.load_state_dict(params, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    model.train()
    hist_vec, cand_vec, batch = head_full_inputs(cfg, input_seed)
    hist_vec.requires_grad_(True)
    cand_vec.requires_grad_(True)
    nh, nc = hist_vec.shape[0], cand_vec.shape[0]
    model.inj.arm([dropout_multiplier(seed, MO.CATEG_HIST, p, (nh, cfg["Dc"])),
                   dropout_multiplier(seed, MO.CATEG_CAND, p, (nc, cfg["Dc"]))])
    out = model.head(hist_vec, cand_vec, batch)
    assert model.inj.k == 2
    out["loss"].backward()
    arrays = {"in_batch_hist": batch["batch_hist"].numpy(), "in_batch_cand": batch["batch_cand"].numpy(),
              "in_labels": batch["labels"].numpy(), "in_batch_size": np.int64(batch["batch_size"]),
              "in_category_hist": batch["x_hist"]["category"].numpy(), "in_category_cand": batch["x_cand"]["category"].numpy(),
              "cfg_input_seed": np.int64(input_seed)}
    arrays.update(cfg_arrays(cfg, param_seed, p, seed))
    for k in ("scores", "y_true", "loss", "disagreement"):
        arrays["out_" + k] = out[k].detach().numpy()
    arrays["out_user_vector"] = out["user_vector"].detach().reshape(-1)[::SAMPLE_STRIDE].numpy().copy()
    named = dict(model.named_parameters())
    store_grads(arrays, named, full=lambda k: False)
    arrays["gin_hist_vec"] = hist_vec.grad.reshape(-1)[::SAMPLE_STRIDE].numpy().copy()
    arrays["gin_cand_vec"] = cand_vec.grad.reshape(-1)[::SAMPLE_STRIDE].numpy().copy()
    size = save(name, arrays)
    print(f"{name}: loss={float(out['loss'].detach()):.6f} disagreement={float(out['disagreement'].detach()):.6f} "
          f"-> {size / 1024:.1f} KiB")


def contract(plm_path):
    src = open(os.path.join(REF, "newsreclib/models/general_rec/miner_module.py")).read()
    kwargs = None
    for node in ast.walk(ast.parse(src)):
        if isinstance(node, ast.ClassDef) and node.name == "MINERModule":
            for f in node.body:
                if isinstance(f, ast.FunctionDef) and f.name == "__init__":
                    kwargs = [a.arg for a in f.args.args[1:]]
    cfg = dict(FULL, T=96, n_categ=19)          # the tiny body's width; everything else as configs/model/miner.yaml
    model = RefMINER(cfg, MO.make_miner_params(cfg, seed=0), plm_path)
    state = {k: list(v.shape) for k, v in model.state_dict().items()}
    out = {"init_kwargs": kwargs, "config": {k: cfg[k] for k in ("T", "Dn", "K", "Cd", "Dc", "n_categ", "score_type")},
           "state_dict": state}
    with open(os.path.join(OUT, "miner_contract.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print(f"miner_contract: {len(kwargs)} kwargs, {len(state)} state-dict keys")


TINY = dict(T=96, Dn=32, K=4, Cd=16, Dc=12, n_categ=7, score_type="weighted", use_categ_bias=True, late_fusion=False,
            apply_reduce_dim=True)


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    with torch.backends.mkldnn.flags(enabled=False):        # see make_golden_lstur.py
        run_tiny("miner_tiny_train", TINY, param_seed=1, p=0.2, seed=5)
        run_tiny("miner_tiny_eval", TINY, param_seed=2)
        run_tiny("miner_tiny_max", dict(TINY, score_type="max"), param_seed=3, p=0.2, seed=6)
        run_tiny("miner_tiny_mean", dict(TINY, score_type="mean"), param_seed=4, p=0.2, seed=7)
        run_tiny("miner_tiny_no_bias", dict(TINY, use_categ_bias=False), param_seed=5, p=0.2, seed=8)
        run_tiny("miner_tiny_late_fusion", dict(TINY, late_fusion=True), param_seed=6, p=0.2, seed=9)
        run_tiny("miner_tiny_no_reduce", dict(TINY, apply_reduce_dim=False), param_seed=7, p=0.2, seed=10)
        run_head_full()
        contract(MO.make_body(tempfile.mkdtemp(), TINY))


if __name__ == "__main__":
    main()
