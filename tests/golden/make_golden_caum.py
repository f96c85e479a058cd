#!/usr/bin/env python3
"""Generate tests/golden/caum_*.npz and caum_contract.json by running the REFERENCE's own CAUM components (same rules as the
other generators).  Imported: ``MHSAAddAtt`` (text.py:179-236), ``LinearEncoder`` (category.py), ``NewsEncoder``
(news.py:9-183), the CAUM ``UserEncoder`` (user/caum.py) and ``DotProduct``; the module wiring (caum_module.py:151-270),
forward (:326-360, with ``to_dense_batch`` restated as loops) and the CE loss are restated around them.  Every
``nn.Dropout`` of the model is replaced by one injector that hands out the library's counter-based masks in call order:
the history call's title embedding / attention output, category, entity embedding / attention output, the same five of the
candidate call, then dropout1 / dropout2 / dropout3 of every candidate slot (streams: tests/caum_oracle.py).

Usage:  python tests/golden/make_golden_caum.py   (from the repo root)
"""
import ast
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REF = "/root/reference"
sys.path.insert(0, REPO)
from tests.caum_oracle import ENT, TXT, USER_STREAM_BASE, make_caum_params, news_masks  # noqa: E402

sys.path.insert(0, REF)

from newsreclib.models.components.encoders.news.category import LinearEncoder  # noqa: E402
from newsreclib.models.components.encoders.news.news import NewsEncoder  # noqa: E402
from newsreclib.models.components.encoders.news.text import MHSAAddAtt  # noqa: E402
from newsreclib.models.components.encoders.user.caum import UserEncoder  # noqa: E402
from newsreclib.models.components.layers.click_predictor import DotProduct  # noqa: E402

from newsreclib_amd.synthetic import add_dkn_fields, batch_from_sizes, make_batch  # noqa: E402
from oracle.nrms_oracle import dropout_multiplier  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
SAMPLE_STRIDE = 97


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


class RefCAUM(torch.nn.Module):
    def __init__(self, params, cfg, use_entities, late_fusion, p=0.2):
        super().__init__()
        attrs = ["title", "category"] + (["title_entities"] if use_entities else [])
        text = MHSAAddAtt(pretrained_embeddings=params[TXT + "embedding_layer.weight"], embed_dim=cfg["D"],
                          num_heads=cfg["Dh"], query_dim=cfg["Q"], dropout_probability=p)
        categ = LinearEncoder(pretrained_embeddings=None, from_pretrained=False, freeze_pretrained_emb=False,
                              num_categories=cfg["n_categ"], embed_dim=cfg["Dc"], use_dropout=True,
                              dropout_probability=p, linear_transform=True, output_dim=cfg["Dc"])
        ent = None
        if use_entities:
            ent = MHSAAddAtt(pretrained_embeddings=params[ENT + "embedding_layer.weight"], embed_dim=cfg["Ed"],
                             num_heads=cfg["Eh"], query_dim=cfg["Q"], dropout_probability=p)
        self.news_encoder = NewsEncoder(dataset_attributes=["title", "abstract", "category", "title_entities"],
                                        attributes2encode=attrs, concatenate_inputs=False, text_encoder=text,
                                        category_encoder=categ, entity_encoder=ent, combine_vectors=True,
                                        combine_type="linear",
                                        input_dim=cfg["D"] + cfg["Dc"] + (cfg["Ed"] if use_entities else 0),
                                        query_dim=None, output_dim=cfg["N"])
        self.late_fusion = late_fusion
        if not late_fusion:
            self.user_encoder = UserEncoder(news_embed_dim=cfg["N"], num_filters=cfg["F"],
                                            dense_att_hidden_dim1=cfg["h1"], dense_att_hidden_dim2=cfg["h2"],
                                            user_vector_dim=cfg["N"], num_heads=cfg["Dh"], dropout_probability=p)
        self.click_predictor = DotProduct()
        res = self.load_state_dict(params, strict=True)
        assert not res.missing_keys and not res.unexpected_keys
        self.inj = Injected()
        text.dropout = self.inj
        categ.dropout = self.inj
        if ent is not None:
            ent.dropout = self.inj
        if not late_fusion:
            self.user_encoder.dropout1 = self.user_encoder.dropout2 = self.user_encoder.dropout3 = self.inj
        self.criterion = torch.nn.CrossEntropyLoss()


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


def arm(model, batch, cfg, p, seed, use_entities):
    if p <= 0.0:
        model.inj.arm([])
        return
    nh, nc, L = batch["x_hist"]["title"].shape[0], batch["x_cand"]["title"].shape[0], batch["x_hist"]["title"].shape[1]
    m = news_masks(seed, p, nh + nc, L, cfg, use_entities)
    seq = []
    for rows in (slice(0, nh), slice(nh, nh + nc)):
        seq += [m["t0"][rows], m["t1"][rows].transpose(0, 1), m["c"][rows]]      # the attention output is seq-first there
        if use_entities:
            seq += [m["e0"][rows], m["e1"][rows].transpose(0, 1)]
    if not model.late_fusion:
        B = batch["batch_size"]
        H = int(torch.bincount(batch["batch_hist"], minlength=B).max())
        C = int(torch.bincount(batch["batch_cand"], minlength=B).max())
        for i in range(C):
            b = USER_STREAM_BASE + 3 * i
            seq += [dropout_multiplier(seed, b, p, (B, cfg["N"])), dropout_multiplier(seed, b + 1, p, (B, H, cfg["N"])),
                    dropout_multiplier(seed, b + 2, p, (B, H, cfg["F"] + cfg["N"]))]
    model.inj.arm(seq)


def ref_forward(model, batch, cfg, p, seed, use_entities):
    arm(model, batch, cfg, p, seed, use_entities)
    B = batch["batch_size"]
    hist_vec = model.news_encoder(batch["x_hist"])
    hist_agg, mask_hist = dense_batch_loops(hist_vec, batch["batch_hist"], B)
    cand_vec = model.news_encoder(batch["x_cand"])
    cand_agg, _ = dense_batch_loops(cand_vec, batch["batch_cand"], B)
    if not model.late_fusion:
        scores = torch.zeros(cand_agg.shape[0], cand_agg.shape[1]).transpose(1, 0)
        for i in range(cand_agg.shape[1]):
            scores[i, :] = model.user_encoder(hist_agg, cand_agg[:, i, :])
        scores = scores.transpose(1, 0)
    else:
        hist_size = mask_hist.sum(dim=1)
        user = torch.div(hist_agg.sum(dim=1), hist_size.unsqueeze(dim=-1))
        scores = model.click_predictor(user.unsqueeze(dim=1), cand_agg.permute(0, 2, 1))
    if p > 0.0:
        assert model.inj.k == len(model.inj.mults), "every injected mask is used"
    y_true, _ = dense_batch_loops(batch["labels"], batch["batch_cand"], B)
    loss = model.criterion(scores, y_true)
    return dict(hist_vec=hist_vec, cand_vec=cand_vec, scores=scores, y_true=y_true, loss=loss)


def run_case(name, batch, cfg, param_seed=1, p=0.0, seed=0, full_grads=False, row_stride=1, use_entities=True,
             late_fusion=False):
    params = make_caum_params(cfg, use_entities=use_entities, late_fusion=late_fusion, seed=param_seed)
    model = RefCAUM(params, cfg, use_entities, late_fusion)
    model.train()
    out = ref_forward(model, batch, cfg, p, seed, use_entities)
    out["loss"].backward()
    arrays = {"in_batch_hist": batch["batch_hist"].numpy(), "in_batch_cand": batch["batch_cand"].numpy(),
              "in_labels": batch["labels"].numpy(), "in_batch_size": np.int64(batch["batch_size"])}
    for side in ("hist", "cand"):
        for k in ("title", "category", "title_entities"):
            arrays[f"in_{k}_{side}"] = batch["x_" + side][k].numpy()
    arrays.update({"cfg_" + k: np.int64(v) for k, v in cfg.items()})
    arrays.update(cfg_param_seed=np.int64(param_seed), cfg_p_drop=np.float64(p), cfg_seed=np.int64(seed),
                  cfg_sample_stride=np.int64(SAMPLE_STRIDE), cfg_row_stride=np.int64(row_stride),
                  cfg_use_entities=np.int64(use_entities), cfg_late_fusion=np.int64(late_fusion))
    for k in ("scores", "y_true", "loss"):
        arrays["out_" + k] = out[k].detach().numpy()
    for k in ("hist_vec", "cand_vec"):
        arrays["out_" + k] = out[k].detach().numpy()[::row_stride].copy()
    sd = model.state_dict(keep_vars=True)
    for k in params:
        g = sd[k].grad if sd[k].grad is not None else torch.zeros_like(sd[k])
        flat = g.detach().reshape(-1).double()
        arrays["gnorm/" + k] = np.float64(flat.norm())
        arrays["gsum/" + k] = np.float64(flat.sum())
        if k.endswith("embedding_layer.weight"):
            rows = torch.nonzero(g.abs().sum(1) > 0).reshape(-1)[:16]
            arrays["grows_idx/" + k] = rows.numpy()
            arrays["grows/" + k] = g[rows].detach().numpy()
        elif full_grads:
            arrays["gfull/" + k] = g.detach().numpy()
        else:
            arrays["gsample/" + k] = g.detach().reshape(-1)[::SAMPLE_STRIDE].numpy().copy()
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **arrays)
    print(f"{name}: loss={float(out['loss'].detach()):.6f} -> {os.path.getsize(path) / 1024:.1f} KiB")
    return arrays


# head dims 8 (text, user) and 5 (entities): both run the head-padded attention
SMALL = dict(vocab=64, n_ent=40, n_categ=19, D=32, Dh=4, Dc=16, Ed=20, Eh=4, Q=16, N=32, F=20, h1=16, h2=12)
# configs/model/caum.yaml widths: text 300 / 20 heads (dh 15), entities 100 / 20 (dh 5), user 400 / 20 (dh 20)
FULL = dict(vocab=2000, n_ent=500, n_categ=19, D=300, Dh=20, Dc=100, Ed=100, Eh=20, Q=200, N=400, F=400, h1=400, h2=256)


def with_fields(b, cfg, seed):
    b = add_dkn_fields(b, n_entities=cfg["n_ent"], seed=seed, max_per_title=4)
    rng = np.random.default_rng(seed + 100)
    for side in ("x_hist", "x_cand"):
        n = b[side]["title"].shape[0]
        b[side] = dict(b[side])
        b[side]["category"] = torch.as_tensor(rng.integers(1, cfg["n_categ"], n))
    return b


def tiny_batch(cfg, seed=11, L=12):
    labels = [0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 1]
    return with_fields(batch_from_sizes([2, 4, 3], [5, 10, 5], labels, vocab=cfg["vocab"], seed=seed, L=L), cfg, seed + 1)


def ragged_batch(cfg):
    """Padded candidate slots, short histories and two histories of exactly max_hist: the circular shift wraps onto a pad
    row for the short ones and onto the last click for the full ones."""
    labels = [1, 0, 0, 0, 0, 1, 0, 0, 1, 0, 0, 1, 0, 0]
    return with_fields(batch_from_sizes([2, 6, 1, 6], [3, 5, 2, 4], labels, vocab=cfg["vocab"], seed=17, L=10), cfg, 18)


def one_user_batch(cfg):
    return with_fields(batch_from_sizes([5], [4], [0, 1, 0, 0], vocab=cfg["vocab"], seed=19, L=10), cfg, 20)


def contract():
    src = open(os.path.join(REF, "newsreclib/models/general_rec/caum_module.py")).read()
    kwargs = None
    for node in ast.walk(ast.parse(src)):
        if isinstance(node, ast.ClassDef) and node.name == "CAUMModule":
            for f in node.body:
                if isinstance(f, ast.FunctionDef) and f.name == "__init__":
                    kwargs = [a.arg for a in f.args.args[1:]]
    cfg = dict(vocab=100, num_entities=60, num_categ_classes=18, text_embed_dim=300, text_num_heads=20, categ_embed_dim=100,
               entity_embed_dim=100, entity_num_heads=20, query_dim=200, news_embed_dim=400, user_vector_dim=400,
               num_filters=400, dense_att_hidden_dim1=400, dense_att_hidden_dim2=256)
    full = dict(FULL, vocab=cfg["vocab"], n_ent=cfg["num_entities"])
    params = make_caum_params(full, seed=0)
    model = RefCAUM(params, full, use_entities=True, late_fusion=False)
    state = {k: list(v.shape) for k, v in model.state_dict().items()}
    out = {"init_kwargs": kwargs, "config": cfg, "state_dict": state}
    with open(os.path.join(OUT, "caum_contract.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print(f"caum_contract: {len(kwargs)} kwargs, {len(state)} state-dict keys")


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    with torch.backends.mkldnn.flags(enabled=False):        # see make_golden_lstur.py
        run_case("caum_tiny_train", tiny_batch(SMALL), SMALL, param_seed=1, p=0.2, seed=5, full_grads=True)
        run_case("caum_tiny_eval", tiny_batch(SMALL, seed=13), SMALL, param_seed=3, full_grads=True)
        run_case("caum_tiny_late_fusion", tiny_batch(SMALL), SMALL, param_seed=2, p=0.2, seed=6, full_grads=True,
                 late_fusion=True)
        run_case("caum_tiny_no_entities", tiny_batch(SMALL), SMALL, param_seed=4, p=0.2, seed=7, full_grads=True,
                 use_entities=False)
        run_case("caum_ragged", ragged_batch(SMALL), SMALL, param_seed=5, full_grads=True)
        run_case("caum_one_user", one_user_batch(SMALL), SMALL, param_seed=6, p=0.2, seed=8, full_grads=True)
        b = with_fields(make_batch(3, vocab=FULL["vocab"], mode="ragged", seed=23, L=10, H=8, neg_ratio=2), FULL, 24)
        run_case("caum_full_train", b, FULL, param_seed=7, p=0.2, seed=9, row_stride=3)
    contract()


if __name__ == "__main__":
    main()
