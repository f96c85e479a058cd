#!/usr/bin/env python3
"""Generate tests/golden/sentidebias_*.npz and sentidebias_contract.json with the REFERENCE's own components (same rules as
make_golden.py, whose ``RefNRMS`` -- reference ``MHSAAddAtt``, ``NewsEncoder``, NRMS ``UserEncoder``, ``DotProduct`` -- is reused)
plus the reference's ``aspect.SentimentEncoder``.  ``senti_debias_module`` itself needs lightning / torch_geometric / torchmetrics,
so what it adds around those components -- the generator's wiring (:164-263), the two-layer discriminator (:23-51), the adversarial
loss (:406-411) and the two-phase train step (:475-530) -- is restated here in this project's words.  Dropout draws are the
project's counter-based masks injected into the reference's dropout module (make_golden.py).

Every fixture asserts that |mean cos| of both news terms and every |cos_user| of ``loss_orth`` is at least 1e-3 -- ten times the
1e-4 output bound, so no sign under an ``abs`` can flip within tolerance; the head seeds below were picked (first hit, counting up
from 1) so that the reference satisfies it.

Usage:  python tests/golden/make_golden_sentidebias.py   (from the repo root)
"""
import ast
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402  (puts the repo root and the reference checkout on sys.path)

from newsreclib.models.components.encoders.news.aspect import SentimentEncoder  # noqa: E402

from newsreclib_amd.synthetic import batch_from_sizes, make_batch  # noqa: E402
from oracle.nrms_oracle import dropout_multiplier  # noqa: E402

sys.path.insert(0, os.path.dirname(HERE))
import sentidebias_oracle as SO  # noqa: E402

ALPHA, BETA = 0.15, 10.0          # configs/model/senti_debias.yaml:54-55
GUARD = 1e-3


class RefSentiDebias(torch.nn.Module):
    """Reference components under the reference's attribute names (=> the reference's state_dict keys)."""

    def __init__(self, params):
        super().__init__()
        nrms = MG.RefNRMS({k[len("generator."):]: v for k, v in params.items()
                           if k.startswith("generator.") and ".sentiment_encoder." not in k})
        self.generator = torch.nn.Module()
        self.generator.news_encoder, self.generator.user_encoder = nrms.news_encoder, nrms.user_encoder
        self.generator.sentiment_encoder = SentimentEncoder(num_sent_classes=SO.N_SENT - 1, sent_embed_dim=SO.SENT_EMB,
                                                            sent_output_dim=SO.D)
        self.discriminator = torch.nn.Module()
        self.discriminator.linear1 = torch.nn.Linear(SO.D, SO.HIDDEN)
        self.discriminator.linear2 = torch.nn.Linear(SO.HIDDEN, SO.N_OUT)
        res = self.load_state_dict(params, strict=True)
        assert not res.missing_keys and not res.unexpected_keys
        self.inj, self.dot = nrms.inj, nrms.click_predictor
        self.ce = torch.nn.CrossEntropyLoss()


def arm(model, batch, p_drop, seed):
    nh, nc = batch["x_hist"]["title"].shape[0], batch["x_cand"]["title"].shape[0]
    L = batch["x_hist"]["title"].shape[1]
    if p_drop > 0:
        m1 = dropout_multiplier(seed, 0, p_drop, (nh + nc, L, SO.D))
        m2 = dropout_multiplier(seed, 1, p_drop, (nh + nc, L, SO.D))
        model.inj.arm([m1[:nh], m2[:nh], m1[nh:], m2[nh:]])
    else:
        model.inj.arm([])


def cosine(a, b):
    return (a * b).sum(-1) / (1e-8 + torch.linalg.norm(a, dim=-1) * torch.linalg.norm(b, dim=-1))


def generator_forward(model, batch, p_drop, seed, late_fusion):
    g, B = model.generator, batch["batch_size"]
    arm(model, batch, p_drop, seed)
    hist_vec = g.news_encoder({"title": batch["x_hist"]["title"]})
    cand_vec = g.news_encoder({"title": batch["x_cand"]["title"]})
    hist_sent, cand_sent = g.sentiment_encoder(batch["x_hist"]["sentiment"]), g.sentiment_encoder(batch["x_cand"]["sentiment"])
    hist_dense, mask = MG.dense_batch_loops(hist_vec, batch["batch_hist"], B)
    cand_dense, _ = MG.dense_batch_loops(cand_vec, batch["batch_cand"], B)
    hist_sent_dense, _ = MG.dense_batch_loops(hist_sent, batch["batch_hist"], B)
    cand_sent_dense, _ = MG.dense_batch_loops(cand_sent, batch["batch_cand"], B)
    if late_fusion:
        n = mask.sum(dim=1, keepdim=True)
        user_free, user_aware = hist_dense.sum(dim=1) / n, hist_sent_dense.sum(dim=1) / n
    else:
        user_free, user_aware = g.user_encoder(hist_dense), g.user_encoder(hist_sent_dense)
    cos_h, cos_c = cosine(hist_vec, hist_sent).mean(), cosine(cand_vec, cand_sent).mean()
    cos_u = cosine(user_free, user_aware).unsqueeze(1)
    loss_orth = (cos_h.abs() + cos_c.abs() + cos_u.abs()).mean()
    free = model.dot(user_free.unsqueeze(1), cand_dense.permute(0, 2, 1))
    aware = model.dot(user_aware.unsqueeze(1), cand_sent_dense.permute(0, 2, 1))
    return dict(combined=free + aware, bias_free=free, loss_orth=loss_orth, hist_vec=hist_vec, cand_vec=cand_vec,
                cos_hist=cos_h, cos_cand=cos_c, cos_user=cos_u.reshape(-1), user_free=user_free, user_aware=user_aware)


def adversarial(model, vec, ids):
    d = model.discriminator
    logits = d.linear2(torch.tanh(d.linear1(vec)))
    target = torch.zeros_like(logits)
    for i in range(ids.shape[0]):
        target[i, ids[i] - 1] = 1.0                     # id 0 -> column -1
    return model.ce(logits, target)


def toggle(model, which):
    for k, p in model.named_parameters():
        p.requires_grad_(k.startswith(which))


def phase_g(model, batch, p_drop, seed, late_fusion):
    toggle(model, "generator.")
    out = generator_forward(model, batch, p_drop, seed, late_fusion)
    y_true, _ = MG.dense_batch_loops(batch["labels"], batch["batch_cand"], batch["batch_size"])
    adv = adversarial(model, out["hist_vec"], batch["x_hist"]["sentiment"]) + \
        adversarial(model, out["cand_vec"], batch["x_cand"]["sentiment"])
    out["g_loss"] = model.ce(out["combined"], y_true) + BETA * out["loss_orth"] - ALPHA * adv
    return out


def phase_d(model, batch, p_drop, seed, late_fusion):
    toggle(model, "discriminator.")
    out = generator_forward(model, batch, p_drop, seed, late_fusion)
    return adversarial(model, out["hist_vec"], batch["x_hist"]["sentiment"]) + \
        adversarial(model, out["cand_vec"], batch["x_cand"]["sentiment"])


def grad_summary(model, prefix, tag):
    out = {}
    for k, p in model.state_dict(keep_vars=True).items():
        if not k.startswith(prefix):
            continue
        g = p.grad if p.grad is not None else torch.zeros_like(p)
        flat = g.detach().reshape(-1).double()
        out[f"{tag}gnorm/{k}"], out[f"{tag}gsum/{k}"] = np.float64(flat.norm()), np.float64(flat.sum())
        out[f"{tag}gsample/{k}"] = g.detach().reshape(-1)[::MG.SAMPLE_STRIDE].numpy().copy()
    return out


def with_sentiment(batch, seed, force=None):
    g = torch.Generator().manual_seed(seed)
    for part in ("x_hist", "x_cand"):
        n = batch[part]["title"].shape[0]
        batch[part]["sentiment"] = torch.randint(0, SO.N_SENT, (n,), generator=g)
        if force is not None:
            batch[part]["sentiment"][: len(force[part])] = torch.tensor(force[part])
    return batch


def inputs(batch, vocab, nrms_seed, head_seed, p_drop, late_fusion, full):
    arrays = MG.batch_arrays(batch)
    arrays.update(in_sent_hist=batch["x_hist"]["sentiment"].numpy(), in_sent_cand=batch["x_cand"]["sentiment"].numpy(),
                  cfg_vocab=np.int64(vocab), cfg_nrms_seed=np.int64(nrms_seed), cfg_head_seed=np.int64(head_seed),
                  cfg_p_drop=np.float64(p_drop), cfg_late_fusion=np.int64(late_fusion), cfg_alpha=np.float64(ALPHA),
                  cfg_beta=np.float64(BETA), cfg_sample_stride=np.int64(MG.SAMPLE_STRIDE),
                  cfg_row_stride=np.int64(1 if full else MG.ROW_STRIDE))
    return arrays


def guard_ok(out):
    return min(float(out["cos_hist"].abs()), float(out["cos_cand"].abs()), float(out["cos_user"].abs().min())) >= GUARD


def run_case(name, batch, vocab, nrms_seed, p_drop=0.0, seed_g=0, seed_d=0, late_fusion=False, full=True):
    for head_seed in range(1, 50):
        params = SO.make_params(vocab, nrms_seed, head_seed)
        model = RefSentiDebias(params).train()
        out = phase_g(model, batch, p_drop, seed_g, late_fusion)
        if guard_ok(out):
            break
    else:
        raise RuntimeError(name + ": no head seed satisfies the |cos| guard")
    out["g_loss"].backward()
    arrays = inputs(batch, vocab, nrms_seed, head_seed, p_drop, late_fusion, full)
    arrays.update(cfg_seed_g=np.int64(seed_g), cfg_seed_d=np.int64(seed_d))
    rs = int(arrays["cfg_row_stride"])
    for k in ("combined", "bias_free", "loss_orth", "g_loss", "cos_hist", "cos_cand", "cos_user", "user_free", "user_aware"):
        arrays["out_" + k] = out[k].detach().numpy()
    for k in ("hist_vec", "cand_vec"):
        arrays["out_" + k] = out[k].detach().numpy()[::rs].copy()
    arrays.update(grad_summary(model, "generator.", ""))
    assert all(p.grad is None for k, p in model.named_parameters() if k.startswith("discriminator."))
    model.zero_grad(set_to_none=True)
    d_loss = phase_d(model, batch, p_drop, seed_d, late_fusion)          # at the SAME (initial) weights
    d_loss.backward()
    arrays["out_d_loss"] = d_loss.detach().numpy()
    arrays.update(grad_summary(model, "discriminator.", "d_"))
    assert all(p.grad is None for k, p in model.named_parameters() if k.startswith("generator."))
    path = os.path.join(MG.OUT, name + ".npz")
    np.savez_compressed(path, **arrays)
    print(f"{name}: head_seed={head_seed} g_loss={float(out['g_loss']):.6f} d_loss={float(d_loss):.6f} loss_orth="
          f"{float(out['loss_orth']):.6f} |cos| h/c/u_min={float(out['cos_hist'].abs()):.4f}/{float(out['cos_cand'].abs()):.4f}/"
          f"{float(out['cos_user'].abs().min()):.4f} -> {os.path.getsize(path) / 1024:.1f} KiB")


def run_step(name, batch, vocab, nrms_seed, p_drop, seeds, lr_g, lr_d):
    """One whole training_step with plain SGD on both sides (a parameter moves linearly with its gradient), then the losses of
    a second step.  seeds = (G1, D1, G2, D2) dropout draws."""
    for head_seed in range(1, 50):
        model = RefSentiDebias(SO.make_params(vocab, nrms_seed, head_seed)).train()
        if guard_ok(phase_g(model, batch, p_drop, seeds[0], False)):
            break
    model = RefSentiDebias(SO.make_params(vocab, nrms_seed, head_seed)).train()
    opt_g = torch.optim.SGD(model.generator.parameters(), lr=lr_g)
    opt_d = torch.optim.SGD(model.discriminator.parameters(), lr=lr_d)
    losses = []
    for s_g, s_d in (seeds[:2], seeds[2:]):
        out = phase_g(model, batch, p_drop, s_g, False)
        assert guard_ok(out)
        out["g_loss"].backward()
        opt_g.step()
        opt_g.zero_grad()
        d_loss = phase_d(model, batch, p_drop, s_d, False)
        d_loss.backward()
        opt_d.step()
        opt_d.zero_grad()
        losses.append((float(out["g_loss"]), float(d_loss)))
        if len(losses) == 1:
            toggle(model, "")
            after = {k: v.detach().clone() for k, v in model.state_dict().items()}
    arrays = inputs(batch, vocab, nrms_seed, head_seed, p_drop, False, True)
    arrays.update(cfg_seeds=np.asarray(seeds, dtype=np.int64), cfg_lr_g=np.float64(lr_g), cfg_lr_d=np.float64(lr_d),
                  out_losses=np.asarray(losses, dtype=np.float64))
    for k, v in after.items():
        arrays["pnorm/" + k] = np.float64(v.double().norm())
        arrays["psample/" + k] = v.reshape(-1)[::MG.SAMPLE_STRIDE].numpy().copy()
    path = os.path.join(MG.OUT, name + ".npz")
    np.savez_compressed(path, **arrays)
    print(f"{name}: head_seed={head_seed} losses={losses} -> {os.path.getsize(path) / 1024:.1f} KiB")


def write_contract():
    """Constructor keyword names (in order) of the reference's classes, read with ``ast``, and the state-dict keys / shapes of the
    restated module at the config's sizes."""
    import newsreclib
    root = os.path.dirname(os.path.dirname(os.path.abspath(newsreclib.__file__)))
    files = {"SentiDebiasModule": "newsreclib/models/fair_rec/senti_debias_module.py",
             "Generator": "newsreclib/models/fair_rec/senti_debias_module.py",
             "Discriminator": "newsreclib/models/fair_rec/senti_debias_module.py",
             "SentimentEncoder": "newsreclib/models/components/encoders/news/aspect.py"}
    out = {"kwargs": {}, "state_dict": {}}
    for cls, rel in files.items():
        tree = ast.parse(open(os.path.join(root, rel)).read())
        for node in ast.walk(tree):
            if isinstance(node, ast.ClassDef) and node.name == cls:
                init = next(f for f in node.body if isinstance(f, ast.FunctionDef) and f.name == "__init__")
                out["kwargs"][cls] = [a.arg for a in init.args.args if a.arg != "self"]
    model = RefSentiDebias(SO.make_params(64, 1, 1))
    out["state_dict"] = {k: list(v.shape) for k, v in model.state_dict().items()}
    with open(os.path.join(MG.OUT, "sentidebias_contract.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    write_contract()
    tiny = lambda: with_sentiment(MG.tiny_batch(), 3)  # noqa: E731
    run_case("sentidebias_tiny_eval", tiny(), 64, nrms_seed=1)
    run_case("sentidebias_tiny_train", tiny(), 64, nrms_seed=1, p_drop=0.2, seed_g=7, seed_d=8)
    run_case("sentidebias_tiny_late_fusion", tiny(), 64, nrms_seed=1, p_drop=0.2, seed_g=7, seed_d=8, late_fusion=True)
    # real rows of sentiment id 0 next to ragged padding: user 0 (1 click, 3 padded slots) clicked an id-0 news, user 1's first
    # two clicks are id 0; candidates start with id 0 too (the adversarial target wraps to the last column)
    zero = with_sentiment(MG.tiny_batch(), 5, force={"x_hist": [0, 0, 0, 2, 1, 3, 0], "x_cand": [0, 1, 0, 2, 3, 0]})
    run_case("sentidebias_tiny_class0", zero, 64, nrms_seed=1)
    one = with_sentiment(batch_from_sizes([3], [5], [0, 1, 0, 0, 0], vocab=64, seed=12), 6)
    run_case("sentidebias_one_user", one, 64, nrms_seed=1, p_drop=0.2, seed_g=3, seed_d=4)
    b32 = with_sentiment(make_batch(32, vocab=5000, mode="ragged", seed=21), 4)
    run_case("sentidebias_32_train", b32, 5000, nrms_seed=2, p_drop=0.2, seed_g=13, seed_d=14, full=False)
    run_step("sentidebias_tiny_step", tiny(), 64, nrms_seed=1, p_drop=0.2, seeds=(7, 8, 9, 10), lr_g=1e-3, lr_d=1e-2)


if __name__ == "__main__":
    main()
