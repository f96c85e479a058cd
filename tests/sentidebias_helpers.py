"""Shared helpers of the SentiDebias tests: fixtures -> batch / parameters / the product module."""
from functools import partial

import torch

from tests import sentidebias_oracle as SO

CASES = ["sentidebias_tiny_eval", "sentidebias_tiny_train", "sentidebias_tiny_late_fusion", "sentidebias_tiny_class0",
         "sentidebias_one_user", "sentidebias_32_train"]
OUTPUTS = {"train": ["preds", "targets", "cand_news_size"], "val": ["preds", "targets", "cand_news_size"],
           "test": ["preds", "targets", "cand_news_size", "hist_news_size", "target_categories", "target_sentiments",
                    "hist_categories", "hist_sentiments", "user_ids", "cand_news_ids"]}


def golden_batch(g, device="cpu"):
    from tests.helpers import golden_batch as base
    b = base(g, device)
    b["x_hist"]["sentiment"] = torch.as_tensor(g["in_sent_hist"]).to(device)
    b["x_cand"]["sentiment"] = torch.as_tensor(g["in_sent_cand"]).to(device)
    return b


def golden_params(g):
    return SO.make_params(int(g["cfg_vocab"]), int(g["cfg_nrms_seed"]), int(g["cfg_head_seed"]), bool(int(g["cfg_late_fusion"])))


def build_module(params, p_drop=0.2, late_fusion=False, device="cuda", alpha=0.15, beta=10.0, opt_g=None, opt_d=None,
                 use_plm=False):
    from newsreclib_amd.senti_debias_module import Discriminator, Generator, SentiDebiasModule, SentimentEncoder
    emb = params["generator.news_encoder.text_encoders.title.embedding_layer.weight"]
    gen = Generator(dataset_attributes=["title", "abstract", "category", "sentiment"], attributes2encode=["title"],
                    late_fusion=late_fusion, use_plm=use_plm, pretrained_embeddings_path=None, plm_model=None, frozen_layers=None,
                    embed_dim=SO.D, num_heads=15, query_dim=200, dropout_probability=float(p_drop),
                    sentiment_encoder=SentimentEncoder(num_sent_classes=SO.N_SENT - 1, sent_embed_dim=SO.SENT_EMB,
                                                       sent_output_dim=SO.D),
                    pretrained_embeddings=torch.zeros_like(emb))
    mod = SentiDebiasModule(outputs=OUTPUTS, generator=gen, discriminator=Discriminator(SO.D, SO.HIDDEN, SO.N_OUT),
                            top_k_list=[5, 10], num_categ_classes=18, num_sent_classes=SO.N_SENT - 1, save_recs=False,
                            recs_fpath=None, optimizer=None, alpha_coefficient=alpha, beta_coefficient=beta,
                            optimizer_generator=opt_g or partial(torch.optim.Adam, lr=1e-5),
                            optimizer_discriminator=opt_d or partial(torch.optim.Adam, lr=2e-5), scheduler=None)
    res = mod.load_state_dict(params, strict=True)          # reference checkpoint keys load as they are
    assert not res.missing_keys and not res.unexpected_keys
    return mod.to(device)


class pinned_seeds:
    """The news encoder's dropout draws, in call order (phase G, phase D, ...)."""

    def __init__(self, seeds):
        self.seeds = list(seeds)

    def __enter__(self):
        import newsreclib_amd.news_encoder as NE
        self.NE, self.orig = NE, NE._draw_seed
        it = iter(self.seeds)
        NE._draw_seed = lambda: int(next(it))
        return self

    def __exit__(self, *exc):
        self.NE._draw_seed = self.orig
        return False
