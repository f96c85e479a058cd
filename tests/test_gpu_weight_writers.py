"""Weight-derived caches against every way the weights can change.

The library keeps state derived from the weights and reused across calls: the per-token q|k|v table of ``MHSAAddAtt`` (pinned by
an evaluation scope, or automatic in eval mode), the matrix-core weight images of ``NrlLinear`` and of the fused attention block
(``FrozenImages``), the lazily updated rows of ``LazyTableAdam`` and the ids the trainer's prefetch builds for the next batch.  A
stale cache gives the exact forward of the OLD weights -- well inside every oracle tolerance of a fresh module -- so each cell here
(1) warms the cache and proves it is hit, (2) changes the weights through one writer, (3) calls again and compares with a float64
reference computed from the NEW weights, after proving that the old weights' answer is at least 100x the tolerance away.

Writers that move no version counter (``p.data.copy_``) are outside the documented contract of the automatic table and of the
images: with frozen weights the remedy is ``ops_blocks.invalidate_frozen_images()``, with trainable weights under a live optimizer
of this library ``ops_blocks.next_optimizer_step()``; those cells apply the remedy.  The pinned table needs none."""
import contextlib
import gc
import os

import numpy as np
import pytest
import torch

from oracle import nrms_oracle as O
from tests.helpers import batch_to, build_module

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

WRITERS = ["adam", "adam_foreach", "adam_fused", "load_state_dict", "load_state_dict_assign", "data_copy", "data_copy_trainer",
           "trainer_dense", "trainer_lazy", "replace_param"]
ADAMS = {"adam": dict(foreach=False), "adam_foreach": dict(foreach=True), "adam_fused": dict(fused=True)}


@pytest.fixture(autouse=True)
def _own_step_drivers():
    # every cell decides for itself which optimizers of this library are alive (another test may have left a process-wide promise)
    from newsreclib_amd import _lib, ops_blocks
    prev = _lib.get_gemm_engine()
    with ops_blocks.no_step_drivers():
        yield
    _lib.set_gemm_engine(prev)
    gc.collect()


def _maxerr(a, b) -> float:
    return float((a.double().cpu() - b.double().cpu()).abs().max())


def _new_values(p: torch.Tensor, seed: int) -> torch.Tensor:
    """W1 of one parameter: far from W0 (scaled, shifted, noised), same shape, on the CPU."""
    g = torch.Generator().manual_seed(seed)
    w0 = p.detach().cpu()
    s = float(w0.std()) if w0.numel() > 1 else 0.1
    return (1.3 * w0 + 0.3 * max(s, 1e-2) * torch.randn(w0.shape, generator=g)).contiguous()


def _replace_parameter(owner: torch.nn.Module, name: str, w1: torch.Tensor) -> bool:
    """Frees the Parameter `owner.name`, then assigns a NEW one holding `w1` (allocated after the free, version counter bumped
    once as the old one's init did).  -> whether the caching allocator handed back the old address."""
    old = getattr(owner, name)
    ptr, shape, rg = old.data_ptr(), tuple(old.shape), old.requires_grad
    setattr(owner, name, None)
    del old
    gc.collect()
    t = torch.empty(shape, dtype=torch.float32, device=DEV)
    t.copy_(w1)
    setattr(owner, name, torch.nn.Parameter(t, requires_grad=rg))
    return t.data_ptr() == ptr


def _write(writer: str, module: torch.nn.Module, names, seed: int, trainer=None, step_batch=None):
    """Changes the parameters `names` of `module` (dotted names) through `writer`.  -> dict with what the cell must know:
    ``remedy`` (the documented call the writer needs, already made) and ``same_address`` (replace_param)."""
    from newsreclib_amd import ops_blocks
    params = dict(module.named_parameters())
    info = {"remedy": None, "same_address": None}
    if writer in ADAMS:
        ps = [params[n] for n in names]
        g = torch.Generator().manual_seed(seed)
        for p in ps:
            p.grad = torch.randn(p.shape, generator=g).to(DEV)
        opt = torch.optim.Adam(ps, lr=0.05, **ADAMS[writer])
        opt.step()
        for p in ps:
            p.grad = None
    elif writer in ("load_state_dict", "load_state_dict_assign"):
        sd = {k: v.clone() for k, v in module.state_dict().items()}
        for i, n in enumerate(names):
            sd[n] = _new_values(params[n], seed + i).to(DEV)
        module.load_state_dict(sd, assign=(writer == "load_state_dict_assign"))
        if writer == "load_state_dict_assign":
            for n in names:                                  # (the module's Parameter objects were replaced, flags kept)
                assert dict(module.named_parameters())[n] is not params[n]
    elif writer in ("data_copy", "data_copy_trainer"):
        for i, n in enumerate(names):
            params[n].data.copy_(_new_values(params[n], seed + i).to(DEV))
        trainable = any(params[n].requires_grad for n in names)
        if trainable and ops_blocks.step_images_allowed(*[params[n] for n in names]):
            ops_blocks.next_optimizer_step()
            info["remedy"] = "next_optimizer_step"
        elif not trainable:
            ops_blocks.invalidate_frozen_images()
            info["remedy"] = "invalidate_frozen_images"
    elif writer in ("trainer_dense", "trainer_lazy"):
        trainer.step(step_batch)
    elif writer == "replace_param":
        vals = [_new_values(params[n], seed + i) for i, n in enumerate(names)]
        params.clear()                                       # (no reference of this function keeps an old Parameter alive)
        same = []
        for n, w1 in zip(names, vals):
            owner_name, _, leaf = n.rpartition(".")
            owner = module.get_submodule(owner_name) if owner_name else module
            same.append(_replace_parameter(owner, leaf, w1))
        info["same_address"] = all(same)
        print(f"replace_param: allocator returned the old address for {sum(same)}/{len(same)} parameters")
    else:
        raise AssertionError(writer)
    return info


# ---------------------------------------------------------------------------------------------------------------------------
# MHSAAddAtt token table (bf16x3 only: ops.token_table_supported)
# ---------------------------------------------------------------------------------------------------------------------------
VOCAB, N_NEWS, L = 2000, 20, 30
TE = "news_encoder.text_encoders.title."
TE_NAMES = [TE + k for k in ("embedding_layer.weight", "multihead_attention.in_proj_weight", "multihead_attention.in_proj_bias",
                             "multihead_attention.out_proj.weight", "multihead_attention.out_proj.bias",
                             "additive_attention.linear.weight", "additive_attention.linear.bias", "additive_attention.query")]


def _ids(seed, n=N_NEWS):
    rng = np.random.default_rng(seed)
    lens = rng.integers(3, L + 1, n)
    ids = rng.integers(1, VOCAB, (n, L))
    ids[np.arange(L)[None, :] >= lens[:, None]] = 0
    return torch.from_numpy(ids).to(DEV)


def _oracle_news(mod, ids):
    """float64 news vectors of the module's CURRENT text-encoder weights."""
    sd = {k: v.detach().double().cpu() for k, v in mod.state_dict().items() if k.startswith(O.NEWS_PREFIX)}
    return O.news_encoder_fwd(ids.cpu(), sd, 15)


def _tableless(mod, fn):
    """`fn()` with the token table out of the way (pinned route replaced by a null scope, automatic route off)."""
    te = mod.news_encoder.text_encoders["title"]
    orig = te.token_table
    te.token_table = lambda: contextlib.nullcontext()
    os.environ["NRL_TOKEN_TABLE"] = "0"
    try:
        return fn()
    finally:
        del os.environ["NRL_TOKEN_TABLE"]
        te.token_table = orig


def _nrms(frozen=False):
    from newsreclib_amd import _lib
    _lib.set_gemm_engine("bf16x3")
    mod = build_module(O.make_params(VOCAB, seed=9), p_drop=0.2, device=DEV)
    if frozen:
        for n, p in mod.named_parameters():
            if n.startswith(TE):
                p.requires_grad_(False)
    te = mod.news_encoder.text_encoders["title"]
    orig = te.forward
    te.forward = lambda text, seed=None, **kw: orig(text, seed=77 if seed is None else seed, **kw)
    return mod


def _train_batch(seed):
    from newsreclib_amd.nrms_module import prepare_batch
    from newsreclib_amd.synthetic import make_batch
    return prepare_batch(batch_to(make_batch(3, VOCAB, "ragged", seed=seed, H=5), DEV))


def _applies(writer, frozen, route):
    if writer in ADAMS and frozen:
        pytest.skip("a frozen weight has no gradient: torch.optim.Adam does not write it")
    if writer in ("trainer_dense", "trainer_lazy") and frozen:
        pytest.skip("a frozen weight has no gradient: the trainer's optimizer does not write it")
    if writer == "replace_param" and not frozen:
        pytest.skip("replacing a trainable Parameter under a live optimizer detaches it from the optimizer (not a writer)")


def _trainer_for(writer, mod):
    from newsreclib_amd.trainer import NRMSTrainer
    if writer in ("data_copy_trainer", "trainer_dense", "trainer_lazy"):
        return NRMSTrainer(mod, lr=1e-2, lazy_adam=(writer == "trainer_lazy"))
    return None


def _check_news(got, mod, ids, w0_ref, tableless):
    ref = _oracle_news(mod, ids)
    tol = 2e-4
    assert _maxerr(w0_ref, ref) >= 100 * tol, "W1 too close to W0: a stale answer could pass"
    assert _maxerr(got, ref) <= tol, _maxerr(got, ref)
    assert torch.equal(got, tableless)


@pytest.mark.parametrize("writer", WRITERS)
def test_pinned_table_over_two_validation_epochs(writer):
    """``on_validation_epoch_start`` -> ``validation_step`` -> ``on_validation_epoch_end`` twice, the weights written in between:
    the second epoch's news vectors are those of the new weights (fp64) and EQUAL to the table-less forward; the table is freed at
    the end of each epoch and rebuilt by the next one (one build per epoch)."""
    from newsreclib_amd.news_encoder import MHSAAddAtt
    frozen = writer in ("replace_param",)
    _applies(writer, frozen, "pinned")
    mod = _nrms(frozen).eval()
    tr = _trainer_for(writer, mod)
    te = mod.news_encoder.text_encoders["title"]
    ids, vbatch = _ids(1), _train_batch(21)
    uses = MHSAAddAtt.TOKEN_TABLE_USES

    def epoch():
        mod.eval()
        b0, f0 = uses["built"], uses["forwards"]
        mod.on_validation_epoch_start()
        with torch.no_grad():
            mod.validation_step(vbatch, 0)
            out = te(ids)
        mod.on_validation_epoch_end()
        assert uses["built"] == b0 + 1 and uses["forwards"] >= f0 + 2     # one build per epoch, every forward from the table
        assert te._tt_buf is None and te._tt_key is None and not te._tt_pinned
        return out

    v0 = epoch()
    w0_ref = _oracle_news(mod, ids)
    assert _maxerr(v0, w0_ref) <= 2e-4
    _write(writer, mod, TE_NAMES, seed=5, trainer=tr, step_batch=_train_batch(31))
    v1 = epoch()
    with torch.no_grad():
        plain = _tableless(mod, lambda: te(ids))
    _check_news(v1, mod, ids, w0_ref, plain)


@pytest.mark.parametrize("writer", WRITERS)
def test_pinned_table_over_two_news_vector_cache_builds(writer):
    """``NewsVectorCache.build`` twice with a writer in between: the second build equals the table-less build bit for bit and
    the fp64 news vectors of the new weights; no table is left behind after either build."""
    from newsreclib_amd.evaluation import DeviceNewsTable, NewsVectorCache
    frozen = writer in ("replace_param",)
    _applies(writer, frozen, "pinned")
    mod = _nrms(frozen)
    tr = _trainer_for(writer, mod)
    te = mod.news_encoder.text_encoders["title"]
    ids = _ids(2, n=150)
    table = DeviceNewsTable({"title": ids.cpu(), "category": torch.ones(150, dtype=torch.int64),
                             "sentiment": torch.ones(150, dtype=torch.int64)})
    v0 = NewsVectorCache(mod, table, chunk=64).build()
    assert te._tt_buf is None
    w0_ref = _oracle_news(mod, ids)
    assert _maxerr(v0, w0_ref) <= 2e-4
    _write(writer, mod, TE_NAMES, seed=6, trainer=tr, step_batch=_train_batch(32))
    v1 = NewsVectorCache(mod, table, chunk=64).build()
    assert te._tt_buf is None
    plain = _tableless(mod, lambda: NewsVectorCache(mod, table, chunk=64).build())
    _check_news(v1, mod, ids, w0_ref, plain)


@pytest.mark.parametrize("frozen", [True, False])
@pytest.mark.parametrize("writer", WRITERS)
def test_automatic_table_follows_the_writer(writer, frozen):
    """Automatic route (eval mode + no_grad): frozen weights with no optimizer of this library alive, trainable weights under a
    live ``NRMSTrainer`` that owns them.  After the writer, every forward -- the first one, and those after the table was built
    again -- is the fp64 forward of the new weights and equal to the table-less forward."""
    from newsreclib_amd import ops_blocks
    from newsreclib_amd.news_encoder import MHSAAddAtt
    from newsreclib_amd.trainer import NRMSTrainer
    _applies(writer, frozen, "auto")
    if writer == "data_copy_trainer" and frozen:
        pytest.skip("frozen weights: a live trainer does not own them, the cell is data_copy")
    if writer == "data_copy" and not frozen:
        pytest.skip("trainable weights use the automatic table only under a live trainer: the cell is data_copy_trainer")
    mod = _nrms(frozen).eval()
    tr = None if frozen else (_trainer_for(writer, mod) or NRMSTrainer(mod, lr=1e-2, lazy_adam=False))
    assert frozen or ops_blocks.step_images_allowed(*mod.news_encoder.text_encoders["title"]._params())
    mod.eval()
    te = mod.news_encoder.text_encoders["title"]
    ids = _ids(3)
    uses = MHSAAddAtt.TOKEN_TABLE_USES

    def run():
        with torch.no_grad():
            return te(ids)

    b0 = uses["built"]
    outs = [run() for _ in range(5)]                 # 600 positions per forward, V = 2000: the 4th builds, the 5th is served
    assert uses["built"] == b0 + 1 and te._tt_key is not None
    f0 = uses["forwards"]
    run()
    assert uses["forwards"] == f0 + 1               # hit
    w0_ref = _oracle_news(mod, ids)
    assert _maxerr(outs[-1], w0_ref) <= 2e-4
    _write(writer, mod, TE_NAMES, seed=7, trainer=tr, step_batch=_train_batch(33))
    mod.eval()
    first = run()
    later = [run() for _ in range(5)]
    with torch.no_grad():
        plain = _tableless(mod, lambda: te(ids))
    _check_news(first, mod, ids, w0_ref, plain)
    for o in later:
        assert torch.equal(o, plain)


# ---------------------------------------------------------------------------------------------------------------------------
# NrlLinear (both engines) and the fused attention block (bf16x3)
# ---------------------------------------------------------------------------------------------------------------------------
LIN_WRITERS = ["adam", "adam_foreach", "adam_fused", "load_state_dict", "load_state_dict_assign", "data_copy", "data_copy_trainer",
               "replace_param"]


def _grad_of(p):
    g = getattr(p, "main_grad", None)
    return g if g is not None else p.grad


def _live_driver(writer, module, frozen):
    """This library's fused optimizer alive (what an ``NRMSTrainer`` holds: ``FlatParams`` + ``FusedAdam``): owning the trainable
    `module`'s parameters for every writer but `data_copy` (the setting without one), and for a frozen `module` in the
    `data_copy_trainer` cell (then owning another parameter: frozen weights belong to no optimizer)."""
    from newsreclib_amd.trainer import FlatParams, FusedAdam
    if writer == "data_copy" or (frozen and writer != "data_copy_trainer"):
        return None
    flat = FlatParams(module.parameters() if not frozen else [torch.nn.Parameter(torch.zeros(64, device=DEV))])
    return flat, FusedAdam(flat, 1e-3, (0.9, 0.999), 1e-8)


@pytest.mark.parametrize("engine_name", ["bf16x3", "f32"])
@pytest.mark.parametrize("D", [64, 300])
@pytest.mark.parametrize("frozen", [True, False])
@pytest.mark.parametrize("writer", LIN_WRITERS)
def test_nrl_linear_images_follow_the_writer(writer, frozen, D, engine_name):
    """``NrlLinear`` over a frozen weight (``_images``) or a trainable one (``_step_images``, kept only under a live optimizer of
    this library): after the writer the output, the input gradient and (trainable) the weight gradient are the fp64 ones of the new
    weights."""
    from newsreclib_amd import _lib
    from newsreclib_amd.news_encoder import NrlLinear
    if writer in ADAMS and frozen:
        pytest.skip("a frozen weight has no gradient: torch.optim.Adam does not write it")
    if writer == "replace_param" and not frozen:
        pytest.skip("replacing a trainable Parameter under a live optimizer detaches it from the optimizer (not a writer)")
    _lib.set_gemm_engine(engine_name)
    torch.manual_seed(D)
    lin = torch.nn.Linear(D, D).to(DEV)
    nl = NrlLinear(lin)
    del lin
    for p in nl.parameters():
        p.requires_grad_(not frozen)
    drv = _live_driver(writer, nl, frozen)
    cache = nl._images if frozen else nl._step_images
    x = torch.randn(600, D, device=DEV, requires_grad=True)
    g = torch.randn(600, D, device=DEV)

    def run():
        x.grad = None
        for p in nl.parameters():
            p.grad = None
            if getattr(p, "main_grad", None) is not None:
                p.main_grad.zero_()
        y = nl(x)
        y.backward(g)
        return y.detach().clone(), x.grad.clone(), (None if frozen else _grad_of(nl.weight).clone())

    def refs():
        w, b, xd, gd = nl.weight.detach().double(), nl.bias.detach().double(), x.detach().double(), g.double()
        return torch.nn.functional.linear(xd, w, b), gd @ w, gd.t() @ xd

    def tol(r):
        return 1e-4 * float(r.abs().max())

    run()
    y0, dx0, dw0 = run()
    if frozen or drv is not None:
        assert cache._key.get("fwd") is not None and cache._key.get("bwd") is not None     # kept: the second call was served
    r0 = refs()
    assert _maxerr(y0, r0[0]) <= tol(r0[0]) and _maxerr(dx0, r0[1]) <= tol(r0[1])
    _write(writer, nl, ["weight", "bias"], seed=D + 1)
    y1, dx1, dw1 = run()
    r1 = refs()
    assert _maxerr(r0[0], r1[0]) >= 100 * tol(r1[0]) and _maxerr(r0[1], r1[1]) >= 100 * tol(r1[1])
    assert _maxerr(y1, r1[0]) <= tol(r1[0]), _maxerr(y1, r1[0])
    assert _maxerr(dx1, r1[1]) <= tol(r1[1]), _maxerr(dx1, r1[1])
    if not frozen:
        assert _maxerr(dw1, r1[2]) <= tol(r1[2])
    del drv


def _attention_layer(frozen):
    """One roberta-type attention half (D = 256, 4 heads of 64: the fused block's geometry) with the fused forward swapped in."""
    from transformers import RobertaConfig, RobertaModel

    from newsreclib_amd import news_encoder as ne
    cfg = RobertaConfig(vocab_size=100, hidden_size=256, num_hidden_layers=1, num_attention_heads=4, intermediate_size=512,
                        max_position_embeddings=40, type_vocab_size=1, pad_token_id=1, hidden_dropout_prob=0.0,
                        attention_probs_dropout_prob=0.0)
    torch.manual_seed(4)
    body = RobertaModel(cfg, add_pooling_layer=False).to(DEV)
    assert ne.register_body_attention()
    body.config._attn_implementation = ne.NRL_ATTENTION
    assert ne.swap_linears(body.encoder) > 0 and ne.swap_output_blocks(body.encoder) > 0
    assert ne.swap_attention_blocks(body.encoder) == 1
    att = body.encoder.layer[0].attention
    with torch.no_grad():      # (weights at 1 / sqrt(D): the attention branch, not the residual, dominates the output)
        for lin in (att.self.query, att.self.key, att.self.value, att.output.dense):
            lin.weight.normal_(0.0, 256 ** -0.5)
            lin.bias.normal_(0.0, 0.1)
        att.output.LayerNorm.weight.uniform_(0.5, 1.5)
        att.output.LayerNorm.bias.uniform_(-0.3, 0.3)
    for p in att.parameters():
        p.requires_grad_(not frozen)
    return att


ATT_NAMES = ["self.query.weight", "self.query.bias", "self.key.weight", "self.key.bias", "self.value.weight", "self.value.bias",
             "output.dense.weight", "output.dense.bias"]


@pytest.mark.parametrize("frozen", [True, False])
@pytest.mark.parametrize("writer", LIN_WRITERS)
def test_attention_block_images_follow_the_writer(writer, frozen):
    """The fused attention block (``swap_attention_blocks``: q|k|v images in ``_nrl_qkv_images`` / ``_nrl_qkv_step_images``, the
    output projection's in its ``NrlLinear``): after the writer, output and input gradient (and the weight gradients of a trainable
    block) match fp64 torch of the new weights.  bf16x3 only: the fused block does not exist under the exact-fp32 engine."""
    from newsreclib_amd import _lib
    from newsreclib_amd import news_encoder as ne
    if writer in ADAMS and frozen:
        pytest.skip("a frozen weight has no gradient: torch.optim.Adam does not write it")
    if writer == "replace_param" and not frozen:
        pytest.skip("replacing a trainable Parameter under a live optimizer detaches it from the optimizer (not a writer)")
    _lib.set_gemm_engine("bf16x3")
    att = _attention_layer(frozen)
    drv = _live_driver(writer, att, frozen)
    N, Lt, D, H = 6, 40, 256, 4
    x = (0.3 * torch.randn(N, Lt, D, device=DEV)).requires_grad_(True)
    gy = torch.randn(N, Lt, D, device=DEV)
    fb0 = ne.FALLBACK_CALLS["attention_block_cuda"]

    def run():
        x.grad = None
        for p in att.parameters():
            p.grad = None
            if getattr(p, "main_grad", None) is not None:
                p.main_grad.zero_()
        y = att(x)[0]
        y.backward(gy)
        return y.detach().clone(), x.grad.clone(), {n: _grad_of(p).clone() for n, p in att.named_parameters() if not frozen}

    def refs():
        sd = {n: p.detach().double() for n, p in att.named_parameters()}
        xd = x.detach().double().requires_grad_(True)
        ps = {n: t.clone().requires_grad_(not frozen) for n, t in sd.items()}
        lin = lambda t, n: torch.nn.functional.linear(t, ps[n + ".weight"], ps[n + ".bias"])  # noqa: E731
        heads = lambda t: t.view(N, Lt, H, D // H).transpose(1, 2)  # noqa: E731
        a = torch.nn.functional.scaled_dot_product_attention(heads(lin(xd, "self.query")), heads(lin(xd, "self.key")),
                                                             heads(lin(xd, "self.value")))
        ref = torch.nn.functional.layer_norm(lin(a.transpose(1, 2).reshape(N, Lt, D), "output.dense") + xd, (D,),
                                             ps["output.LayerNorm.weight"], ps["output.LayerNorm.bias"],
                                             att.output.LayerNorm.eps)
        ref.backward(gy.double())
        return ref.detach(), xd.grad, {n: t.grad for n, t in ps.items() if not frozen}

    def close(a, b, tol=2e-4):
        return _maxerr(a, b) <= tol * max(1e-6, float(b.abs().max()))

    run()
    y0, dx0, _ = run()
    r0 = refs()
    assert close(y0, r0[0]) and close(dx0, r0[1])
    _write(writer, att, ATT_NAMES, seed=11)
    y1, dx1, dw1 = run()
    r1 = refs()
    assert ne.FALLBACK_CALLS["attention_block_cuda"] == fb0, "the fused block did not run"
    assert _maxerr(r0[0], r1[0]) >= 100 * 2e-4 * float(r1[0].abs().max())
    assert close(y1, r1[0]), _maxerr(y1, r1[0])
    assert close(dx1, r1[1]), _maxerr(dx1, r1[1])
    if not frozen:
        for n in ATT_NAMES:
            if n == "self.key.bias":         # (softmax is shift-invariant: no gradient, rounding noise only)
                continue
            assert close(dw1[n], r1[2][n]), n
    del drv


# ---------------------------------------------------------------------------------------------------------------------------
# LazyTableAdam rows read outside a step; the prefetched lazy-table ids
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reader", ["eval_forward", "news_vector_cache", "state_dict"])
def test_lazy_table_read_outside_a_step_equals_the_dense_trainer(reader):
    """k steps with the lazy table optimizer and k with the dense one; then ONE reader -- an eval-mode forward, a
    ``NewsVectorCache.build`` or ``state_dict()`` -- without a manual flush must see what the dense trainer's module holds
    (the comparison of ``test_trainer_with_lazy_table_adam_tracks_the_dense_trainer``)."""
    from newsreclib_amd import _lib
    from newsreclib_amd.evaluation import DeviceNewsTable, NewsVectorCache
    from newsreclib_amd.trainer import NRMSTrainer
    _lib.set_gemm_engine("bf16x3")
    params = O.make_params(VOCAB, seed=3)
    mods, trs = [], []
    for lazy in (True, False):
        mod = build_module(params, p_drop=0.2, device=DEV)
        te = mod.news_encoder.text_encoders["title"]
        orig = te.forward
        te.forward = (lambda o: (lambda text, seed=None, **kw: o(text, seed=77, **kw)))(orig)
        mods.append(mod)
        trs.append(NRMSTrainer(mod, lr=1e-3, lazy_adam=lazy))
    assert trs[0].lazy is not None and trs[1].lazy is None
    batches = [_train_batch(60 + i) for i in range(6)]
    for b in batches:
        la, lb = float(trs[0].step(dict(b))), float(trs[1].step(dict(b)))
        assert abs(la - lb) <= 2e-5 * max(1.0, abs(lb))
    assert trs[0].lazy.pending
    emb = TE + "embedding_layer.weight"
    if reader == "eval_forward":
        with torch.no_grad():
            ea, eb = (m.eval()(dict(batches[0])).cpu() for m in mods)
        assert _maxerr(ea, eb) <= 3e-4
    elif reader == "news_vector_cache":
        ids = _ids(8, n=100)
        table = DeviceNewsTable({"title": ids.cpu(), "category": torch.ones(100, dtype=torch.int64),
                                 "sentiment": torch.ones(100, dtype=torch.int64)})
        va, vb = (NewsVectorCache(m, table, chunk=64).build().cpu() for m in mods)
        assert _maxerr(va, vb) <= 3e-4
    else:
        wa, wb = (m.state_dict()[emb].cpu() for m in mods)
        d = (wa - wb).abs()
        assert float(d.max()) <= 6 * 2.1e-3 and float((d > 2e-5).float().mean()) <= 0.02
    assert not trs[0].lazy.pending, "the reader must have seen a flushed table"
    # the same rows also through the other route, and fp64 news vectors of the weights the reader saw
    ids = _ids(9)
    mods[0].eval()
    with torch.no_grad():
        got = mods[0].news_encoder.text_encoders["title"](ids)
    assert _maxerr(got, _oracle_news(mods[0], ids)) <= 2e-4


@pytest.mark.parametrize("engine_name", ["bf16x3", "f32"])
def test_prefetched_lazy_ids_are_not_served_for_a_refilled_batch(engine_name, monkeypatch):
    """A multi-attribute text encoder (LSTUR: title + abstract through ONE encoder) concatenates its ids for the lazy table
    optimizer, so the prefetch's ids are a COPY.  A caller that prepares its own batches and refills one of them in place after
    it was announced and consumed must get the rows of the NEW ids: every row they name stands at the current step after the
    update, and the losses follow a trainer run without the prefetch (NRL_PREFETCH_IDS=0)."""
    from newsreclib_amd import _lib
    from newsreclib_amd.synthetic import add_lstur_fields, make_batch
    from newsreclib_amd.trainer import NRMSTrainer
    from oracle.lstur_oracle import make_lstur_params
    from tests.helpers import build_lstur_module
    _lib.set_gemm_engine(engine_name)
    cfg = dict(vocab=VOCAB, n_categ=19, n_users=300, D=64, F=64, W=3, Q=32, categ_dim=32,
               text_attrs=("title", "abstract"), text_order=("title", "abstract"), method="ini", p_drop=0.0, p_mask=0.0)
    params = make_lstur_params(VOCAB, cfg["n_categ"], cfg["n_users"], embed_dim=64, num_filters=64, query_dim=32, categ_dim=32,
                               seed=4)

    def raw(seed):
        return batch_to(add_lstur_fields(make_batch(2, vocab=VOCAB, mode="fixed", seed=seed, H=5), VOCAB, cfg["n_categ"],
                                         cfg["n_users"], 20, seed=seed + 100), DEV)

    def refill(dst, src):
        for k, v in src.items():
            if isinstance(v, dict):
                refill(dst[k], v)
            elif torch.is_tensor(v) and torch.is_tensor(dst.get(k)) and dst[k].shape == v.shape:
                dst[k].copy_(v)

    results = {}
    for mode in ("plain", "prefetch"):
        if mode == "plain":
            monkeypatch.setenv("NRL_PREFETCH_IDS", "0")
        else:
            monkeypatch.delenv("NRL_PREFETCH_IDS", raising=False)
        mod = build_lstur_module(cfg, params)
        tr = NRMSTrainer(mod, lr=1e-3)
        assert tr.lazy is not None
        b = [mod._prepare(raw(70 + i)) for i in range(4)]
        assert all(mod._prepare(x) is x for x in b)           # a prepared dict comes back as it is
        losses = [float(tr.step(b[3]))]                          # b3's rows get moments, then lag
        losses.append(float(tr.step(b[0], b[1])))                # b1 announced ...
        losses.append(float(tr.step(b[1])))                     # ... and consumed
        refill(b[1], mod._prepare(raw(73)))                      # the caller reuses b1's buffers for b3's content
        losses.append(float(tr.step(b[1])))
        ids = tr.lazy_tables[0][1](b[1])
        assert bool((tr.lazy.last[ids] == tr.opt.step_count).all()), "rows of the refilled batch were not brought to the step"
        assert "_lazy_ids" not in b[1]
        tr.flush()
        torch.cuda.synchronize()
        results[mode] = (losses, tr.flat.flat.clone())
    for a, c in zip(results["plain"][0], results["prefetch"][0]):
        assert abs(a - c) <= 1e-5 * max(1.0, abs(a)), (results["plain"][0], results["prefetch"][0])
    assert _maxerr(results["plain"][1], results["prefetch"][1]) <= 2.1e-3 * 4
