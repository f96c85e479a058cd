"""Op-level shape sweep of the ops under LSTUR, NAML, TANR, CenNewsRec and MINS against a float64 evaluation of their CPU
restatements, each op through its autograd Function: ``CnnEncoderFn``, ``GruFn``, ``EmbeddingRowsFn`` (ops_lstur.py),
``AdditiveAttentionFn`` and ``LinearActFn`` (ops_blocks.py), under both GEMM engines.  Inputs, case tables and references:
tests/sweep_inputs_lstur_naml.py; the coverage of the tables, the exactness of the grid-valued ReLU gate inputs and the
float32 yardstick are asserted on the host in tests/test_lstur_naml_sweep_host.py.  Branches reached (each is named in a case
id or in the comment above its case table):

* CNN encoder (nrl_api_lstur.hip): the convolution on planes (W = 3, L <= 63, F <= 320) and off it, its k-tiles at L = 31 /
  32, the row-panel kernel (D, F, Q <= 320) at its three image widths (208 / 212, 304 / 308) and off it, the additive
  attention on planes (F % 16 == 12, F <= 304, Q <= 224) and off it for each reason, the cleared last 32-row tile (M % 32),
  the even padding of the x and dc plane blocks, W = 1, 5, 7 with windows wider than the title, the live-row table gradient
  with no padding id, a whole padded title, only padding ids, more than 2048 news, and one short title -- shapes whose
  backward was refused for want of room for the live-row list until the buffer was sized for the list;
* GRU (nrl_gru_fused.h, ``nrl_gru_fwd``): the unit clamp and the k-tail loads (Hd = 4 .. 36), a wave's second k-tile slot, all
  24 slots, TR 1 -> 2 at 512, the row clamp on both sides of the 16 / 32-row tiles, workgroup counts 1, 7, 8, 9, 17, 18 through
  the XCD remapping (an unwritten tile of h_t is NaN from the poisoned pool), the two-launch forward at Hd = 772 under bf16x3,
  the weight-gradient kernel switch at 3 Hd > 512, T = 1, all lengths 1, all lengths T;
* pooling kernels (``pool_fwd_kernel``, ``pool_bwd_pre_kernel``): row-groups 256, 85, 3, 1 in both, idle threads beside
  RG = 1 (D = 1020), the second column pass (D = 1028), 1, 2 and 4 ``accq`` slots, S on both sides of 16 and 64 and at 8192,
  the backward grid at 2047, 2048 and 2049 groups (persistent above 2048); 256 < Q <= 512 (Q = 300 here, 320 and 324 in the
  CNN cases), where the flush of the query gradient used to leave ``dq_a[256:]`` at zero;
* ``LinearActFn``: the q-tile limits (208 under f32, 224 under bf16x3), the weight-gradient switch at N > 512, M = 0, a null
  ``d_a``; ``EmbeddingRowsFn``: n = 0, 1, 300, one hot row, only the padding id.

Bounds are the project's own: ``Report.fwd`` / ``Report.grad``; the CNN encoder's forward, whose outputs reach ~70 on grid
inputs, the bound of ``test_cnn_encoder_matches_oracle`` (ftol max(1, |want|_max)) through ``Report.bound``; a case above the
width a bound was set at (Hd > 700, D or Q > 400 in the pooling kernels, N > 400 or K > 100 in ``LinearActFn``) the larger of
the project's number and 4x the float32 oracle's own error, through ``Report.bound``.  Every comparison prints a ``SWEEP``
line (``tools/sweep_errors.py --tests lstur_naml`` collects them into profiles/lstur_naml_sweep_errors.txt).

Not swept here: the environment switches (``NRL_CONV_*``, ``NRL_GRU_PERSISTENT``: read once per process, each has its
subprocess test in tests/test_gpu_lstur.py), ``CnnMhsaEncoderFn``, ``MhaFn`` and the MINS / CenNewsRec user encoders."""
import pytest
import torch

from tests import sweep_inputs_lstur_naml as S
from tests.sweep_inputs import Report

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(autouse=True, params=["f32", "bf16x3"])
def engine(request):
    from newsreclib_amd import _lib
    prev = _lib.get_gemm_engine()
    _lib.set_gemm_engine(request.param)
    yield request.param
    _lib.set_gemm_engine(prev)


def _ids(cases):
    return [c["name"] for c in cases]


def _leaf(x):
    return x.to(DEV).requires_grad_(True)


def _refs(family, index):
    return S.cached(family, index, "float64"), S.cached(family, index, "float32")


def _fwd(rep, wide, what, got, want, want32):
    if wide:
        rep.bound(what, got, want, want32, 5 * rep.ftol)
    else:
        rep.fwd(what, got, want, want32)


def _grad(rep, wide, what, got, want, want32):
    if wide:
        rep.bound(what, got, want, want32, rep.gtol, rel=True)
    else:
        rep.grad(what, got, want, want32)


def _zero(t):
    return t.numel() == 0 or float(t.detach().abs().max()) == 0.0


# ---- CNN text encoder -------------------------------------------------------------------------------------------------------
# every case with the module's counting sort (order=None); the ``mixed`` cases also with an external argsort
CNN_PARAMS = [(i, o) for i, c in enumerate(S.CNN_CASES) for o in (("sort", "argsort") if c["ids"] == "mixed" else ("sort",))]


@pytest.mark.parametrize("index,order", CNN_PARAMS, ids=[f"{S.CNN_CASES[i]['name']}-{o}" for i, o in CNN_PARAMS])
def test_cnn_encoder_sweep(index, order, engine):
    """The ``tiny_*`` cases are one short title.  Under bf16x3 the backward of (L, Q) = (1, 4), (1, 8), (2, 4) and (4, 4) used to
    be refused with ``cnn_encoder_bwd: scratch for the live-row list`` after the forward had accepted the shape."""
    from newsreclib_amd.ops_lstur import CnnEncoderFn
    case, inp = S.CNN_CASES[index], S.cached_inputs("cnn", index)
    r64, r32 = _refs("cnn", index)
    rep = Report("cnn_encoder", f"{case['name']}/{order}", engine)
    ids = inp["ids"].to(DEV)
    dev = [_leaf(inp["params"][k]) for k in S.CNN_KEYS]
    ext = torch.argsort(ids.reshape(-1)) if order == "argsort" else None
    out = CnnEncoderFn.apply(ids, *dev, case["p"], S.DROP_SEED, S.STREAM0, None, ext)
    out.backward(inp["d_out"].to(DEV))
    rep.bound("out", out, r64["out"], r32["out"], rep.ftol, rel=True)
    for k, t in zip(S.CNN_KEYS, dev):
        rep.grad("d_" + k, t.grad, r64["grads"][k], r32["grads"][k])
    rep.check("the padding row of the table gradient is exactly 0", _zero(dev[0].grad[0]))
    if case["ids"] == "all_pad":
        rep.check("only padding ids: the table gradient is exactly 0", _zero(dev[0].grad))
    rep.done()


# ---- GRU --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", range(len(S.GRU_CASES)), ids=_ids(S.GRU_CASES))
def test_gru_sweep(index, engine):
    from newsreclib_amd.ops_lstur import GruFn
    case, inp = S.GRU_CASES[index], S.cached_inputs("gru", index)
    r64, r32 = _refs("gru", index)
    rep = Report("gru", case["name"], engine)
    dev = {k: _leaf(inp[k]) for k in S.GRU_KEYS}
    out = GruFn.apply(dev["hist"], inp["lengths"].to(DEV), dev["h0"] if case["with_h0"] else None,
                      *(dev[k] for k in S.GRU_KEYS[2:]), None)
    out.backward(inp["d_out"].to(DEV))
    _fwd(rep, case["wide"], "out", out, r64["out"], r32["out"])
    for k in S.GRU_KEYS:
        if k == "h0" and not case["with_h0"]:
            continue
        _grad(rep, case["wide"], "d_" + k, dev[k].grad, r64["d_" + k], r32["d_" + k])
    pad = torch.arange(case["T"])[None, :] >= inp["lengths"][:, None]
    rep.check("d_hist past a sequence's length is exactly 0", _zero(dev["hist"].grad.cpu()[pad]))
    rep.done()


# ---- additive attention -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", range(len(S.AA_CASES)), ids=_ids(S.AA_CASES))
def test_additive_attention_sweep(index, engine):
    from newsreclib_amd.ops_blocks import AdditiveAttentionFn
    case, inp = S.AA_CASES[index], S.cached_inputs("aa", index)
    r64, r32 = _refs("aa", index)
    rep = Report("additive_attention", case["name"], engine)
    dev = {k: _leaf(inp[k]) for k in S.AA_KEYS}
    out = AdditiveAttentionFn.apply(*(dev[k] for k in S.AA_KEYS), None)
    out.backward(inp["d_out"].to(DEV))
    _fwd(rep, case["wide"], "out", out, r64["out"], r32["out"])
    for k in S.AA_KEYS:
        _grad(rep, case["wide"], "d_" + k, dev[k].grad, r64["d_" + k], r32["d_" + k])
    if case["G"] == 0:
        rep.check("no group: an empty output", tuple(out.shape) == (0, case["D"]) and tuple(dev["y"].grad.shape) == (0, case["S"], case["D"]))
        rep.check("no group: parameter gradients exactly 0", all(_zero(dev[k].grad) for k in ("w", "b", "q")))
    rep.done()


def _aa_args(G, S_, D, Q):
    g = torch.Generator().manual_seed(11)
    return [_leaf(torch.randn(s, generator=g) * 0.3) for s in ((G, S_, D), (Q, D), (Q,), (Q,))]


def test_additive_attention_refuses_S8193():
    """Refused by the FORWARD (``addatt_check``: S <= 8192, the softmax row in dynamic LDS), before any launch."""
    from newsreclib_amd.ops_blocks import AdditiveAttentionFn
    with pytest.raises(RuntimeError, match="bad additive-attention shape"):
        AdditiveAttentionFn.apply(*_aa_args(1, 8193, 4, 4), None)


def test_additive_attention_refuses_Q4100():
    """Q = 4100 needs a fifth ``accq`` slot.  The forward has no such limit and runs; the BACKWARD is refused by
    ``pool_bwd_pre`` on the host, before its first launch."""
    from newsreclib_amd.ops_blocks import AdditiveAttentionFn
    out = AdditiveAttentionFn.apply(*_aa_args(1, 2, 4, 4100), None)
    assert tuple(out.shape) == (1, 4) and bool(torch.isfinite(out).all())
    with pytest.raises(RuntimeError, match="query_dim > 4096 unsupported"):
        out.sum().backward()


# ---- linear + activation ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", range(len(S.LIN_CASES)), ids=_ids(S.LIN_CASES))
def test_linear_act_sweep(index, engine):
    """``relu`` cases are grid-valued: the kernel's gates are the reference's, so the gradients are compared as they are."""
    from newsreclib_amd.ops_blocks import LinearActFn
    case, inp = S.LIN_CASES[index], S.cached_inputs("lin", index)
    r64, r32 = _refs("lin", index)
    rep = Report("linear_act", case["name"], engine)
    a = _leaf(inp["a"]) if case["need_da"] else inp["a"].to(DEV)
    w, b = _leaf(inp["w"]), _leaf(inp["b"])
    out = LinearActFn.apply(a, w, b, case["act"], None)
    out.backward(inp["d_c"].to(DEV))
    wide = case["wide"]
    _fwd(rep, wide, "out", out, r64["out"], r32["out"])
    if case["act"] == "relu":
        rep.check("the gates are the reference's", torch.equal(out.detach().cpu() > 0, r64["out"] > 0))
    if case["need_da"]:
        _grad(rep, wide, "d_a", a.grad, r64["d_a"], r32["d_a"])
    else:
        rep.check("no gradient for an input that needs none", a.grad is None)
    _grad(rep, wide, "d_w", w.grad, r64["d_w"], r32["d_w"])
    _grad(rep, wide, "d_b", b.grad, r64["d_b"], r32["d_b"])
    if case["M"] == 0:
        rep.check("no row: an empty output", tuple(out.shape) == (0, case["N"]) and tuple(a.grad.shape) == (0, case["K"]))
        rep.check("no row: d_w and d_b exactly 0", _zero(w.grad) and _zero(b.grad))
    rep.done()


# ---- embedding rows ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", range(len(S.EMB_CASES)), ids=_ids(S.EMB_CASES))
def test_embedding_rows_sweep(index, engine):
    from newsreclib_amd.ops_lstur import EmbeddingRowsFn
    case, inp = S.EMB_CASES[index], S.cached_inputs("emb", index)
    r64, r32 = _refs("emb", index)
    rep = Report("embedding_rows", case["name"], engine)
    table = _leaf(inp["table"])
    out = EmbeddingRowsFn.apply(inp["ids"].to(DEV), table, case["p"], S.DROP_SEED, S.EMB_STREAM, None)
    out.backward(inp["d_out"].to(DEV))
    rep.fwd("out", out, r64["out"], r32["out"])
    rep.check("out equals the float32 restatement bit for bit (x * {0, 1, 2})", torch.equal(out.detach().cpu(), r32["out"]))
    rep.grad("d_table", table.grad, r64["d_table"], r32["d_table"])
    rep.check("the padding row of the table gradient is exactly 0", _zero(table.grad[0]))
    if case["n"] == 0 or case["ids"] == "all_zero":
        rep.check("no live id: the table gradient is exactly 0", _zero(table.grad))
    if case["n"] == 0:
        rep.check("no id: an empty output", tuple(out.shape) == (0, case["D"]))
    rep.done()
