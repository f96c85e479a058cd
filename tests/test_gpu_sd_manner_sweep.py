"""Op-level shape sweep of the SentiDebias head (nrl_sentidebias.hip) and of the MANNeR kernels (nrl_manner.hip) against a
float64 evaluation of their CPU restatements (tests/sentidebias_oracle.py, tests/manner_oracle.py), each op through its
autograd Function / entry point in ops_sentidebias.py and ops_manner.py: the float4 lane loops at D / 4 = 1, 63, 64, 65, the
register arrays at 1, 2, 3, 4 and 8 classes, slabs of 64 rows at 63, 64, 65 and 129 rows with the history / candidate split
at 0, 1, N - 1, N and inside a wave stride, more than 64 history rows and candidates per user, empty histories and candidate
lists, ids outside the table, every padding of the discriminator slab, the 48 KiB of LDS bins filled exactly (one step over
it is refused on the host), the scorer's register slots up to max_cand = 2048, its index clamp and its degenerate rows, the
SupCon pad kernel at each N % 4 and a second chunk of 4 columns.

The inputs come from tests/sweep_inputs_sd_manner.py; their conditions are asserted on the host in
tests/test_sd_manner_sweep_host.py.  Bounds: the project's own (test_kernels_against_float64), or 4x the float32 CPU
restatement's error against float64 at the case where that is larger; the MANNeR ops keep their rule of 4x the torch-fp32
error (x3 for SupCon under bf16x3).  Every comparison prints a ``SWEEP`` line (tools/sweep_errors.py collects them into
profiles/sd_manner_sweep_errors.txt)."""
import pytest
import torch

from tests import sweep_inputs_sd_manner as S
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


# ---- SentiDebias ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", range(len(S.ROWCOS_CASES)), ids=_ids(S.ROWCOS_CASES))
def test_sd_rowcos_sweep(index, engine):
    from newsreclib_amd import ops_sentidebias as SD
    case, inp = S.ROWCOS_CASES[index], S.cached_inputs("rowcos", index)
    r64, r32 = _refs("rowcos", index)
    rep = Report("sd_rowcos", case["name"], engine)
    ids, w = inp["ids"].to(DEV), inp["w"].to(DEV)

    def run():
        news, T = _leaf(inp["news"]), _leaf(inp["T"])
        out = SD.RowCosFn.apply(news, T, ids, case["n_hist"])
        (out * w).sum().backward()
        return out, news.grad, T.grad

    out, d_news, d_T = run()
    rep.bound("out", out, r64["out"], r32["out"], S.COS_VALUE)
    if case["special"] == "zero_row":
        # the forward of the all-zero row is 0 and its gradient g T[id] / 1e-8: compared on its own, so that its size does
        # not loosen the bound of the other rows
        z, rest = S.ZERO_ROW, torch.arange(case["N"]) != S.ZERO_ROW
        rep.bound("d_news (zero row)", d_news[z], r64["d_news"][z], r32["d_news"][z], S.COS_DNEWS, rel=True)
        rep.bound("d_news (other rows)", d_news.cpu()[rest], r64["d_news"][rest], r32["d_news"][rest], S.COS_DNEWS, rel=True)
    else:
        rep.bound("d_news", d_news, r64["d_news"], r32["d_news"], S.COS_DNEWS, rel=True)
    rep.bound("d_T", d_T, r64["d_T"], r32["d_T"], S.D_TABLE, rel=True)
    if case["special"] == "bad_ids":
        rep.check("d_news of a row with an id outside the table is exactly 0", bool((d_news[list(S.BAD_ROWS)] == 0).all()))
    if case["n_hist"] in (0, case["N"]):
        rep.check("the mean of the empty side is exactly 0", float(out.detach()[0 if case["n_hist"] == 0 else 1]) == 0.0)
    rep.check("d_T bit-identical over two runs", torch.equal(run()[2], d_T))
    rep.done()


@pytest.mark.parametrize("index", range(len(S.HIST_CASES)), ids=_ids(S.HIST_CASES))
def test_sd_dense_history_sweep(index, engine):
    from newsreclib_amd import ops_sentidebias as SD
    case, inp = S.HIST_CASES[index], S.cached_inputs("hist", index)
    r64, r32 = _refs("hist", index)
    rep = Report("sd_hist", case["name"], engine)
    ids, off, g = inp["ids"].to(DEV), inp["off"].to(DEV), inp["d_dense"].to(DEV)

    def run():
        T = _leaf(inp["T"])
        dense = SD.SentHistFn.apply(T, ids, off, case["B"], case["H"])
        dense.backward(g)
        return dense.detach(), T.grad

    dense, d_T = run()
    # (the float64 gather cast to float: bit for bit, the zeros of the padded slots and of the skipped ids included)
    rep.check("dense == float64 gather cast to float, bit for bit", torch.equal(dense.cpu(), r64["dense"].float()))
    pad = torch.arange(case["H"]).unsqueeze(0) >= torch.tensor(case["hs"]).unsqueeze(1)
    rep.check("padded slots are exactly 0", bool((dense.cpu()[pad] == 0).all()))
    rep.bound("d_T", d_T, r64["d_T_dense"], r32["d_T_dense"], S.D_TABLE, rel=True)
    rep.check("d_T bit-identical over two runs", torch.equal(run()[1], d_T))
    rep.done()


@pytest.mark.parametrize("index", range(len(S.HIST_CASES)), ids=_ids(S.HIST_CASES))
def test_sd_late_fusion_sweep(index, engine):
    from newsreclib_amd import ops_sentidebias as SD
    case, inp = S.HIST_CASES[index], S.cached_inputs("hist", index)
    r64, r32 = _refs("hist", index)
    rep = Report("sd_late", case["name"], engine)
    ids, off = inp["ids"].to(DEV), inp["off"].to(DEV)
    empty = torch.tensor([n == 0 for n in case["hs"]])
    if bool(empty.any()):
        # an empty history is the reference's 0 / 0: a NaN row, pinned forward only (its gradient is NaN by the same division)
        with torch.no_grad():
            u = SD.LateUserFn.apply(inp["T"].to(DEV), ids, off, case["B"]).cpu()
        rep.check("an empty history gives a NaN row", bool(torch.isnan(u[empty]).all()))
        rep.bound("u", u[~empty], r64["u"][~empty], r32["u"][~empty], S.LATE_U)
        rep.done()
        return

    def run():
        T = _leaf(inp["T"])
        u = SD.LateUserFn.apply(T, ids, off, case["B"])
        u.backward(inp["d_u"].to(DEV))
        return u.detach(), T.grad

    u, d_T = run()
    rep.bound("u", u, r64["u"], r32["u"], S.LATE_U)
    rep.bound("d_T", d_T, r64["d_T_late"], r32["d_T_late"], S.D_TABLE, rel=True)
    rep.check("d_T bit-identical over two runs", torch.equal(run()[1], d_T))
    rep.done()


@pytest.mark.parametrize("index", range(len(S.SCORE_CASES)), ids=_ids(S.SCORE_CASES))
def test_sd_combined_scores_sweep(index, engine):
    from newsreclib_amd import ops_sentidebias as SD
    case, inp = S.SCORE_CASES[index], S.cached_inputs("scores", index)
    r64, r32 = _refs("scores", index)
    rep = Report("sd_scores", case["name"], engine)
    ids, off = inp["ids"].to(DEV), inp["off"].to(DEV)

    def run():
        free, u, T = _leaf(inp["free"]), _leaf(inp["u"]), _leaf(inp["T"])
        out = SD.CombinedScoresFn.apply(free, u, T, ids, off)
        out.backward(inp["d_out"].to(DEV))
        return out.detach(), free.grad, u.grad, T.grad

    out, d_free, d_u, d_T = run()
    rep.bound("out", out, r64["out"], r32["out"], S.SCORES)
    rep.check("padded slots equal `free` exactly", torch.equal(out.cpu()[~inp["mask"]], inp["free"][~inp["mask"]]))
    for name, got in (("d_free", d_free), ("d_u", d_u), ("d_T", d_T)):
        rep.bound(name, got, r64[name], r32[name], S.SCORES_GRAD, rel=True)
    rep.check("d_T bit-identical over two runs", torch.equal(run()[3], d_T))
    rep.done()


@pytest.mark.parametrize("mode", list(S.DISC_MODES))
@pytest.mark.parametrize("index", range(len(S.DISC_CASES)), ids=_ids(S.DISC_CASES))
def test_sd_discriminator_sweep(index, mode, engine):
    """``requires_grad`` decides what is computed: phase G of the adversarial step asks for the gradient of the news rows and
    no weight gradient, phase D for the reverse; each is compared with float64."""
    from newsreclib_amd import ops_sentidebias as SD
    case, inp = S.DISC_CASES[index], S.cached_inputs("disc", index)
    r64, r32 = _refs("disc", index)
    rep = Report("sd_disc", f"{case['name']}/{mode}", engine)
    need_x, need_w = S.DISC_MODES[mode]
    tol = S.DISC[engine]
    x = inp["x"].to(DEV).requires_grad_(need_x)
    p = {k: inp[k].to(DEV).requires_grad_(need_w) for k in S.DISC_KEYS}
    out = SD.DiscriminatorLossFn.apply(x, *(p[k] for k in S.DISC_KEYS), inp["ids"].to(DEV), case["n_hist"])
    (out * inp["w"].to(DEV)).sum().backward()
    rep.bound("out", out, r64["out"], r32["out"], tol, rel=True)
    if need_x:
        rep.bound("d_x", x.grad, r64["d_x"], r32["d_x"], tol, rel=True)
    else:
        rep.check("no activation gradient in phase D", x.grad is None)
    for k in S.DISC_KEYS:
        if need_w:
            rep.bound("d_" + k, p[k].grad, r64["d_" + k], r32["d_" + k], tol, rel=True)
        else:
            rep.check(f"no gradient of {k} in phase G", p[k].grad is None)
    if case["O"] == 1:
        grads = [t.grad for t in [x] + list(p.values()) if t.grad is not None]
        rep.check("one output: loss and gradients exactly 0", float(out.abs().max()) == 0.0 and
                  all(float(g.abs().max()) == 0.0 for g in grads))
    rep.done()


# ---- MANNeR -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", range(len(S.MANNER_CASES)), ids=_ids(S.MANNER_CASES))
def test_manner_scores_sweep(index, engine):
    from newsreclib_amd.ops_manner import manner_scores
    case, inp = S.MANNER_CASES[index], S.cached_inputs("manner", index)
    r64, r32 = _refs("manner", index)
    rep = Report("manner_scores", case["name"], engine)
    e32, _ = S.manner_errors(case, inp, r64, r32)
    bound = 4 * e32                                          # the rule of tests/test_gpu_manner.py, from the oracle alone
    off = lambda sizes: torch.tensor([0] + torch.tensor(sizes).cumsum(0).tolist(), device=DEV)  # noqa: E731
    out = manner_scores([t.to(DEV) for t in inp["tables"]], inp["weights"], torch.cat(inp["raw_hist"]).to(DEV), off(case["hs"]),
                        torch.cat(inp["raw_cand"]).to(DEV), off(case["cs"]), case["max_cand"]).cpu()
    rep.check("shape", out.shape == (len(case["hs"]), case["max_cand"]))
    for b, kind in enumerate(inp["kinds"]):
        n = case["cs"][b]
        rep.check(f"row {b}: padded slots are exactly 0", bool((out[b, n:] == 0).all()))
        if kind == "nan":
            rep.check(f"row {b}: every real slot is NaN", bool(torch.isnan(out[b, :n]).all()))
        elif kind == "real":
            rep.within(f"row {b} (hist {case['hs'][b]}, cand {n})", out[b, :n], r64["rows"][b], r32["rows"][b], bound)
    rep.done()


@pytest.mark.parametrize("index", range(len(S.SUPCON_CASES)), ids=_ids(S.SUPCON_CASES))
def test_supcon_embed_sweep(index, engine):
    from newsreclib_amd.ops_manner import supcon_embed_fwd_bwd
    case, inp = S.SUPCON_CASES[index], S.cached_inputs("supcon", index)
    r64, r32 = _refs("supcon", index)
    rep = Report("supcon", case["name"], engine)
    E, labels, T = inp["E"].to(DEV), inp["labels"].to(DEV), case["T"]
    loss, dE = supcon_embed_fwd_bwd(E, labels, T)
    f = 4.0 * (3.0 if engine == "bf16x3" else 1.0)           # the rule of tests/test_gpu_manner.py
    e_loss = abs(float(r32["loss"]) - float(r64["loss"]))
    e_grad = float((r32["grad"].double() - r64["grad"]).abs().max())
    rep.within("loss", loss.reshape(1), r64["loss"].reshape(1), r32["loss"].reshape(1), f * e_loss)
    rep.within("dE", dE, r64["grad"], r32["grad"], f * e_grad)
    if case["labels"] is not None:
        rep.check("exactly 0", float(loss) == 0.0 and float(dE.abs().max()) == 0.0)
    loss2, dE2 = supcon_embed_fwd_bwd(E, labels, T)
    rep.check("bit-identical over two runs", torch.equal(loss, loss2) and torch.equal(dE, dE2))
    _, dE4 = supcon_embed_fwd_bwd(E, labels, T, grad_scale=4.0)
    rep.check("grad_scale scales dE linearly", torch.allclose(dE4, 4.0 * dE, rtol=1e-6, atol=0.0))
    rep.done()


# ---- refused on the host, before any launch: each refusal is the last thing its test does -----------------------------------
def test_sd_rowcos_bwd_refuses_bins_over_48k(engine):
    from newsreclib_amd import ops_sentidebias as SD
    g = torch.Generator().manual_seed(1)
    news, T = _leaf(torch.randn(5, 388, generator=g)), _leaf(torch.tanh(torch.randn(8, 388, generator=g)))
    out = SD.RowCosFn.apply(news, T, torch.arange(5, device=DEV), 2)
    with pytest.raises(RuntimeError, match="exceeds the LDS bins"):
        out.sum().backward()


def test_sd_hist_bwd_refuses_bins_over_48k(engine):
    from newsreclib_amd import ops_sentidebias as SD
    T = _leaf(torch.tanh(torch.randn(8, 388, generator=torch.Generator().manual_seed(2))))
    dense = SD.SentHistFn.apply(T, torch.arange(5, device=DEV), torch.tensor([0, 2, 5], device=DEV), 2, 3)
    with pytest.raises(RuntimeError, match="exceeds the LDS bins"):
        dense.sum().backward()


def test_sd_disc_bwd_refuses_bins_over_48k(engine):
    from newsreclib_amd import ops_sentidebias as SD
    g = torch.Generator().manual_seed(3)
    Hd, O, D = 384, 8, 12
    x = torch.randn(5, D, generator=g).to(DEV)
    p = [_leaf(torch.randn(s, generator=g) * 0.1) for s in ((Hd, D), (Hd,), (O, Hd), (O,))]
    out = SD.DiscriminatorLossFn.apply(x, *p, torch.arange(5, device=DEV), 2)
    with pytest.raises(RuntimeError, match="exceeds the LDS bins"):
        out.sum().backward()


def test_manner_scores_refuses_max_cand_2049(engine):
    from newsreclib_amd.ops_manner import manner_scores
    table = torch.randn(8, 4, generator=torch.Generator().manual_seed(4)).to(DEV)
    off = torch.tensor([0, 2], device=DEV)
    idx = torch.tensor([0, 1], device=DEV)
    with pytest.raises((ValueError, RuntimeError), match="max_cand"):
        manner_scores([table], [1.0], idx, off, idx, off, 2049)
