"""Input generators and float64 / float32 CPU references of the NPA / DKN op-level shape sweep
(tests/test_gpu_npa_dkn_sweep.py); their properties are asserted on the host in tests/test_npa_host.py and
tests/test_dkn_host.py, and the ``Report`` helper every sweep file prints and asserts through (the SentiDebias / MANNeR
generators are in tests/sweep_inputs_sd_manner.py).  Plain module: no fixtures, no GPU.

Two constructions make a ReLU or arg-max decision the same in fp32 and in float64 ("Shape sweeps against
float64"):

* grid-valued gate inputs (NPA): table entries are multiples of 1/8, weights multiples of 1/16 in [-1/2, 1/2], biases
  k/128 + 1/256.  Every product is a multiple of 1/128 and every partial sum of up to 1536 of them stays below 2^24 / 256,
  so a pre-activation is exact in fp32 in any summation order and under the bf16x3 engine (the operands have at most
  5 significant bits: the low plane is zero), is an odd multiple of 1/256 -- never zero, |z| >= 1/256 -- and a dropout
  multiplier of 2 (p = 0.5) keeps all of that.
* the fragile-output mask (DKN, where tanh sits in front of the convolution): a pooled output whose top-two gap over time,
  or whose |max|, is below 10x the engine's forward tolerance in the float64 oracle gets d_out = 0 on both sides; at most
  2 % of a case's pooled outputs may be fragile, which the committed seeds meet."""
from __future__ import annotations

import functools

import numpy as np
import torch
import torch.nn.functional as F

from oracle.nrms_oracle import dropout_multiplier, to_dense_batch
from tests import dkn_oracle as DO
from tests import npa_oracle as NO

TOL = {"f32": (2e-5, 2e-4), "bf16x3": (1e-4, 5e-4)}      # (forward, gradient): the project's own, as test_gpu_shapes.py
DROP_SEED = 1234
FRAGILE_CAP = 0.02


def grid(rng, shape, step, lim):
    k = int(round(lim / step))
    return torch.from_numpy((rng.integers(-k, k + 1, shape) * step).astype(np.float32))


def grid_bias(rng, n):
    return torch.from_numpy((rng.integers(-16, 17, n) / 128.0 + 1.0 / 256.0).astype(np.float32))


def normal(rng, shape, scale):
    return torch.from_numpy((rng.standard_normal(shape) * scale).astype(np.float32))


def _split(n, parts):
    """n rows over `parts` owners, uneven, every owner at least one row when n >= parts."""
    base = [n // parts] * parts
    base[0] += n - sum(base)
    if parts > 2 and base[1] > 1:
        base[1] -= 1
        base[2] += 1
    return base


def _offsets(counts):
    return torch.tensor([0] + list(np.cumsum(counts)), dtype=torch.int64)


def _leaf(t, dtype):
    return t.to(dtype).clone().requires_grad_(True)


# ---- the printed comparison of every sweep file (tests/test_gpu_npa_dkn_sweep.py, tests/test_gpu_sd_manner_sweep.py) ----------
class Report:
    """Prints every figure of a case, then asserts them all."""

    def __init__(self, family, case, engine):
        self.tag, self.engine, self.bad = f"{family}/{case}", engine, []
        self.ftol, self.gtol = TOL[engine]

    def _line(self, what, got, want, want32, tol):
        got = got.detach().cpu().double()
        err = float((got - want).abs().max()) if want.numel() else 0.0
        e32 = float((want32.double() - want).abs().max()) if want.numel() else 0.0
        ok = err <= tol and bool(torch.isfinite(got).all())
        print(f"SWEEP {self.tag} {self.engine} {what}: kernel {err:.3e} oracle32 {e32:.3e} tol {tol:.3e}" + ("" if ok else " FAIL"))
        if not ok:
            self.bad.append((what, err, tol))

    def fwd(self, what, got, want, want32):
        self._line(what, got, want, want32, 5 * self.ftol)

    def grad(self, what, got, want, want32):
        self._line(what, got, want, want32, self.gtol * max(1.0, float(want.abs().max()) if want.numel() else 0.0))

    def bound(self, what, got, want, want32, tol, rel=False):
        """A bound set at the configured shape, carried to a wider one: the larger of the project's number (times
        max(1, |want|_max) when ``rel``) and 4x the float32 CPU oracle's own error against float64 at this case."""
        scale = max(1.0, float(want.abs().max()) if want.numel() else 0.0) if rel else 1.0
        e32 = float((want32.double() - want).abs().max()) if want.numel() else 0.0
        self._line(what, got, want, want32, max(tol * scale, 4 * e32))

    def within(self, what, got, want, want32, tol):
        """A bound the caller derived from the float32 oracle's error alone."""
        self._line(what, got, want, want32, tol)

    def check(self, what, ok):
        if not ok:
            print(f"SWEEP {self.tag} {self.engine} {what}: FAIL")
            self.bad.append((what,))

    def done(self):
        assert not self.bad, (self.tag, self.engine, self.bad)


# ---- NPA text encoder -------------------------------------------------------------------------------------------------------
def _enc(name, N, L, D, F_, layout, p, seed):
    return dict(name=name, N=N, L=L, D=D, F=F_, layout=layout, p=p, seed=seed)


_LAY = ["module", "one", "gaps"]
NPA_ENCODER_CASES = (
    # every float4-chunk count of the pooling kernels and both sides of 256/260 and 512/516, at two embedding widths
    [_enc(f"F{f}_D{d}", 9 + i % 3, 7, d, f, _LAY[(i + j) % 3], (0.0, 0.5)[(i + j) % 2], 100 + 10 * i + j)
     for i, f in enumerate([4, 64, 256, 260, 516, 772, 1024]) for j, d in enumerate([8, 48])]
    # fewer tokens than waves, exactly one round, one more, many
    + [_enc(f"L{l}", 10, l, 48, 64, _LAY[i % 3], (0.5, 0.0)[i % 2], 300 + i) for i, l in enumerate([1, 2, 3, 4, 5, 30])]
    + [_enc("full", 12, 30, 300, 400, "module", 0.5, 400)])
NPA_RANDOM_CASE = _enc("random", 11, 30, 48, 260, "module", 0.0, 401)     # no grid: forward only


def npa_encoder_inputs(case, grid_valued=True):
    N, L, D, F_ = case["N"], case["L"], case["D"], case["F"]
    rng = np.random.default_rng(case["seed"])
    V = 29
    ids = rng.integers(0, V, (N, L))
    ids[0, 0] = 0                                   # the padding id takes part like any other row of the table
    ids[N - 1, L - 1] = 0
    if grid_valued:
        emb, w, b = grid(rng, (V, D), 1 / 8, 1.0), grid(rng, (F_, D, 3), 1 / 16, 0.5), grid_bias(rng, F_)
    else:
        emb, w, b = normal(rng, (V, D), 0.3), normal(rng, (F_, D, 3), (3 * D) ** -0.5), normal(rng, F_, 0.05)
    if case["layout"] == "one":                     # one query owns every row
        counts = [N]
    elif case["layout"] == "gaps":                  # queries 0, 2 and 4 own no rows
        counts = [0, N // 3, 0, N - N // 3, 0]
    else:                                           # [history; candidates] of 3 users: query b / 3 + b
        n_hist = N - N // 3
        counts = _split(n_hist, 3) + _split(N // 3, 3)
    nq = len(counts)
    owner = torch.repeat_interleave(torch.arange(nq), torch.tensor(counts)).to(torch.int32)
    z_rms = max(1.0, 0.19 * (3 * D) ** 0.5) if grid_valued else 1.0
    queries = torch.from_numpy((rng.uniform(-1, 1, (nq, F_)) * 2.0 / (F_ ** 0.5 * z_rms)).astype(np.float32))
    d_out = normal(rng, (N, F_), 1.0)
    return dict(ids=torch.from_numpy(ids), emb=emb, w=w, b=b, queries=queries, owner=owner, offsets=_offsets(counts),
                d_out=d_out, counts=counts)


def npa_conv_pre(inp, dtype):
    """Pre-activations of the convolution, (N, L, F), without dropout."""
    x = inp["emb"].to(dtype)[inp["ids"]]
    return F.conv1d(x.permute(0, 2, 1), inp["w"].to(dtype), inp["b"].to(dtype), padding=1).permute(0, 2, 1)


def npa_encoder_ref(case, inp, dtype, grads=True):
    N, L, D, F_ = case["N"], case["L"], case["D"], case["F"]
    emb, w, b, q = [_leaf(inp[k], dtype) for k in ("emb", "w", "b", "queries")]
    params = {NO.PRE + "embedding_layer.weight": emb, NO.PRE + "cnn.weight": w, NO.PRE + "cnn.bias": b}
    m1 = m2 = None
    if case["p"] > 0:
        m1 = dropout_multiplier(DROP_SEED, 0, case["p"], (N, L, D))
        m2 = dropout_multiplier(DROP_SEED, 1, case["p"], (N, L, F_))
    c = NO._conv_features(inp["ids"], params, m1, m2)
    out = NO._pers_att(c, q[inp["owner"].long()])
    ref = dict(out=out.detach(), c=c.detach())
    with torch.no_grad():
        ref["features"] = NO._conv_features(inp["ids"], params, None, None)
    if grads:
        g = torch.autograd.grad(out, [emb, w, b, q], inp["d_out"].to(dtype))
        g[0][0] = 0.0                               # padding_idx = 0
        ref.update(d_emb=g[0], d_w=g[1], d_b=g[2], d_queries=g[3])
    return ref


# ---- NPA user queries -------------------------------------------------------------------------------------------------------
def _qry(name, U, Pw, Pn, F_, B, p, seed, repeat=False):
    return dict(name=name, U=U, Pw=Pw, Pn=Pn, F=F_, B=B, p=p, seed=seed, repeat=repeat)


NPA_QUERY_CASES = [
    _qry("U1_P1_3", 1, 1, 3, 4, 3, 0.0, 500),                   # fewer features than waves
    _qry("U10_P24_20", 10, 24, 20, 64, 6, 0.5, 501),             # the small golden configuration (Pw > Pn)
    _qry("U50_P20_24", 50, 20, 24, 12, 5, 0.5, 502),             # Pn > Pw: the workspace stride is the news head's
    _qry("U65_P64_65", 65, 64, 65, 8, 4, 0.0, 503),              # U > 64: the lane loop iterates
    _qry("U130_P257_200", 130, 257, 200, 12, 3, 0.5, 504),       # P > 256: the thread loop iterates
    _qry("U50_P200_200", 50, 200, 200, 400, 7, 0.0, 505, repeat=True),   # the full configuration; one user three times
    _qry("late_fusion", 10, 24, 0, 16, 4, 0.5, 506),             # news parameters None
    _qry("B1", 50, 20, 24, 12, 1, 0.0, 507),
]
QUERY_KEYS = ("table", "tp_w", "tp_b", "ta_w", "ta_b", "np_w", "np_b", "na_w", "na_b")


def npa_query_inputs(case):
    """The projections (the ReLU gate's inputs) are grid-valued, the table in [0, 1] as ``torch.rand`` initialises it; the
    attention layers behind the gate are random."""
    U, Pw, Pn, F_, B = case["U"], case["Pw"], case["Pn"], case["F"], case["B"]
    rng = np.random.default_rng(case["seed"])
    n_users = 9
    user_idx = rng.integers(0, n_users, B)
    if case["repeat"]:
        user_idx[[0, 3, B - 1]] = 4
    h_rms = max(0.25, 0.2 * U ** 0.5)
    inp = dict(user_idx=torch.from_numpy(user_idx), table=grid(rng, (n_users, U), 1 / 8, 1.0).abs(),
               tp_w=grid(rng, (Pw, U), 1 / 16, 0.5), tp_b=grid_bias(rng, Pw),
               ta_w=normal(rng, (F_, Pw), 0.7 / (Pw ** 0.5 * h_rms)), ta_b=normal(rng, F_, 0.05),
               d_text=normal(rng, (2 * B, F_), 1.0))
    if Pn:
        inp.update(np_w=grid(rng, (Pn, U), 1 / 16, 0.5), np_b=grid_bias(rng, Pn),
                   na_w=normal(rng, (F_, Pn), 0.7 / (Pn ** 0.5 * h_rms)), na_b=normal(rng, F_, 0.05),
                   d_news=normal(rng, (B, F_), 1.0))
    return inp


def npa_query_pre(case, inp, dtype):
    """Pre-activations of the projections' ReLU, per head, with the user dropout applied."""
    B, U, p = case["B"], case["U"], case["p"]
    u = inp["table"].to(dtype)[inp["user_idx"]] * dropout_multiplier(DROP_SEED, 2, p, (B, U)).to(dtype)
    heads = [("tp_w", "tp_b")] + ([("np_w", "np_b")] if case["Pn"] else [])
    return [u @ inp[w].to(dtype).t() + inp[b].to(dtype) for w, b in heads]


def npa_query_ref(case, inp, dtype):
    B, U, Pw, Pn, p = case["B"], case["U"], case["Pw"], case["Pn"], case["p"]
    keys = [k for k in QUERY_KEYS if k in inp]
    leaves = {k: _leaf(inp[k], dtype) for k in keys}
    params = {NO.TEXT_PROJ + "weight": leaves["tp_w"], NO.TEXT_PROJ + "bias": leaves["tp_b"],
              NO.TEXT_ATT + "weight": leaves["ta_w"], NO.TEXT_ATT + "bias": leaves["ta_b"]}
    if Pn:
        params.update({NO.NEWS_PROJ + "weight": leaves["np_w"], NO.NEWS_PROJ + "bias": leaves["np_b"],
                       NO.NEWS_ATT + "weight": leaves["na_w"], NO.NEWS_ATT + "bias": leaves["na_b"]})
    m = [None] * 4
    if p > 0:                                       # streams 2..5: u, history text query, candidate text query, news query
        m = [dropout_multiplier(DROP_SEED, 2 + i, p, s) for i, s in enumerate([(B, U), (B, Pw), (B, Pw), (B, max(Pn, 1))])]
    u = leaves["table"][inp["user_idx"]]
    if m[0] is not None:
        u = u * m[0].to(u.dtype)
    text = torch.cat([NO._query(u, params, NO.TEXT_PROJ, NO.TEXT_ATT, m[1]),
                      NO._query(u, params, NO.TEXT_PROJ, NO.TEXT_ATT, m[2])])
    outs, douts = [text], [inp["d_text"].to(dtype)]
    if Pn:
        outs.append(NO._query(u, params, NO.NEWS_PROJ, NO.NEWS_ATT, m[3]))
        douts.append(inp["d_news"].to(dtype))
    g = torch.autograd.grad(outs, [leaves[k] for k in keys], douts)
    ref = {"d_" + k: gr for k, gr in zip(keys, g)}
    ref.update(text=text.detach(), news=outs[1].detach() if Pn else None)
    return ref


# ---- NPA user attention -----------------------------------------------------------------------------------------------------
# (max_hist, F): one history row, one round of the waves, one more, the module's 50, and the 256-thread loop iterating
NPA_ATT_CASES = [dict(name=f"H{h}_F{f}", max_hist=h, F=f, seed=600 + i)
                 for i, (h, f) in enumerate([(1, 4), (4, 400), (5, 1024), (50, 400), (300, 4), (300, 1024)])]


def npa_att_inputs(case):
    mh, F_ = case["max_hist"], case["F"]
    rng = np.random.default_rng(case["seed"])
    lengths = [min(3, mh), 0, mh, 1, mh // 2, 0]    # an empty history between long ones, and one at the end
    n = sum(lengths)
    return dict(lengths=lengths, offsets=_offsets(lengths), hist=normal(rng, (n, F_), 0.5),
                q=torch.from_numpy((rng.uniform(-1, 1, (len(lengths), F_)) * 3.0 / F_ ** 0.5).astype(np.float32)),
                d_out=normal(rng, (len(lengths), F_), 1.0))


def npa_att_ref(case, inp, dtype):
    B = len(inp["lengths"])
    hist, q = _leaf(inp["hist"], dtype), _leaf(inp["q"], dtype)
    batch = torch.repeat_interleave(torch.arange(B), torch.tensor(inp["lengths"]))
    dense, _ = to_dense_batch(hist, batch, B)
    out = NO._pers_att(dense, q)
    g = torch.autograd.grad(out, [hist, q], inp["d_out"].to(dtype))
    return dict(out=out.detach(), d_hist=g[0], d_q=g[1])


# ---- DKN encoder ------------------------------------------------------------------------------------------------------------
def _dkn(name, N, L, windows, D, Ed, F_, ctx, ents, seed, last=False):
    return dict(name=name, N=N, L=L, windows=windows, D=D, Ed=Ed, F=F_, ctx=ctx, ents=ents, seed=seed, last=last)


# seeds chosen on the host so that the float64 oracle alone meets FRAGILE_CAP under both engines' thresholds
DKN_ENCODER_CASES = [
    _dkn("L1_M257", 257, 1, [1], 4, 4, 4, True, "mixed", 700),                  # W = L = 1; N L = 257: two row chunks
    _dkn("L4_M256_D256", 64, 4, [1, 4], 256, 12, 4, False, "none_zero", 701),   # W = L; exactly one chunk; one column per thread
    _dkn("L5_M255_D260", 51, 5, [1, 2, 3, 4], 260, 12, 100, True, "all_zero", 702),   # second column per thread; Ed: 2 slices
    _dkn("L255_last", 2, 255, [1, 4], 256, 4, 4, True, "mixed", 703, last=True),      # the one-byte argmax at its limit
    _dkn("D512_Ed100", 7, 5, [1, 2, 3, 4], 512, 100, 4, True, "mixed", 704),
    _dkn("F100_Ed100", 5, 4, [1, 4], 48, 100, 100, False, "mixed", 705),
]


def dkn_encoder_inputs(case):
    N, L, D, Ed, F_, windows = case["N"], case["L"], case["D"], case["Ed"], case["F"], case["windows"]
    rng = np.random.default_rng(case["seed"])
    V, n_ent, C = max(2 * L, 64), 23, 3 if case["ctx"] else 2
    # distinct word ids inside a title (a repeated word repeats a window: an exact tie of the max); id 0 takes part
    ids = np.stack([rng.permutation(V - 1 if case["last"] else V)[:L] for _ in range(N)])
    ents = rng.integers(1, n_ent, (N, L))
    if case["ents"] == "all_zero":
        ents[:] = 0
    elif case["ents"] == "mixed":
        ents[rng.random((N, L)) < 0.6] = 0
    p = {DO.WORD: normal(rng, (V, D), 0.3), DO.ENT: normal(rng, (n_ent, Ed), 0.5)}
    if case["ctx"]:
        p[DO.CTX] = normal(rng, (n_ent, Ed), 0.5)
    p[DO.TM] = normal(rng, (Ed, D), Ed ** -0.5)
    p[DO.TB] = normal(rng, D, 0.05)
    for x in windows:
        p[DO.conv_key(x, "weight")] = normal(rng, (F_, C, x, D), 3.0 * (C * x * D) ** -0.5)
        p[DO.conv_key(x, "bias")] = normal(rng, F_, 0.05)
    if case["last"]:
        # a word met only at the last token of title 0, aligned with filter 0 of every window's last tap: the maximum of
        # (title 0, filter 0) sits at the last valid position L - W of each window
        star = sum(torch.sign(p[DO.conv_key(x, "weight")][0, 0, x - 1]) for x in windows)
        ids[0, L - 1] = V - 1
        p[DO.WORD][V - 1] = 0.5 * star
    return dict(ids=torch.from_numpy(ids), ents=torch.from_numpy(ents), params=p,
                d_out=normal(rng, (N, len(windows) * F_), 1.0))


def dkn_fragile(conv_maps, thr):
    """(N, nw F) bool from the float64 pre-ReLU maps (N, F, L - W + 1) of each window."""
    out = []
    for c in conv_maps:
        top = torch.topk(c, min(2, c.shape[-1]), dim=-1)[0]
        gap = top[..., 0] - top[..., 1] if c.shape[-1] > 1 else torch.full_like(top[..., 0], float("inf"))
        out.append((gap < thr) | (top[..., 0].abs() < thr))
    return torch.cat(out, dim=1)


def dkn_encoder_ref(case, inp, dtype, thr=None):
    """thr: the fragile threshold (10 x the engine's forward tolerance); the mask always comes from float64."""
    keys = list(inp["params"])
    leaves = {k: _leaf(inp["params"][k], dtype) for k in keys}
    out = DO.kcnn(inp["ids"], inp["ents"], leaves, case["windows"])
    ref = dict(out=out.detach())
    if thr is not None:
        with torch.no_grad():
            maps = DO.kcnn_conv(inp["ids"], inp["ents"], {k: v.double() for k, v in inp["params"].items()}, case["windows"])
        ref["fragile"] = dkn_fragile(maps, thr)
        ref["argmax"] = torch.cat([m.argmax(dim=-1) for m in maps], dim=1)
        d_out = inp["d_out"].masked_fill(ref["fragile"], 0.0)
        g = torch.autograd.grad(out, [leaves[k] for k in keys], d_out.to(dtype))
        ref["grads"] = dict(zip(keys, g))
        for k in (DO.WORD, DO.ENT, DO.CTX):         # padding_idx = 0
            if k in ref["grads"]:
                ref["grads"][k][0] = 0.0
        ref["d_out"] = d_out
    return ref


# ---- DKN click --------------------------------------------------------------------------------------------------------------
DKN_CLICK_CASES = [
    dict(name="Hd1_dim4", Hd=1, dim=4, hist=[0, 1, 3, 2], cand=[2, 0, 3, 1], seed=800),
    dict(name="Hd16_dim32", Hd=16, dim=32, hist=[255, 256, 257, 0, 1], cand=[2, 3, 1, 2, 2], seed=801),
    dict(name="Hd64_dim400", Hd=64, dim=400, hist=[1024, 5, 0], cand=[3, 0, 2], seed=802),
    dict(name="Hd16_dim1024", Hd=16, dim=1024, hist=[3, 257, 1, 0], cand=[2, 2, 5, 1], seed=803),
]
CLICK_KEYS = ("aw1", "ab1", "aw2", "ab2", "pw1", "pb1", "pw2", "pb2")


def dkn_click_inputs(case):
    Hd, dim = case["Hd"], case["dim"]
    rng = np.random.default_rng(case["seed"])
    inp = dict(hist=normal(rng, (sum(case["hist"]), dim), 0.5), cand=normal(rng, (sum(case["cand"]), dim), 0.5),
               hist_offsets=_offsets(case["hist"]), cand_offsets=_offsets(case["cand"]),
               d_scores=normal(rng, (len(case["cand"]), max(case["cand"])), 1.0))
    for k, (shape, scale) in zip(CLICK_KEYS, [((Hd, 2 * dim), (2 * dim) ** -0.5), (Hd, 0.05), ((1, Hd), Hd ** -0.5), (1, 0.05)] * 2):
        inp[k] = normal(rng, shape, 2.0 * scale if k == "aw1" else scale)
    return inp


def dkn_click_ref(case, inp, dtype):
    B = len(case["cand"])
    keys = ["hist", "cand"] + list(CLICK_KEYS)
    leaves = {k: _leaf(inp[k], dtype) for k in keys}
    params = {DO.UE + "0.weight": leaves["aw1"], DO.UE + "0.bias": leaves["ab1"], DO.UE + "1.weight": leaves["aw2"],
              DO.UE + "1.bias": leaves["ab2"], DO.CP + "0.weight": leaves["pw1"], DO.CP + "0.bias": leaves["pb1"],
              DO.CP + "2.weight": leaves["pw2"], DO.CP + "2.bias": leaves["pb2"]}
    bh = torch.repeat_interleave(torch.arange(B), torch.tensor(case["hist"]))
    bc = torch.repeat_interleave(torch.arange(B), torch.tensor(case["cand"]))
    hd, mh = to_dense_batch(leaves["hist"], bh, B)
    cd, mc = to_dense_batch(leaves["cand"], bc, B)
    user = DO.user_attention(hd, cd, mh, mc, params)
    cat = torch.cat([cd, user], dim=-1)
    pre = cat @ params[DO.CP + "0.weight"].t() + params[DO.CP + "0.bias"]
    scores = torch.where(mc, DO.dnn_predictor(user, cd, params), torch.zeros((), dtype=dtype))
    g = torch.autograd.grad(scores, [leaves[k] for k in keys], inp["d_scores"].to(dtype))
    ref = {"d_" + k: gr for k, gr in zip(keys, g)}
    ref.update(scores=scores.detach(), user=user.detach(), mask_c=mc, min_pre=float(pre.detach()[mc].abs().min()))
    return ref


# ---- one reference per (case, dtype[, engine]) for the whole session: computed once, never modified -----------------------
@functools.lru_cache(maxsize=None)
def cached(family: str, index: int, dtype_name: str, engine: str = ""):
    dtype = getattr(torch, dtype_name)
    if family == "npa_encoder":
        case = NPA_ENCODER_CASES[index]
        inp = cached_inputs(family, index)
        return npa_encoder_ref(case, inp, dtype)
    if family == "npa_random":
        return npa_encoder_ref(NPA_RANDOM_CASE, cached_inputs(family, index), dtype, grads=False)
    if family == "npa_query":
        return npa_query_ref(NPA_QUERY_CASES[index], cached_inputs(family, index), dtype)
    if family == "npa_att":
        return npa_att_ref(NPA_ATT_CASES[index], cached_inputs(family, index), dtype)
    if family == "dkn_encoder":
        return dkn_encoder_ref(DKN_ENCODER_CASES[index], cached_inputs(family, index), dtype, thr=10 * TOL[engine][0])
    if family == "dkn_click":
        return dkn_click_ref(DKN_CLICK_CASES[index], cached_inputs(family, index), dtype)
    raise KeyError(family)


@functools.lru_cache(maxsize=None)
def cached_inputs(family: str, index: int):
    if family == "npa_encoder":
        return npa_encoder_inputs(NPA_ENCODER_CASES[index])
    if family == "npa_random":
        return npa_encoder_inputs(NPA_RANDOM_CASE, grid_valued=False)
    if family == "npa_query":
        return npa_query_inputs(NPA_QUERY_CASES[index])
    if family == "npa_att":
        return npa_att_inputs(NPA_ATT_CASES[index])
    if family == "dkn_encoder":
        return dkn_encoder_inputs(DKN_ENCODER_CASES[index])
    if family == "dkn_click":
        return dkn_click_inputs(DKN_CLICK_CASES[index])
    raise KeyError(family)
