"""Input generators and float64 / float32 CPU references of the SentiDebias / MANNeR op-level shape sweep
(tests/test_gpu_sd_manner_sweep.py); their properties are asserted on the host in tests/test_sd_manner_sweep_host.py.
Plain module: no fixtures, no GPU.  The references are the existing restatements (tests/sentidebias_oracle.py:
``cos_rows``, ``dense``, ``discriminator_losses``, ``wrapped_target``; tests/manner_oracle.py: ``supcon_embed``,
``ensemble_scores``) run in float64 and, as the yardstick, in float32.

Nothing here has a ReLU or arg-max gate; what the inputs must rule out instead is a comparison that amplifies rounding:
a cosine whose |a| |b| is near the 1e-8 of its divisor, a z-score over scores without spread, a SupCon row loss so close
to 0 that the reducer's ``> 0`` decides differently in fp32.  The rules are stated per family below and asserted for every
committed seed on the host."""
from __future__ import annotations

import functools

import numpy as np
import torch

from tests import manner_oracle as MO
from tests import sentidebias_oracle as SO
from tests.sweep_inputs import _leaf, _offsets, normal

# the project's own bounds (test_kernels_against_float64 in tests/test_gpu_sentidebias.py)
COS_VALUE, COS_DNEWS, D_TABLE, LATE_U, SCORES, SCORES_GRAD = 1e-6, 1e-6, 1e-5, 1e-6, 1e-4, 1e-5
DISC = {"f32": 1e-5, "bf16x3": 1e-4}
EPS32 = float(torch.finfo(torch.float32).eps)


def _table(rng, S, D):
    return torch.tanh(normal(rng, (S, D), 1.0))


def _ids(rng, n, S):
    """n ids in [0, S) that hold every class when n allows it."""
    ids = rng.integers(0, S, n)
    if n >= S:
        ids[rng.permutation(n)[:S]] = np.arange(S)
    return torch.from_numpy(ids)


def gather(T, ids):
    """T[id] at the valid ids, a zero row at an id outside [0, S): what every kernel's guard makes of such a row."""
    S = T.shape[0]
    ok = (ids >= 0) & (ids < S)
    return T[ids.clamp(0, S - 1)] * ok.to(T.dtype).unsqueeze(-1)


def _pad_to(x, width):
    """(B, w, ...) -> (B, width, ...) zero padded (``SO.dense`` stops at the longest list)."""
    if x.shape[1] == width:
        return x
    return torch.cat([x, x.new_zeros((x.shape[0], width - x.shape[1]) + tuple(x.shape[2:]))], dim=1)


def _dense(rows, sizes, width):
    if max(sizes) == 0:
        return rows.new_zeros((len(sizes), width) + tuple(rows.shape[1:])) + 0 * rows.sum()
    return _pad_to(SO.dense(rows, sizes), width)


# ---- SentiDebias row cosines ------------------------------------------------------------------------------------------------
def _cos(name, N, n_hist, D, S, seed, special=None):
    return dict(name=name, N=N, n_hist=n_hist, D=D, S=S, seed=seed, special=special)


# D4 = D / 4 at 1, 63, 64, 65, 75 (and 96: S D = 3072, the whole 48 KiB of bins); slabs of 64 rows at N = 63, 64, 65, 129;
# n_hist at 0, 1, N - 1, N and inside a wave stride of the second slab
ROWCOS_CASES = [
    _cos("N1_h0_D4_S1", 1, 0, 4, 1, 900),
    _cos("N1_h1_D300_S4", 1, 1, 300, 4, 901),
    _cos("N63_h1_D252_S2", 63, 1, 252, 2, 902),
    _cos("N64_h63_D256_S4", 64, 63, 256, 4, 903),
    _cos("N64_h64_D260_S8", 64, 64, 260, 8, 904),
    _cos("N65_h0_D260_S4", 65, 0, 260, 4, 905),
    _cos("N129_h66_D300_S8", 129, 66, 300, 8, 906),
    _cos("N129_h128_D384_S8", 129, 128, 384, 8, 907),
    _cos("zero_row", 65, 33, 8, 4, 908, special="zero_row"),
    _cos("bad_ids", 65, 30, 12, 4, 909, special="bad_ids"),
]
ZERO_ROW = 64           # the all-zero news row of the "zero_row" case: the only row of the second slab
BAD_ROWS = {3: -1, 17: 4, 30: 4, 64: -1}      # row -> id of the "bad_ids" case (S = 4): both sides, both slabs


def rowcos_inputs(case):
    N, D, S = case["N"], case["D"], case["S"]
    rng = np.random.default_rng(case["seed"])
    inp = dict(news=normal(rng, (N, D), 1.0), T=_table(rng, S, D), ids=_ids(rng, N, S), w=normal(rng, 2, 1.0))
    if case["special"] == "zero_row":
        inp["news"][ZERO_ROW] = 0.0
    if case["special"] == "bad_ids":
        for r, v in BAD_ROWS.items():
            inp["ids"][r] = v
    return inp


def rowcos_ref(case, inp, dtype):
    N, nh = case["N"], case["n_hist"]
    news, T = _leaf(inp["news"], dtype), _leaf(inp["T"], dtype)
    ok = ((inp["ids"] >= 0) & (inp["ids"] < case["S"])).to(dtype)
    c = SO.cos_rows(news, gather(T, inp["ids"])) * ok          # a skipped row adds nothing; the divisor keeps counting it
    zero = c.sum() * 0
    out = torch.stack([c[:nh].sum() / nh if nh else zero, c[nh:].sum() / (N - nh) if N - nh else zero])
    g = torch.autograd.grad((out * inp["w"].to(dtype)).sum(), [news, T])
    return dict(out=out.detach(), d_news=g[0], d_T=g[1])


def rowcos_norm_products(case, inp):
    """|a| |b| of every row that takes part (float64)."""
    ok = (inp["ids"] >= 0) & (inp["ids"] < case["S"])
    prod = inp["news"].double().norm(dim=-1) * gather(inp["T"].double(), inp["ids"]).norm(dim=-1)
    if case["special"] == "zero_row":
        ok[ZERO_ROW] = False
    return prod[ok]


# ---- SentiDebias dense history and late fusion ------------------------------------------------------------------------------
def _hist(name, H, hs, D, S, seed, bad=False):
    return dict(name=name, B=len(hs), H=H, hs=hs, D=D, S=S, seed=seed, bad=bad)


# B H slots in slabs of 64: 1, 64, 65, 65, 129, 260; histories empty, of one row and full; H above the longest history;
# more than 64 rows of one user (the lane loop of the late fusion); S D = 3072 (all 48 KiB of LDS bins)
HIST_CASES = [
    _hist("B1_H1_D4_S1", 1, [1], 4, 1, 920),
    _hist("B1_H64_D260_S4", 64, [64], 260, 4, 921),
    _hist("B1_H65_D384_S8", 65, [65], 384, 8, 922),
    _hist("B5_H13_D260_S4", 13, [13, 0, 1, 7, 13], 260, 4, 923),
    _hist("B5_H13_full_D4_S8", 13, [13, 5, 1, 7, 13], 4, 8, 924),
    _hist("B3_H43_D4_S8", 43, [43, 1, 0], 4, 8, 925),
    _hist("B3_H43_full_D260_S1", 43, [43, 1, 22], 260, 1, 926),
    _hist("B2_H130_D260_S4", 130, [130, 67], 260, 4, 927),
    _hist("B4_H5_D8_S1", 5, [3, 2, 0, 3], 8, 1, 928),
    _hist("bad_ids", 9, [9, 4, 6], 12, 4, 929, bad=True),
]


def hist_inputs(case):
    B, H, D, S, hs = case["B"], case["H"], case["D"], case["S"], case["hs"]
    rng = np.random.default_rng(case["seed"])
    ids = _ids(rng, sum(hs), S)
    if case["bad"]:
        ids[1], ids[8], ids[10], ids[18] = -1, S, S, -1
    return dict(T=_table(rng, S, D), ids=ids, off=_offsets(hs), d_dense=normal(rng, (B, H, D), 1.0), d_u=normal(rng, (B, D), 1.0))


def hist_ref(case, inp, dtype):
    """The dense history and, from it, the late-fusion user: its sum over the slots divided by the history size (0 / 0 = NaN
    for an empty history, as the reference).  The late-fusion gradient only where no history is empty."""
    T = _leaf(inp["T"], dtype)
    dense = _dense(gather(T, inp["ids"]), case["hs"], case["H"])
    u = dense.sum(1) / torch.tensor(case["hs"], dtype=dtype).unsqueeze(1)
    ref = dict(dense=dense.detach(), u=u.detach(), d_T_dense=torch.autograd.grad(dense, T, inp["d_dense"].to(dtype), retain_graph=True)[0])
    if min(case["hs"]) > 0:
        ref["d_T_late"] = torch.autograd.grad(u, T, inp["d_u"].to(dtype))[0]
    return ref


# ---- SentiDebias combined scores --------------------------------------------------------------------------------------------
def _sc(name, C, cs, D, S, seed, bad=False):
    return dict(name=name, B=len(cs), C=C, cs=cs, D=D, S=S, seed=seed, bad=bad)


SCORE_CASES = [
    _sc("B1_C1_D4_S1", 1, [1], 4, 1, 940),
    _sc("B4_C63_D260_S8", 63, [63, 0, 17, 62], 260, 8, 941),
    _sc("B5_C64_D4_S8", 64, [64, 1, 0, 33, 64], 4, 8, 942),
    _sc("B1_C65_D260_S1", 65, [65], 260, 1, 943),
    _sc("B4_C65_short_D300_S8", 65, [64, 63, 2, 0], 300, 8, 944),       # C above every list
    _sc("B5_C130_D12_S8", 130, [130, 65, 0, 129, 3], 12, 8, 945),
    _sc("bad_ids", 9, [9, 4, 6], 12, 4, 946, bad=True),
]


def score_inputs(case):
    B, C, D, S, cs = case["B"], case["C"], case["D"], case["S"], case["cs"]
    rng = np.random.default_rng(case["seed"])
    ids = _ids(rng, sum(cs), S)
    if case["bad"]:
        ids[1], ids[8], ids[10], ids[18] = -1, S, S, -1
    return dict(free=normal(rng, (B, C), 1.0), u=normal(rng, (B, D), 1.0), T=_table(rng, S, D), ids=ids, off=_offsets(cs),
                d_out=normal(rng, (B, C), 1.0), mask=torch.arange(C).unsqueeze(0) < torch.tensor(cs).unsqueeze(1))


def score_ref(case, inp, dtype):
    free, u, T = (_leaf(inp[k], dtype) for k in ("free", "u", "T"))
    out = free + torch.einsum("bd,bcd->bc", u, _dense(gather(T, inp["ids"]), case["cs"], case["C"]))
    g = torch.autograd.grad(out, [free, u, T], inp["d_out"].to(dtype))
    return dict(out=out.detach(), d_free=g[0], d_u=g[1], d_T=g[2])


# ---- SentiDebias discriminator ----------------------------------------------------------------------------------------------
def _disc(name, N, n_hist, D, Hd, O, seed):
    return dict(name=name, N=N, n_hist=n_hist, D=D, Hd=Hd, O=O, seed=seed)


# O Hd + O = 1, 2, 3, 0 mod 4 (O = 1, 2, 3, 8: the slab's padding of 3, 2, 1, 0 floats); Hd / 4 at 1, 63, 64, 65 and 95
# (O = 8, Hd = 380: 48,768 of the 49,152 bytes of bins); N and n_hist as the row cosines
DISC_CASES = [
    _disc("N1_h0_Hd4_O1", 1, 0, 8, 4, 1, 960),
    _disc("N65_h1_Hd260_O1", 65, 1, 12, 260, 1, 961),
    _disc("N1_h1_Hd252_O2", 1, 1, 8, 252, 2, 962),
    _disc("N63_h62_Hd256_O3", 63, 62, 300, 256, 3, 963),
    _disc("N64_h64_Hd4_O2", 64, 64, 12, 4, 2, 964),
    _disc("N64_h0_Hd260_O8", 64, 0, 12, 260, 8, 965),
    _disc("N129_h66_Hd380_O8", 129, 66, 12, 380, 8, 966),
    _disc("N129_h128_Hd252_O3", 129, 128, 8, 252, 3, 967),
]
DISC_KEYS = ("linear1.weight", "linear1.bias", "linear2.weight", "linear2.bias")
DISC_MODES = {"all": (True, True), "phase_g": (True, False), "phase_d": (False, True)}     # (news rows, weights) need a gradient


def disc_inputs(case):
    N, D, Hd, O = case["N"], case["D"], case["Hd"], case["O"]
    rng = np.random.default_rng(case["seed"])
    ids = rng.integers(0, O + 1, N)                    # 0 .. O: id 0 and id O both name the last column
    if N >= 2:
        ids[0], ids[N - 1] = 0, O
    else:
        ids[0] = 0 if case["seed"] % 2 else O
    p = {"linear1.weight": normal(rng, (Hd, D), D ** -0.5), "linear1.bias": normal(rng, Hd, 0.3),
         "linear2.weight": normal(rng, (O, Hd), Hd ** -0.5), "linear2.bias": normal(rng, O, 0.3)}
    return dict(x=normal(rng, (N, D), 0.3), ids=torch.from_numpy(ids), w=normal(rng, 2, 1.0), **p)


def disc_ref(case, inp, dtype):
    nh, N = case["n_hist"], case["N"]
    x = _leaf(inp["x"], dtype)
    p = {"discriminator." + k: _leaf(inp[k], dtype) for k in DISC_KEYS}
    ids = inp["ids"]
    if dtype == torch.float64:
        # an empty side has no loss (the kernels' mean of an empty side is 0): the restatement is handed the other side twice
        # and the empty side's value is dropped
        h, ih = (x[:nh], ids[:nh]) if nh else (x, ids)
        c, ic = (x[nh:], ids[nh:]) if N - nh else (x, ids)
        a, b = SO.discriminator_losses(p, h, c, ih, ic)
    else:
        # (``discriminator_losses`` promotes to float64: the float32 yardstick writes its one line out in float32)
        w1, b1, w2, b2 = (p["discriminator." + k] for k in DISC_KEYS)
        logits = torch.tanh(x @ w1.T + b1) @ w2.T + b2
        a = SO.adversarial_loss(logits[:nh] if nh else logits, ids[:nh] if nh else ids)
        b = SO.adversarial_loss(logits[nh:] if N - nh else logits, ids[nh:] if N - nh else ids)
    a, b = (a if nh else a * 0), (b if N - nh else b * 0)
    w = inp["w"].to(dtype)
    g = torch.autograd.grad(a * w[0] + b * w[1], [x] + list(p.values()))
    ref = dict(out=torch.stack([a, b]).detach(), d_x=g[0])
    ref.update({"d_" + k: gr for k, gr in zip(DISC_KEYS, g[1:])})
    return ref


# ---- MANNeR scorer ----------------------------------------------------------------------------------------------------------
def _mn(name, D, k, V, max_cand, hs, cs, seed, identical=(), clamp=False):
    return dict(name=name, D=D, k=k, V=V, max_cand=max_cand, hs=hs, cs=cs, seed=seed, identical=tuple(identical), clamp=clamp)


# D / 4 at 1, 63, 64, 65 and 256 (the workgroup size); max_cand on both sides of 256 (register slot 1), at 513 (slot 2) and
# at the limit 2048 (slot 7), the long ones at D = 4 and a small V; histories of 1, 65 and 300 rows; the degenerate rows the
# reference defines: an empty history (NaN), no candidate (all 0), one candidate (NaN), four identical candidates (NaN)
MANNER_CASES = [
    _mn("D252_k2_mc255", 252, 2, 97, 255, [1, 65, 300, 0, 3], [255, 1, 0, 4, 17], 980, identical=(3,), clamp=True),
    _mn("D256_k3_mc256", 256, 3, 301, 256, [65], [256], 981),
    _mn("D260_k1_mc257", 260, 1, 301, 257, [300, 1, 2, 65, 7], [257, 2, 256, 3, 100], 982),
    _mn("D4_k2_mc513", 4, 2, 16, 513, [1], [513], 983),
    _mn("D4_k3_mc2048", 4, 3, 32, 2048, [3, 1, 65, 2, 5], [2048, 513, 1, 0, 1025], 984),
    _mn("D1024_k1_mc9", 1024, 1, 40, 9, [1, 65, 0, 4, 9], [5, 9, 3, 4, 1], 985, identical=(3,), clamp=True),
]
MANNER_WEIGHTS = (1.0, -0.3, 0.25)


def manner_kinds(case):
    """Per impression: "nan" (empty history, one candidate, identical candidates), "zero" (no candidate) or "real"."""
    out = []
    for b, (h, c) in enumerate(zip(case["hs"], case["cs"])):
        out.append("zero" if c == 0 else ("nan" if h == 0 or c == 1 or b in case["identical"] else "real"))
    return out


def manner_inputs(case):
    V, D, k = case["V"], case["D"], case["k"]
    g = torch.Generator().manual_seed(case["seed"])
    hist = [torch.randint(0, V, (n,), generator=g) for n in case["hs"]]
    cand = [torch.randint(0, V, (n,), generator=g) for n in case["cs"]]
    for b in case["identical"]:
        cand[b][:] = int(cand[b][0])
    raw_hist, raw_cand = [h.clone() for h in hist], [c.clone() for c in cand]
    if case["clamp"]:
        # indices outside the table score as its first and its last row: the raw lists go to the kernel, the clamped ones
        # to the oracle
        b = manner_kinds(case).index("real")
        hist[b][0], raw_hist[b][0] = 0, -3
        cand[b][0], raw_cand[b][0] = V - 1, V + 7
        cand[b][len(cand[b]) - 1], raw_cand[b][len(cand[b]) - 1] = 0, -3
        b2 = len(hist) - 1 - manner_kinds(case)[::-1].index("real")
        hist[b2][len(hist[b2]) - 1], raw_hist[b2][len(hist[b2]) - 1] = V - 1, V + 7
    return dict(tables=MO.random_tables(k, V, D, case["seed"]), weights=list(MANNER_WEIGHTS[:k]), hist=hist, cand=cand,
                raw_hist=raw_hist, raw_cand=raw_cand, kinds=manner_kinds(case))


def manner_ref(case, inp, dtype):
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                 # torch.std of one or of no value: the reference's NaN, with a warning
        rows = MO.ensemble_scores([t.to(dtype) for t in inp["tables"]], inp["weights"], inp["hist"], inp["cand"])
    return dict(rows=rows)


def manner_errors(case, inp, r64, r32):
    """(largest float32-oracle error over the real rows, largest |float64 score|)."""
    real = [b for b, kind in enumerate(inp["kinds"]) if kind == "real"]
    e32 = max(float((r32["rows"][b].double() - r64["rows"][b]).abs().max()) for b in real)
    return e32, max(float(r64["rows"][b].abs().max()) for b in real)


# ---- MANNeR SupCon ----------------------------------------------------------------------------------------------------------
def _sup(name, N, D, classes, T, seed, singleton=True, labels=None):
    return dict(name=name, N=N, D=D, classes=classes, T=T, seed=seed, singleton=singleton, labels=labels)


# N % 4 at 1, 2, 3, 0 (the pad kernel copies N of Np rows); one chunk of 128 anchors, and a second one of 4 (N = 125 .. 129
# pad to 128 / 132) or 132 columns; the exactly-zero batches of one anchor and of two
SUPCON_CASES = [
    _sup("N1_D4", 1, 4, 1, 0.9, 1000, labels=[3]),
    _sup("N2_equal_D4", 2, 4, 1, 0.05, 1001, labels=[5, 5]),
    _sup("N2_differ_D8", 2, 8, 2, 0.9, 1002, labels=[0, 1]),
    _sup("N5_D8_T0.05", 5, 8, 2, 0.05, 1003),
    _sup("N6_D4_T0.9", 6, 4, 2, 0.9, 1004),
    _sup("N7_D8_T0.9", 7, 8, 3, 0.9, 1005),
    _sup("N125_D4_T0.05", 125, 4, 7, 0.05, 1006),
    _sup("N128_D8_T0.9", 128, 8, 5, 0.9, 1007),
    _sup("N129_D4_T0.9", 129, 4, 7, 0.9, 1008),
    _sup("N129_D8_T0.05", 129, 8, 5, 0.05, 1009),
    _sup("N132_D8_T0.05", 132, 8, 7, 0.05, 1010),
]


def supcon_inputs(case):
    """Fixed labels: the exactly-zero batches.  Otherwise ``MO.supcon_case``'s seed search (float64 row losses exactly 0 or
    >= 1e-3) with the last row a singleton class, continued until the float32 restatement's own error is at least a quarter
    ulp of the loss and of the largest gradient entry: four times a yardstick that happens to be 0 bounds nothing, and fp32
    cannot be asked to be exact."""
    N, D, T = case["N"], case["D"], case["T"]
    if case["labels"] is not None:
        g = torch.Generator().manual_seed(case["seed"])
        return dict(E=torch.randn(N, D, generator=g) * 0.5, labels=torch.tensor(case["labels"]), seed=case["seed"])
    seed = case["seed"]
    for _ in range(20):
        E, labels = MO.supcon_case(N, D, case["classes"], T, seed=seed, singleton=case["singleton"])
        l64, g64 = MO.supcon_embed_with_grad(E, labels, T, torch.float64)
        l32, g32 = MO.supcon_embed_with_grad(E, labels, T, torch.float32)
        if abs(float(l32) - float(l64)) >= 0.25 * EPS32 * abs(float(l64)) and \
                float((g32.double() - g64).abs().max()) >= 0.25 * EPS32 * float(g64.abs().max()):
            return dict(E=E, labels=labels, seed=seed)
        seed += 50
    raise AssertionError("no seed gives the float32 restatement a non-zero error")


def supcon_ref(case, inp, dtype):
    loss, grad = MO.supcon_embed_with_grad(inp["E"], inp["labels"], case["T"], dtype)
    rows = MO.supcon_rows(inp["E"].to(dtype), inp["labels"], case["T"])
    return dict(loss=loss, grad=grad, rows=rows)


# ---- one reference per (case, dtype) for the whole session: computed once, never modified -----------------------------------
FAMILIES = {
    "rowcos": (ROWCOS_CASES, rowcos_inputs, rowcos_ref),
    "hist": (HIST_CASES, hist_inputs, hist_ref),
    "scores": (SCORE_CASES, score_inputs, score_ref),
    "disc": (DISC_CASES, disc_inputs, disc_ref),
    "manner": (MANNER_CASES, manner_inputs, manner_ref),
    "supcon": (SUPCON_CASES, supcon_inputs, supcon_ref),
}


@functools.lru_cache(maxsize=None)
def cached_inputs(family: str, index: int):
    cases, make, _ = FAMILIES[family]
    return make(cases[index])


@functools.lru_cache(maxsize=None)
def cached(family: str, index: int, dtype_name: str):
    cases, _, ref = FAMILIES[family]
    return ref(cases[index], cached_inputs(family, index), getattr(torch, dtype_name))
