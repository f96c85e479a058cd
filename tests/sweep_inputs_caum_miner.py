"""Input generators and float64 / float32 CPU references of the CAUM / MINER op-level shape sweep
(tests/test_gpu_caum_miner_sweep.py); their properties are asserted on the host in tests/test_caum_miner_sweep_host.py.
Plain module: no fixtures, no GPU.  Each op has ONE dtype-parametric restatement, run in float64 (the reference) and in
float32 (the yardstick), gradients by autograd.  The restatements are the existing ones: tests/miner_oracle.py
(``categ_bias_flat``, ``poly_attention`` over ``to_dense_batch``, ``aggregate``, ``cosine_3d``, ``cosine_2d``), the lines of
``user_encoder_slot`` in tests/caum_oracle.py (the host test composes the CAUM pieces below into that function and compares)
and ``oracle.nrms_oracle.dropout_multiplier``.

How an op whose kernel takes an INTERMEDIATE as its input is fed through a restatement that computes that intermediate itself:
* ``PolyFn`` takes P = tanh(E W^T) as a tensor.  ``poly_attention(emb, mask, w, codes, bias)`` is called with
  emb = [E | atanh(P)] and w = [0 | I]: its projection is tanh(0 E + atanh P) = P, its output [user_vector | unused].
* ``ScoreFn`` (weighted) takes Z = user_vector Wt^T.  ``aggregate`` is called with ``user_vector=Z`` and ``wt=I``.

Input conditions ("Shape sweeps against float64"), each asserted per committed seed on the host:
* max mode: the top-two gap over k of every real candidate's matching scores is >= 5e-3 in float64 (10x the looser
  engine's forward tolerance), so fp32 and float64 take the same arg-max; the one exception is the constructed tie;
* cosines without epsilon (category bias, ``CosDisagreementFn`` with eps = 0): every row norm >= 0.1;
* ``CosDisagreementFn`` with eps = 1e-8: every row norm >= 0.1 or exactly 0, exactly one zero row, in one case;
* dropout: p in {0, 0.2, 0.5}, a stream base != 0.
The tolerances are absolute below 1, so the generators keep the compared values well above them: cosine rows share a
component and take an upstream gradient that undoes the mean's 1 / (G R R), and a softmax over more than 256 rows is peaked
at its first and last row and on both sides of the thread stride (``cscore_inputs``)."""
from __future__ import annotations

import functools

import numpy as np
import torch

from oracle.nrms_oracle import dropout_multiplier, to_dense_batch
from tests import miner_oracle as MO
from tests.sweep_inputs import TOL, _leaf, _offsets, normal

DROP_SEED = 1234
MAX_GAP = 5e-3                  # 10 x the looser engine's forward tolerance (``Report.fwd`` under bf16x3: 5 x 1e-4)
MIN_NORM = 0.1
# the configured widths (a case above one of them is ``wide``: its bound is the larger of the project's and 4x oracle32)
MINER_CFG = dict(Dn=256, K=32, Cd=200, Dc=100, max_hist=50)
CAUM_CFG = dict(U=400, F=400, N2=200)


def _batch(sizes):
    return torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes))


# ---- MINER: bias-free linear ------------------------------------------------------------------------------------------------
def _lin(M, N, K, seed):
    return dict(name=f"M{M}_N{N}_K{K}", M=M, N=N, K=K, seed=seed, wide=K > MINER_CFG["Dn"] or N > MINER_CFG["Dn"])


# The planned (M, N, K) (``WGRAD_CASES`` below has them unchanged) with N moved to a multiple of 4:
# ``nrl_linear_bwd_img`` (d_x) refuses N % 4 != 0 on the host and ``nrl_linear_act_fwd`` does too (MINER's N is context_code_dim or news_embed_dim, both multiples of 4 for the poly and
# score kernels).  1 -> 4; 15 -> 12, 17 -> 20, 33 -> 36: the neighbour that keeps N % 16 != 0 (the ``n >= N`` break of
# ``miner_wgrad_kernel``, in the first, second and third block of 16 weight rows).  M = 1, 63, 64, 65, 129: the slabs of 64
# rows; K = 68, 256, 260: 16 K / 4 > 256.
LIN_CASES = [_lin(1, 4, 4, 1100), _lin(63, 12, 64, 1101), _lin(64, 16, 64, 1102), _lin(65, 20, 68, 1103),
             _lin(129, 36, 260, 1104), _lin(70, 200, 256, 1105)]
LIN_ACTS = (None, "tanh")


def lin_inputs(case):
    M, N, K = case["M"], case["N"], case["K"]
    rng = np.random.default_rng(case["seed"])
    return dict(x=normal(rng, (M, K), 0.5), w=normal(rng, (N, K), 1.5 * K ** -0.5), d_out=normal(rng, (M, N), 1.0))


def lin_ref(case, inp, dtype):
    ref = {}
    for act in LIN_ACTS:
        x, w = _leaf(inp["x"], dtype), _leaf(inp["w"], dtype)
        c = x @ w.t()
        c = torch.tanh(c) if act == "tanh" else c
        g = torch.autograd.grad(c, [x, w], inp["d_out"].to(dtype))
        ref[act] = dict(out=c.detach(), d_x=g[0], d_w=g[1])
    return ref


# The weight-gradient entry itself takes any N (only K % 4 == 0): the planned (M, N, K), unchanged, through ``nrl_miner_wgrad``
WGRAD_CASES = [_lin(1, 1, 4, 1110), _lin(63, 15, 64, 1111), _lin(64, 16, 64, 1112), _lin(65, 17, 68, 1113),
               _lin(129, 33, 260, 1114), _lin(70, 200, 256, 1115)]


def wgrad_ref(case, inp, dtype):
    """d_w of ``x w^T`` under d_out (the projection's own restatement: no activation)."""
    x, w = inp["x"].to(dtype), _leaf(inp["w"], dtype)
    (d_w,) = torch.autograd.grad(x @ w.t(), [w], inp["d_out"].to(dtype))
    return dict(d_w=d_w)


# ---- MINER: category bias ---------------------------------------------------------------------------------------------------
def _cb(name, Dc, hs, cs, seed):
    return dict(name=name, Dc=Dc, B=len(hs), hs=hs, cs=cs, seed=seed, wide=Dc > MINER_CFG["Dc"])


# Dc / 4 at 1, 25, 64, 65, 257 (both strided loops); users without candidates / without history; n_hist % 4 = 1, 0, 2, 1, 1, 3
# and n_cand % 4 = 2, 3, 2, 0, 1, 1 (rn_h / rn_c are padded to 4 floats); B5_Dc256 user 0: more than 4 rows of both
CB_CASES = [
    _cb("B1_Dc4", 4, [5], [6], 1120),
    _cb("B5_Dc256", 256, [6, 0, 1, 3, 2], [7, 2, 0, 1, 1], 1121),
    _cb("B3_Dc260", 260, [0, 5, 1], [3, 0, 7], 1122),
    _cb("B3_Dc100", 100, [4, 0, 1], [0, 5, 3], 1123),
    _cb("B5_Dc1028", 1028, [5, 1, 0, 2, 1], [5, 0, 1, 1, 2], 1124),
    _cb("B1_Dc260", 260, [3], [1], 1125),
]


def cb_inputs(case):
    rng = np.random.default_rng(case["seed"])
    nh, nc, Dc = sum(case["hs"]), sum(case["cs"]), case["Dc"]
    # a shared component makes the cosines ~0.3 instead of ~Dc^-1/2, and d_bias ~ sqrt(Dc) makes the gradients of the unit
    # rows ~1: values and gradients well above the absolute tolerances at every width
    common = normal(rng, (1, Dc), 0.35)
    return dict(hc=normal(rng, (nh, Dc), 0.5) + common, cc=normal(rng, (nc, Dc), 0.5) + common,
                d_bias=normal(rng, nh, Dc ** 0.5),
                batch_hist=_batch(case["hs"]), batch_cand=_batch(case["cs"]),
                hist_off=_offsets(case["hs"]), cand_off=_offsets(case["cs"]))


def cb_ref(case, inp, dtype):
    hc, cc = _leaf(inp["hc"], dtype), _leaf(inp["cc"], dtype)
    bias = MO.categ_bias_flat(hc, cc, inp["batch_hist"], inp["batch_cand"], case["B"])
    g = torch.autograd.grad(bias, [hc, cc], inp["d_bias"].to(dtype))
    return dict(bias=bias.detach(), d_hc=g[0], d_cc=g[1])


# ---- MINER: poly attention --------------------------------------------------------------------------------------------------
def _poly(name, mh, hs, D, Cd, K, bias, seed):
    lds = (K + D) * mh * 4
    wide = mh > MINER_CFG["max_hist"] or D > MINER_CFG["Dn"] or Cd > MINER_CFG["Cd"] or K > MINER_CFG["K"]
    return dict(name=name, max_hist=mh, hs=hs, B=len(hs), D=D, Cd=Cd, K=K, bias=bias, seed=seed, lds=lds, wide=wide)


LDS_MAX, LDS_RAISE = 160 * 1024, 64 * 1024
# n in {0, 1, max_hist - 1, max_hist} in one batch (n = max_hist: no fill term, the maximum starts at -inf); K in {1, 4, 5,
# 32}; with and without bias; n = 70, K = 5: the lane loops and K n > 256; LDS requests of 82 KiB (the attribute raise), of
# exactly 160 KiB (still the tile) and one step over it (``tile_in_lds = 0``), one full history among short ones
POLY_CASES = [
    _poly("mh6_K1_bias", 6, [0, 1, 5, 6], 8, 4, 1, True, 1140),
    _poly("mh7_K4_nobias", 7, [7, 0, 6, 1], 12, 8, 4, False, 1141),
    _poly("mh50_K32_D256_Cd200_bias", 50, [0, 1, 49, 50], 256, 200, 32, True, 1142),
    _poly("n70_K5_lane_loops", 72, [70, 3], 8, 4, 5, True, 1143),
    _poly("lds_82k_raise", 128, [128, 2], 160, 8, 4, False, 1144),
    _poly("lds_160k_tile", 128, [128, 1, 0], 316, 8, 4, True, 1145),
    _poly("lds_over_cache_path", 128, [128, 1, 0], 320, 8, 4, True, 1146),
]


def poly_inputs(case):
    rng = np.random.default_rng(case["seed"])
    nh, D, Cd, K, B = sum(case["hs"]), case["D"], case["Cd"], case["K"], case["B"]
    inp = dict(E=normal(rng, (nh, D), 0.5), P=torch.tanh(normal(rng, (nh, Cd), 0.8)), codes=normal(rng, (K, Cd), 1.5 * Cd ** -0.5),
               bias=normal(rng, nh, 0.3) if case["bias"] else None, d_uv=normal(rng, (B, K, D), 1.0),
               batch_hist=_batch(case["hs"]), hist_off=_offsets(case["hs"]))
    return inp


def poly_ref(case, inp, dtype):
    B, D, Cd, mh = case["B"], case["D"], case["Cd"], case["max_hist"]
    E, P, codes = _leaf(inp["E"], dtype), _leaf(inp["P"], dtype), _leaf(inp["codes"], dtype)
    bias = _leaf(inp["bias"], dtype) if case["bias"] else None
    dense, mask = to_dense_batch(torch.cat([E, torch.atanh(P)], dim=1), inp["batch_hist"], B, mh)
    w = torch.cat([torch.zeros(Cd, D, dtype=dtype), torch.eye(Cd, dtype=dtype)], dim=1)
    # (the bias of the reference is (B, H, n_cand) and enters as its mean over the last axis: one column is its own mean)
    bias_dense = to_dense_batch(bias.unsqueeze(1), inp["batch_hist"], B, mh)[0] if bias is not None else None
    out, weights = MO.poly_attention(dense, mask, w, codes, bias_dense)
    uv = out[..., :D]
    leaves = [E, P, codes] + ([bias] if bias is not None else [])
    g = torch.autograd.grad(uv, leaves, inp["d_uv"].to(dtype))
    ref = dict(uv=uv.detach(), weights=weights.detach(), d_E=g[0], d_P=g[1], d_codes=g[2])
    if bias is not None:
        ref["d_bias"] = g[3]
    return ref


# ---- MINER: scores ----------------------------------------------------------------------------------------------------------
def _sc(name, K, D, cs, max_cand, seed, modes=MO.SCORE_TYPES, tie=None):
    wide = K > MINER_CFG["K"] or D > MINER_CFG["Dn"]
    return dict(name=name, K=K, D=D, B=len(cs), cs=cs, max_cand=max_cand, seed=seed, modes=tuple(modes), tie=tie, wide=wide)


# every K in {1, 2, 63, 64, 65, 255} (lane k owns codes k, k + 64, ...; the one-byte arg-max at K = 255) and every D in {4, 64,
# 68, 256} in every mode; candidate counts 0, 1, 3, 4, 5 (the four-wave round) and 31, 32, 33, 65 (the backward's tile of 32);
# max_cand above every count, once by more than 256 (the zero-fill stride); weighted at K = 255, D = 76: 158,296 bytes of LDS
SCORE_CASES = [
    _sc("K1_D4", 1, 4, [0, 1, 3, 4, 5], 6, 1160),
    _sc("K2_D68", 2, 68, [31, 32, 33], 34, 1161),
    _sc("K63_D64", 63, 64, [65, 0, 4], 66, 1202),
    _sc("K64_D256", 64, 256, [5, 0, 1, 4, 3], 6, 1163),
    _sc("K65_D64_fill300", 65, 64, [3], 300, 1164),
    _sc("K255_D64", 255, 64, [33, 31, 32], 34, 1285),
    _sc("K255_D76_lds_limit", 255, 76, [5, 0, 2], 6, 1166, modes=("weighted",)),
    _sc("tie_K5_D8", 5, 8, [6, 3], 7, 1167, modes=("max",), tie=(0, 1, 3)),       # (user, k1, k2)
]
TIE_ROWS = 3                     # candidates 0 .. 2 of the tie user point along the doubled interest row


def score_inputs(case):
    rng = np.random.default_rng(case["seed"])
    K, D, B, nc = case["K"], case["D"], case["B"], sum(case["cs"])
    inp = dict(cand=normal(rng, (nc, D), 0.5), uv=normal(rng, (B, K, D), 0.5), Z=normal(rng, (B, K, D), 1.0),
               d_scores=normal(rng, (B, case["max_cand"]), 1.0), cand_off=_offsets(case["cs"]), batch_cand=_batch(case["cs"]))
    if case["tie"]:
        b, k1, k2 = case["tie"]
        inp["uv"][b, k2] = inp["uv"][b, k1]
        c0 = int(inp["cand_off"][b])
        inp["cand"][c0:c0 + TIE_ROWS] = 2.0 * inp["uv"][b, k1] + 0.05 * inp["cand"][c0:c0 + TIE_ROWS]
    return inp


def lowest_index_max(S):
    """max over the last axis with the whole gradient at the LOWEST index of the maximum, written out (not ``torch.max``)."""
    K = S.shape[-1]
    rank = torch.arange(K, 0, -1, dtype=S.dtype)                     # K, K - 1, ..., 1: distinct, largest at the lowest index
    idx = ((S == S.max(dim=-1, keepdim=True)[0]).to(S.dtype) * rank).argmax(dim=-1)
    return S.gather(-1, idx.unsqueeze(-1)).squeeze(-1), idx


def score_matching(case, inp, dtype, leaves=None):
    """-> (S (B, max_cand, K) matching scores, dense candidates, mask)."""
    cand, uv = leaves if leaves is not None else (inp["cand"].to(dtype), inp["uv"].to(dtype))
    dense, mask = to_dense_batch(cand, inp["batch_cand"], case["B"], case["max_cand"])
    return dense @ uv.permute(0, 2, 1), dense, mask


def score_gaps(case, inp):
    """float64 top-two gap over k of every real candidate (inf at K = 1); the tie pair counts as one code."""
    S, _, mask = score_matching(case, inp, torch.float64)
    if case["tie"]:
        S = S.clone()
        S[case["tie"][0], :, case["tie"][2]] = -float("inf")
    if case["K"] == 1:
        return torch.full((int(mask.sum()),), float("inf"), dtype=torch.float64)
    top = torch.topk(S, 2, dim=-1)[0]
    return (top[..., 0] - top[..., 1])[mask]


def score_ref(case, inp, dtype):
    ref = {}
    for mode in case["modes"]:
        cand, uv, Z = _leaf(inp["cand"], dtype), _leaf(inp["uv"], dtype), _leaf(inp["Z"], dtype)
        S, dense, mask = score_matching(case, inp, dtype, (cand, uv))
        if case["tie"]:
            agg, idx = lowest_index_max(S)
        else:
            agg = MO.aggregate(S, mode, Z, dense, torch.eye(case["D"], dtype=dtype))
        scores = torch.where(mask, agg, torch.zeros((), dtype=dtype))
        leaves = [cand, uv] + ([Z] if mode == "weighted" else [])
        g = torch.autograd.grad(scores, leaves, inp["d_scores"].to(dtype))
        ref[mode] = dict(scores=scores.detach(), mask=mask, d_cand=g[0], d_uv=g[1])
        if mode == "weighted":
            ref[mode]["d_Z"] = g[2]
        if case["tie"]:
            ref[mode]["argmax"] = idx
    return ref


# ---- MINER: cosine disagreement ---------------------------------------------------------------------------------------------
def _cosd(name, G, R, D, eps, seed, zero_row=None):
    return dict(name=name, G=G, R=R, D=D, eps=eps, seed=seed, zero_row=zero_row, wide=R > MINER_CFG["K"] or D > MINER_CFG["Dn"])


# R = 1, 2, 4, 5, 32 (one row per wave: both sides of the 4 waves) and 65; D / 4 = 1, 64, 65, 257 (the lane loop and the
# 256-thread loop); one group and three; eps 1e-8 (the disagreement loss) and 0 (its late-fusion form: one group of the
# users' mean vectors); one zero row under eps = 1e-8
COSD_CASES = [
    _cosd("G1_R1_D4_eps", 1, 1, 4, 1e-8, 1180),
    _cosd("G3_R2_D256_eps", 3, 2, 256, 1e-8, 1181),
    _cosd("G3_R4_D260_eps0", 3, 4, 260, 0.0, 1182),
    _cosd("G1_R5_D1028_eps", 1, 5, 1028, 1e-8, 1183),
    _cosd("G3_R32_D4_eps0", 3, 32, 4, 0.0, 1184),
    _cosd("late_fusion_G1_R65_D256_eps0", 1, 65, 256, 0.0, 1185),
    _cosd("zero_row_G3_R5_D8_eps", 3, 5, 8, 1e-8, 1186, zero_row=(1, 2)),
]


def cosd_inputs(case):
    rng = np.random.default_rng(case["seed"])
    G, R, D = case["G"], case["R"], case["D"]
    # a shared component per group makes the cosines ~0.3 instead of ~D^-1/2; the upstream gradient G R |x| undoes the
    # 1 / (G R R) of the mean and the 1 / |x| of the normalisation, so that d_x is ~1 and not below the tolerance itself
    x = normal(rng, (G, R, D), 0.5) + normal(rng, (G, 1, D), 0.35)
    if case["zero_row"]:
        x[case["zero_row"]] = 0.0
    return dict(x=x, w=torch.tensor(G * R * 0.6 * D ** 0.5 * (1.0 + float(rng.random())), dtype=torch.float32))


def cosd_ref(case, inp, dtype):
    x = _leaf(inp["x"], dtype)
    if case["eps"] > 0:
        loss = MO.cosine_3d(x).mean()
    else:
        loss = torch.stack([MO.cosine_2d(x[g], x[g], zero_diagonal=True) for g in range(case["G"])]).mean()
    (d_x,) = torch.autograd.grad(loss * inp["w"].to(dtype), [x])
    return dict(loss=loss.detach(), d_x=d_x)


# ---- CAUM: the three dropout ops --------------------------------------------------------------------------------------------
def _drop(B, C, H, D, F_, U, p, base, seed):
    return dict(name=f"B{B}_C{C}_H{H}_D{D}_F{F_}_U{U}_p{p}_base{base}", B=B, C=C, H=H, D=D, F=F_, U=U, p=p, base=base, seed=seed,
                wide=False)


# B in {1, 3}, C in {1, 4}, H in {1, 3}; D, F, U each at 1, 3, 4, 5, 8; p in {0, 0.2, 0.5}; stream bases != 0, also ones that
# are no multiple of 3 and not the module's 16
DROP_CASES = [
    _drop(1, 1, 1, 1, 1, 1, 0.5, 16, 1200),
    _drop(3, 4, 3, 3, 3, 5, 0.2, 19, 1201),
    _drop(3, 4, 1, 4, 4, 3, 0.5, 16, 1202),
    _drop(1, 4, 3, 5, 5, 4, 0.0, 22, 1203),
    _drop(3, 1, 3, 8, 8, 1, 0.2, 7, 1204),
    _drop(3, 4, 3, 8, 1, 8, 0.5, 100, 1205),
]


def slot_masks(case, i):
    """The masks of candidate slot i as ``caum_oracle.caum_forward`` numbers them (streams base + 3 i + {0, 1, 2}):
    dropout1 over (B, D), dropout2 over (B, H, D), dropout3 over (B, H, F + U)."""
    B, H, D, W, p = case["B"], case["H"], case["D"], case["F"] + case["U"], case["p"]
    b = case["base"] + 3 * i
    return [dropout_multiplier(DROP_SEED, b, p, (B, D)), dropout_multiplier(DROP_SEED, b + 1, p, (B, H, D)),
            dropout_multiplier(DROP_SEED, b + 2, p, (B, H, W))]


def drop_inputs(case):
    B, C, H, D, F_, U = (case[k] for k in ("B", "C", "H", "D", "F", "U"))
    rng = np.random.default_rng(case["seed"])
    R = B * C * H
    return dict(h=normal(rng, (B, H, D), 1.0), c=normal(rng, (B, C, D), 1.0), cnn=normal(rng, (R, F_), 1.0), a=normal(rng, (R, U), 1.0),
                d_h=normal(rng, (B, H, D), 1.0), d_hd=normal(rng, (B, C, H, D), 1.0), d_cd=normal(rng, (B, C, D), 1.0),
                d_z=normal(rng, (R, F_ + U), 1.0))


def drop_ref(case, inp, dtype):
    """In float32 every forward value is one product, and so is every backward value but ``d_h`` of the expand op, a sum over
    the slots in slot order from 0: the float32 evaluation is what the kernels must give bit for bit (the backward where the
    multipliers are 1 or 2)."""
    B, C, H, D, F_, U = (case[k] for k in ("B", "C", "H", "D", "F", "U"))
    t = lambda k: inp[k].to(dtype)  # noqa: E731
    m = [[x.to(dtype) for x in slot_masks(case, i)] for i in range(C)]
    m1 = torch.stack([m[i][0] for i in range(C)], dim=1)             # (B, C, D)
    m2 = torch.stack([m[i][1] for i in range(C)], dim=1)             # (B, C, H, D)
    m3 = torch.stack([m[i][2] for i in range(C)], dim=1)             # (B, C, H, F + U)
    plain = dropout_multiplier(DROP_SEED, case["base"], case["p"], (B, H, D)).to(dtype)      # ``DropoutFn``: one stream
    ref = dict(y=t("h") * plain, d_x=t("d_h") * plain)
    ref["hd"], ref["cd"] = t("h").unsqueeze(1) * m2, t("c") * m1
    d_h = torch.zeros((B, H, D), dtype=dtype)
    for i in range(C):
        d_h = d_h + t("d_hd")[:, i] * m2[:, i]
    ref["d_h"], ref["d_c"] = d_h, t("d_cd") * m1
    z = torch.cat([t("cnn"), t("a")], dim=1).reshape(B, C, H, F_ + U) * m3
    dz = t("d_z").reshape(B, C, H, F_ + U) * m3
    ref["z"] = z.reshape(-1, F_ + U)
    ref["d_cnn"], ref["d_a"] = dz.reshape(-1, F_ + U)[:, :F_].contiguous(), dz.reshape(-1, F_ + U)[:, F_:].contiguous()
    return ref


# ---- CAUM: candi-CNN + linear2 from their parts -----------------------------------------------------------------------------
def _comb(B, C, H, F_, U, hs, seed):
    return dict(name=f"B{B}_C{C}_H{H}_F{F_}_U{U}_hs{hs}", B=B, C=C, H=H, F=F_, U=U, hs=hs, seed=seed,
                wide=F_ > CAUM_CFG["F"] or U > CAUM_CFG["U"])


# H = 1 (left = self = right) and 2 (left = right); the history per slot (hs = C) and shared (hs = 1: d_P sums over the
# slots); F, U at 1, 3, 4, 5; the configured width
COMB_CASES = [
    _comb(1, 1, 1, 1, 1, 1, 1220),
    _comb(2, 3, 2, 3, 4, 3, 1221),
    _comb(2, 3, 3, 4, 5, 1, 1222),
    _comb(1, 3, 7, 5, 3, 3, 1223),
    _comb(3, 1, 2, 4, 1, 1, 1224),
    _comb(2, 3, 1, 5, 4, 1, 1225),
    _comb(2, 2, 5, 400, 400, 2, 1226),
]


def comb_inputs(case):
    B, C, H, F_, U, hs = (case[k] for k in ("B", "C", "H", "F", "U", "hs"))
    rng = np.random.default_rng(case["seed"])
    return dict(P=normal(rng, (B * hs * H, 3 * F_ + U), 0.5), Q=normal(rng, (B * C, F_ + U), 0.5),
                d_cnn=normal(rng, (B * C * H, F_), 1.0), d_s=normal(rng, (B * C * H, U), 1.0))


def combine(P, Q, B, C, H, F_, U, hs):
    """user/caum.py:97-110 after the projections are split by input block (``caum_oracle.user_encoder_slot``: ``left`` is the
    row above, circular, ``right`` the row below): P (B hs H, [W1a h | W1b h | W1c h | W2b h]), Q (B C, [W1d c | W2a c])."""
    P = P.reshape(B, hs, H, 3 * F_ + U).expand(B, C, H, 3 * F_ + U) if hs == 1 else P.reshape(B, C, H, 3 * F_ + U)
    Q = Q.reshape(B, C, 1, F_ + U)
    a, b, c, d = P[..., :F_], P[..., F_:2 * F_], P[..., 2 * F_:3 * F_], P[..., 3 * F_:]
    left = torch.cat([a[:, :, -1:], a[:, :, :-1]], dim=-2)
    right = torch.cat([c[:, :, 1:], c[:, :, :1]], dim=-2)
    return (left + b + right + Q[..., :F_]).reshape(-1, F_), (d + Q[..., F_:]).reshape(-1, U)


def comb_ref(case, inp, dtype):
    P, Q = _leaf(inp["P"], dtype), _leaf(inp["Q"], dtype)
    cnn, s = combine(P, Q, *(case[k] for k in ("B", "C", "H", "F", "U", "hs")))
    g = torch.autograd.grad([cnn, s], [P, Q], [inp["d_cnn"].to(dtype), inp["d_s"].to(dtype)], retain_graph=True)
    g_cnn = torch.autograd.grad(cnn, [P, Q], inp["d_cnn"].to(dtype))          # only d_cnn arrives: d_s is None
    return dict(cnn=cnn.detach(), s=s.detach(), d_P=g[0], d_Q=g[1], d_P_cnn_only=g_cnn[0], d_Q_cnn_only=g_cnn[1])


# ---- CAUM: grouped tanh -----------------------------------------------------------------------------------------------------
GTANH_CASES = [dict(name=f"G{g}_rows{r}_N{n}", G=g, rows=r, N=n, seed=1240 + i, wide=False)
               for i, (g, r, n) in enumerate([(1, 1, 1), (3, 7, 5), (4, 50, 200)])]


def gtanh_inputs(case):
    G, r, N = case["G"], case["rows"], case["N"]
    rng = np.random.default_rng(case["seed"])
    return dict(a=normal(rng, (G * r, N), 0.7), g=normal(rng, (G, N), 0.7), d_z=normal(rng, (G * r, N), 1.0))


def group_tanh(a, g, rows):
    """DenseAttention's first layer (``tanh(linear([x, rep]))`` in ``caum_oracle.user_encoder_slot``) from its history part a
    (G rows, N) and its candidate part g (G, N), the bias inside either."""
    return torch.tanh(a + g.repeat_interleave(rows, dim=0))


def gtanh_ref(case, inp, dtype):
    a, g = _leaf(inp["a"], dtype), _leaf(inp["g"], dtype)
    z = group_tanh(a, g, case["rows"])
    gr = torch.autograd.grad(z, [a, g], inp["d_z"].to(dtype))
    return dict(z=z.detach(), d_a=gr[0], d_g=gr[1])


# ---- CAUM: DenseAttention's last layer, softmax, user vector, score ---------------------------------------------------------
def _cs(name, B, C, H, N2, U, counts, slot0, seed):
    return dict(name=name, B=B, C=C, H=H, N2=N2, U=U, counts=counts, slot0=slot0, seed=seed,
                wide=N2 > CAUM_CFG["N2"] or U > CAUM_CFG["U"])


# R = B C H at 1, 63, 64, 65, 129 (the 64-row chunks of the column sum) and 514; H in {1, 3, 4, 5, 64, 257} (H > 256: the
# strided weight loop) and the limit 8192; N2 and U on both sides of 64 lanes and 256 threads; ragged candidate lists with a
# user without candidates, slot0 in {0, 2}
CSCORE_CASES = [
    _cs("R1", 1, 1, 1, 1, 1, [1], 0, 1260),
    _cs("R63_slot2", 3, 7, 3, 63, 63, [9, 0, 4], 2, 1261),
    _cs("R64", 4, 4, 4, 64, 64, [4, 0, 2, 1], 0, 1262),
    _cs("R64_H64", 1, 1, 64, 65, 65, [1], 0, 1263),
    _cs("R65_slot2_N200_U400", 1, 13, 5, 200, 400, [9], 2, 1264),
    _cs("R129_U257", 43, 1, 3, 1, 257, [1, 0, 2] * 14 + [1], 0, 1265),
    _cs("H257", 1, 2, 257, 5, 4, [1], 0, 1266),
    _cs("H8192_limit", 1, 1, 8192, 1, 1, [3], 2, 1267),
]


def cscore_peaks(H):
    return (0, 255, 256, H - 1)


def cscore_inputs(case):
    B, C, H, N2, U = (case[k] for k in ("B", "C", "H", "N2", "U"))
    rng = np.random.default_rng(case["seed"])
    R = B * C * H
    valid = (case["slot0"] + torch.arange(C)).unsqueeze(0) < torch.tensor(case["counts"]).unsqueeze(1)
    z2, w3 = torch.tanh(normal(rng, (R, N2), 1.0)), normal(rng, (1, N2), 1.5 * N2 ** -0.5)
    if H > 256:
        # a softmax over thousands of near-equal logits gives every row a weight below the forward tolerance, and a row that
        # is dropped or read twice would not show: the first and last row and both sides of the 256-thread stride take
        # most of the weight (logit 12 against at most 4.8 elsewhere)
        w3[0, 0] = 12.0
        z2[:, 0] *= 0.4
        z2.reshape(B * C, H, N2)[:, list(cscore_peaks(H)), 0] = 0.999
    return dict(z2=z2, w3=w3, b3=normal(rng, 1, 0.3),
                x=normal(rng, (R, U), 0.5), cd=normal(rng, (B * C, U), 0.5), d_scores=normal(rng, (B, C), 1.0),
                cand_off=_offsets(case["counts"]), valid=valid,
                prefill_w3=normal(rng, (1, N2), 1.0), prefill_b3=normal(rng, 1, 1.0))


def dense_att_score(z2, w3, b3, x, cd, G, H):
    """The last lines of ``caum_oracle.user_encoder_slot`` for G = B C (impression, slot) groups at once: layer 3, the softmax
    over the H history slots, the user vector, the score.  -> (G)."""
    w = torch.softmax((z2 @ w3.t() + b3).reshape(G, H), dim=-1)
    user = torch.bmm(w.unsqueeze(1), x.reshape(G, H, -1)).squeeze(1)
    return (cd * user).sum(-1)


def cscore_ref(case, inp, dtype):
    B, C, H = case["B"], case["C"], case["H"]
    keys = ("z2", "w3", "b3", "x", "cd")
    leaves = [_leaf(inp[k], dtype) for k in keys]
    s = dense_att_score(*leaves, B * C, H).reshape(B, C)
    scores = torch.where(inp["valid"], s, torch.zeros((), dtype=dtype))
    g = torch.autograd.grad(scores, leaves, inp["d_scores"].to(dtype))
    ref = {"d_" + k: gr for k, gr in zip(keys, g)}
    ref["scores"] = scores.detach()
    return ref


# ---- one reference per (case, dtype) for the whole session: computed once, never modified -----------------------------------
FAMILIES = {
    "lin": (LIN_CASES, lin_inputs, lin_ref),
    "wgrad": (WGRAD_CASES, lin_inputs, wgrad_ref),
    "cb": (CB_CASES, cb_inputs, cb_ref),
    "poly": (POLY_CASES, poly_inputs, poly_ref),
    "score": (SCORE_CASES, score_inputs, score_ref),
    "cosd": (COSD_CASES, cosd_inputs, cosd_ref),
    "drop": (DROP_CASES, drop_inputs, drop_ref),
    "comb": (COMB_CASES, comb_inputs, comb_ref),
    "gtanh": (GTANH_CASES, gtanh_inputs, gtanh_ref),
    "cscore": (CSCORE_CASES, cscore_inputs, cscore_ref),
}


def tolerance(case, kind, want, want32, engine="f32"):
    """The asserted bound of one comparison: ``Report.fwd`` / ``Report.grad``, and for a ``wide`` case ``Report.bound`` over
    the same number (the larger of it and 4x the float32 restatement's error)."""
    ftol, gtol = TOL[engine]
    top = float(want.abs().max()) if want.numel() else 0.0
    tol = 5 * ftol if kind == "fwd" else gtol * max(1.0, top)
    if case["wide"]:
        e32 = float((want32.double() - want).abs().max()) if want.numel() else 0.0
        tol = max(tol, 4 * e32)
    return tol


@functools.lru_cache(maxsize=None)
def cached_inputs(family: str, index: int):
    cases, make, _ = FAMILIES[family]
    return make(cases[index])


@functools.lru_cache(maxsize=None)
def cached(family: str, index: int, dtype_name: str):
    cases, _, ref = FAMILIES[family]
    return ref(cases[index], cached_inputs(family, index), getattr(torch, dtype_name))
