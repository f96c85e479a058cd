"""Input generators, case tables and float64 / float32 CPU references of the op-level shape sweep of the ops under LSTUR, NAML,
TANR, CenNewsRec and MINS (tests/test_gpu_lstur_naml_sweep.py): ``CnnEncoderFn``, ``GruFn``, ``EmbeddingRowsFn``
(ops_lstur.py), ``AdditiveAttentionFn`` and ``LinearActFn`` (ops_blocks.py).  Their properties are asserted on the host in
tests/test_lstur_naml_sweep_host.py.  Plain module: no fixtures, no GPU.

References are the existing restatements, called with float64 leaves (the reference) and float32 leaves (the yardstick):
``oracle.lstur_oracle.cnn_text_encoder_fwd`` and ``gru_last_hidden``, ``oracle.nrms_oracle.additive_attention``; linear +
activation is ``act(a @ w.T + b)``, the embedding rows are ``table[ids] * mult`` and ``index_add_``.  Gradients by autograd.

ReLU gates (the convolution of the CNN encoder, ``LinearActFn`` with ``relu``) get the grid-valued gate inputs of the NPA
sweep (tests/sweep_inputs.py, DESIGN.md "Shape sweeps against float64"): table / input entries multiples of 1/8 in [-1, 1],
weights multiples of 1/16 in [-1/2, 1/2], biases k/128 + 1/256, dropout p in {0, 0.5}.  A pre-activation is then exact in
fp32 in any summation order and under bf16x3, and an odd multiple of 1/256: no gate decides differently anywhere.  Grid
pre-activations have rms ~0.25 sqrt(W D), so ``W_a`` is scaled by 1 / (sqrt(F) z_rms) and the tanh projection does not
saturate.  Everything without a gate (GRU, additive attention, linear with ``none`` / ``tanh``) gets random inputs at the
scales of tests/test_gpu_lstur.py and tests/test_gpu_naml.py.

The ``*_predicates`` functions restate the library's shape predicates (nrl_api_lstur.hip, nrl_gru_fused.h, the pooling
kernels of nrl_kernels.hip, ``gemm_fwd`` / ``gemm_wgrad`` of nrl_api_internal.h) in Python: the host test asserts with them
that both outcomes of every predicate are in the tables."""
from __future__ import annotations

import functools

import numpy as np
import torch

from oracle.lstur_oracle import CNN_KEYS, cnn_text_encoder_fwd, gru_last_hidden
from oracle.nrms_oracle import additive_attention, dropout_multiplier
from tests.sweep_inputs import DROP_SEED, TOL, _leaf, grid, grid_bias, normal  # noqa: F401  (TOL: re-exported)

STREAM0 = 2                      # first dropout stream of the CNN encoder calls
VOCAB = 29
# the widths the project's bounds were set at (tests/test_gpu_lstur.py, tests/test_gpu_naml.py): a case above one is ``wide``
GRU_HD_SET, POOL_WIDTH_SET, LIN_N_SET, LIN_K_SET = 700, 400, 400, 100


# ---- CNN text encoder -------------------------------------------------------------------------------------------------------
ID_PATTERNS = ("mixed", "no_pad", "one_all_pad_title", "all_pad")


def _cnn(name, N, L, D, F_, W, Q, p, seed, ids="mixed"):
    return dict(name=name, N=N, L=L, D=D, F=F_, W=W, Q=Q, p=p, seed=seed, ids=ids)


def _p(i):
    return (0.0, 0.5)[i % 2]


CNN_BASE = (5, 9, 16, 12, 3, 12)                 # (N, L, D, F, W, Q)
CNN_CASES = (
    # L: the planes form ends at 63, its k-tiles switch at 31 / 32; one token, fewer tokens than the window
    [_cnn(f"L{l}", 5, l, 16, 12, 3, 12, _p(i), 2000 + i) for i, l in enumerate([1, 2, 3, 15, 16, 17, 31, 32, 33, 63, 64, 65])]
    # W != 3: planes off, row-panel on; L = 2 under W = 5, 7: most taps of every window cross the news boundary
    + [_cnn(f"W{w}_L{l}", 5, l, 16, 12, w, 12, _p(i), 2020 + i) for i, (w, l) in enumerate([(1, 3), (5, 9), (7, 2), (7, 9), (5, 2)])]
    # F: aa planes on at 12, 28, 300; off at 16, 32, 304 (F % 16 == 0), 316 (> 304); conv planes / row-panel off above 320
    + [_cnn(f"F{f}", 5, 9, 16, f, 3, 12, _p(i), 2030 + i) for i, f in enumerate([12, 28, 16, 32, 300, 304, 316, 320, 324, 400])]
    # Q: rp_nblk_for 13 -> 19 at 208 / 212, aa planes last / off at 224 / 228, row-panel off above 320
    + [_cnn(f"Q{q}", 5, 9, 16, 12, 3, q, _p(i), 2040 + i) for i, q in enumerate([4, 8, 208, 212, 224, 228, 320, 324])]
    # D: cnn_ncb_x's even padding (4, 12 -> 2; 16, 28 -> 2 / 2; 32 -> 4), rp_nblk_for 19 -> 20 at 304 / 308, row-panel off above 320
    + [_cnn(f"D{d}", 5, 9, d, 12, 3, 12, _p(i), 2050 + i) for i, d in enumerate([4, 12, 28, 32, 300, 304, 308, 320, 324])]
    # M % 32 (F = 12: the cleared last tile of the c / d_pre planes)
    + [_cnn(f"M{n * l}", n, l, 16, 12, 3, 12, _p(i), 2060 + i) for i, (n, l) in enumerate([(4, 8), (3, 11), (8, 8)])]
    # one news; more than 2048 news: the persistent loop of pool_bwd_pre_kernel
    + [_cnn("N1", 1, 9, 16, 12, 3, 12, 0.5, 2070), _cnn("N2049_L1", 2049, 1, 16, 12, 3, 12, 0.0, 2071),
       _cnn("N2049_L2", 2049, 2, 16, 12, 3, 12, 0.5, 2072)]
    # id patterns (``mixed`` is the F12 case above)
    + [_cnn("ids_no_pad", *CNN_BASE, 0.5, 2080, ids="no_pad"), _cnn("ids_one_all_pad_title", *CNN_BASE, 0.0, 2081, ids="one_all_pad_title"),
       _cnn("ids_all_pad", *CNN_BASE, 0.5, 2082, ids="all_pad"), _cnn("ids_all_pad_N1", 1, 9, 16, 12, 3, 12, 0.0, 2083, ids="all_pad")]
    # one short title: M Q < 2 M + ceil(M / 2048) + 8 (the live-row list did not fit the tanh buffer) and the first shapes past it
    + [_cnn(f"tiny_L{l}_Q{q}", 1, l, 16, 12, 3, q, _p(i), 2090 + i, ids="no_pad")
       for i, (l, q) in enumerate([(1, 4), (1, 8), (2, 4), (4, 4), (1, 12), (2, 8), (5, 4)])]
    + [_cnn("full", 5, 30, 300, 300, 3, 200, 0.5, 2099)])
CNN_TINY_REFUSED = [(1, 1, 4), (1, 1, 8), (1, 2, 4), (1, 4, 4)]        # (N, L, Q): refused by the backward before the fix
CNN_TINY_ACCEPTED = [(1, 1, 12), (1, 2, 8), (1, 5, 4)]


def live_list_fits(N, L, Q):
    """The condition ``cnn_dx_table_grad`` used to require of the tanh buffer (M Q floats) it carved the list out of."""
    M = N * L
    return M * Q >= 2 * M + -(-M // 2048) + 8


def cnn_predicates(c):
    """nrl_api_lstur.hip under bf16x3 with every switch at its default."""
    N, L, D, F_, W, Q = (c[k] for k in ("N", "L", "D", "F", "W", "Q"))
    nblk = lambda n: 13 if n <= 208 else (19 if n <= 304 else 20)  # noqa: E731
    conv_planes = W == 3 and L <= 63 and F_ <= 320
    rp = D <= 320 and F_ <= 320 and Q <= 320
    x_planes = conv_planes and rp
    aa_planes = x_planes and F_ % 16 == 12 and F_ <= 304 and Q <= 224
    return dict(conv_planes=conv_planes, kt=1 if L <= 31 else 2, rp=rp, x_planes=x_planes, aa_planes=aa_planes,
                nblk=(nblk(D), nblk(F_), nblk(Q)) if rp else None, m_rem=(N * L) % 32 != 0,
                ncb_x_padded=((D + 16) // 16) % 2 == 1, ncb_dc_padded=((F_ + 15) // 16) % 2 == 1,
                live=rp, persistent_pool=N > 2048)


def cnn_ids(case, rng):
    N, L = case["N"], case["L"]
    ids = rng.integers(1, VOCAB, (N, L))
    pat = case["ids"]
    if pat == "mixed":                               # id 0 first in one title, in the middle of another, a tail of pads
        ids[0, 0] = 0
        ids[1 % N, L // 2] = 0
        ids[N - 1, L - max(1, L // 4):] = 0
    elif pat == "one_all_pad_title":
        ids[N // 2, :] = 0
    elif pat == "all_pad":
        ids[:] = 0
    return torch.from_numpy(ids)


def cnn_inputs(case):
    N, L, D, F_, W, Q = (case[k] for k in ("N", "L", "D", "F", "W", "Q"))
    rng = np.random.default_rng(case["seed"])
    ids = cnn_ids(case, rng)
    z_rms = max(1.0, 0.25 * (W * D) ** 0.5)
    params = [grid(rng, (VOCAB, D), 1 / 8, 1.0), grid(rng, (F_, 1, W, D), 1 / 16, 0.5), grid_bias(rng, F_),
              normal(rng, (Q, F_), 1.0 / (F_ ** 0.5 * z_rms)), normal(rng, Q, 0.05), normal(rng, Q, 0.1)]
    return dict(ids=ids, params=dict(zip(CNN_KEYS, params)), d_out=normal(rng, (N, F_), 1.0))


def cnn_masks(case):
    N, L, D, F_, p = (case[k] for k in ("N", "L", "D", "F", "p"))
    if p <= 0:
        return None, None
    return dropout_multiplier(DROP_SEED, STREAM0, p, (N, L, D)), dropout_multiplier(DROP_SEED, STREAM0 + 1, p, (N, L, F_))


def cnn_pre(case, inp, dtype):
    """Pre-activations of the convolution (N, L, F) in the windowed form of ``cnn_text_encoder_fwd``, post-embedding dropout
    applied."""
    W, D, F_, N, L = (case[k] for k in ("W", "D", "F", "N", "L"))
    m1, _ = cnn_masks(case)
    x = inp["params"][CNN_KEYS[0]].to(dtype)[inp["ids"]]
    if m1 is not None:
        x = x * m1.to(dtype)
    pad = (W - 1) // 2
    xp = torch.zeros(N, L + 2 * pad, D, dtype=dtype)
    xp[:, pad:pad + L] = x
    win = torch.cat([xp[:, t:t + L] for t in range(W)], dim=2)
    return win @ inp["params"][CNN_KEYS[1]].to(dtype).reshape(F_, W * D).t() + inp["params"][CNN_KEYS[2]].to(dtype)


def cnn_ref(case, inp, dtype):
    leaves = {k: _leaf(v, dtype) for k, v in inp["params"].items()}
    m1, m2 = cnn_masks(case)
    if m1 is not None:
        m1, m2 = m1.to(dtype), m2.to(dtype)
    out = cnn_text_encoder_fwd(inp["ids"], leaves, "", m1, m2)
    g = list(torch.autograd.grad(out, [leaves[k] for k in CNN_KEYS], inp["d_out"].to(dtype)))
    g[0][0] = 0.0                                    # padding_idx = 0
    return dict(out=out.detach(), grads=dict(zip(CNN_KEYS, g)))


# ---- GRU --------------------------------------------------------------------------------------------------------------------
def _gru(name, B, T, Din, Hd, h0, seed, lengths="mixed"):
    return dict(name=name, B=B, T=T, Din=Din, Hd=Hd, with_h0=h0, seed=seed, lengths=lengths, wide=Hd > GRU_HD_SET)


GRU_CASES = (
    # Hd: the k + 3 < Hd / k + 7 < Hd loads and the unit clamp (4 .. 36), a wave's second k-tile slot (128 / 132), 3 Hd at 504 /
    # 516 (the weight-gradient kernel switch), TR 1 -> 2 (508 / 512), all 24 slots (768), the two-launch forward under bf16x3 (772)
    [_gru(f"Hd{h}", 5, 3, 8, h, i % 2 == 0, 2100 + i) for i, h in enumerate([4, 16, 20, 32, 36, 128, 132, 168, 172])]
    + [_gru("Hd508", 5, 2, 8, 508, True, 2110), _gru("Hd512", 5, 2, 8, 512, False, 2111), _gru("Hd768", 5, 2, 8, 768, True, 2112),
       _gru("Hd772_two_launch", 3, 2, 4, 772, True, 2113)]
    # rows: the clamp at B - 1 and the row tiles of 16 (TR = 1) and 32 (TR = 2)
    + [_gru(f"B{b}_Hd16", b, 3, 8, 16, i % 2 == 1, 2120 + i) for i, b in enumerate([1, 15, 16, 17, 33])]
    + [_gru(f"B{b}_Hd512", b, 2, 4, 512, i % 2 == 0, 2130 + i) for i, b in enumerate([31, 32, 33])]
    # workgroup counts 7 and 17 (1, 8, 9 are B1_Hd16, Hd128, Hd132) and 2 x 9 = 18 with two row tiles: the XCD remapping
    + [_gru("grid7", 5, 3, 8, 100, True, 2140), _gru("grid17", 5, 3, 8, 260, False, 2141), _gru("grid18_rows2", 17, 3, 8, 132, True, 2142)]
    # T and lengths
    + [_gru("T1", 5, 1, 8, 16, True, 2150), _gru("T5_len1", 5, 5, 8, 16, True, 2151, lengths="ones"),
       _gru("T4_full", 5, 4, 8, 16, False, 2152, lengths="full"), _gru("T4_full_h0", 5, 4, 8, 16, True, 2153, lengths="full")]
    # Din
    + [_gru(f"Din{d}", 5, 3, d, 16, i % 2 == 0, 2160 + i) for i, d in enumerate([4, 36, 324])]
    # h0 the other way on three of the cases above
    + [_gru("Hd36_no_h0", 5, 3, 8, 36, False, 2104), _gru("Hd512_h0", 5, 2, 8, 512, True, 2111), _gru("Hd772_no_h0", 3, 2, 4, 772, False, 2113)])


def gru_predicates(c):
    """nrl_gru_fwd under bf16x3: the fused step (nrl_gru_fused.h), or the two-launch ``gemm_step`` forward."""
    B, Hd = c["B"], c["Hd"]
    fused = Hd % 4 == 0 and Hd <= 768
    tr = 2 if Hd >= 512 else 1
    nk = -(-Hd // 32)
    return dict(fused=fused, tr=tr if fused else None, slots=-(-nk // 4) if fused else None,
                grid=-(-B // (16 * tr)) * -(-Hd // 16) if fused else None, row_tiles=-(-B // (16 * tr)),
                wgrad_big=3 * Hd > 512, row_clamp=B % (16 * tr) != 0, unit_clamp=Hd % 16 != 0, k_tail=Hd % 32 != 0)


def gru_lengths(case, rng):
    B, T = case["B"], case["T"]
    if case["lengths"] == "ones":
        return torch.ones(B, dtype=torch.int64)
    if case["lengths"] == "full":
        return torch.full((B,), T, dtype=torch.int64)
    lengths = torch.from_numpy(rng.integers(1, T + 1, B))
    lengths[0] = T
    return lengths


def gru_inputs(case):
    B, T, Din, Hd = (case[k] for k in ("B", "T", "Din", "Hd"))
    rng = np.random.default_rng(case["seed"])
    inp = dict(hist=normal(rng, (B, T, Din), 0.5), h0=normal(rng, (B, Hd), 0.5), lengths=gru_lengths(case, rng),
               w_ih=normal(rng, (3 * Hd, Din), Din ** -0.5), w_hh=normal(rng, (3 * Hd, Hd), Hd ** -0.5),
               b_ih=normal(rng, 3 * Hd, 0.05), b_hh=normal(rng, 3 * Hd, 0.05), d_out=normal(rng, (B, Hd), 1.0))
    return inp


GRU_KEYS = ("hist", "h0", "w_ih", "w_hh", "b_ih", "b_hh")


def gru_ref(case, inp, dtype):
    leaves = {k: _leaf(inp[k], dtype) for k in GRU_KEYS}
    h0 = leaves["h0"] if case["with_h0"] else torch.zeros(case["B"], case["Hd"], dtype=dtype)
    out = gru_last_hidden(leaves["hist"], inp["lengths"], h0, *(leaves[k] for k in GRU_KEYS[2:]))
    keys = [k for k in GRU_KEYS if k != "h0" or case["with_h0"]]
    g = torch.autograd.grad(out, [leaves[k] for k in keys], inp["d_out"].to(dtype))
    ref = {"d_" + k: gr for k, gr in zip(keys, g)}
    ref["out"] = out.detach()
    return ref


# ---- additive attention -----------------------------------------------------------------------------------------------------
def _aa(G, S, D, Q, seed):
    return dict(name=f"G{G}_S{S}_D{D}_Q{Q}", G=G, S=S, D=D, Q=Q, seed=seed, wide=D > POOL_WIDTH_SET or Q > POOL_WIDTH_SET,
                peaked=S > 256)


AA_CASES = (
    # S: the 16-row walk of the backward, the 64-lane softmax loops, the dynamic LDS at its limit
    [_aa(3, s, 8, 8, 2200 + i) for i, s in enumerate([1, 2, 15, 16, 17, 63, 64, 65, 129])] + [_aa(1, 8192, 4, 4, 2210)]
    # D: row-groups 256 (4), 85 with an idle thread (12), 3 (300), 1 with one idle thread (1020), 1 (1024), a second column pass (1028);
    # S = 1 at 1020: the idle thread and the column's owner have the same work
    + [_aa(3, 5, d, 8, 2220 + i) for i, d in enumerate([4, 12, 300, 1020, 1024, 1028])] + [_aa(3, 1, 1020, 8, 2226)]
    # Q: the same row-groups in the backward (4, 12, 300, 1024), 200, a second accq slot (1028), all four (4096)
    + [_aa(3, 5, 8, q, 2230 + i) for i, q in enumerate([4, 12, 200, 300, 1024, 1028])] + [_aa(2, 5, 8, 4096, 2236)]
    # G: no group; one; the backward grid on both sides of its persistent limit
    + [_aa(g, 2, 4, 4, 2240 + i) for i, g in enumerate([0, 1, 2047, 2048, 2049])])
AA_PEAKS = lambda S: (0, 63, 64, 255, 256, S - 1)  # noqa: E731


def aa_predicates(c):
    G, S, D, Q = (c[k] for k in ("G", "S", "D", "Q"))
    rg = lambda n: 256 // min(n // 4, 256)  # noqa: E731
    return dict(rg_fwd=rg(D), rg_bwd=rg(Q), idle_fwd=256 % min(D // 4, 256) != 0, idle_bwd=256 % min(Q // 4, 256) != 0,
                second_pass_fwd=D // 4 > 256, accq_slots=-(-(Q // 4) // 256), persistent=G > 2048,
                s16=S > 16, s64=S > 64, unroll_wrap=S > 8 * rg(Q),
                flush_strides=rg(Q) > 1 and Q > 256)        # the row-groups' sums: more floats than the workgroup has threads


def aa_inputs(case):
    G, S, D, Q = (case[k] for k in ("G", "S", "D", "Q"))
    rng = np.random.default_rng(case["seed"])
    inp = dict(y=normal(rng, (G, S, D), 0.5), w=normal(rng, (Q, D), D ** -0.5), b=normal(rng, Q, 0.05), q=normal(rng, Q, 0.1),
               d_out=normal(rng, (G, D), 1.0))
    if case["peaked"]:
        # a softmax over thousands of near-equal logits gives every row a weight below the forward tolerance, and a row that
        # is dropped or read twice would not show: the first and last row and both sides of the 64-lane and 256-thread
        # strides take most of the weight (logit 3 sum tanh(2) = 11.6 against ~1.2 rms elsewhere); D = Q = 4
        assert D == Q == 4
        inp["y"] = inp["y"] * 0.2
        inp["y"][:, list(AA_PEAKS(S)), :] = 1.0
        inp["w"], inp["b"], inp["q"] = 2.0 * torch.eye(4), torch.zeros(4), torch.full((4,), 3.0)
    return inp


AA_KEYS = ("y", "w", "b", "q")


def aa_ref(case, inp, dtype):
    leaves = [_leaf(inp[k], dtype) for k in AA_KEYS]
    out = additive_attention(*leaves)
    g = torch.autograd.grad(out, leaves, inp["d_out"].to(dtype))
    ref = {"d_" + k: gr for k, gr in zip(AA_KEYS, g)}
    ref["out"] = out.detach()
    return ref


# ---- linear + activation ----------------------------------------------------------------------------------------------------
ACTS = ("none", "tanh", "relu")


def _lin(M, N, K, act, seed, need_da=True):
    return dict(name=f"M{M}_N{N}_K{K}_{act}" + ("" if need_da else "_no_d_a"), M=M, N=N, K=K, act=act, seed=seed, need_da=need_da,
                wide=N > LIN_N_SET or K > LIN_K_SET)


LIN_CASES = (
    # N: the q-tile limits (208 under f32, 224 under bf16x3) and the weight-gradient switch at 512, every activation
    [_lin(9, n, 8, a, 2300 + 10 * i + j) for i, n in enumerate([4, 208, 212, 224, 228, 512, 516]) for j, a in enumerate(ACTS)]
    # M: no row (early return), one, both sides of 256
    + [_lin(m, 8, 8, a, 2400 + 10 * i + j) for i, m in enumerate([0, 1, 255, 256, 257]) for j, a in enumerate(ACTS)]
    # K: one k-step and its neighbours; 900 (the grid stays exact: 900 / 128 < 2^24 / 256)
    + [_lin(9, 8, k, "relu", 2500 + 10 * i) for i, k in enumerate([4, 28, 32, 36, 900])]
    + [_lin(9, 212, 8, "relu", 2600, need_da=False)])


def lin_predicates(c):
    return dict(q_tile_f32=c["N"] <= 208, q_tile_x3=c["N"] <= 224, wgrad_big=c["N"] > 512, empty=c["M"] == 0)


def lin_inputs(case):
    M, N, K = case["M"], case["N"], case["K"]
    rng = np.random.default_rng(case["seed"])
    if case["act"] == "relu":
        a, w, b = grid(rng, (M, K), 1 / 8, 1.0), grid(rng, (N, K), 1 / 16, 0.5), grid_bias(rng, N)
    else:
        a, w, b = normal(rng, (M, K), 1.0), normal(rng, (N, K), K ** -0.5), normal(rng, N, 0.1)
    return dict(a=a, w=w, b=b, d_c=normal(rng, (M, N), 1.0))


def lin_pre(case, inp, dtype):
    return inp["a"].to(dtype) @ inp["w"].to(dtype).t() + inp["b"].to(dtype)


def lin_ref(case, inp, dtype):
    a, w, b = (_leaf(inp[k], dtype) for k in ("a", "w", "b"))
    pre = a @ w.t() + b
    out = {"none": pre, "tanh": torch.tanh(pre), "relu": torch.relu(pre)}[case["act"]]
    g = torch.autograd.grad(out, [a, w, b], inp["d_c"].to(dtype))
    return dict(out=out.detach(), d_a=g[0], d_w=g[1], d_b=g[2])


# ---- embedding rows ---------------------------------------------------------------------------------------------------------
EMB_STREAM = 8


def _emb(n, V, D, p, seed, ids="random"):
    return dict(name=f"n{n}_V{V}_D{D}_p{p}" + ("" if ids == "random" else "_" + ids), n=n, V=V, D=D, p=p, seed=seed, ids=ids)


EMB_CASES = ([_emb(n, 40, d, p, 2700 + 4 * i + 2 * j + k) for i, n in enumerate([0, 1, 300]) for j, d in enumerate([4, 100])
              for k, p in enumerate([0.0, 0.5])]
             + [_emb(300, 40, 100, 0.5, 2720, ids="hot_row"), _emb(300, 40, 4, 0.0, 2721, ids="all_zero")])


def emb_inputs(case):
    n, V, D = case["n"], case["V"], case["D"]
    rng = np.random.default_rng(case["seed"])
    ids = rng.integers(0, V, n)
    if case["ids"] == "hot_row":
        ids[:] = 7
    elif case["ids"] == "all_zero":
        ids[:] = 0
    elif n > 1:
        ids[0] = 0
    return dict(ids=torch.from_numpy(ids), table=normal(rng, (V, D), 1.0), d_out=normal(rng, (n, D), 1.0))


def emb_ref(case, inp, dtype):
    n, p = case["n"], case["p"]
    mult = (dropout_multiplier(DROP_SEED, EMB_STREAM, p, (n,)) if p > 0 and n > 0 else torch.ones(n)).to(dtype)
    table = inp["table"].to(dtype)
    out = table[inp["ids"]] * mult[:, None]
    d_table = torch.zeros_like(table).index_add_(0, inp["ids"], inp["d_out"].to(dtype) * mult[:, None])
    d_table[0] = 0.0                                 # padding_idx = 0
    return dict(out=out, d_table=d_table)


# ---- one reference per (family, index, dtype) for the whole session: computed once, never modified --------------------------
FAMILIES = {
    "cnn": (CNN_CASES, cnn_inputs, cnn_ref),
    "gru": (GRU_CASES, gru_inputs, gru_ref),
    "aa": (AA_CASES, aa_inputs, aa_ref),
    "lin": (LIN_CASES, lin_inputs, lin_ref),
    "emb": (EMB_CASES, emb_inputs, emb_ref),
}


@functools.lru_cache(maxsize=None)
def cached_inputs(family: str, index: int):
    cases, make, _ = FAMILIES[family]
    return make(cases[index])


@functools.lru_cache(maxsize=None)
def cached(family: str, index: int, dtype_name: str):
    cases, _, ref = FAMILIES[family]
    return ref(cases[index], cached_inputs(family, index), getattr(torch, dtype_name))
