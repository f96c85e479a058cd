"""CPU float64 reference of the full-catalogue rank of held-out rows under the MINER, DKN and NPA scorers
(``nrl_catalogue_interest_ranks`` / ``nrl_catalogue_relu_ranks`` / ``nrl_catalogue_pooled_ranks``), shared by test_catalogue_rank_scorers_host.py and
test_gpu_catalogue_rank_scorers.py.

Scores: ``interest_scores64`` (the aggregates of ``ops_miner.SCORE_MODES`` over ``s[b, j, v] = E64[b, j] . T64[v]``) and
``topk_dnn_ref.relu_scores64`` / ``topk_dnn_ref.scores64`` and ``topk_npa_ref.exact_case`` / ``topk_npa_ref.scores64`` with
their derived bounds.  Population, ranks and rank intervals are those of ``tests/catalogue_ref.py``.

Bounds of the MINER aggregates (derived, not measured), from the dot-product bound ``bs_j = D 2^-23 sum_i |e_ji| |t_i|`` of one fp32
dot product of length D in any order (``bl_j`` likewise from the gate rows):

  max       max_j bs_j                                   the maximum of perturbed values moves by at most the largest perturbation
  mean      max_j bs_j + K 2^-23 max_j |s_j|             K - 1 additions and one division, 2^-24 relative each, rounded up
  weighted  max_j bs_j + (max_j s_j - min_j s_j) (expm1(2 max_j bl_j) + (K + 8) 2^-23) + K 2^-23 max_j |s_j|
            a convex combination moves by at most its spread times the relative change of its weights: logits off by bl_j change
            the weight ratios by up to exp(2 bl); expf, the subtraction and the two sums add (K + 8) 2^-23."""
import functools

import torch

from tests import catalogue_ref as C
from tests import topk_dnn_ref as DR
from tests import topk_npa_ref as NR

EPS = 2.0 ** -23
MODES = ("max", "mean", "weighted")


def interest_scores64(E, T, mode, G=None):
    """float64 (B, V) aggregated scores of interests E (B, K, D) against T (V, D) and the derived fp32 bound (B, V)."""
    K, D = E.shape[1], E.shape[2]
    s = torch.einsum("bkd,vd->bkv", E.double(), T.double())
    bs = C.dot_bound(E.reshape(-1, D), T).reshape(E.shape[0], K, -1)
    if mode == "max":
        agg = s.max(dim=1)[0]
        agg[torch.isnan(s).any(dim=1)] = float("nan")           # (torch's max propagates NaN as well; spelled out)
        return agg, bs.max(dim=1)[0]
    if mode == "mean":
        return s.sum(dim=1) / K, bs.max(dim=1)[0] + K * EPS * s.abs().max(dim=1)[0]
    lg = torch.einsum("bkd,vd->bkv", G.double(), T.double())
    bl = C.dot_bound(G.reshape(-1, D), T).reshape(E.shape[0], K, -1)
    agg = (torch.softmax(lg, dim=1) * s).sum(dim=1)
    spread = s.max(dim=1)[0] - s.min(dim=1)[0]
    return agg, bs.max(dim=1)[0] + spread * (torch.expm1(2 * bl.max(dim=1)[0]) + (K + 8) * EPS) + K * EPS * s.abs().max(dim=1)[0]


# ---- the inputs both tiers use -----------------------------------------------------------------------------------------------------
REAL_MINER = dict(B=9, K=3, V=300, D=20, seed=11)
REAL_DKN = dict(B=20, V=300, dim=16, Hd=16, seed=12)
REAL_NPA = dict(B=9, V=300, L=5, F=36, seed=13)


def _lists(g, B, V):
    targets = [torch.randint(0, V, (int(n),), generator=g).tolist() for n in torch.randint(1, 6, (B,), generator=g)]
    excl = [torch.randint(0, V, (int(n),), generator=g).tolist() for n in torch.randint(0, 10, (B,), generator=g)]
    return targets, excl


@functools.lru_cache(maxsize=None)
def real_miner():
    """N(0, 1) interests, gate and table; 1 to 5 targets and 0 to 9 exclusions a user.  Read-only."""
    c = REAL_MINER
    g = torch.Generator().manual_seed(c["seed"])
    E, G = torch.randn(c["B"], c["K"], c["D"], generator=g), torch.randn(c["B"], c["K"], c["D"], generator=g)
    T = torch.randn(c["V"], c["D"], generator=g)
    targets, excl = _lists(g, c["B"], c["V"])
    return dict(E=E, G=G, T=T, targets=targets, excl=excl)


@functools.lru_cache(maxsize=None)
def real_dkn():
    """N(0, 1) user and news vectors and ``topk_dnn_ref.make_weights``; q and proj are the fp32 factors ``topk_dnn_ref.scores64``
    bounds (one fp32 matmul each, the bias added once).  Read-only."""
    c = REAL_DKN
    g = torch.Generator().manual_seed(c["seed"])
    U, T = torch.randn(c["B"], c["dim"], generator=g), torch.randn(c["V"], c["dim"], generator=g)
    _, pred = DR.make_weights(g, c["dim"], c["Hd"])
    w1, b1, w2, b2 = pred
    proj, q = T @ w1[:, :c["dim"]].T, U @ w1[:, c["dim"]:].T + b1
    targets, excl = _lists(g, c["B"], c["V"])
    s, bound = DR.scores64(U, T, pred)
    return dict(q=q, proj=proj, w2=w2.reshape(-1), b2=b2, targets=targets, excl=excl, s=s, bound=bound)


@functools.lru_cache(maxsize=None)
def real_npa():
    """The real family of ``topk_npa_ref`` at a small shape: maps relu(N(0, 1)), q = tanh(0.25 N(0, 1)), user = N(0, 1) / sqrt(F),
    with ``topk_npa_ref.scores64`` and its bound.  Read-only."""
    c = REAL_NPA
    g = torch.Generator().manual_seed(c["seed"])
    feat = torch.relu(torch.randn(c["V"], c["L"], c["F"], generator=g))
    q = torch.tanh(0.25 * torch.randn(c["B"], c["F"], generator=g))
    user = torch.randn(c["B"], c["F"], generator=g) / c["F"] ** 0.5
    targets, excl = _lists(g, c["B"], c["V"])
    s, bound = NR.scores64(q, user, feat)
    return dict(q=q, user=user, feat=feat, targets=targets, excl=excl, s=s, bound=bound)
