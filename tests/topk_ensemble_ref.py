"""What the host and the GPU tests of the z-scored ensemble top-k (``nrl_topk_ensemble_scores``) share: the inputs, the float64
statistics, the derived worst case of the fp32 statistics and a CPU emulation of their prescribed reduction order.

The bound (not a measurement).  u = 2^-24 is the unit roundoff, EPS = 2^-23.  Every raw score is off by at most
``bs[v] = D EPS sum_i |u_i| |t_i|`` (one fp32 dot product of length D).  Over a population of n rows with S = max |s| + max bs,
tiles_per_chunk = ceil(ceil(V / 128) / 64), chunks = ceil(ceil(V / 128) / tiles_per_chunk) and L = tiles_per_chunk + chunks:

* a tile mean is 8 roundings (the lane's add, the six levels of the wave reduction, the division) of values up to S: 8 u S; a
  pairwise update ``mean_a + d n_b / n`` is a convex combination of its inputs, so their errors do not grow, and adds 4 roundings
  of terms up to 2 S: 8 u S again.  A user's mean goes through one tile and at most L - 2 updates; with a factor two for the
  second-order terms, ``r = 8 EPS S L`` and

      dmu = mean(bs) + r;

* sd: (a) the perturbed scores move sd by at most the sd of the perturbation, ``max(bs) q`` with q = sqrt(n / (n - 1));
  (b) M2 is a sum of non-negative terms: a tile's M2 carries 10 roundings, every update 11 (d, d d, n_a, n_b, / n and the two
  additions), so at most (6 L + 5) EPS relative, half of it on sd, plus the division and the root: ``sd (3 L + 4) EPS``;
  (c) d itself is off by up to 2 r, which changes the update terms by 2 d dd n_a n_b / n; summed over every update with
  Cauchy-Schwarz (sum n_a n_b / n d^2 <= M2, sum n_a n_b / n <= 2 n) this moves M2 by at most 4 r sqrt(2 n M2), i.e. sd by
  ``2 sqrt(2) r q <= 3 r q``:

      dsd = max(bs) q + sd (3 L + 4) EPS + 3 r q.

``emulate_stats`` runs the prescribed order (tile -> chunk -> user) in fp32 on the CPU; tests/test_topk_ensemble_host.py checks
that it stays inside these bounds and that the bounds are below 1 % of sd on the inputs used."""
import functools

import torch

from tests import catalogue_ref as C

EPS = 2.0 ** -23
BV, STAT_CHUNKS = 128, 64
STATS_V, STATS_D = (2, 127, 128, 129, 1000, 8200), (4, 300, 768)
STATS_B, STATS_T = 65, 3


def chunk_plan(V):
    nvt = -(-V // BV)
    tpc = max(-(-nvt // STAT_CHUNKS), 1)
    return tpc, -(-nvt // tpc) if nvt else 0


def real_case(seed, T, B, V, D):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(B, D, generator=g) for _ in range(T)], [torch.randn(V, D, generator=g) for _ in range(T)]


@functools.lru_cache(maxsize=None)
def stats_case(V, D):
    """Inputs of the statistics tests at (V, D): 65 users, three tables, an eligibility mask that clears row 0, the last row and a
    few more (from V = 127 on: below that nothing would be left), exclusion lists (with entries outside V: ``bad`` says so) of
    which user 0's is empty, user 1's has duplicates, user 2's has 150 entries and user 3's holds an index outside V."""
    users, tables = real_case(V * 7 + D, STATS_T, STATS_B, V, D)
    g = torch.Generator().manual_seed(V + D)
    eligible = torch.ones(V, dtype=torch.uint8)
    if V >= 127:
        eligible[[0, 5, 64, V - 2, V - 1]] = 0
    excl = [torch.randint(0, V, (int(n),), generator=g).tolist() for n in torch.randint(0, 51, (STATS_B,), generator=g)]
    excl[0] = []
    excl[1] = [3 % V, 3 % V, 9 % V, 3 % V] if V > 2 else [1, 1]
    excl[2] = torch.randint(0, V, (150,), generator=g).tolist() if V > 300 else [1] * 150
    excl[3] = [7 % V, V, -1] if V > 2 else [V, -1]
    return users, tables, eligible, tuple(tuple(x) for x in excl)


def stats64(users, tables, pop):
    """Per table t: float64 scores s (B, V), bs (B, V), and over the population n (B), mean (B), unbiased sd (B)."""
    out = []
    for U, Tb in zip(users, tables):
        s = U.double() @ Tb.double().T
        bs = C.dot_bound(U, Tb)
        n = pop.sum(1).double()
        mean = (s * pop).sum(1) / n
        sd = (((s - mean[:, None]) ** 2 * pop).sum(1) / (n - 1)).sqrt()
        out.append((s, bs, n, mean, sd))
    return out


def stat_bounds(s, bs, n, sd, pop, V):
    """dmu (B), dsd (B) of the module docstring."""
    tpc, chunks = chunk_plan(V)
    L = tpc + chunks
    neg = torch.zeros_like(s).masked_fill(~pop, float("-inf"))
    S = (s.abs() + neg).max(1)[0] + (bs + neg).max(1)[0]
    r = 8 * EPS * S * L
    q = (n / (n - 1)).sqrt()
    dmu = (bs * pop).sum(1) / n + r
    dsd = (bs + neg).max(1)[0] * q + sd * (3 * L + 4) * EPS + 3 * r * q
    return dmu, dsd


def ensemble64(users, tables, weights, pop):
    """float64 (B, V) ensemble scores over the population and their derived tolerance:

      tol[v] = sum_t |w_t| ((bs_t[v] + dmu_t) / sd_t + |z_t[v]| dsd_t / sd_t) + 8 EPS sum_t |w_t z_t[v]|"""
    V = tables[0].shape[0]
    agg, tol, mag = 0.0, 0.0, 0.0
    for w, (s, bs, n, mean, sd) in zip(weights, stats64(users, tables, pop)):
        dmu, dsd = stat_bounds(s, bs, n, sd, pop, V)
        z = (s - mean[:, None]) / sd[:, None]
        agg = agg + w * z
        tol = tol + abs(w) * ((bs + dmu[:, None]) / sd[:, None] + z.abs() * (dsd / sd)[:, None])
        mag = mag + (w * z).abs()
    return agg, tol + 8 * EPS * mag


def _wave_sum(v):
    """the xor tree of ``wave_sum`` over the last axis (64 lanes), fp32"""
    lanes = torch.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        v = v + v[..., lanes ^ off]
    return v[..., 0]


def _fold(na, ma, qa, nb, mb, qb):
    n = na + nb
    d = mb - ma
    fa, fb, fn = na.float(), nb.float(), n.float()
    mean = ma + d * fb / fn
    m2 = (qa + qb) + d * d * fa * fb / fn
    take_b, keep_a = (na == 0), (nb == 0)
    mean = torch.where(take_b, mb, torch.where(keep_a, ma, mean))
    m2 = torch.where(take_b, qb, torch.where(keep_a, qa, m2))
    return n, mean, m2


def emulate_stats(s32, pop):
    """fp32 (mean, sd) per user of the (B, V) fp32 scores over ``pop`` in the order the kernels prescribe."""
    B, V = s32.shape
    tpc, chunks = chunk_plan(V)
    pad = chunks * tpc * BV - V
    s = torch.cat([s32, torch.zeros(B, pad)], 1).reshape(B, chunks, tpc, BV)
    p = torch.cat([pop & ~torch.isnan(s32), torch.zeros(B, pad, dtype=torch.bool)], 1).reshape(B, chunks, tpc, BV)
    zero = torch.zeros(B)
    un, um, uq = torch.zeros(B, dtype=torch.int64), zero.clone(), zero.clone()
    for c in range(chunks):
        cn, cm, cq = torch.zeros(B, dtype=torch.int64), zero.clone(), zero.clone()
        for t in range(tpc):
            x, m = s[:, c, t], p[:, c, t]
            nb = m.sum(1)
            xz = torch.where(m, x, torch.zeros(()))
            mb = _wave_sum(xz[:, :64] + xz[:, 64:]) / nb.float()
            mb = torch.where(nb > 0, mb, zero)
            dev = torch.where(m, x - mb[:, None], torch.zeros(()))
            qb = _wave_sum(dev[:, :64] * dev[:, :64] + dev[:, 64:] * dev[:, 64:])
            cn, cm, cq = _fold(cn, cm, cq, nb, mb, qb)
        un, um, uq = _fold(un, um, uq, cn, cm, cq)
    sd = torch.where(un >= 2, (uq / (un - 1).float()).sqrt(), torch.full((B,), float("nan")))
    return torch.where(un > 0, um, torch.full((B,), float("nan"))), sd
