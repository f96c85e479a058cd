"""Shared by test_topk_npa_host.py and test_gpu_topk_npa.py: the float64 value of NPA's personalized-pooling score over cached
feature maps, its derived fp32 error bound, an fp32 emulation on the CPU, and the two input families.  Population, order and the
floor check are ``tests/catalogue_ref.py``'s.

The score: with ``c`` (V, L, F) the feature maps, ``q`` (B, F) the users' text queries and ``user`` (B, F) the user vectors,

    a[u, v, t] = c[v, t] . q[u]      s[u, v, t] = c[v, t] . user[u]      score(u, v) = sum_t softmax_t(a[u, v, :])[t] s[u, v, t]

Exact family (``exact_case``): integer maps in [0, 4], ``q`` in {-1, 0, 1}, ``user`` in [-4, 4].  Columns 0 and 1 are peak columns:
``user`` is 0 there, ``q[u]`` is (1, 0) or (0, 1) -- the user picks which peak counts -- and ``c[v, t, j]`` is 1000 on the tokens of
news v's peak set j (n in {1, 2, 4, 8} tokens) and 0 elsewhere.  The columns 2 ... 1 + nl, nl = (F - 2) // 2, are the only other
ones where ``q`` is not 0, and there a news has ONE row of values on all the tokens of its two peak sets, so the logits of a peak
set are equal; every other logit is more than 1000 - 8 nl > 800 below them, and exp of that is exactly 0 in fp32 and in float64.
The weights are then exactly 1 / n on the peak set and the score is an integer sum divided by a power of two: exact whatever the
order of the sums, for an online softmax as for a two-pass one, for a division as for a reciprocal.  These cases compare with
``torch.equal`` and have many ties.

Real family (``real_case``): maps relu(N(0, 1)), q = tanh(0.25 N(0, 1)), user = N(0, 1) / sqrt(F).

Bound (derived, not measured), EPS = 2^-23, per (u, v), with w = softmax(a) in float64:

    e_a   = F EPS max_t (|c_t| . |q|)                 a length-F fp32 dot product, any order
    e_s,t = F EPS (|c_t| . |user|)
    S     = sum_t w_t |s_t|
    K     = 2 (L (U_EXP + 2) + 208)                   numerator and denominator; per weight at most L rescale / exp factors of U_EXP
                                                      ulp each, and 2 EPS |x| of argument rounding with sum |x| <= 104 (beyond
                                                      that p = 0)
    bound = sum_t w_t e_s,t + S (2 e_a + K EPS) + (L + 2) EPS S

``U_EXP = 4`` is a deliberately generous allowance for the device's fast exponential, whose accuracy is not documented where this
was written.  With U_EXP = 4 the K term is under 3 % of the bound on the real case, because the worst-case logit term 2 e_a S
dominates: the exact value of U_EXP decides no assertion."""
import functools

import torch

EPS = 2.0 ** -23
U_EXP = 4
REAL = dict(B=37, V=2000, L=30, F=400, k=10, seed=9)
PEAK = 1000.0


@functools.lru_cache(maxsize=None)
def exact_case(seed, B, V, L, F, ns=(1, 2, 4, 8)):
    """(q, user, features, float64 scores) of the exact family; peak-set sizes drawn from ``ns`` (those <= L).  Shared, never
    modified."""
    g = torch.Generator().manual_seed(seed)
    nl = (F - 2) // 2
    assert F >= 4 and PEAK - 8 * nl > 800
    sizes = torch.tensor([n for n in ns if n <= L])
    feat = torch.randint(0, 5, (V, L, F), generator=g).float()
    either = torch.zeros(V, L, dtype=torch.bool)
    for j in range(2):
        n_v = sizes[torch.randint(0, len(sizes), (V,), generator=g)]
        rank = torch.rand(V, L, generator=g).argsort(1).argsort(1)
        member = rank < n_v[:, None]
        feat[:, :, j] = member.float() * PEAK
        either |= member
    common = torch.randint(0, 5, (V, 1, nl), generator=g).float().expand(V, L, nl)
    feat[:, :, 2:2 + nl] = torch.where(either[:, :, None], common, feat[:, :, 2:2 + nl])
    q = torch.zeros(B, F)
    q[torch.arange(B), torch.randint(0, 2, (B,), generator=g)] = 1.0
    q[:, 2:2 + nl] = torch.randint(-1, 2, (B, nl), generator=g).float()
    user = torch.randint(-4, 5, (B, F), generator=g).float()
    user[:, :2] = 0.0
    return q, user, feat, scores64(q, user, feat)[0]


@functools.lru_cache(maxsize=None)
def real_case():
    """q, user, features (V, L, F: 96 MB, built once), exclusion lists of 0 - 50 rows, and the float64 scores and bound (B, V).
    Treated as read-only by every test."""
    c = REAL
    g = torch.Generator().manual_seed(c["seed"])
    feat = torch.relu(torch.randn(c["V"], c["L"], c["F"], generator=g))
    q = torch.tanh(0.25 * torch.randn(c["B"], c["F"], generator=g))
    user = torch.randn(c["B"], c["F"], generator=g) / c["F"] ** 0.5
    excl = [torch.randint(0, c["V"], (int(n),), generator=g).tolist() for n in torch.randint(0, 51, (c["B"],), generator=g)]
    raw, bound = scores64(q, user, feat)
    return dict(q=q, user=user, feat=feat, excl=excl, raw=raw, bound=bound)


def scores64(q, user, feat, chunk=256):
    """float64 score (B, V) from fp32 ``q`` / ``user`` (B, F) and ``feat`` (V, L, F), and its fp32 bound (B, V)."""
    V, L, F = feat.shape
    B = q.shape[0]
    q64, u64 = q.double(), user.double()
    score = torch.empty(B, V, dtype=torch.float64)
    bound = torch.empty(B, V, dtype=torch.float64)
    k_term = 2 * (L * (U_EXP + 2) + 208)
    for lo in range(0, V, chunk):
        c = feat[lo:lo + chunk].double()                     # (v, L, F)
        a, s = c @ q64.T, c @ u64.T                          # (v, L, B)
        w = torch.softmax(a, dim=1)
        e_a = F * EPS * (c.abs() @ q64.abs().T).max(dim=1)[0]                 # (v, B)
        e_s = F * EPS * (c.abs() @ u64.abs().T)              # (v, L, B)
        S = (w * s.abs()).sum(dim=1)
        score[:, lo:lo + chunk] = (w * s).sum(dim=1).T
        bound[:, lo:lo + chunk] = ((w * e_s).sum(dim=1) + S * (2 * e_a + k_term * EPS) + (L + 2) * EPS * S).T
    return score, bound


def emulate_fp32(q, user, feat):
    """The score in fp32 on the CPU by the kernel's online form, tokens ascending: m' = max(m, a); r = exp(m - m');
    p = exp(a - m'); l = l r + p; o = o r + p s from m = -inf, l = o = 0; then o / l.  -> (B, V) fp32."""
    V, L, F = feat.shape
    B = q.shape[0]
    m = torch.full((V, B), float("-inf"))
    l, o = torch.zeros(V, B), torch.zeros(V, B)
    for t in range(L):
        c = feat[:, t, :]
        a, s = c @ q.T, c @ user.T
        mn = torch.maximum(m, a)
        r, p = torch.exp(m - mn), torch.exp(a - mn)
        l = l * r + p
        o = o * r + p * s
        m = mn
    return (o / l).T.contiguous()
