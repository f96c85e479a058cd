"""Restatement of ``nrl_grid_metrics`` (``include/newsreclib_amd.h`` states the semantics) on the CPU, in plain loops and float64,
plus the inputs the grid tests share.  Imports nothing of the library.

The score of a candidate under a weight row is restated in float32 as the kernel forms it (terms with weight 0 skipped, the first
remaining term a product, every later one a fused multiply-add).  The fma is emulated through float64, which rounds twice; on the
inputs built here -- components on a grid of eighths, weights on a grid of eighths, both small -- every product and sum is exact
in float32, so the restated scores ARE the kernel's and the ties they contain are the kernel's ties.  The per-impression values
are then float64; the bound against them is abs 2e-5, the one ``tests/test_gpu_metrics_stream.py`` derives for these values."""
import math

import torch

TOL = 2e-5
WAVE_C, MAX_C, TARGET_BLOCKS = 128, 4096, 2048


# ---- the launch plan ---------------------------------------------------------------------------------------------------------------
def configs_per_block(B, G):
    """Configs one workgroup loops over: from G and B alone, aiming at about 2048 workgroups of four impressions each."""
    if B <= 0 or G <= 0:
        return 1
    blocks = -(-B // 4)
    ranges = min(G, max(1, -(-TARGET_BLOCKS // blocks)))
    return -(-G // ranges)


# ---- scores ------------------------------------------------------------------------------------------------------------------------
def scores(comp, w):
    """(N) float32 scores of one weight row ``w`` (T) over ``comp`` (T, N) float32."""
    acc = None
    for t in range(comp.shape[0]):
        wt = float(w[t])
        if wt == 0.0:
            continue
        wt32 = torch.tensor(wt, dtype=torch.float32)
        if acc is None:
            acc = wt32 * comp[t]
        else:
            acc = (wt32.double() * comp[t].double() + acc.double()).float()
    return acc if acc is not None else torch.zeros(comp.shape[1], dtype=torch.float32)


def rank(p):
    """0-based position of every candidate in the stable descending ranking (NaN first, -0 == +0)."""
    order = torch.argsort(p + 0.0, descending=True, stable=True)
    r = torch.empty_like(order)
    r[order] = torch.arange(order.numel())
    return order, r


# ---- per-impression values, float64 ------------------------------------------------------------------------------------------------
def ranking_row(p, t, ks):
    order, _ = rank(p)
    ts = t[order].double().tolist()
    rr = 0.0
    for pos, v in enumerate(ts):
        if v > 0:
            rr = 1.0 / (pos + 1)
            break
    ideal = sorted(t.double().tolist(), reverse=True)
    row = [rr]
    for k in ks:
        dcg = sum(v / math.log2(pos + 2) for pos, v in enumerate(ts[:k]))
        idcg = sum(v / math.log2(pos + 2) for pos, v in enumerate(ideal[:k]))
        row.append(dcg / idcg if idcg > 0 else 0.0)
    return row


def aspect_row(p, a, h, nc, ks):
    """(div@k ..., pers@k ...): entropy of the top-k class distribution over log(nc); sum(min) / sum(max) of the top-k class counts
    against the history's; both 0 when every candidate id is 0."""
    if not int((a != 0).sum()):
        return [0.0] * (2 * len(ks))
    order, _ = rank(p)
    hist = [0] * nc
    for c in h.tolist():
        hist[c] += 1
    div, pers = [], []
    for k in ks:
        top = a[order[:k]].tolist()
        cnt = [0] * nc
        for c in top:
            cnt[c] += 1
        n = len(top)
        div.append(-sum((x / n) * math.log(x / n) for x in cnt if x > 0) / math.log(nc))
        smin, smax = sum(min(x, y) for x, y in zip(cnt, hist)), sum(max(x, y) for x, y in zip(cnt, hist))
        pers.append(smin / smax if smax > 0 else 0.0)
    return div + pers


def rows(comp, weights, targets, csz, ks, aspects=(), hsz=None):
    """(G, B, cols) float64: the rows of every weight row, impression by impression."""
    G, B = len(weights), len(csz)
    cols = 1 + len(ks) * (1 + 2 * len(aspects))
    out = torch.zeros(G, B, cols, dtype=torch.float64)
    for g in range(G):
        s = scores(comp, weights[g])
        c0 = h0 = 0
        for b, cs in enumerate(csz.tolist()):
            hs = int(hsz[b]) if hsz is not None else 0
            p, t = s[c0:c0 + cs], targets[c0:c0 + cs]
            row = ranking_row(p, t, ks)
            for ca, ha, nc in aspects:
                row += aspect_row(p, ca[c0:c0 + cs], ha[h0:h0 + hs], nc, ks)
            out[g, b] = torch.tensor(row, dtype=torch.float64)
            c0, h0 = c0 + cs, h0 + hs
    return out


def configs_ranking_differently(comp, weights, csz):
    """How many weight rows rank SOME impression differently from row 0."""
    base = scores(comp, weights[0])
    n = 0
    for g in range(1, len(weights)):
        s = scores(comp, weights[g])
        c0, differs = 0, False
        for cs in csz.tolist():
            if not torch.equal(rank(s[c0:c0 + cs])[1], rank(base[c0:c0 + cs])[1]):
                differs = True
                break
            c0 += cs
        n += differs
    return n


def assert_not_vacuous(comp, weights, csz):
    """At least half the weight rows rank some impression differently from row 0 (else the grid test would pass on a kernel that
    ranks every row by row 0's scores)."""
    G = len(weights)
    n = configs_ranking_differently(comp, weights, csz)
    assert G == 1 or 2 * n >= G, (n, G)
    return n


# ---- shared inputs -----------------------------------------------------------------------------------------------------------------
LEVELS = 5          # components take the values -1, -0.5, 0, 0.5, 1: ties everywhere, different ones under different rows


def grid_weight_rows(G, T, seed=0):
    """(G, T) float32 on a grid of eighths in [-1, 1]: no row of zeros, zeros in every position, negative weights, a repeated row
    (row G - 1 repeats row 0 when G >= 5)."""
    g = torch.Generator().manual_seed(1000 + 7 * G + T + seed)
    w = torch.randint(-8, 9, (G, T), generator=g).float() / 8
    for r in range(G):
        if T > 1 and r % 3 == 1:
            w[r, (r // 3) % T] = 0.0
        if not bool((w[r] != 0).any()):
            w[r, r % T] = 1.0 if r % 2 else -0.5
    if T == 1:                              # one component: only the sign of the weight changes a ranking
        w = w.abs()
        w[1:] = -w[1:]
    if G >= 5:
        w[G - 1] = w[0]
    return w


def case(seed, T, csz, hsz=None, n_classes=()):
    """Quantised components (T, N), graded targets (N), and per aspect (candidate ids, history ids, classes)."""
    g = torch.Generator().manual_seed(seed)
    csz = torch.as_tensor(csz)
    N = int(csz.sum())
    comp = (torch.randint(0, LEVELS, (T, N), generator=g).float() - (LEVELS - 1) / 2) / 2
    targets = torch.randint(0, 3, (N,), generator=g).float() * (torch.rand(N, generator=g) < 0.3)
    aspects = []
    if n_classes:
        hsz = torch.as_tensor(hsz)
        M = int(hsz.sum())
        for nc in n_classes:
            aspects.append((torch.randint(0, nc, (N,), generator=g), torch.randint(0, nc, (M,), generator=g), nc))
    return comp, targets, csz, hsz, aspects
