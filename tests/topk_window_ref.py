"""Per-user time windows on top of the full-catalogue contract (``tests/catalogue_ref.py``): row ``v`` belongs to user ``u``'s
population iff it does there and ``win_lo[u] <= row_time[v] <= win_hi[u]`` (closed, int32; ``lo > hi`` is an empty window).
CPU only, float64; ``newsreclib_amd`` is not imported.  The order, the ties, ``+0`` for ``-0`` and the rank stay written once, in
``catalogue_ref``: this module only ANDs the window into its population."""
import torch

from tests import catalogue_ref as C

INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1


def window_mask(row_time, lo, hi):
    """-> (B, V) bool: ``lo[b] <= row_time[v] <= hi[b]``"""
    t = torch.as_tensor(row_time).long()[None, :]
    return (torch.as_tensor(lo).long()[:, None] <= t) & (t <= torch.as_tensor(hi).long()[:, None])


def population(s, row_time, lo, hi, excl=None, eligible=None):
    """-> ((B, V) bool, whether a NaN score was dropped from a position that is allowed AND inside its user's window)"""
    ok = C.allowed(*s.shape, excl, eligible) & window_mask(row_time, lo, hi)
    nan = torch.isnan(s)
    return ok & ~nan, bool((ok & nan).any())


def expected_topk(s, k, row_time, lo, hi, excl=None, eligible=None):
    return C.topk(s, population(s, row_time, lo, hi, excl, eligible)[0], k)


def expected_ranks(s, targets, row_time, lo, hi, excl=None, eligible=None):
    return C.ranks(s, population(s, row_time, lo, hi, excl, eligible)[0], targets)


def window_mix(B, row_time, shift=0):
    """The windows the exact cases run, cycled over the users from kind ``shift`` on: all-inclusive; a single time value; bounds
    that fall on rows 127 / 128 (or the last row of a shorter table); one beyond both ends of the column; an empty one;
    ``lo == hi`` at either int32 end."""
    t = torch.as_tensor(row_time).long()
    V = int(t.numel())
    tmin, tmax = (int(t.min()), int(t.max())) if V else (0, 0)
    mid = int(t[V // 2]) if V else 0
    edge = (int(t[min(127, V - 1)]), int(t[min(128, V - 1)])) if V else (0, 0)
    kinds = [(INT32_MIN, INT32_MAX), (mid, mid), (min(edge), max(edge)), (int(t[min(128, V - 1)]) if V else 0, tmax),
             (tmin - 5, tmax + 5), (tmin, int(t[min(127, V - 1)]) if V else 0), (mid + 1, mid), (INT32_MIN, INT32_MIN),
             (INT32_MAX, INT32_MAX)]
    lo = torch.tensor([kinds[(b + shift) % len(kinds)][0] for b in range(B)], dtype=torch.int32)
    hi = torch.tensor([kinds[(b + shift) % len(kinds)][1] for b in range(B)], dtype=torch.int32)
    return lo, hi
