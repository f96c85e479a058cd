"""What the host and the GPU tests of the full-catalogue rank under MANNeR's ensemble (``nrl_catalogue_ensemble_ranks``) share.

Two references, both on the CPU:

* ``ranks_from_bits``: the exact one.  From each table's raw fp32 score matrix and the (mean, sd) the library returned, the
  ensemble score ``z = w_0 ((s_0 - mu_0) / sd_0) + w_1 (...) + w_2 (...)`` is formed in fp32, one rounded operation at a time in
  ascending t (torch on the CPU rounds every elementwise operation on its own), and the rank is counted in the order of the
  entry: higher z first, equal z by ascending row, -0 equal to +0.  Rows that are ineligible, excluded or NaN are outside the
  population; a user whose statistics cannot standardise (some sd not positive and finite) has ranks 0 and population 0.
* ``catalogue_ref.rank_intervals``: the independent one, float64 under the derived tolerance of
  ``topk_ensemble_ref.ensemble64``, the worst-case error of an fp32 ensemble score.  The tolerance grows with D (it is a worst
  case), so the intervals are only sharp at small D; ``interval_case`` lists the inputs and
  tests/test_catalogue_rank_ensemble_host.py checks on the reference alone that at least two thirds of them collapse to one
  point and none is wider than 2."""
import functools

import torch

from tests import catalogue_ref as C
from tests import topk_ensemble_ref as R

WEIGHTS = (1.0, 0.2, -0.25)
NEG_INF = float("-inf")
INTERVAL_SHAPES = ((9, 300, 20), (9, 1000, 64))             # (B, V, D), D <= 64


def sd_ok(sd):
    return (sd > 0) & (sd < float("inf"))


def ensemble_from_bits(raw, stats, weights):
    """(B, V) fp32 ensemble scores from the raw fp32 score matrices ``raw[t]`` (B, V) and ``stats`` (B, T, 2), as the kernels
    form them; +0 for -0 (the entry order does not tell them apart and the outputs come back as +0)."""
    z = None
    for t, (s, w) in enumerate(zip(raw, weights)):
        zt = torch.tensor(float(w), dtype=torch.float32) * ((s - stats[:, t, 0:1]) / stats[:, t, 1:2])
        z = zt if z is None else z + zt
    return z + 0.0


def ranks_from_bits(raw, stats, weights, targets, excl=None, eligible=None):
    """rank int32 (n), score fp32 (n), ranked int32 (B): the exact reference of the module docstring."""
    z = ensemble_from_bits(raw, stats, weights)
    pop = C.population(z, excl, eligible)[0]
    pop[~sd_ok(stats[:, :, 1]).all(1)] = False              # a refused user's population is empty
    return C.ranks(z, pop, targets)


@functools.lru_cache(maxsize=None)
def interval_case(B, V, D):
    """``real_case(31 + D, 3, ...)`` with the weights 1.0 / 0.2 / -0.25, 0 to 9 exclusions and 1 to 5 clicks a user ->
    (users, tables, excl, clicks, pop, intervals)."""
    users, tables = R.real_case(31 + D, 3, B, V, D)
    g = torch.Generator().manual_seed(D)
    excl = tuple(tuple(torch.randint(0, V, (int(n),), generator=g).tolist()) for n in torch.randint(0, 10, (B,), generator=g))
    clicks = tuple(tuple(torch.randint(0, V, (int(n),), generator=g).tolist()) for n in torch.randint(1, 6, (B,), generator=g))
    pop = C.allowed(B, V, excl)
    agg, tol = R.ensemble64(users, tables, WEIGHTS, pop)
    return users, tables, excl, clicks, pop, C.rank_intervals(agg, tol, pop, clicks)


def click_lists(seed, B, V, excl=None, eligible=None):
    """Clicks for the exact tests: 0 to 32 a user (user 0 has 32, the last user none when B > 1), and in user 0's list a duplicate,
    a row of its own exclusion list, an ineligible row and one row outside the table at either end."""
    g = torch.Generator().manual_seed(seed)
    clicks = [torch.randint(0, V, (int(n),), generator=g).tolist() for n in torch.randint(0, 33, (B,), generator=g)]
    first = torch.randint(0, V, (32,), generator=g).tolist()
    first[1] = first[0]
    first[2], first[3] = -1, V
    if excl is not None and len(excl[0]):
        first[4] = excl[0][0]
    if eligible is not None and not bool(eligible.all()):
        first[5] = int(torch.nonzero(eligible == 0)[0])
    clicks[0] = first
    if B > 1:
        clicks[-1] = []
    return clicks
