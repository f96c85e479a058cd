"""Gumbel top-k, restated for the tests of ``nrl_topk_sampled_scores`` / ``nrl_gumbel_noise``.  CPU only, numpy / torch float64;
``newsreclib_amd`` is not imported.

* the noise, as the header states it, with every integer step in uint64 reduced mod 2^32: ``call_key``, ``user_key``, ``mantissa``,
  ``uniform`` (exact in fp32) and ``gumbel64`` (float64 ``-log(-log(u))``: what the device's fp32 value is measured against);
* ``expected``: the list of ``catalogue_ref.topk`` over ``z = fl32(fl32(s * inv_temp) + g32)`` with ``g32`` GIVEN (the device's own
  noise, checked separately against ``gumbel64``): on scores that are exact in fp32 the result is exact, ties included;
* ``pl_marginals``: the first- and second-slot distributions of the Plackett-Luce policy, for the chi-square test."""
import numpy as np
import torch

from tests import catalogue_ref as C

M32 = 0xFFFFFFFF
CHI2_7_1E6 = 40.52                                          # upper 1e-6 quantile of chi-square with 7 degrees of freedom


def lowbias32(x):
    """csrc/nrl_common.h, on uint64 arrays (or Python ints) holding values below 2^32"""
    x = np.asarray(x, dtype=np.uint64) & np.uint64(M32)
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7FEB352D)) & np.uint64(M32)
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846CA68B)) & np.uint64(M32)
    x = x ^ (x >> np.uint64(16))
    return x


def call_key(seed):
    seed = int(seed)
    assert 0 <= seed < 2 ** 64
    return lowbias32((seed & M32) ^ int(lowbias32(((seed >> 32) + 0x9E3779B9) & M32)))


def user_key(k0, key):
    """``key``: int64 values, reinterpreted as uint64"""
    key = np.asarray(key, dtype=np.int64).view(np.uint64)
    return lowbias32((key & np.uint64(M32)) ^ lowbias32((key >> np.uint64(32)) ^ np.uint64(int(k0))))


def mantissa(seed, key, row):
    """m (23 bits) of the pairs (key[i], row[i]), broadcast against each other"""
    ku = user_key(call_key(seed), key)
    row = np.asarray(row, dtype=np.int64).astype(np.uint64)
    h = lowbias32((row * np.uint64(0x9E3779B1) + ku) & np.uint64(M32))
    return h >> np.uint64(9)


def uniform(seed, key, row):
    """u = (2 m + 1) 2^-24 as float32 (exact)"""
    m = mantissa(seed, key, row)
    u = ((2 * m + 1).astype(np.float64) * 2.0 ** -24)
    assert np.array_equal(u.astype(np.float32).astype(np.float64), u)
    return u.astype(np.float32)


def gumbel64(u):
    u = np.asarray(u, dtype=np.float64)
    return -np.log(-np.log(u))


def perturbed(s, g32, inv_temp):
    """z (B, V) float32 = fl32(fl32(s * inv_temp) + g32): two separate fp32 roundings on the CPU.  ``s``: scores that are exact in
    fp32 (float64 or float32 tensor)."""
    scaled = (s.float() * torch.tensor(inv_temp, dtype=torch.float32)).float()
    return scaled + torch.as_tensor(g32, dtype=torch.float32)


def expected(s64, g32, inv_temp, k, excl=None, eligible=None):
    """-> (idx (B, k) int64, key (B, k) float32: z, score (B, k) float32: the raw score, -inf in the empty slots)"""
    z = perturbed(s64, g32, inv_temp)
    pop = C.population(z.double(), excl, eligible)[0]
    idx, key = C.topk(z.double(), pop, k)
    raw = torch.full(idx.shape, C.NEG_INF, dtype=torch.float32)
    got = idx >= 0
    raw[got] = (s64.float() + 0.0).gather(1, idx.clamp(min=0))[got]
    return idx, key, raw


def pl_marginals(s, inv_temp):
    """(p1, p2): the distributions of the first and of the second drawn row under Plackett-Luce over softmax(s * inv_temp)"""
    w = np.exp(np.asarray(s, dtype=np.float64) * inv_temp)
    p = w / w.sum()
    p2 = np.array([sum(p[i] * p[j] / (1.0 - p[i]) for i in range(len(p)) if i != j) for j in range(len(p))])
    return p, p2


def chi2(counts, p):
    counts = np.asarray(counts, dtype=np.float64)
    e = counts.sum() * np.asarray(p, dtype=np.float64)
    return float(((counts - e) ** 2 / e).sum())
