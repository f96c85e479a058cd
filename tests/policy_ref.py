"""The Plackett-Luce policy of the sampled entries, restated for the tests of ``nrl_catalogue_logz`` / ``nrl_list_logprob``.  CPU only,
numpy float64; ``newsreclib_amd`` is not imported.

The policy is ``softmax(t)`` over a user's population, ``t = s * inv_temp`` (the tests choose scores and temperatures for which the
fp32 product is exact, so ``t`` is the device's).  A list is one draw without replacement: slot j is drawn from the softmax over
what the slots before it left.

* ``stats``: the population's size, ``max t``, ``log sum exp(t - max)`` and the entropy of ``softmax(t)`` in nats;
* ``pl_logprobs``: per slot ``log p(row | the slots before it)`` in the TAIL form -- the denominator of slot j is the mass of the
  rows NOT listed plus the mass of slots j, j + 1, ..., accumulated from the last slot backwards, positive terms only, and
  carried as its logarithm (``logaddexp``) so that no term underflows;
* ``pl_logprobs_subtractive``: the obvious form, ``Z - sum_{i < j}``, kept to show where it breaks."""
import numpy as np

NEG_INF = float("-inf")


def stats(s, inv_temp, pop):
    """``s`` (V) scores, ``pop`` (V) bool -> (max, logsum, entropy, n); an empty population gives (-inf, -inf, 0.0, 0)."""
    s, pop = np.asarray(s, dtype=np.float64), np.asarray(pop, dtype=bool)
    t = s[pop] * float(inv_temp)
    n = int(t.size)
    if n == 0:
        return NEG_INF, NEG_INF, 0.0, 0
    m = float(t.max())
    x = np.sort(t - m)                                     # ascending: the small terms first
    e = np.exp(x)
    S = float(e.sum())
    W = float((x * e).sum())
    return m + 0.0, float(np.log(S)), float(np.log(S) - W / S), n


def pl_logprobs(s, inv_temp, pop, lists):
    """``lists``: a sequence of rows, ``-1`` in trailing empty slots; every row is in ``pop`` and none is listed twice ->
    (logp (k) float64: ``+0`` in the empty slots, total)."""
    s, pop = np.asarray(s, dtype=np.float64), np.asarray(pop, dtype=bool).copy()
    rows = [int(r) for r in lists if int(r) != -1]
    assert len(set(rows)) == len(rows) and all(0 <= r < s.size and pop[r] for r in rows)
    assert all(int(r) == -1 for r in list(lists)[len(rows):])
    pop[rows] = False
    a = s[rows] * float(inv_temp)
    tail = s[pop] * float(inv_temp)
    logp = np.zeros(len(lists), dtype=np.float64)
    L = NEG_INF                                            # log of the mass of what is left, against the running maximum
    if tail.size:
        L = float(tail.max()) + float(np.log(np.exp(np.sort(tail - tail.max())).sum()))
    for j in range(len(rows) - 1, -1, -1):
        L = float(a[j]) if L == NEG_INF else float(np.logaddexp(L, a[j]))
        logp[j] = a[j] - L
    return logp + 0.0, float(logp.sum())


def pl_logprobs_subtractive(s, inv_temp, pop, lists):
    """The same numbers by ``Z - sum_{i < j} exp(t_i)``: cancels once the first slots hold the mass."""
    s, pop = np.asarray(s, dtype=np.float64), np.asarray(pop, dtype=bool)
    t = s * float(inv_temp)
    M = float(t[pop].max())
    Z = float(np.exp(t[pop] - M).sum())
    logp = np.zeros(len(lists), dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        for j, r in enumerate(lists):
            if int(r) == -1:
                break
            logp[j] = (t[r] - M) - np.log(Z)
            Z -= float(np.exp(t[r] - M))
    return logp, float(logp.sum())
