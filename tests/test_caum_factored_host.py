"""CPU tier of the factored CAUM evaluation: the float64 restatement (tests/caum_factored_ref.py) against the reference
restatement slot by slot, the pass planner's properties, and the new entry points' declarations."""
import os
import re

import pytest
import torch

from tests import caum_oracle as CO
from tests.caum_factored_ref import factored_scores

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _inputs(B, H, heads, sizes, seed=0):
    """float64 parameters, a history with zero tails (one of them empty when B > 1) and the ragged candidates."""
    D = 4 * heads
    cfg = dict(vocab=8, n_ent=8, n_categ=4, D=8, Dh=2, Dc=4, Ed=8, Eh=2, Q=8, N=D, F=D + 4, h1=12, h2=8)
    params = {k: v.double() for k, v in CO.make_caum_params(cfg, seed=seed).items()}
    g = torch.Generator().manual_seed(seed + 1)
    h = torch.randn(B, H, D, generator=g, dtype=torch.float64)
    for b in range(B):
        h[b, H - (b % (H + 1)):] = 0.0                      # user b keeps H - b % (H + 1) history rows
    if B > 1:
        h[B - 1] = 0.0                                      # an empty history
    c = torch.randn(sum(sizes), D, generator=g, dtype=torch.float64)
    offs = [0]
    for s in sizes:
        offs.append(offs[-1] + s)
    return params, h, c, offs


@pytest.mark.parametrize("B,H,heads,sizes", [(1, 1, 2, [3]), (3, 5, 4, [4, 1, 7]), (5, 2, 2, [1, 1, 1, 1, 9]),
                                             (6, 4, 4, [2, 5, 3, 5, 1, 4])])
def test_restatement_equals_the_reference_slot_by_slot(B, H, heads, sizes):
    params, h, c, offs = _inputs(B, H, heads, sizes)
    got = factored_scores(h, c, offs, params, heads)
    C = max(sizes)
    dense = torch.zeros(B, C, c.shape[1], dtype=torch.float64)
    for b in range(B):
        dense[b, :sizes[b]] = c[offs[b]:offs[b + 1]]
    worst = 0.0
    for i in range(C):
        assert all(bool((dense[b, i] == 0).all()) for b in range(B) if i >= sizes[b])      # the oracle's padded slots are 0
        want = CO.user_encoder_slot(h, dense[:, i], params, heads)
        for b in range(B):
            if i < sizes[b]:
                worst = max(worst, abs(float(got[offs[b] + i] - want[b])))
    print(f"B={B} H={H}: largest difference {worst:.3e}")
    assert worst <= 1e-12


def _check_plan(slot_counts, H, budget):
    from newsreclib_amd.ops_caum import plan_pair_chunks
    chunks = plan_pair_chunks(slot_counts, H, budget)
    total = sum(slot_counts)
    # contiguous ranges of the pair list, every pair exactly once
    assert [j0 for j0, _ in chunks] == [0] * bool(chunks) + [j1 for _, j1 in chunks[:-1]]
    assert all(j0 < j1 for j0, j1 in chunks)
    assert (chunks[-1][1] if chunks else 0) == total
    # pairs * H within the budget, except that a single pair always fits
    assert all((j1 - j0) * H <= budget or j1 - j0 == 1 for j0, j1 in chunks)
    return chunks


def test_plan_every_slot_fits():
    chunks = _check_plan([5, 5, 3, 1], 4, 5 * 4)
    assert chunks == [(0, 5), (5, 10), (10, 14)]            # whole slots while they fit


def test_plan_budget_smaller_than_a_slot():
    chunks = _check_plan([7, 3, 1], 5, 4 * 5)
    starts = {0, 7, 10, 11}
    assert any(j1 not in starts for _, j1 in chunks)        # a chunk ends inside a slot
    assert chunks == [(0, 4), (4, 7), (7, 11)]


def test_plan_budget_of_one_pair():
    assert _check_plan([3, 2], 6, 6) == [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5)]
    assert _check_plan([3, 2], 6, 1) == [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5)]       # less than one pair: one pair still fits


def test_plan_empty_batch():
    assert _check_plan([], 5, 100) == []
    assert _check_plan([0, 0], 5, 100) == []


def test_chunk_table_covers_the_range_slot_by_slot():
    from newsreclib_amd.ops_caum import pair_chunk_table
    rows, items = pair_chunk_table([130, 70, 2], 100, 201, H=3, heads=4)
    assert rows == [[0, 100, 30, 0], [1, 130, 70, 12], [2, 200, 1, 36]]
    assert items == 48


def test_new_entry_points_are_declared_and_typed():
    from newsreclib_amd import _lib
    header = open(os.path.join(ROOT, "include", "newsreclib_amd.h")).read()
    for name, count in (("nrl_caum_eval_attn", 19), ("nrl_caum_eval_add", 13)):
        decl = re.search(r"\bint %s\(([^;]*)\);" % name, header)
        assert decl and name in _lib.SIGNATURES, name
        params = [p for p in decl.group(1).split(",") if p.strip()]
        assert len(params) == count == len(_lib.SIGNATURES[name][1]), name
    assert _lib.ABI_VERSION == 19 and re.search(r"#define NRL_ABI_VERSION 19\b", header)
    assert not any(n.startswith("nrl_caum_eval") and n.endswith("_workspace_bytes") for n in _lib.SIGNATURES)
