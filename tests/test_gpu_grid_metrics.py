"""A grid of ensemble weights in one pass (``nrl_manner_zscores``, ``nrl_grid_metrics``, ``metrics.GridStreamingMetrics``,
``evaluate_weight_grid``), under both GEMM engines.

First yardstick: the existing path run once per weight row -- ``ops_manner.manner_scores`` with the tables filtered to the non-zero
weights, ``ops.impression_metrics``, ``StreamingMetrics``, ``evaluate_impressions(device_metrics=True)`` -- to the bit.  Second
yardstick: the float64 restatement of ``tests/grid_metrics_ref.py`` at abs 2e-5 (the bound ``tests/test_gpu_metrics_stream.py``
derives for these values), on components and weights on a grid of eighths, where the restated float32 scores are exact."""
import pytest
import torch

from tests import builders
from tests import grid_metrics_ref as R
from tests.catalogue_ref import sync_debug_honoured

pytestmark = pytest.mark.gpu

E_TOO_LONG, E_ASPECT, E_OFFSETS = 1, 2, 4


@pytest.fixture(autouse=True, params=["f32", "bf16x3"])
def engine(request):
    from newsreclib_amd import _lib
    prev = _lib.get_gemm_engine()
    _lib.set_gemm_engine(request.param)
    yield request.param
    _lib.set_gemm_engine(prev)


def _off(sizes):
    sizes = torch.as_tensor(sizes).long()
    return torch.cat([torch.zeros(1, dtype=torch.long), torch.cumsum(sizes, 0)])


def _bits(x):
    return x.contiguous().view(torch.int32)


def _same_bits(a, b):
    """Equal bit for bit outside NaN, and NaN in the same places."""
    a, b = a.cpu(), b.cpu()
    nan = torch.isnan(a)
    return a.shape == b.shape and torch.equal(nan, torch.isnan(b)) and torch.equal(_bits(a)[~nan], _bits(b)[~nan])


def _dev_aspects(aspects):
    return [(ca.cuda(), ha.cuda(), nc) for ca, ha, nc in aspects]


def _grid(comp, w, targets, csz, ks, aspects=(), hsz=None, **kw):
    from newsreclib_amd import ops
    kw.setdefault("want_rows", True)
    kw.setdefault("want_preds", True)
    return ops.grid_metrics(comp.cuda(), w, targets.cuda(), _off(csz).cuda(), ks, _dev_aspects(aspects),
                            _off(hsz).cuda() if aspects else None, **kw)


def _loop_rows(preds, targets, csz, ks, aspects=(), hsz=None):
    """The first yardstick: ``impression_metrics`` once per row of ``preds`` (G, N) -> (G, B, cols) and the OR of the status words."""
    from newsreclib_amd import ops
    asp, off, hoff, t = _dev_aspects(aspects), _off(csz).cuda(), _off(hsz).cuda() if aspects else None, targets.cuda()
    rows, flags = [], 0
    for g in range(preds.shape[0]):
        _, r, st = ops.impression_metrics(preds[g].contiguous(), t, off, ks, asp, hoff, want_rank=False)
        rows.append(r)
        flags |= int(st)
    return torch.stack(rows), flags


# ---- 1. z-scores -------------------------------------------------------------------------------------------------------------------
Z_CAND, Z_HIST = [1, 2, 63, 64, 65, 300, 1025, 5], [3, 0, 1, 50, 7, 50, 1, 0]


def _tables(T, D, V=211, seed=5):
    g = torch.Generator().manual_seed(seed + D)
    return [torch.randn(V, D, generator=g).cuda() for _ in range(T)]


def _index_lists(V, cand, hist, seed=9):
    g = torch.Generator().manual_seed(seed)
    hi, ci = torch.randint(0, V, (sum(hist),), generator=g), torch.randint(0, V, (sum(cand),), generator=g)
    ci[3], hi[2] = V + 5, -4                                  # clamped, as in the scorer
    return hi.cuda(), _off(hist).cuda(), ci.cuda(), _off(cand).cuda()


def _flat(padded, cand):
    return torch.cat([padded[b, :n] for b, n in enumerate(cand)])


@pytest.mark.parametrize("D", [8, 768])
@pytest.mark.parametrize("T", [1, 2, 3])
def test_zscores_have_the_bits_of_the_single_table_calls(T, D):
    from newsreclib_amd.ops_manner import manner_scores, manner_zscores
    tables = _tables(T, D)
    hi, ho, ci, co = _index_lists(211, Z_CAND, Z_HIST)
    z = manner_zscores(tables, hi, ho, ci, co, max(Z_CAND))
    assert z.shape == (T, sum(Z_CAND)) and z.dtype == torch.float32
    nan_rows = 0
    for t in range(T):
        want = _flat(manner_scores([tables[t]], [1.0], hi, ho, ci, co, max(Z_CAND)), Z_CAND)
        assert _same_bits(z[t], want), t
        nan_rows += int(torch.isnan(want).sum())
    # the quirks are in: one candidate (impressions 0 and 7) and empty histories (1 and 7) are NaN, the rest is finite
    per = torch.split(z[0].cpu(), Z_CAND)
    assert all(bool(torch.isnan(per[b]).all()) for b in (0, 1, 7)) and all(bool(torch.isfinite(per[b]).all()) for b in (2, 3, 4, 5, 6))
    assert nan_rows == T * (1 + 2 + 5)


# ---- 2. scores ---------------------------------------------------------------------------------------------------------------------
SCORE_ROWS = [[1.0, 0.2, -0.25],                               # the module's own weights
              [0.0, 0.5, -0.25], [1.0, 0.0, -0.25], [1.0, 0.2, 0.0], [0.0, 0.0, 1.0], [0.0, -0.7, 0.0],      # zeros in every position
              [-1.3, -0.2, 0.9], [1.0, 0.2, -0.25], [0.1, 0.3, 0.7]]                                         # negative; a repeated row


@pytest.mark.parametrize("D", [8, 768])
def test_grid_scores_have_the_bits_of_manner_scores(D):
    from newsreclib_amd.ops_manner import manner_scores, manner_zscores
    cand, hist = [2, 63, 64, 65, 300, 129, 7], [3, 1, 50, 7, 50, 2, 9]
    tables = _tables(3, D, seed=21)
    hi, ho, ci, co = _index_lists(211, cand, hist, seed=4)
    comp = manner_zscores(tables, hi, ho, ci, co, max(cand))
    targets = torch.zeros(sum(cand))
    _, preds, status = _grid(comp, SCORE_ROWS, targets, cand, (5,))
    assert int(status) == 0 and preds.shape == (len(SCORE_ROWS), sum(cand))
    for g, row in enumerate(SCORE_ROWS):
        keep = [t for t in range(3) if row[t] != 0]
        want = _flat(manner_scores([tables[t] for t in keep], [row[t] for t in keep], hi, ho, ci, co, max(cand)), cand)
        assert bool(torch.isfinite(want).all())
        assert torch.equal(_bits(preds[g].cpu()), _bits(want.cpu())), (g, row)
    assert torch.equal(preds[0], preds[7]) and not torch.equal(preds[0], preds[8])


# ---- 3. rows -----------------------------------------------------------------------------------------------------------------------
# name: (T, G, configs_per_block, candidate counts, history sizes, classes per aspect, top_k)
ROW_CASES = {
    "one_row_one_long_impression": (1, 1, 0, [129], [4], (), (5,)),
    "k_above_C": (2, 2, 0, [1, 2, 127], [0, 3, 9], (4,), (1, 200)),
    "ragged_range": (3, 7, 3, [128, 129, 300, 1], [5, 0, 50, 2], (19, 4), (5, 10, 3)),
    "many_rows": (4, 65, 16, [1024, 2, 1025, 127, 128], [7, 1, 0, 12, 50], (6, 3), (1, 5, 10, 64)),
    "nine_impressions": (3, 7, 0, [4096, 5, 300, 128, 129, 1, 1025, 64, 2], [3, 0, 8, 50, 1, 2, 0, 6, 4], (1024,), (5, 10)),
    "long_then_short": (2, 2, 1, [300, 5, 6, 700, 9], [1, 2, 3, 4, 5], (), (5, 10)),
}
_REF = {}


def _row_case(name):
    """The case's inputs and its float64 rows, built once (both engines share them; nothing changes them)."""
    if name not in _REF:
        T, G, cpb, csz, hsz, classes, ks = ROW_CASES[name]
        comp, targets, csz_t, hsz_t, aspects = R.case(len(name) + T, T, csz, hsz, classes)
        w = R.grid_weight_rows(G, T)
        differing = R.assert_not_vacuous(comp, w, csz_t)
        _REF[name] = (comp, targets, w, aspects, R.rows(comp, w, targets, csz_t, ks, aspects, hsz_t if aspects else None), differing)
    return _REF[name]


@pytest.mark.parametrize("name", list(ROW_CASES))
def test_rows_have_the_bits_of_impression_metrics_and_meet_float64(name):
    T, G, cpb, csz, hsz, classes, ks = ROW_CASES[name]
    comp, targets, w, aspects, ref, differing = _row_case(name)
    rows, preds, status = _grid(comp, w, targets, csz, ks, aspects, hsz, configs_per_block=cpb)
    assert int(status) == 0 and rows.shape == (G, len(csz), 1 + len(ks) * (1 + 2 * len(classes)))
    # the restated scores are exact on these inputs: the ties the reference ranks are the kernel's
    for g in range(G):
        assert torch.equal(preds[g].cpu() + 0.0, R.scores(comp, w[g]) + 0.0), g
    want, flags = _loop_rows(preds, targets, csz, ks, aspects, hsz)
    assert flags == 0 and torch.equal(_bits(rows.cpu()), _bits(want.cpu()))
    err = float((rows.double().cpu() - ref).abs().max())
    print(f"{name}: {differing} of {G} rows rank some impression differently from row 0; max abs err against float64 {err:.3e} "
          f"(bound {R.TOL:.0e})")
    assert err <= R.TOL
    assert float(ref.abs().max()) > 0.1


# ---- 4. accumulator ----------------------------------------------------------------------------------------------------------------
def _step(comp, targets, csz, hsz, aspects, preds=None):
    """The tuple ``model_step`` returns, as far as the metrics read it (categ = aspect 0, sent = aspect 1)."""
    e = torch.empty(0, dtype=torch.long, device="cuda")
    a = [(ca.cuda(), ha.cuda()) for ca, ha, _ in aspects] + [(e, e)] * (2 - len(aspects))
    return (torch.zeros((), device="cuda"), preds, targets.cuda(), torch.as_tensor(csz).cuda(), torch.as_tensor(hsz).cuda(),
            a[0][0], a[1][0], a[0][1], a[1][1], e, e)


def test_accumulator_rows_have_the_bits_of_streaming_metrics_and_merge_adds():
    from newsreclib_amd.metrics import GridStreamingMetrics, StreamingMetrics
    T, G, ks, classes = 3, 7, (5, 10), (19, 4)
    w = R.grid_weight_rows(G, T)
    batches = [R.case(31, T, [40, 129, 3, 75, 128], [5, 0, 50, 2, 9], classes), R.case(32, T, [9, 300, 64], [1, 7, 0], classes)]
    grid, half = GridStreamingMetrics(w, ks, *classes), GridStreamingMetrics(w, ks, *classes)
    singles = [StreamingMetrics(ks, *classes) for _ in range(G)]
    for n, (comp, targets, csz, hsz, aspects) in enumerate(batches):
        step = _step(comp, targets, csz, hsz, aspects)
        grid.update(comp.cuda(), step)
        if n == 1:
            half.update(comp.cuda(), step)
        _, preds, _ = _grid(comp, w, targets, csz, ks, aspects, hsz, want_rows=False)
        for g in range(G):
            singles[g].update(_step(comp, targets, csz, hsz, aspects, preds[g].contiguous()))
    assert int(grid.count) == 8 and int(grid.status) == 0 and grid.sums.shape == (G, 11)
    for g in range(G):
        assert torch.equal(grid.count, singles[g].count)
        assert torch.equal(grid.sums[g].view(torch.int64), singles[g].sums.view(torch.int64)), g
    out = grid.compute()
    assert out["columns"] == singles[0].columns and out["weights"] == w.tolist()
    for g in range(G):
        single = singles[g].compute()
        assert all(out["values"][g][j] == single[c] for j, c in enumerate(out["columns"])), g
    # merge: the first batch alone + the second alone = both, in the order the accumulator adds them
    first = GridStreamingMetrics(w, ks, *classes)
    first.update(batches[0][0].cuda(), _step(*batches[0]))
    assert first.merge(half) is first
    assert int(first.count) == 8 and int(half.count) == 3 and torch.equal(first.sums, grid.sums)
    assert first.compute() == out


# ---- 5. flags ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flaw", ["offsets", "aspect", "too_long"])
def test_a_flagged_impression_is_zero_under_every_row_and_absent_from_the_count(flaw):
    from newsreclib_amd import ops
    T, G, ks = 3, 7, (5, 10)
    csz, hsz = [12, 30, 4097 if flaw == "too_long" else 200, 7, 140], [3, 0, 9, 5, 20]
    comp, targets, _, _, aspects = R.case(77, T, csz, hsz, (6,))
    w = R.grid_weight_rows(G, T)
    ca, ha, nc = aspects[0]
    off = _off(csz)
    if flaw == "aspect":
        ca = ca.clone()
        ca[int(off[2]) + 17] = 6
    elif flaw == "offsets":
        off = off.clone()
        off[3] = off[2] - 1                               # impression 2 runs backwards (and impression 3 starts early: still inside)
    sums, count = torch.zeros(G, 7, dtype=torch.float64, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda")
    rows, preds, status = ops.grid_metrics(comp.cuda(), w, targets.cuda(), off.cuda(), ks, [(ca.cuda(), ha.cuda(), nc)],
                                           _off(hsz).cuda(), sums=sums, count=count, want_rows=True, want_preds=True,
                                           configs_per_block=3)
    assert int(status) == {"offsets": E_OFFSETS, "aspect": E_ASPECT, "too_long": E_TOO_LONG}[flaw]
    assert float(rows[:, 2].abs().max()) == 0.0
    assert int(count) == 4
    # the neighbours: what the existing kernel gives the same offsets and row g's scores, rows and accumulator
    for g in range(G):
        one_sums, one_count = torch.zeros(7, dtype=torch.float64, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda")
        _, want, st = ops.impression_metrics(preds[g].contiguous(), targets.cuda(), off.cuda(), ks, [(ca.cuda(), ha.cuda(), nc)],
                                             _off(hsz).cuda(), sums=one_sums, count=one_count, want_rank=False)
        assert int(st) == int(status) and int(one_count) == 4
        keep = [0, 1, 3, 4]
        assert torch.equal(_bits(rows[g, keep].cpu()), _bits(want[keep].cpu())) and float(want[keep].abs().max()) > 0
        assert torch.equal(sums[g].view(torch.int64), one_sums.view(torch.int64)), g


# ---- 6. invariance -----------------------------------------------------------------------------------------------------------------
def test_a_rows_values_do_not_depend_on_the_grid_around_it_or_on_the_batch_split():
    T, ks, classes = 3, (5, 10), (19, 4)
    csz, hsz = [40, 129, 3, 75, 128, 300, 9], [5, 0, 50, 2, 9, 1, 7]
    comp, targets, _, _, aspects = R.case(55, T, csz, hsz, classes)
    w = R.grid_weight_rows(21, T)
    from newsreclib_amd import ops
    full_sums, full_count = torch.zeros(21, 11, dtype=torch.float64, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda")
    full, _, _ = _grid(comp, w, targets, csz, ks, aspects, hsz, sums=full_sums, count=full_count)
    pick = [13, 2, 20]
    for sub, cpb in ((w[pick], 0), (w[pick], 2), (w[13:14], 0), (torch.cat([w[5:6], w[pick], w[:9]]), 5)):
        sums, count = torch.zeros(len(sub), 11, dtype=torch.float64, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda")
        rows, _, _ = _grid(comp, sub, targets, csz, ks, aspects, hsz, sums=sums, count=count, configs_per_block=cpb)
        where = [i for i in range(len(sub)) if any(torch.equal(sub[i], w[p]) for p in pick)]
        for i in where:
            g = next(p for p in range(21) if torch.equal(sub[i], w[p]))
            assert torch.equal(_bits(rows[i].cpu()), _bits(full[g].cpu())), (i, g, cpb)
            assert torch.equal(sums[i].view(torch.int64), full_sums[g].view(torch.int64))
        assert int(count) == 7
    # the batch split: the rows of a sub-batch are the rows of the whole
    for lo, hi in ((0, 3), (3, 7), (5, 6)):
        c0, c1, h0, h1 = int(_off(csz)[lo]), int(_off(csz)[hi]), int(_off(hsz)[lo]), int(_off(hsz)[hi])
        part_asp = [(ca[c0:c1], ha[h0:h1], nc) for ca, ha, nc in aspects]
        rows, _, _ = _grid(comp[:, c0:c1].contiguous(), w, targets[c0:c1], csz[lo:hi], ks, part_asp, hsz[lo:hi])
        assert torch.equal(_bits(rows.cpu()), _bits(full[:, lo:hi].contiguous().cpu())), (lo, hi)
    assert ops.GRID_MAX_CONFIGS >= 21


# ---- 7. zero-weight skip -------------------------------------------------------------------------------------------------------------
def test_a_nan_component_under_weight_zero_changes_nothing():
    T, ks = 3, (5, 10)
    csz, hsz = [40, 129, 3, 300], [5, 0, 50, 2]
    comp, targets, _, _, aspects = R.case(66, T, csz, hsz, (6,))
    w = torch.tensor([[1.0, 0.0, -0.25], [0.5, 0.0, 0.5], [1.0, 0.25, 0.5]])
    poisoned = comp.clone()
    poisoned[1] = float("nan")
    rows_p, preds_p, st = _grid(poisoned, w, targets, csz, ks, aspects, hsz)
    rows_2, preds_2, _ = _grid(comp[[0, 2]].contiguous(), w[:, [0, 2]].contiguous(), targets, csz, ks, aspects, hsz)
    assert int(st) == 0
    for g in (0, 1):
        assert torch.equal(_bits(preds_p[g].cpu()), _bits(preds_2[g].cpu())) and torch.equal(_bits(rows_p[g].cpu()), _bits(rows_2[g].cpu()))
    assert bool(torch.isnan(preds_p[2]).all()) and bool(torch.isfinite(preds_p[:2]).all())


# ---- 8. no host synchronisation ------------------------------------------------------------------------------------------------------
def test_grid_metrics_and_update_do_not_synchronise_with_the_host():
    from newsreclib_amd import ops
    from newsreclib_amd.metrics import GridStreamingMetrics
    T, ks, classes = 3, (5, 10), (19, 4)
    csz, hsz = [40, 129, 3], [5, 0, 50]
    comp, targets, _, _, aspects = R.case(44, T, csz, hsz, classes)
    w = R.grid_weight_rows(7, T)
    comp_d, t_d, off, hoff, asp, w_d = comp.cuda(), targets.cuda(), _off(csz).cuda(), _off(hsz).cuda(), _dev_aspects(aspects), w.cuda()
    step = _step(comp, targets, csz, hsz, aspects)
    grid = GridStreamingMetrics(w, ks, *classes)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        if not sync_debug_honoured():
            pytest.skip("this torch build does not raise on synchronising calls under set_sync_debug_mode('error')")
        rows, preds, status = ops.grid_metrics(comp_d, w_d, t_d, off, ks, asp, hoff, want_rows=True, want_preds=True)
        grid.update(comp_d, step)
        grid.update(comp_d, step)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert int(status) == 0 and rows.shape == (7, 3, 11) and int(grid.count) == 6


# ---- 9. end to end -------------------------------------------------------------------------------------------------------------------
def test_weight_grid_equals_one_evaluation_per_point(tmp_path):
    from newsreclib_amd.evaluation import MannerVectorCache, evaluate_impressions, evaluate_weight_grid
    cr, ac, asent = builders.manner_modules(tmp_path)
    table, imps = builders.manner_table_and_impressions()
    points = [(cw, sw) for cw in (0.0, 0.2, -0.4) for sw in (-0.25, 0.0, 0.3)]
    full = MannerVectorCache(builders.manner_ensemble(cr, ac, asent, 1.0, 1.0), table)
    out = evaluate_weight_grid(full, imps, [[1.0, cw, sw] for cw, sw in points], batch_size=4, num_categ_classes=5, num_sent_classes=4)
    assert len(out["values"]) == 9 and out["columns"][:3] == ["mrr", "ndcg@5", "ndcg@10"]
    distinct = set()
    for g, (cw, sw) in enumerate(points):
        one = evaluate_impressions(MannerVectorCache(builders.manner_ensemble(cr, ac, asent, cw, sw), table), imps, batch_size=4,
                                   num_categ_classes=5, num_sent_classes=4, device_metrics=True)
        shared = [c for c in out["columns"] if c in one]
        assert {"mrr", "ndcg@5", "ndcg@10", "categ_div@5", "sent_pers@10"} <= set(shared)
        for c in shared:
            assert out["values"][g][out["columns"].index(c)] == one[c], (cw, sw, c)
        distinct.add(tuple(out["values"][g]))
    assert len(distinct) >= 5                                # the nine points are not one ranking


# ---- 10. argument errors -------------------------------------------------------------------------------------------------------------
def test_ops_refuses_bad_arguments():
    from newsreclib_amd import ops
    comp, t, off = torch.zeros(2, 5, device="cuda"), torch.zeros(5, device="cuda"), torch.tensor([0, 5]).cuda()
    ids = torch.zeros(5, dtype=torch.long, device="cuda")
    with pytest.raises(ValueError, match="all zeros"):
        ops.grid_metrics(comp, [[1.0, 0.5], [0.0, 0.0]], t, off, (5,))
    with pytest.raises(ValueError, match="non-finite"):
        ops.grid_metrics(comp, [[1.0, float("inf")]], t, off, (5,))
    with pytest.raises(ValueError, match="one entry per component: 2"):
        ops.grid_metrics(comp, [[1.0, 0.5, 0.2]], t, off, (5,))
    with pytest.raises(ValueError, match="one entry per component: 2"):
        ops.grid_metrics(comp, torch.ones(3, 3, device="cuda"), t, off, (5,))
    with pytest.raises(NotImplementedError, match="at most 4 components"):
        ops.grid_metrics(torch.zeros(5, 5, device="cuda"), torch.ones(2, 5), t, off, (5,))
    with pytest.raises(NotImplementedError, match="4096 rows"):
        ops.grid_metrics(comp, torch.ones(4097, 2), t, off, (5,))
    with pytest.raises(NotImplementedError, match="4096 rows"):
        ops.grid_metrics(comp, torch.ones(4097, 2, device="cuda"), t, off, (5,))
    with pytest.raises(ValueError, match="top_k"):
        ops.grid_metrics(comp, [[1.0, 0.5]], t, off, (1, 2, 3, 4, 5))
    with pytest.raises(ValueError, match="aspects need hist_offsets"):
        ops.grid_metrics(comp, [[1.0, 0.5]], t, off, (5,), [(ids, ids, 4)])
    with pytest.raises(ValueError, match="targets of N entries"):
        ops.grid_metrics(comp, [[1.0, 0.5]], t[:4], off, (5,))
    with pytest.raises(ValueError, match=r"sums must be \(1, 2\)"):
        ops.grid_metrics(comp, [[1.0, 0.5]], t, off, (5,), sums=torch.zeros(2, dtype=torch.float64, device="cuda"),
                         count=torch.zeros(1, dtype=torch.int64, device="cuda"))
    with pytest.raises(ValueError, match="go together"):
        ops.grid_metrics(comp, [[1.0, 0.5]], t, off, (5,), sums=torch.zeros(1, 2, dtype=torch.float64, device="cuda"))
    with pytest.raises(TypeError, match="float32"):
        ops.grid_metrics(comp.double(), [[1.0, 0.5]], t, off, (5,))
    rows, preds, status = ops.grid_metrics(torch.zeros(2, 0, device="cuda"), [[1.0, 0.5]], torch.zeros(0, device="cuda"),
                                           torch.zeros(1, dtype=torch.long, device="cuda"), (5,), want_rows=True, want_preds=True)
    assert rows.shape == (1, 0, 2) and preds.shape == (1, 0) and int(status) == 0
