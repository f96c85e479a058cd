"""Device-side streaming evaluation metrics (``nrl_impression_metrics``, ``metrics.StreamingMetrics``).

Yardsticks: the ranks against a per-impression stable descending argsort on the CPU (exact); rr / nDCG against the float64
per-impression restatement below; diversity / personalization against ``oracle/metrics_oracle.py`` per impression.  The bound on
every per-impression value is abs 2e-5: the values lie in [0, 1], counts and ranks are exact integers, and a value is at most
~3 k fp32 operations of a few ulp each (< 1e-5 at k = 64).  The existing torch metrics are a consistency check at 1e-4 (float32
means)."""
import math

import numpy as np
import pytest
import torch

from oracle import metrics_oracle as MO

from tests import builders

pytestmark = pytest.mark.gpu

TOL = 2e-5
WAVE_C = 128            # impressions up to this many candidates are ranked by one wave, longer ones by the workgroup


# ---- float64 restatement ---------------------------------------------------------------------------------------------------------
def _ref_rank(p):
    order = torch.argsort(p, descending=True, stable=True)
    rank = torch.empty_like(order)
    rank[order] = torch.arange(order.numel())
    return order, rank


def _ref_ranking_row(p, t, ks):
    """(rr, ndcg@k ...) of one impression in float64, plain loops."""
    order, _ = _ref_rank(p)
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


def _ref_aspect_row(p, a, h, nc, ks):
    """(div@k ..., pers@k ...) of one impression from the oracle's per-impression functions."""
    if not int(a.sum()):
        return [0.0] * (2 * len(ks))
    return [MO.diversity(p, a, nc, k) for k in ks] + [MO.personalization(p, a, h, nc, k) for k in ks]


def _ref_rows(preds, targets, csz, ks, aspects=(), hsz=None):
    rows, c0, h0 = [], 0, 0
    for b, cs in enumerate(csz.tolist()):
        hs = int(hsz[b]) if hsz is not None else 0
        p, t = preds[c0:c0 + cs], targets[c0:c0 + cs]
        row = _ref_ranking_row(p, t, ks)
        for ca, ha, nc in aspects:
            row += _ref_aspect_row(p, ca[c0:c0 + cs], ha[h0:h0 + hs], nc, ks)
        rows.append(row)
        c0, h0 = c0 + cs, h0 + hs
    return torch.tensor(rows, dtype=torch.float64).reshape(len(rows), 1 + len(ks) * (1 + 2 * len(aspects)))


def _rows_of(out, ks, prefixes=()):
    from newsreclib_amd import ops
    return torch.stack([out[c] for c in ops.metrics_columns(ks, prefixes)], dim=1).double().cpu()


def _check(name, got, want, tol=TOL):
    err = float((got - want).abs().max()) if got.numel() else 0.0
    print(f"{name}: max abs err {err:.3e} (bound {tol:.0e})")
    assert err <= tol, (name, err)


# ---- exact ranks -----------------------------------------------------------------------------------------------------------------
def test_ranks_equal_the_stable_descending_argsort():
    from newsreclib_amd import metrics
    g = torch.Generator().manual_seed(3)
    sizes = [1, 2, 63, 64, 65, WAVE_C - 1, WAVE_C, WAVE_C + 1, 255, 256, 257, 300, 511, 512, 513, 1023, 1024, 1025, 4096]
    preds = [torch.randn(n, generator=g) for n in sizes]
    targets = [(torch.rand(n, generator=g) < 0.2).float() for n in sizes]
    # all scores equal; few score levels with positives and negatives on the same level; strictly increasing; strictly decreasing
    preds += [torch.full((70,), 0.25), torch.randint(0, 4, (140,), generator=g).float() / 4, torch.arange(130).float() / 7,
              -torch.arange(50).float() / 3, torch.randint(0, 3, (40,), generator=g).float()]
    targets += [(torch.arange(70) % 5 == 3).float(), (torch.rand(140, generator=g) < 0.5).float(), (torch.arange(130) % 9 == 0).float(),
                (torch.arange(50) % 9 == 8).float(), (torch.arange(40) % 2).float()]
    # signed zeros compare equal; infinities are ordinary scores
    preds.append(torch.tensor([0.0, -0.0, 1.0, -0.0, 0.0, float("inf"), float("-inf"), -1.0]))
    targets.append(torch.tensor([0.0, 1.0, 0.0, 0.0, 1.0, 0.0, 1.0, 0.0]))
    perm = torch.randperm(len(preds), generator=g).tolist()          # long and short impressions share workgroups
    preds, targets = [preds[i] for i in perm], [targets[i] for i in perm]
    csz = torch.tensor([p.numel() for p in preds])
    assert len(preds) % 4 != 0
    P, T = torch.cat(preds), torch.cat(targets)
    out = metrics.impression_metrics(P.cuda(), T.cuda(), csz.cuda(), (1, 5, 10, 64))
    assert int(out["status"]) == 0
    want = torch.cat([_ref_rank(p)[1] for p in preds]).to(torch.int32)
    assert out["rank"].dtype == torch.int32 and torch.equal(out["rank"].cpu(), want)
    _check("ranking rows of the rank batch", _rows_of(out, (1, 5, 10, 64)), _ref_rows(P, T, csz, (1, 5, 10, 64)))


# ---- per-impression values ---------------------------------------------------------------------------------------------------------
def _value_batch(seed, nc0, nc1):
    g = torch.Generator().manual_seed(seed)
    csz = torch.tensor([3, 1, 17, 64, 65, 140, 9, 300, 40, 2, 80, 33, 5, 12, 70, 129, 26])          # 17 impressions: k > C, both paths
    hsz = torch.tensor([4, 0, 50, 1, 7, 30, 0, 12, 50, 3, 9, 2, 1, 20, 6, 50, 11])                  # histories of length 0
    N, M = int(csz.sum()), int(hsz.sum())
    preds = torch.randn(N, generator=g)
    preds[20:60] = torch.round(preds[20:60] * 2) / 2                                                # ties
    targets = torch.randint(0, 4, (N,), generator=g).float() * (torch.rand(N, generator=g) < 0.4)   # graded {0, 1, 2, 3}
    off = torch.cat([torch.zeros(1, dtype=torch.long), torch.cumsum(csz, 0)])
    targets[off[2]:off[3]] = 0.0                                                                    # no positive
    targets[off[8]:off[9]] = 1.0                                                                    # all positive
    asp = []
    for nc in (nc0, nc1):
        ca, ha = torch.randint(0, nc, (N,), generator=g), torch.randint(0, nc, (M,), generator=g)
        ca[off[4]:off[5]] = 0                                                                       # candidate aspects all 0 -> 0
        ca[off[3]], ca[off[5] + 1], ha[0] = nc - 1, nc - 1, nc - 1                                  # the last class
        asp.append((ca, ha, nc))
    return preds, targets, csz, hsz, asp


@pytest.mark.parametrize("nc0,nc1", [(2, 4), (19, 64), (65, 285), (1024, 18)])
def test_per_impression_values_against_float64(nc0, nc1):
    from newsreclib_amd import metrics
    ks = (1, 5, 10, 64)
    preds, targets, csz, hsz, asp = _value_batch(nc0, nc0, nc1)
    out = metrics.impression_metrics(preds.cuda(), targets.cuda(), csz.cuda(), ks,
                                     {"categ": tuple(x.cuda() if torch.is_tensor(x) else x for x in asp[0]),
                                      "sent": tuple(x.cuda() if torch.is_tensor(x) else x for x in asp[1])}, hist_news_size=hsz.cuda())
    assert int(out["status"]) == 0
    got, want = _rows_of(out, ks, ("categ", "sent")), _ref_rows(preds, targets, csz, ks, asp, hsz)
    assert torch.equal(out["rank"].cpu(), torch.cat([_ref_rank(p)[1] for p in torch.split(preds, csz.tolist())]).to(torch.int32))
    _check(f"rows, num_classes ({nc0}, {nc1})", got, want)
    assert float(got[4, 5:].abs().max()) == 0.0 and float(got[2, :5].abs().max()) == 0.0      # all-zero aspects; no positive
    for b in (1, 6):                                                                          # empty history: personalization 0
        assert float(got[b, 9:13].abs().max()) == 0.0 and float(got[b, 17:21].abs().max()) == 0.0
    assert float(want[:, 5:].abs().max()) > 0.1


def test_single_impression_and_empty_batch():
    from newsreclib_amd import metrics
    preds, targets = torch.tensor([0.2, 0.9, 0.9, -1.0, 0.5]), torch.tensor([0.0, 0.0, 2.0, 1.0, 0.0])
    ca, ha = torch.tensor([1, 2, 2, 0, 3]), torch.tensor([2, 2, 3])
    out = metrics.impression_metrics(preds.cuda(), targets.cuda(), torch.tensor([5]).cuda(), (5, 10), {"categ": (ca.cuda(), ha.cuda(), 4)},
                                     hist_news_size=torch.tensor([3]).cuda())
    want = _ref_rows(preds, targets, torch.tensor([5]), (5, 10), [(ca, ha, 4)], torch.tensor([3]))
    _check("B = 1", _rows_of(out, (5, 10), ("categ",)), want)
    assert out["rank"].cpu().tolist() == [3, 0, 1, 4, 2] and int(out["status"]) == 0
    e = torch.empty(0, device="cuda")
    out = metrics.impression_metrics(e, e, torch.empty(0, dtype=torch.long, device="cuda"), (5, 10))
    assert out["mrr"].shape == (0,) and out["ndcg@10"].shape == (0,) and out["rank"].numel() == 0 and int(out["status"]) == 0
    sm = metrics.StreamingMetrics((5, 10))
    el = torch.empty(0, dtype=torch.long, device="cuda")
    sm.update((torch.zeros((), device="cuda"), e, e, el, el, el, el, el, el, el, el))
    assert sm.compute() == {"mrr": 0.0, "ndcg@5": 0.0, "ndcg@10": 0.0, "auc": 0.0}


# ---- epoch values ------------------------------------------------------------------------------------------------------------------
_EPOCH = {}


def _epoch():
    """A MIND-shaped epoch of 553 impressions (18 + 1 categories, 3 + 1 sentiments) with its float64 reference, built once."""
    if _EPOCH:
        return _EPOCH
    g = torch.Generator().manual_seed(11)
    B = 553
    csz = torch.randint(1, 75, (B,), generator=g)
    csz[5], csz[200], csz[552] = 300, 129, 128
    hsz = torch.randint(0, 51, (B,), generator=g)
    N, M = int(csz.sum()), int(hsz.sum())
    preds = torch.randn(N, generator=g)
    targets = (torch.rand(N, generator=g) < 0.1).float()
    tc, ts = torch.randint(0, 19, (N,), generator=g), torch.randint(0, 4, (N,), generator=g)
    hc, hs = torch.randint(0, 19, (M,), generator=g), torch.randint(0, 4, (M,), generator=g)
    ref = _ref_rows(preds, targets, csz, (5, 10), [(tc, hc, 19), (ts, hs, 4)], hsz)
    _EPOCH.update(B=B, csz=csz, hsz=hsz, preds=preds, targets=targets, tc=tc, ts=ts, hc=hc, hs=hs, ref=ref)
    return _EPOCH


def _steps(E, splits):
    """The 11-tuples ``model_step`` returns, for consecutive batches of the given sizes."""
    coff = torch.cat([torch.zeros(1, dtype=torch.long), torch.cumsum(E["csz"], 0)]).tolist()
    hoff = torch.cat([torch.zeros(1, dtype=torch.long), torch.cumsum(E["hsz"], 0)]).tolist()
    steps, b0 = [], 0
    for n in splits:
        b1 = b0 + n
        c, h = slice(coff[b0], coff[b1]), slice(hoff[b0], hoff[b1])
        steps.append(tuple(x.cuda() for x in (torch.zeros(()), E["preds"][c], E["targets"][c], E["csz"][b0:b1], E["hsz"][b0:b1],
                                              E["tc"][c], E["ts"][c], E["hc"][h], E["hs"][h], torch.arange(b0, b1),
                                              torch.arange(coff[b0], coff[b1]))))
        b0 = b1
    assert b0 == E["B"]
    return steps


def _run(steps):
    from newsreclib_amd.metrics import StreamingMetrics
    sm = StreamingMetrics((5, 10), 19, 4)
    for s in steps:
        sm.update(s)
    return sm


def test_epoch_in_uneven_batches_equals_one_update_the_reference_and_the_torch_metrics():
    from newsreclib_amd.metrics import aspect_metrics, ranking_metrics
    E = _epoch()
    whole, parts = _run(_steps(E, [E["B"]])), _run(_steps(E, [1, 7, 512, 33]))
    assert int(whole.count) == int(parts.count) == E["B"]
    rel = float(((whole.sums - parts.sums).abs() / whole.sums.abs()).max())
    print(f"batched against whole epoch: max rel diff of the sums {rel:.3e}")
    assert rel <= 1e-12
    got = parts.compute()
    # the float64 restatement is the yardstick
    want = dict(zip(parts.columns, E["ref"].mean(0).tolist()))
    for k, v in want.items():
        print(f"{k}: streaming {got[k]:.9f} float64 {v:.9f}")
        assert abs(got[k] - v) <= TOL, (k, got[k], v)
    # consistency with the existing (float32-mean) functions, same keys, AUC bit-equal
    P, T, csz, hsz = E["preds"].cuda(), E["targets"].cuda(), E["csz"].cuda(), E["hsz"].cuda()
    old = ranking_metrics(P, T, csz, (5, 10))
    old.update(aspect_metrics(P, E["tc"].cuda(), E["hc"].cuda(), csz, hsz, 19, (5, 10), prefix="categ"))
    old.update(aspect_metrics(P, E["ts"].cuda(), E["hs"].cuda(), csz, hsz, 4, (5, 10), prefix="sent"))
    assert set(got) == set(old)
    for k, v in old.items():
        assert abs(got[k] - v) <= 1e-4, (k, got[k], v)
    assert got["auc"] == old["auc"]
    # reset clears the state
    parts.reset()
    assert parts.compute() == {} and parts.sums is None


def test_accumulator_is_deterministic():
    E = _epoch()
    a, b = _run(_steps(E, [100, 453])), _run(_steps(E, [100, 453]))
    assert torch.equal(a.sums, b.sums) and torch.equal(a.count, b.count) and int(a.status) == 0


def test_merge_of_two_halves_equals_the_whole():
    E = _epoch()
    steps = _steps(E, [200, 77, 276])
    whole, first, second = _run(steps), _run(steps[:1]), _run(steps[1:])
    first.merge(second)
    assert int(first.count) == E["B"]
    assert float(((whole.sums - first.sums).abs() / whole.sums.abs()).max()) <= 1e-12
    a, b = whole.compute(), first.compute()
    assert set(a) == set(b) and a["auc"] == b["auc"]
    from newsreclib_amd.metrics import StreamingMetrics
    with pytest.raises(ValueError, match="configured differently"):
        first.merge(StreamingMetrics((5,), 19, 4))


# ---- status word -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["aspect_too_large", "aspect_negative", "too_long"])
def test_refused_input_raises_and_leaves_the_other_impressions_correct(case):
    """Validated inputs: the kernel bounds-checks them before they index anything, flags the impression and goes on."""
    from newsreclib_amd import metrics, ops
    g = torch.Generator().manual_seed(5)
    long = ops.METRICS_MAX_CAND + 1 if case == "too_long" else 90
    csz, hsz = torch.tensor([12, 30, long, 7, 140]), torch.tensor([3, 0, 9, 5, 20])
    N, M = int(csz.sum()), int(hsz.sum())
    preds, targets = torch.randn(N, generator=g), (torch.rand(N, generator=g) < 0.2).float()
    ca, ha = torch.randint(0, 6, (N,), generator=g), torch.randint(0, 6, (M,), generator=g)
    bad = 2
    if case == "aspect_too_large":
        ca[12 + 30 + 17] = 6
    elif case == "aspect_negative":
        ha[3 + 4] = -1
    out = metrics.impression_metrics(preds.cuda(), targets.cuda(), csz.cuda(), (5, 10), {"categ": (ca.cuda(), ha.cuda(), 6)},
                                     hist_news_size=hsz.cuda())
    flag = int(out["status"])
    assert flag == (1 if case == "too_long" else 2)
    got = _rows_of(out, (5, 10), ("categ",))
    ca_ok, ha_ok = ca.clamp(0, 5), ha.clamp(0, 5)
    want = _ref_rows(preds, targets, csz, (5, 10), [(ca_ok, ha_ok, 6)], hsz)
    keep = [b for b in range(5) if b != bad]
    _check(f"{case}: the other impressions", got[keep], want[keep])
    assert float(got[bad].abs().max()) == 0.0
    ranks = torch.split(out["rank"].cpu(), csz.tolist())
    assert bool((ranks[bad] == -1).all())
    for b in keep:
        assert torch.equal(ranks[b], _ref_rank(torch.split(preds, csz.tolist())[b])[1].to(torch.int32))
    sm = metrics.StreamingMetrics((5, 10), 6, None)
    el = torch.empty(0, dtype=torch.long, device="cuda")
    sm.update((torch.zeros((), device="cuda"), preds.cuda(), targets.cuda(), csz.cuda(), hsz.cuda(), ca.cuda(), el, ha.cuda(), el, el, el))
    assert int(sm.count) == 4
    with pytest.raises(ValueError, match="candidates" if case == "too_long" else "aspect id"):
        sm.compute()


def test_offsets_that_decrease_or_leave_the_buffer_are_flagged():
    from newsreclib_amd import ops
    preds, targets = torch.tensor([0.1, 0.9, 0.3, 0.5, 0.2, 0.8, 0.7, 0.4]), torch.tensor([0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0])
    off = torch.tensor([0, 5, 3, 8, 12])            # impression 1 runs backwards, impression 3 leaves the buffer
    rank, rows, status = ops.impression_metrics(preds.cuda(), targets.cuda(), off.cuda(), (5,))
    assert int(status) == 4
    want0 = _ref_ranking_row(preds[0:5], targets[0:5], (5,))
    want2 = _ref_ranking_row(preds[3:8], targets[3:8], (5,))
    rows = rows.double().cpu()
    assert float((rows[0] - torch.tensor(want0)).abs().max()) <= TOL and float((rows[2] - torch.tensor(want2)).abs().max()) <= TOL
    assert float(rows[1].abs().max()) == 0.0 and float(rows[3].abs().max()) == 0.0


# ---- no device-to-host transfer in update ------------------------------------------------------------------------------------------
def test_update_does_not_synchronise_with_the_host():
    """``update`` under ``torch.cuda.set_sync_debug_mode("error")``.  By inspection: it builds the offsets with a device cumsum,
    reads only shapes (``numel``) on the host, and the ctypes call enqueues three kernels; the status word is read by ``compute``."""
    E = _epoch()
    steps = _steps(E, [100, 453])
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        honoured = False
        try:
            float(torch.ones(1, device="cuda").sum())
        except RuntimeError:
            honoured = True
        if not honoured:
            pytest.skip("this torch build does not raise on synchronising calls under set_sync_debug_mode('error')")
        sm = _run(steps)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert int(sm.count) == E["B"]


# ---- wiring ------------------------------------------------------------------------------------------------------------------------
def _eval_setup(n_imp=40):
    from newsreclib_amd.evaluation import DeviceNewsTable, NewsVectorCache
    from oracle import nrms_oracle as O
    from tests.helpers import build_module
    rng = np.random.default_rng(11)
    vocab, n_news = 400, 500
    mod = build_module(O.make_params(vocab, seed=2)).eval()
    table = DeviceNewsTable(builders.news_table(rng, n_news, vocab))
    return mod, table, NewsVectorCache(mod, table), builders.impressions(rng, n_imp, n_news, max_hist=50, max_cand=300)


def test_evaluate_impressions_with_device_metrics_equals_the_default():
    from newsreclib_amd.evaluation import evaluate_impressions
    _, _, cache, imps = _eval_setup()
    old = evaluate_impressions(cache, imps, batch_size=16, num_categ_classes=19, num_sent_classes=4)
    new = evaluate_impressions(cache, imps, batch_size=16, num_categ_classes=19, num_sent_classes=4, device_metrics=True)
    assert set(old) == set(new) and "sent_pers@10" in new
    for k, v in old.items():
        assert abs(new[k] - v) <= 1e-4, (k, new[k], v)
    assert new["auc"] == old["auc"]


def test_module_with_device_metrics_logs_the_same_test_keys():
    mod, table, _, imps = _eval_setup(20)
    outputs = {"train": [], "val": ["preds", "targets", "cand_news_size"],
               "test": ["preds", "targets", "cand_news_size", "hist_news_size", "target_categories", "target_sentiments",
                        "hist_categories", "hist_sentiments", "user_ids", "cand_news_ids"]}
    batches = []
    for lo in range(0, 20, 8):
        ch = imps[lo:lo + 8]
        batches.append(table.build_batch(torch.cat([i["hist"] for i in ch]), torch.tensor([len(i["hist"]) for i in ch]),
                                         torch.cat([i["cand"] for i in ch]), torch.tensor([len(i["cand"]) for i in ch]),
                                         torch.cat([i["labels"] for i in ch])))
    logged = {}
    for flag in (False, True):
        mod._init_step_outputs(outputs)
        mod.logged = {}
        mod.device_metrics = flag
        mod.on_test_epoch_start()
        with torch.no_grad():
            for j, b in enumerate(batches):
                mod.test_step(b, j)
        if flag:                                        # nothing but the accumulator is kept
            assert all(len(v) == 0 for v in mod.test_step_outputs.values())
        mod.on_test_epoch_end()
        logged[flag] = {k: float(v) for k, v in mod.logged.items() if k.startswith("test/")}
        # a validation epoch through the same switch
        mod.on_validation_epoch_start()
        with torch.no_grad():
            mod.validation_step(batches[0], 0)
        mod.on_validation_epoch_end()
        logged[flag].update({k: float(v) for k, v in mod.logged.items() if k.startswith("val/") and k != "val/loss_best"})
    assert set(logged[True]) == set(logged[False])
    assert {"test/loss", "test/auc", "test/mrr", "test/ndcg@5", "test/categ_div@5", "test/sent_pers@10", "val/ndcg@10"} <= set(logged[True])
    for k, v in logged[False].items():
        assert abs(logged[True][k] - v) <= 1e-4, (k, logged[True][k], v)
