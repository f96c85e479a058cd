#!/usr/bin/env python3
"""Times the class-capped full-catalogue top-k against what it is built on and against torch, in ONE process on one GPU, the legs
alternating (A, B, C, D, A, ...) after a shared warm-up, device-event timed (nothing is read back inside the timed region),
median / min / max of --iters:

* capped:      ``ops.topk_scores_capped`` with m = --cap rows per class;
* uncapped:    ``ops.topk_scores`` of the same build (what the cap costs on top of the plain list);
* capped m=k:  ``ops.topk_scores_capped`` with m = k: the same lists as uncapped, so the difference is the consumer's own overhead
               (the tags, the class ballots) without any effect of the lower threshold;
* torch:       the same capped result in torch ops -- ``user @ table.T``, ``-inf`` at the excluded positions, a full descending
               sort per user, a per-class running count along the sorted order, the first k admitted rows.

Shape: --users users, --news table rows, D = 300 and 400, k = --k, --classes classes with a Zipf-like frequency (class c with
weight 1 / (c + 1)), ragged exclusion lists of 0..50 rows per user.  Then the ensemble (``ops.topk_ensemble_scores_capped``,
``ops.topk_ensemble_scores``, m = k, torch) at D = 768, T = 3.  Peak allocated memory of each leg is the allocator's high-water
mark above the inputs.  The capped and the torch lists are compared (the torch GEMM rounds differently, so rows may swap where
scores are within rounding of each other; the report counts them).  Last, what the cap bought: ``categ_div@k`` (and ``pers``) of
the capped and the uncapped lists from ``metrics.recommendation_aspect_metrics`` with the exclusion lists as the histories, and
the mean score of the lists.  Needs a GPU: there is no CPU path to time."""
import argparse
import os
import socket
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), torch.cuda.max_memory_allocated() - base, out


def zipf_classes(V, n_cls, generator):
    w = 1.0 / torch.arange(1, n_cls + 1, dtype=torch.float64)
    return torch.multinomial(w / w.sum(), V, replacement=True, generator=generator).to(torch.int32)


def capped_from_scores(s, row_class, k, m):
    """The capped lists of a (B, V) score matrix (-inf: may not be returned) in torch ops -> idx (B, k), score (B, k)."""
    B, V = s.shape
    val, order = torch.sort(s, dim=1, descending=True, stable=True)
    c_sorted = row_class.long()[order]
    admitted = torch.zeros_like(order, dtype=torch.bool)
    for c in torch.unique(row_class).tolist():              # (the class ids are an input: known before the timed region in a real use)
        is_c = c_sorted == c
        admitted |= is_c & (is_c.cumsum(1) <= m)
    admitted &= val > float("-inf")
    pos = torch.where(admitted, torch.arange(V, device=s.device).expand(B, V), torch.full_like(order, V))
    first = torch.topk(pos, k, dim=1, largest=False, sorted=True).values
    ok = first < V
    at = first.clamp_max(V - 1)
    idx = torch.where(ok, order.gather(1, at), torch.full_like(at, -1))
    score = torch.where(ok, val.gather(1, at), torch.full_like(val[:, :k], float("-inf")))
    return idx, score


def run_legs(legs, warmup, iters):
    for _ in range(warmup):
        for _, fn in legs:
            fn()
    times, peaks, outs = {n: [] for n, _ in legs}, {}, {}
    for _ in range(iters):
        for name, fn in legs:
            ms, peak, out = timed(fn)
            times[name].append(ms)
            peaks[name] = max(peaks.get(name, 0), peak)
            outs[name] = out
    return times, peaks, outs


def report_legs(lines, legs, times, peaks):
    med = {}
    for name, _ in legs:
        t = sorted(times[name])
        med[name] = t[len(t) // 2]
        lines.append(f"  {name:11s} median {med[name]:8.3f} ms  min {t[0]:8.3f}  max {t[-1]:8.3f}   peak allocated above the inputs "
                     f"{peaks[name] / 2 ** 20:9.2f} MiB")
    lines.append(f"  capped / uncapped time: {med['capped'] / med['uncapped']:.3f}   capped m=k / uncapped: "
                 f"{med['capped m=k'] / med['uncapped']:.3f}   capped / torch: {med['capped'] / med['torch']:.3f}   capped / torch "
                 f"peak memory: {peaks['capped'] / max(peaks['torch'], 1):.4f}")


def compare(lines, outs, k):
    ci, cs, status = outs["capped"][:3]
    ti, ts = outs["torch"]
    same = ci == ti
    B = ci.shape[0]
    lines.append(f"  status word {int(status)}; capped against torch: rows equal in {int(same.sum())} of {same.numel()} slots, same row "
                 f"sets for {int((ci.sort(1).values == ti.sort(1).values).all(1).sum())} of {B} users, largest score difference "
                 f"{float((cs - ts)[torch.isfinite(cs) & torch.isfinite(ts)].abs().max()):.3e}")
    ui, us = outs["uncapped"][:2]
    mi, ms = outs["capped m=k"][:2]
    lines.append(f"  capped m=k equals uncapped bit for bit: {bool(torch.equal(ui, mi) and torch.equal(us.view(torch.int32), ms.view(torch.int32)))}")


def bought(lines, outs, row_class, n_cls, excl_idx, excl_off, k):
    from newsreclib_amd.metrics import recommendation_aspect_metrics
    for name in ("capped", "uncapped"):
        idx, score = outs[name][:2]
        got = recommendation_aspect_metrics(idx, score, row_class, excl_idx, excl_off, n_cls, (k,), "categ")
        lines.append(f"  {name:9s} lists: categ_div@{k} {got[f'categ_div@{k}']:.4f}  categ_pers@{k} {got[f'categ_pers@{k}']:.4f}  mean score "
                     f"{float(score[idx >= 0].double().mean()):.4f}  filled slots {int((idx >= 0).sum())} of {idx.numel()}")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--users", type=int, default=512)
    ap.add_argument("--news", type=int, default=65536)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--cap", type=int, default=2)
    ap.add_argument("--classes", type=int, default=19)
    ap.add_argument("--iters", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--dims", default="300,400", help="the D of the dot-product legs (a kernel trace is easier to read with one)")
    ap.add_argument("--no-ensemble", action="store_true", help="leave the ensemble legs out")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("topk_capped_time: no GPU; a time measured anywhere else says nothing about this path")
    from newsreclib_amd import _lib, ops
    B, V, k, m, n_cls = args.users, args.news, args.k, args.cap, args.classes
    lines = [f"topk_capped_time: B = {B} users, V = {V} news, k = {k}, at most m = {m} of each of {n_cls} classes (frequency ~ 1 / rank), "
             f"exclusion lists of 0..50 rows; {torch.cuda.get_device_name()} on {socket.gethostname()}; library build id "
             f"{_lib.load().nrl_build_id().decode()}; torch {torch.__version__}; warm-up {args.warmup}, {args.iters} alternating "
             f"repeats, device events"]

    def masks(g):
        sizes = torch.randint(0, 51, (B,), generator=g)
        excl_idx = torch.randint(0, V, (int(sizes.sum()),), generator=g).cuda()
        excl_off = torch.cat([torch.zeros(1, dtype=torch.int64), sizes.cumsum(0)]).cuda()
        return excl_idx, excl_off, torch.repeat_interleave(torch.arange(B), sizes).cuda()

    for D in (int(d) for d in args.dims.split(",") if d):
        g = torch.Generator().manual_seed(args.seed + D)
        user, table = torch.randn(B, D, generator=g).cuda(), torch.randn(V, D, generator=g).cuda()
        row_class = zipf_classes(V, n_cls, g).cuda()
        excl_idx, excl_off, excl_user = masks(g)

        def torch_ops():
            s = user @ table.T
            s[excl_user, excl_idx] = float("-inf")
            return capped_from_scores(s, row_class, k, m)

        legs = [("capped", lambda: ops.topk_scores_capped(user, table, k, row_class, m, excl_idx, excl_off)),
                ("uncapped", lambda: ops.topk_scores(user, table, k, excl_idx, excl_off)),
                ("capped m=k", lambda: ops.topk_scores_capped(user, table, k, row_class, k, excl_idx, excl_off)),
                ("torch", torch_ops)]
        times, peaks, outs = run_legs(legs, args.warmup, args.iters)
        lines.append(f"D = {D}: score matrix {B * V * 4 / 2 ** 20:.1f} MiB, {2.0 * B * V * D / 1e9:.1f} GFLOP")
        report_legs(lines, legs, times, peaks)
        compare(lines, outs, k)
        bought(lines, outs, row_class, n_cls, excl_idx, excl_off, k)

    if not args.no_ensemble:
        ensemble_legs(lines, args, ops, masks)

    report = "\n".join(lines)
    print(report)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(report + "\n")


def ensemble_legs(lines, args, ops, masks):
    B, V, k, m, n_cls = args.users, args.news, args.k, args.cap, args.classes
    D, T = 768, 3
    g = torch.Generator().manual_seed(args.seed + D)
    users = [torch.randn(B, D, generator=g).cuda() for _ in range(T)]
    tables = [torch.randn(V, D, generator=g).cuda() for _ in range(T)]
    weights = [1.0, 0.2, -0.25]
    row_class = zipf_classes(V, n_cls, g).cuda()
    excl_idx, excl_off, excl_user = masks(g)

    def torch_ensemble():
        pop = torch.ones((B, V), dtype=torch.bool, device="cuda")
        pop[excl_user, excl_idx] = False
        n = pop.sum(1, keepdim=True).float()
        z = None
        for u, t, w in zip(users, tables, weights):
            s = u @ t.T
            mean = (s * pop).sum(1, keepdim=True) / n
            sd = ((((s - mean) ** 2) * pop).sum(1, keepdim=True) / (n - 1)).sqrt()
            zt = w * ((s - mean) / sd)
            z = zt if z is None else z + zt
        return capped_from_scores(z.masked_fill(~pop, float("-inf")), row_class, k, m)

    legs = [("capped", lambda: ops.topk_ensemble_scores_capped(users, tables, weights, k, row_class, m, excl_idx, excl_off)),
            ("uncapped", lambda: ops.topk_ensemble_scores(users, tables, weights, k, excl_idx, excl_off)),
            ("capped m=k", lambda: ops.topk_ensemble_scores_capped(users, tables, weights, k, row_class, k, excl_idx, excl_off)),
            ("torch", torch_ensemble)]
    times, peaks, outs = run_legs(legs, args.warmup, args.iters)
    lines.append(f"ensemble, T = {T}, D = {D}: {T} score matrices of {B * V * 4 / 2 ** 20:.1f} MiB, {2.0 * 2 * T * B * V * D / 1e9:.1f} GFLOP "
                 f"(two passes over the tables)")
    report_legs(lines, legs, times, peaks)
    compare(lines, outs, k)
    bought(lines, outs, row_class, n_cls, excl_idx, excl_off, k)


if __name__ == "__main__":
    main()
