#!/usr/bin/env python3
"""Times the evaluation of a grid of MANNeR ensemble weights two ways, in ONE process on one GPU, on the MIND-small-dev-shaped epoch
of ``tools/metrics_time.py`` (ragged candidate counts, histories of 0..50, 19 categories, 4 sentiments, k = 5, 10) with three
D = 768 news-vector tables of 65 536 rows:

* grid: per batch one ``manner_zscores`` and one ``GridStreamingMetrics.update`` (``nrl_grid_metrics``: all G rows in one launch);
* loop: per batch and per weight row one ``manner_scores`` over the tables of the non-zero weights and one
        ``StreamingMetrics.update`` -- the path the library had, and the reference's cost model (one evaluation per point).

G = 1, 21 and 441 (categ / sent weights -1 ... 1 in steps of 0.1; the CR weight is 1).  The legs alternate (grid, loop, grid, loop ...)
after a shared warm-up; a leg is one pass over --batches batches (default: the whole epoch of 143), timed as a whole by device
events around work that ends in the status read; medians, and min / max as the spread of the repeated leg.  When --batches is less
than the epoch, the report says so and scales nothing.

--parent-lib PATH also times ``nrl_manner_scores`` and ``nrl_impression_metrics`` of this build against the library of the parent
commit in the order parent, this build, parent (raw C calls on the same buffers; the metrics call with sums and count, so that the
two reductions run), checks that they return the parent's bits, and prints the spread between the parent's own two runs next to
the difference.

--profile G runs --batches grid batches of G rows and nothing else (for a ``rocprofv3 --kernel-trace --stats`` run of its own).
Needs a GPU: there is no CPU path to time."""
import argparse
import ctypes
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools.metrics_time import make_steps  # noqa: E402

KS, V, D = (5, 10), 65536, 768


def weight_rows(G):
    if G == 1:
        return torch.tensor([[1.0, 0.2, -0.25]])
    axis = [round(-1.0 + 0.1 * i, 1) for i in range(21)]
    if G == 21:
        return torch.tensor([[1.0, cw, -0.25] for cw in axis])
    assert G == 441
    return torch.tensor([[1.0, cw, sw] for cw in axis for sw in axis])


def make_batches(steps, seed):
    """Per step: index lists into the tables (histories of at least one click: an empty one is a NaN row on both paths alike)."""
    g = torch.Generator().manual_seed(seed + 1)
    out = []
    for s in steps:
        csz, hsz = s[3].cpu(), s[4].cpu().clamp(min=1)
        n, m = int(csz.sum()), int(hsz.sum())
        off = lambda z: torch.cat([torch.zeros(1, dtype=torch.long), torch.cumsum(z, 0)]).cuda()  # noqa: E731
        step = list(s)
        step[4] = hsz.cuda()
        step[7], step[8] = torch.randint(0, 19, (m,), generator=g).cuda(), torch.randint(0, 4, (m,), generator=g).cuda()
        max_cand = int(csz.max())
        flat = (torch.arange(max_cand)[None, :] < csz[:, None]).reshape(-1).nonzero().reshape(-1).cuda()      # padded -> flat
        out.append(dict(step=tuple(step), hist_idx=torch.randint(0, V, (m,), generator=g).cuda(), hist_off=off(hsz),
                        cand_idx=torch.randint(0, V, (n,), generator=g).cuda(), cand_off=off(csz), max_cand=max_cand, csz=csz,
                        flat=flat))
    return out


def grid_leg(tables, batches, w):
    from newsreclib_amd.metrics import GridStreamingMetrics
    from newsreclib_amd.ops_manner import manner_zscores
    gm = GridStreamingMetrics(w, KS, 19, 4)
    for b in batches:
        comp = manner_zscores(tables, b["hist_idx"], b["hist_off"], b["cand_idx"], b["cand_off"], b["max_cand"])
        gm.update(comp, b["step"])
    return gm.compute()["values"]


def loop_leg(tables, batches, w):
    from newsreclib_amd.metrics import StreamingMetrics
    from newsreclib_amd.ops_manner import manner_scores
    values = []
    for row in w.tolist():
        keep = [t for t in range(len(row)) if row[t] != 0]
        sm = StreamingMetrics(KS, 19, 4)
        for b in batches:
            padded = manner_scores([tables[t] for t in keep], [row[t] for t in keep], b["hist_idx"], b["hist_off"], b["cand_idx"],
                                   b["cand_off"], b["max_cand"])
            step = list(b["step"])
            step[1] = padded.reshape(-1)[b["flat"]]
            sm.update(tuple(step))
        flags = int(sm.status)
        assert flags == 0, flags
        n = int(sm.count)
        values.append((sm.sums / max(n, 1)).tolist())
    return values


def timed(fn):
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def stats(ts):
    t = sorted(ts)
    return t[len(t) // 2], t[0], t[-1]


def open_lib(path):
    from newsreclib_amd import _lib
    lib = ctypes.CDLL(path)
    for name in ("nrl_manner_scores", "nrl_impression_metrics", "nrl_impression_metrics_workspace_bytes"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    return lib


def parent_comparison(parent_path, tables, b, iters):
    """nrl_manner_scores / nrl_impression_metrics: the parent's library, this build's, the parent's again, on the same buffers."""
    from newsreclib_amd import _lib
    libs = [("parent (1st)", open_lib(parent_path)), ("this build", open_lib(_lib.LIB_PATH)), ("parent (2nd)", open_lib(parent_path))]
    B, N = int(b["cand_off"].numel()) - 1, int(b["cand_idx"].numel())
    ptrs = (ctypes.c_void_p * 3)(*[t.data_ptr() for t in tables])
    wts = (ctypes.c_float * 3)(1.0, 0.2, -0.25)
    step = b["step"]
    preds, targets = step[1].float().contiguous(), step[2].float().contiguous()
    ks = (ctypes.c_int32 * 2)(*KS)
    lines = []

    def scores(lib, out):
        rc = lib.nrl_manner_scores(ptrs, wts, 3, V, b["hist_idx"].data_ptr(), b["hist_off"].data_ptr(), b["cand_idx"].data_ptr(),
                                   b["cand_off"].data_ptr(), B, b["max_cand"], D, out.data_ptr(), None)
        assert rc == 0, rc

    def metrics(lib, rows, rank, sums, count, status, ws):
        # sums / count given: the call runs all three kernels of the entry (the impressions and the two reductions)
        rc = lib.nrl_impression_metrics(preds.data_ptr(), targets.data_ptr(), b["cand_off"].data_ptr(), N, B, 2, step[5].data_ptr(),
                                        step[7].data_ptr(), 19, step[6].data_ptr(), step[8].data_ptr(), 4, b["hist_off"].data_ptr(),
                                        int(step[7].numel()), ks, 2, rank.data_ptr(), rows.data_ptr(), sums.data_ptr(), count.data_ptr(),
                                        status.data_ptr(), ws.data_ptr(), ws.numel(), None)
        assert rc == 0, rc

    for what in ("nrl_manner_scores", "nrl_impression_metrics"):
        med, outs = {}, {}
        for name, lib in libs:
            if what == "nrl_manner_scores":
                out = torch.zeros(B, b["max_cand"], device="cuda")
                run = lambda: scores(lib, out)  # noqa: E731
                keep = lambda: (out.clone(),)  # noqa: E731
            else:
                rows, rank = torch.zeros(B, 11, device="cuda"), torch.zeros(N, dtype=torch.int32, device="cuda")
                status = torch.zeros(1, dtype=torch.int32, device="cuda")
                sums, count = torch.zeros(11, dtype=torch.float64, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda")
                ws = torch.empty(lib.nrl_impression_metrics_workspace_bytes(N, B, 2, 2), dtype=torch.uint8, device="cuda")
                run = lambda: metrics(lib, rows, rank, sums, count, status, ws)  # noqa: E731
                # (every library accumulates over the same 5 + iters calls from zero: the sums are comparable bit for bit)
                keep = lambda: (rows.clone(), rank.clone(), sums.view(torch.int32).clone(), count.view(torch.int32).clone())  # noqa: E731
            for _ in range(5):
                run()
            ts = [timed(run)[0] for _ in range(iters)]
            med[name], outs[name] = stats(ts), keep()
        same = all(torch.equal(x.view(torch.int32), y.view(torch.int32))
                   for other in ("this build", "parent (2nd)") for x, y in zip(outs["parent (1st)"], outs[other]))
        p1, p2, new = med["parent (1st)"][0], med["parent (2nd)"][0], med["this build"][0]
        lo, hi = min(p1, p2), max(p1, p2)
        outputs = "out" if what == "nrl_manner_scores" else "rows, rank, sums and count (the reductions included)"
        lines.append(f"{what} (B = {B}, one call, median of {iters}): parent {1e3 * p1:.2f} us, this build {1e3 * new:.2f} us, parent again "
                     f"{1e3 * p2:.2f} us; spread between the parent's two runs {1e3 * (hi - lo):.2f} us; this build is "
                     f"{'inside' if lo <= new <= hi else ('below' if new < lo else 'ABOVE')} it "
                     f"({1e3 * (new - hi):+.2f} us against the slower parent run); {outputs} bit-equal to the parent's: {same}")
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--impressions", type=int, default=73152)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--batches", type=int, default=0, help="batches of one leg (0: the whole epoch)")
    ap.add_argument("--grids", type=int, nargs="+", default=[1, 21, 441])
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--profile", type=int, default=0)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("grid_metrics_time: no GPU; a time measured anywhere else says nothing about this path")
    steps, csz = make_steps(args.impressions, args.batch, args.seed, "cuda")
    n_steps = len(steps)
    if args.batches:
        steps = steps[:args.batches]
    batches = make_batches(steps, args.seed)
    g = torch.Generator().manual_seed(args.seed + 2)
    tables = [torch.randn(V, D, generator=g).cuda() for _ in range(3)]
    if args.profile:
        w = weight_rows(args.profile)
        for _ in range(2):
            grid_leg(tables, batches, w)
        torch.cuda.synchronize()
        return
    lines = [f"grid_metrics_time: {len(batches)} of the epoch's {n_steps} batches of {args.batch} impressions "
             f"({sum(int(b['csz'].sum()) for b in batches)} candidates, mean {float(csz.float().mean()):.1f} max {int(csz.max())} per impression), "
             f"three ({V}, {D}) tables, 19 categories, 4 sentiments, k = 5, 10; {torch.cuda.get_device_name()}; warm-up {args.warmup}, "
             f"{args.iters} alternating repeats; a leg = one pass over these batches for all G rows, status read included"]
    for G in args.grids:
        w = weight_rows(G)
        sides = [("grid", lambda: grid_leg(tables, batches, w)), ("loop", lambda: loop_leg(tables, batches, w))]
        for _ in range(args.warmup):
            for _, fn in sides:
                fn()
        times, outs = {n: [] for n, _ in sides}, {}
        for _ in range(args.iters):
            for name, fn in sides:
                ms, outs[name] = timed(fn)
                times[name].append(ms)
        same = outs["grid"] == outs["loop"]
        gm, lm = stats(times["grid"]), stats(times["loop"])
        lines.append(f"G = {G:3d}: grid median {gm[0]:10.3f} ms (min {gm[1]:.3f}, max {gm[2]:.3f})   loop median {lm[0]:10.3f} ms "
                     f"(min {lm[1]:.3f}, max {lm[2]:.3f})   loop / grid {lm[0] / gm[0]:7.2f}   per batch: grid {gm[0] / len(batches):.3f} ms, "
                     f"loop {lm[0] / len(batches):.3f} ms   means equal to the bit: {same}")
    if args.parent_lib:
        lines += parent_comparison(args.parent_lib, tables, batches[0], 200)
    report = "\n".join(lines)
    print(report)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(report + "\n")


if __name__ == "__main__":
    main()
