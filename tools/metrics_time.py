#!/usr/bin/env python3
"""Times one evaluation epoch end two ways, in ONE process on one GPU, the two sides alternating (A, B, A, B, ...) after a shared
warm-up, device-event timed around work that ends in a host read (both sides return Python floats), median / min / max of --iters:

* torch:     the epoch end as it is by default -- ``torch.cat`` of the kept step outputs, ``metrics.ranking_metrics`` and two
             ``metrics.aspect_metrics`` (category, sentiment) over the whole epoch;
* streaming: ``metrics.StreamingMetrics`` -- the sum of one ``update`` per step (``nrl_impression_metrics`` into the epoch
             accumulator) plus ``compute`` (status word, means, the global AUC sort over the flat vectors).

The step outputs are synthetic and MIND-small-dev shaped: --impressions impressions in steps of --batch, ragged candidate counts
(log-normal, mean ~37, one of 300), histories of 0..50 clicks, 18 + 1 categories, 3 + 1 sentiments, k = 5, 10.  Peak allocated
memory of each side is the allocator's high-water mark above what the step outputs themselves occupy.  The two result dicts are
compared key by key.  Needs a GPU: there is no CPU path to time."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def make_steps(n_imp, batch, seed, device):
    g = torch.Generator().manual_seed(seed)
    csz = torch.exp(torch.randn(n_imp, generator=g) * 0.8 + 3.3).round().clamp(2, 300).long()
    csz[n_imp // 2] = 300
    hsz = torch.randint(0, 51, (n_imp,), generator=g)
    steps = []
    for lo in range(0, n_imp, batch):
        c, h = csz[lo:lo + batch], hsz[lo:lo + batch]
        n, m = int(c.sum()), int(h.sum())
        step = (torch.zeros(()), torch.randn(n, generator=g), (torch.rand(n, generator=g) < 0.06).float(), c, h,
                torch.randint(0, 19, (n,), generator=g), torch.randint(0, 4, (n,), generator=g),
                torch.randint(0, 19, (m,), generator=g), torch.randint(0, 4, (m,), generator=g),
                torch.arange(lo, lo + c.numel()), torch.arange(n))
        steps.append(tuple(t.to(device) for t in step))
    return steps, csz


def torch_epoch_end(steps, ks):
    from newsreclib_amd.metrics import aspect_metrics, ranking_metrics
    cat = lambda j: torch.cat([s[j] for s in steps])  # noqa: E731
    out = ranking_metrics(cat(1), cat(2), cat(3), ks)
    out.update(aspect_metrics(cat(1), cat(5), cat(7), cat(3), cat(4), 19, ks, prefix="categ"))
    out.update(aspect_metrics(cat(1), cat(6), cat(8), cat(3), cat(4), 4, ks, prefix="sent"))
    return out


def streaming_epoch(steps, ks):
    from newsreclib_amd.metrics import StreamingMetrics
    sm = StreamingMetrics(ks, 19, 4)
    for s in steps:
        sm.update(s)
    return sm.compute()


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


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--impressions", type=int, default=73152)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--iters", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("metrics_time: no GPU; a time measured anywhere else says nothing about this path")
    ks = (5, 10)
    steps, csz = make_steps(args.impressions, args.batch, args.seed, "cuda")
    sides = [("torch", lambda: torch_epoch_end(steps, ks)), ("streaming", lambda: streaming_epoch(steps, ks))]
    for _ in range(args.warmup):
        for _, fn in sides:
            fn()
    times, peaks, outs = {n: [] for n, _ in sides}, {}, {}
    for _ in range(args.iters):
        for name, fn in sides:
            ms, peak, out = timed(fn)
            times[name].append(ms)
            peaks[name] = max(peaks.get(name, 0), peak)
            outs[name] = out
    lines = [f"metrics_time: {args.impressions} impressions in steps of {args.batch} ({len(steps)} steps), {int(csz.sum())} candidates, "
             f"candidates per impression mean {float(csz.float().mean()):.1f} max {int(csz.max())}, histories 0..50, 19 categories, "
             f"4 sentiments, k = 5, 10; {torch.cuda.get_device_name()}; warm-up {args.warmup}, {args.iters} alternating repeats"]
    for name, _ in sides:
        t = sorted(times[name])
        lines.append(f"{name:10s} epoch end: median {t[len(t) // 2]:9.3f} ms  min {t[0]:9.3f}  max {t[-1]:9.3f}   "
                     f"peak allocated above the step outputs {peaks[name] / 2 ** 20:9.1f} MiB")
    med = {n: sorted(t)[len(t) // 2] for n, t in times.items()}
    lines.append(f"streaming / torch time: {med['streaming'] / med['torch']:.3f}   "
                 f"streaming / torch peak memory: {peaks['streaming'] / max(peaks['torch'], 1):.4f}")
    assert set(outs["torch"]) == set(outs["streaming"])
    worst = max(outs["torch"], key=lambda k: abs(outs["torch"][k] - outs["streaming"][k]))
    lines.append(f"largest difference between the two result dicts: {abs(outs['torch'][worst] - outs['streaming'][worst]):.3e} ({worst}); "
                 f"auc equal: {outs['torch']['auc'] == outs['streaming']['auc']}")
    report = "\n".join(lines)
    print(report)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(report + "\n")


if __name__ == "__main__":
    main()
