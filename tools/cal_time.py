#!/usr/bin/env python3
"""Times the calibrated greedy re-ranking against its neighbours, in ONE process on one GPU, the legs alternating after a shared
warm-up, device-event timed (nothing is read back inside the timed region), median / min / max of --iters whole calls:

* cal:     ``ops.calibrated_rerank`` at lambda 0.5, mu 0.25, gamma 0.5 (Gram matrix, penalty and calibration term in one launch);
* cal_mu0: the same at mu = 0 (lambda 0.5, gamma 0.5, no table): the form without the Gram stage;
* cal_g0:  the same at gamma = 0, mu = 1 - lambda: the lists of ``ops.mmr_rerank``, through the new kernel;
* mmr:     ``ops.mmr_rerank`` of the same build at lambda 0.5;
* torch:   the lists of the cal leg in torch ops -- the (B, N, D) gather, the (B, N, N) ``bmm``, the scaling, and a Python loop
  of k steps that carries the class counts and forms the (B, S, S) minima and maxima of the calibration term.

With --parent-lib (the shared library of a checkout of the parent commit) ``nrl_mmr_rerank`` and ``nrl_topk_scores`` of that
library are called through ctypes on the same tensors, TWICE each per repeat as two separate legs (parent_a, parent_b), beside
the same entry of this build's library reached through the same ctypes call (mmr_lib, topk_lib: the argument checks of the ops
wrappers run between the two events, so a wrapper leg against a bare call would compare Python, not libraries).  The three take
turns at the three places of their group (the first place runs behind another kind of leg and finds other things in the
caches).  The repeats come in --rounds rounds; a leg's median over one round is one run of it.  The range
of the parent's 2 * rounds runs is the spread this session shows between runs of the same code, and the median run of the new
build's entry is compared against that range.  Rows and score bits of both entries are compared too.

Shape: --users users, --news table rows around --topics topic centres, a news' class is its topic modulo S = --classes; a user has
a ragged history of 5 ... 50 news drawn from three topics of its own, its vector is the mean of its history's rows and its target
the integer class counts of that history (``ops.class_targets``).  D = 300 and 400, N = 64 and 128, k = --k, cosine, normalised
relevance.  Peak allocated memory of each leg is the allocator's high-water mark above the inputs.  The report also quotes
``metrics.recommendation_aspect_metrics`` (categ_pers@k, categ_div@k) and the mean list score of the first k of the pool and of the
calibrated lists at three gamma values.  Needs a GPU: there is no CPU path to time."""
import argparse
import ctypes
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


def parent_entries(path):
    """``nrl_topk_scores`` and ``nrl_mmr_rerank`` of the library at ``path`` with the arguments of ``ops.topk_scores`` /
    ``ops.mmr_rerank`` (cosine, normalised)"""
    from newsreclib_amd import _lib, ops
    lib = ctypes.CDLL(path)
    for name in ("nrl_topk_scores_workspace_bytes", "nrl_topk_scores", "nrl_mmr_rerank"):
        getattr(lib, name).restype, getattr(lib, name).argtypes = _lib.SIGNATURES[name]
    lib.nrl_build_id.restype = ctypes.c_char_p

    def topk(user, table, k):
        B, D, V = user.shape[0], user.shape[1], table.shape[0]
        idx, score, status = ops._topk_outputs(B, k, user.device)
        ws = ops.workspace(lib.nrl_topk_scores_workspace_bytes(B, V, D, k, 0), user.device)
        rc = lib.nrl_topk_scores(user.data_ptr(), table.data_ptr(), B, V, D, k, None, None, None, 0, idx.data_ptr(), score.data_ptr(),
                                 status.data_ptr(), ws.data_ptr(), ws.numel(), ops._stream())
        assert rc == 0, rc
        return idx, score, status

    def mmr(pool_idx, pool_score, table, k, lam):
        B, N = pool_idx.shape
        idx, score, status = ops._topk_outputs(B, k, pool_idx.device)
        out = torch.empty((B, k), dtype=torch.float32, device=pool_idx.device)
        rc = lib.nrl_mmr_rerank(pool_idx.data_ptr(), pool_score.data_ptr(), table.data_ptr(), B, N, table.shape[0], table.shape[1], k,
                                float(lam), 0, 1, idx.data_ptr(), score.data_ptr(), out.data_ptr(), status.data_ptr(), ops._stream())
        assert rc == 0, rc
        return idx, score, out, status

    return topk, mmr, lib.nrl_build_id().decode()


def torch_calibrated(pool_idx, pool_score, table, row_class, target, k, lam, mu, gamma):
    """The definition in torch ops (every slot live and every class in range: the pool of ``topk_scores`` over a table larger
    than N has no empty slot)."""
    B, N = pool_idx.shape
    S = target.shape[1]
    rows = table[pool_idx]                                                    # (B, N, D)
    gram = torch.bmm(rows, rows.transpose(1, 2))
    r = torch.diagonal(gram, dim1=1, dim2=2).sqrt().reciprocal()
    sim = gram * (r.unsqueeze(2) * r.unsqueeze(1))
    lo, hi = pool_score.min(1, keepdim=True).values, pool_score.max(1, keepdim=True).values
    rel = lam * ((pool_score - lo) / (hi - lo))
    cls = row_class[pool_idx].long()                                          # (B, N)
    pen = torch.zeros_like(pool_score)
    taken = torch.zeros_like(pool_score, dtype=torch.bool)
    counts = torch.zeros_like(target)
    users = torch.arange(B, device=pool_idx.device)
    eye = torch.eye(S, device=pool_idx.device).unsqueeze(0)
    tgt = target.unsqueeze(1)                                                 # (B, 1, S)
    picks = []
    for t in range(k):
        plus = counts.unsqueeze(1) + eye                                      # (B, S, S): row c = the counts with one more of class c
        cal = torch.minimum(plus, tgt).sum(2) / torch.maximum(plus, tgt).sum(2)
        obj = (rel - mu * pen + gamma * cal.gather(1, cls)).masked_fill(taken, float("-inf"))
        c = obj.argmax(1)
        picks.append(c)
        taken[users, c] = True
        counts[users, cls[users, c]] += 1.0
        row = sim[users, c]
        pen = row if t == 0 else torch.maximum(pen, row)
    slots = torch.stack(picks, 1)
    return pool_idx.gather(1, slots), pool_score.gather(1, slots)


def median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--users", type=int, default=512)
    ap.add_argument("--news", type=int, default=65536)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--classes", type=int, default=19)
    ap.add_argument("--iters", type=int, default=15, help="repeats per round")
    ap.add_argument("--rounds", type=int, default=5, help="rounds: a leg's median over one round is one run of it")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--topics", type=int, default=256, help="topic centres the news vectors are drawn around")
    ap.add_argument("--pools", type=int, nargs="+", default=[64, 128])
    ap.add_argument("--dims", type=int, nargs="+", default=[300, 400])
    ap.add_argument("--gammas", type=float, nargs="+", default=[0.25, 0.5, 1.0])
    ap.add_argument("--parent-lib", default=None, help="shared library of a checkout of the parent commit")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("cal_time: no GPU; a time measured anywhere else says nothing about this path")
    from newsreclib_amd import _lib, ops
    from newsreclib_amd.metrics import recommendation_aspect_metrics
    B, V, k, S = args.users, args.news, args.k, args.classes
    lam, mu, gamma = 0.5, 0.25, 0.5
    lines = [f"cal_time: B = {B} users, V = {V} news, k = {k}, S = {S} classes, {args.topics} topics, cosine, normalised relevance; timed "
             f"legs at lambda {lam}, mu {mu}, gamma {gamma}; {torch.cuda.get_device_name()} on {socket.gethostname()}; library build id "
             f"{_lib.load().nrl_build_id().decode()}; torch {torch.__version__}; warm-up {args.warmup}, {args.rounds} rounds of {args.iters} "
             "alternating repeats of whole calls, device events"]
    parent = None
    if args.parent_lib and os.path.exists(args.parent_lib):
        from newsreclib_amd import _build
        parent, this_lib = parent_entries(args.parent_lib), parent_entries(_build.LIB)
        lines.append(f"parent legs: nrl_mmr_rerank and nrl_topk_scores of {os.path.basename(args.parent_lib)} with build id {parent[2]}, "
                     "loaded beside this build's library")
    else:
        lines.append("parent legs: NOT measured (no library of the parent commit was given with --parent-lib)")
    inside = []
    for D in args.dims:
        for N in args.pools:
            g = torch.Generator().manual_seed(args.seed + D + N)
            centres = torch.randn(args.topics, D, generator=g)
            topic = torch.randint(0, args.topics, (V,), generator=g)
            table = ((centres[topic] + torch.randn(V, D, generator=g)) * 0.5 ** 0.5).cuda()
            row_class = (topic % S).to(torch.int32).cuda()
            # ragged histories from three topics per user; the user vector is the mean of the history's rows
            sizes = torch.randint(5, 51, (B,), generator=g)
            by_topic = torch.argsort(topic, stable=True)
            starts = torch.searchsorted(topic[by_topic], torch.arange(args.topics))
            ends = torch.searchsorted(topic[by_topic], torch.arange(args.topics), right=True)
            hist = []
            for u in range(B):
                mine = torch.randint(0, args.topics, (3,), generator=g)
                pick = mine[torch.randint(0, 3, (int(sizes[u]),), generator=g)]
                width = (ends[pick] - starts[pick]).clamp_min(1)
                hist.append(by_topic[starts[pick] + torch.minimum((torch.rand(pick.shape, generator=g) * width).long(), width - 1)])
            hist_idx = torch.cat(hist).cuda()
            hist_off = torch.cat([torch.zeros(1, dtype=torch.int64), sizes.cumsum(0)]).cuda()
            owner = torch.repeat_interleave(torch.arange(B), sizes).cuda()
            user = torch.zeros(B, D, device="cuda").index_add_(0, owner, table[hist_idx]) / sizes.cuda()[:, None]
            target = ops.class_targets(hist_idx, hist_off, row_class, S)
            pool_idx, pool_score, _ = ops.topk_scores(user, table, N, hist_idx, hist_off)
            head = [("cal", lambda: ops.calibrated_rerank(pool_idx, pool_score, table, row_class, target, k, lam, mu, gamma)),
                    ("cal_mu0", lambda: ops.calibrated_rerank(pool_idx, pool_score, None, row_class, target, k, lam, 0.0, gamma)),
                    ("cal_g0", lambda: ops.calibrated_rerank(pool_idx, pool_score, table, row_class, target, k, lam, 1.0 - lam, 0.0))]
            mmr_legs = [("mmr", lambda: ops.mmr_rerank(pool_idx, pool_score, table, k, lam))]
            torch_leg = [("torch", lambda: torch_calibrated(pool_idx, pool_score, table, row_class, target, k, lam, mu, gamma))]
            topk_legs = [("topk", lambda: ops.topk_scores(user, table, N))]
            if parent is not None:
                # library against library: this build's entries through the very ctypes calls that reach the parent's (the
                # checks of the ops wrappers run between the two events and cost the same few microseconds in either build)
                mmr_legs += [("mmr_lib", lambda: this_lib[1](pool_idx, pool_score, table, k, lam)),
                             ("mmr_parent_a", lambda: parent[1](pool_idx, pool_score, table, k, lam)),
                             ("mmr_parent_b", lambda: parent[1](pool_idx, pool_score, table, k, lam))]
                topk_legs += [("topk_lib", lambda: this_lib[0](user, table, N)), ("topk_parent_a", lambda: parent[0](user, table, N)),
                              ("topk_parent_b", lambda: parent[0](user, table, N))]
            legs = head + mmr_legs + torch_leg + topk_legs
            for _ in range(args.warmup):
                for _, fn in legs:
                    fn()
            times, runs, peaks, outs = {n: [] for n, _ in legs}, {n: [] for n, _ in legs}, {}, {}
            for rnd in range(args.rounds):
                for it in range(args.iters):
                    # What ran just before a leg decides what it finds in the caches (the torch leg streams the gathered rows
                    # through them, a top-k leg leaves the table in the last-level cache), so the legs that are compared with each
                    # other sit side by side and take turns at every place of their group.
                    # (the ops legs open their groups; behind them this build's library and the parent's two legs rotate)
                    a, b = (1 + it % 3, 1 + it % 3) if parent else (1, 1)
                    for name, fn in head + mmr_legs[:1] + mmr_legs[a:] + mmr_legs[1:a] + torch_leg + topk_legs[:1] + topk_legs[b:] + \
                            topk_legs[1:b]:
                        ms, peak, out = timed(fn)
                        times[name].append(ms)
                        peaks[name] = max(peaks.get(name, 0), peak)
                        outs[name] = out
                for name, _ in legs:
                    runs[name].append(median(times[name][-args.iters:]))
            lines.append(f"D = {D}, N = {N}: gathered pool rows {B * N * D * 4 / 2 ** 20:.1f} MiB, Gram matrices {B * N * N * 4 / 2 ** 20:.1f} "
                         f"MiB, (B, S, S) term operands {B * S * S * 4 / 2 ** 20:.2f} MiB")
            med = {}
            for name, _ in legs:
                med[name] = median(times[name])
                lines.append(f"  {name:14s} median {med[name]:8.3f} ms  min {min(times[name]):8.3f}  max {max(times[name]):8.3f}   peak allocated "
                             f"above the inputs {peaks[name] / 2 ** 20:8.2f} MiB")
            lines.append(f"  cal / torch time: {med['cal'] / med['torch']:.3f}   cal / mmr: {med['cal'] / med['mmr']:.3f}   cal_g0 / mmr: "
                         f"{med['cal_g0'] / med['mmr']:.3f}   cal_mu0 / cal: {med['cal_mu0'] / med['cal']:.3f}   cal / topk (the pool): "
                         f"{med['cal'] / med['topk']:.3f}")
            ci, ti = outs["cal"][0], outs["torch"][0]
            g0, mm = outs["cal_g0"], outs["mmr"]
            lines.append(f"  status words {int(outs['cal'][4])} / {int(outs['cal_mu0'][4])} / {int(g0[4])}; rows equal to torch's in "
                         f"{int((ci == ti).sum())} of {ci.numel()} slots, same lists for {int((ci == ti).all(1).sum())} of {B} users; "
                         f"cal_g0 against mmr: same rows {torch.equal(g0[0], mm[0])}, same score bits "
                         f"{torch.equal(g0[1].view(torch.int32), mm[1].view(torch.int32))}, objectives equal {torch.equal(g0[2], mm[2])}")
            if parent is not None:
                for entry, new in (("mmr", "mmr_lib"), ("topk", "topk_lib")):
                    # a run = the median of one round of one leg: the parent has 2 * rounds runs, this build rounds runs
                    theirs, ours = runs[f"{entry}_parent_a"] + runs[f"{entry}_parent_b"], runs[new]
                    lo, hi, mid = min(theirs), max(theirs), median(theirs)
                    po, no = outs[f"{entry}_parent_a"], outs[entry]      # (the bits: what the ops wrapper of this build returns)
                    same = torch.equal(no[0], po[0]) and all(torch.equal(x.view(torch.int32), y.view(torch.int32))
                                                             for x, y in zip(no[1:-1], po[1:-1]))
                    ok = lo <= median(ours) <= hi
                    inside.append(ok and same)
                    lines.append(f"  {entry}: runs of the parent's library {lo:.4f} ... {hi:.4f} ms (median {mid:.4f}, spread "
                                 f"{100 * (hi - lo) / mid:.2f} %); runs of this build {min(ours):.4f} ... {max(ours):.4f} ms, median "
                                 f"{median(ours):.4f} = {100 * (median(ours) - mid) / mid:+.2f} % against the parent's median "
                                 f"({'inside' if ok else 'OUTSIDE'} the parent's own spread); same rows and bits as the parent: {same}")
            stats = recommendation_aspect_metrics(pool_idx[:, :k].contiguous(), pool_score[:, :k].contiguous(), row_class, hist_idx, hist_off,
                                                  S, (k,))
            lines.append(f"  first {k} of the pool:          categ_pers@{k} {stats[f'categ_pers@{k}']:.4f}   categ_div@{k} "
                         f"{stats[f'categ_div@{k}']:.4f}   mean list score {float(pool_score[:, :k].mean()):.4f}")
            for gm in args.gammas:
                for m, tbl in ((0.0, None), (mu, table)):
                    idx, score, _, cal, _ = ops.calibrated_rerank(pool_idx, pool_score, tbl, row_class, target, k, lam, m, gm)
                    # the kernel's own order is the list's order: score the slots by their position
                    order = torch.arange(k, 0, -1, device="cuda").float().expand(B, k).contiguous()
                    stats = recommendation_aspect_metrics(idx, order, row_class, hist_idx, hist_off, S, (k,))
                    lines.append(f"  over {N:3d} at gamma {gm:4.2f}, mu {m:4.2f}: categ_pers@{k} {stats[f'categ_pers@{k}']:.4f}   categ_div@{k} "
                                 f"{stats[f'categ_div@{k}']:.4f}   mean list score {float(score.mean()):.4f}   mean out_cal[k - 1] "
                                 f"{float(cal[:, k - 1].mean()):.4f}")
    if parent is not None:
        lines.append(f"mmr_rerank and topk_scores against the parent's library: {sum(inside)} of {len(inside)} comparisons with the same bits and "
                     "inside the spread between runs of the parent itself")
    report = "\n".join(lines)
    print(report)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(report + "\n")


if __name__ == "__main__":
    main()
