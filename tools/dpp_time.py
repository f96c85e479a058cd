#!/usr/bin/env python3
"""Times the greedy DPP re-ranking against its neighbours, in ONE process on one GPU, the legs alternating after a shared warm-up,
device-event timed (nothing is read back inside the timed region), median / min / max of whole calls:

* dpp:   ``ops.dpp_rerank`` at --alpha (Gram matrix, kernel matrix and the k Cholesky steps in one launch);
* mmr:   ``ops.mmr_rerank`` of the same build at lambda 0.5, the same k;
* torch: the lists of the dpp leg in torch ops -- the (B, N, D) gather, the (B, N, N) ``bmm``, the scaling, and a Python loop of k
  steps over a growing (B, t, N) block of Cholesky rows;
* topk:  ``ops.topk_scores`` producing the pool the others re-rank.

With --parent-lib (the shared library of a checkout of the parent commit) ``nrl_mmr_rerank`` and ``nrl_topk_scores`` of that
library are called through ctypes on the same tensors, TWICE each per repeat as two separate legs (parent_a, parent_b), beside
the same entry of this build's library reached through the same ctypes call (mmr_lib, topk_lib).  The three take turns at the
three places of their group.  The repeats come in --rounds rounds; a leg's median over one round is one run of it.  The range of
the parent's 2 * rounds runs is the spread this session shows between runs of the same code, and the median run of the new build's
entry is compared against that range.  Rows and score bits of both entries are compared too.

Shape: --users users, --news table rows around --topics topic centres; a user has a ragged history of 5 ... 50 news drawn from
three topics of its own and its vector is the mean of its history's rows.  D = 300 and 400, N = 64 and 128, k = 10 and 64, cosine,
normalised relevance.  Peak allocated memory of each leg is the allocator's high-water mark above the inputs.  The report also
quotes ``metrics.intra_list_similarity`` of the first ten of the pool, of the ten MMR lists at lambda 0.5 and of the ten DPP lists
at three alpha values, with the mean list score beside each.  Needs a GPU: there is no CPU path to time."""
import argparse
import os
import socket
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.cal_time import median, parent_entries, timed  # noqa: E402


def torch_dpp(pool_idx, pool_score, table, k, alpha):
    """The fast greedy MAP inference in torch ops (every slot live and the pool of full rank: no eligibility test, no fill)."""
    B, N = pool_idx.shape
    rows = table[pool_idx]                                                    # (B, N, D)
    gram = torch.bmm(rows, rows.transpose(1, 2))
    r = torch.diagonal(gram, dim1=1, dim2=2).sqrt().reciprocal()
    sim = gram * (r.unsqueeze(2) * r.unsqueeze(1))
    lo, hi = pool_score.min(1, keepdim=True).values, pool_score.max(1, keepdim=True).values
    q = torch.exp(alpha * ((pool_score - lo) / (hi - lo)))
    L = (q.unsqueeze(2) * q.unsqueeze(1)) * sim
    d2 = torch.diagonal(L, dim1=1, dim2=2).clone()
    cv = torch.zeros(B, k, N, device=pool_idx.device)
    taken = torch.zeros_like(pool_score, dtype=torch.bool)
    users = torch.arange(B, device=pool_idx.device)
    picks = []
    for t in range(k):
        c = d2.masked_fill(taken, float("-inf")).argmax(1)
        picks.append(c)
        taken[users, c] = True
        acc = (cv[:, :t, :] * cv[users, :t, c].unsqueeze(2)).sum(1) if t else 0.0
        e = (L[users, c] - acc) / d2[users, c].sqrt().unsqueeze(1)
        cv[:, t] = e
        d2 = d2 - e * e
    slots = torch.stack(picks, 1)
    return pool_idx.gather(1, slots), pool_score.gather(1, slots)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--users", type=int, default=512)
    ap.add_argument("--news", type=int, default=65536)
    ap.add_argument("--ks", type=int, nargs="+", default=[10, 64])
    ap.add_argument("--alpha", type=float, default=1.0)
    ap.add_argument("--iters", type=int, default=15, help="repeats per round")
    ap.add_argument("--rounds", type=int, default=5, help="rounds: a leg's median over one round is one run of it")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--topics", type=int, default=256, help="topic centres the news vectors are drawn around")
    ap.add_argument("--pools", type=int, nargs="+", default=[64, 128])
    ap.add_argument("--dims", type=int, nargs="+", default=[300, 400])
    ap.add_argument("--alphas", type=float, nargs="+", default=[0.5, 1.0, 3.0])
    ap.add_argument("--parent-lib", default=None, help="shared library of a checkout of the parent commit")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("dpp_time: no GPU; a time measured anywhere else says nothing about this path")
    from newsreclib_amd import _lib, ops
    from newsreclib_amd.metrics import intra_list_similarity
    B, V, alpha, lam = args.users, args.news, args.alpha, 0.5
    lines = [f"dpp_time: B = {B} users, V = {V} news, {args.topics} topics, cosine, normalised relevance; timed legs at alpha {alpha} (dpp, "
             f"torch) and lambda {lam} (mmr); {torch.cuda.get_device_name()} on {socket.gethostname()}; library build id "
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
            pool_idx, pool_score, _ = ops.topk_scores(user, table, N, hist_idx, hist_off)
            for k in args.ks:
                if k > N:
                    continue
                head = [("dpp", lambda: ops.dpp_rerank(pool_idx, pool_score, table, k, alpha))]
                mmr_legs = [("mmr", lambda: ops.mmr_rerank(pool_idx, pool_score, table, k, lam))]
                torch_leg = [("torch", lambda: torch_dpp(pool_idx, pool_score, table, k, alpha))]
                topk_legs = [("topk", lambda: ops.topk_scores(user, table, N))]
                if parent is not None:
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
                        # what ran just before a leg decides what it finds in the caches, so the legs that are compared with each
                        # other sit side by side and take turns at every place of their group
                        a = 1 + it % 3 if parent else 1
                        for name, fn in head + mmr_legs[:1] + mmr_legs[a:] + mmr_legs[1:a] + torch_leg + topk_legs[:1] + topk_legs[a:] + \
                                topk_legs[1:a]:
                            ms, peak, out = timed(fn)
                            times[name].append(ms)
                            peaks[name] = max(peaks.get(name, 0), peak)
                            outs[name] = out
                    for name, _ in legs:
                        runs[name].append(median(times[name][-args.iters:]))
                lines.append(f"D = {D}, N = {N}, k = {k}: gathered pool rows {B * N * D * 4 / 2 ** 20:.1f} MiB, Gram matrices "
                             f"{B * N * N * 4 / 2 ** 20:.1f} MiB, Cholesky rows {B * k * N * 4 / 2 ** 20:.1f} MiB")
                med = {}
                for name, _ in legs:
                    med[name] = median(times[name])
                    lines.append(f"  {name:14s} median {med[name]:8.3f} ms  min {min(times[name]):8.3f}  max {max(times[name]):8.3f}   peak "
                                 f"allocated above the inputs {peaks[name] / 2 ** 20:8.2f} MiB")
                di, ti = outs["dpp"][0], outs["torch"][0]
                lines.append(f"  torch / dpp time: {med['torch'] / med['dpp']:.1f}   dpp / mmr: {med['dpp'] / med['mmr']:.3f}   dpp / topk (the "
                             f"pool): {med['dpp'] / med['topk']:.3f}   status word {int(outs['dpp'][3])}; rows equal to torch's in "
                             f"{int((di == ti).sum())} of {di.numel()} slots, same lists for {int((di == ti).all(1).sum())} of {B} users")
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
            ten = min(10, N)
            lines.append(f"  D = {D}, N = {N}: intra-list similarity of the first {ten} of the pool {intra_list_similarity(pool_idx[:, :ten], table):.4f}"
                         f" (mean list score {float(pool_score[:, :ten].mean()):.4f})")
            idx, score, _, _ = ops.mmr_rerank(pool_idx, pool_score, table, ten, lam)
            lines.append(f"    mmr over {N:3d} at lambda {lam}: {intra_list_similarity(idx, table):.4f} (mean list score {float(score.mean()):.4f})")
            for al in args.alphas:
                idx, score, gain, status = ops.dpp_rerank(pool_idx, pool_score, table, ten, al)
                lines.append(f"    dpp over {N:3d} at alpha {al:4.2f}: {intra_list_similarity(idx, table):.4f} (mean list score "
                             f"{float(score.mean()):.4f}; mean log det L_S / {ten} {float(gain.log().sum(1).mean()) / ten:.4f}; status "
                             f"{int(status)})")
    if parent is not None:
        lines.append(f"mmr_rerank and topk_scores against the parent's library: {sum(inside)} of {len(inside)} comparisons with the same bits and "
                     "inside the spread between runs of the parent itself")
    lines.append("not measured: the kernel's time alone (whole calls only), LDS bank-conflict counters, other shapes")
    report = "\n".join(lines)
    print(report)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(report + "\n")


if __name__ == "__main__":
    main()
