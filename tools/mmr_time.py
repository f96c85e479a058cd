#!/usr/bin/env python3
"""Times the greedy MMR re-ranking against its neighbours, in ONE process on one GPU, the legs alternating (A, B, C, A, ...) after a
shared warm-up, device-event timed (nothing is read back inside the timed region), median / min / max of --iters whole calls:

* mmr:    ``ops.mmr_rerank`` (``nrl_mmr_rerank``: Gram matrix of the pool by the top-k unit's MFMA tile, greedy loop in one launch);
* torch:  the same result in torch ops -- the (B, N, D) gather, the (B, N, N) ``bmm``, the scaling, a Python loop of k steps;
* pool:   ``ops.topk_scores(k = N)`` alone: what producing the pool costs, so the cost of diversifying reads as a fraction of it;
* parent: ``nrl_topk_scores`` of another build of the library (--parent-lib: the shared library of a checkout of the parent
  commit), called through ctypes on the same tensors as the pool leg, the two swapping places every repeat (the one that runs second finds
  the table in the last-level cache); without --parent-lib the report says it was not measured.

Shape: --users users, --news table rows (standard-normal topic centre + standard-normal noise, scaled to unit variance), D = 300
and 400, N = 64 and 128, k = --k, cosine, normalised relevance, lambda 0.5 for
the timed legs.  Peak allocated memory of each leg is the allocator's high-water mark above the inputs.  The report also quotes
``metrics.intra_list_similarity`` and the mean list score of the first k of the pool and of the re-ranked list at lambda 0.5 and
0.7, and how many of the mmr leg's rows the torch leg returns as well (the torch ``bmm`` rounds differently, so near-ties may go
the other way).  Needs a GPU: there is no CPU path to time."""
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


def parent_topk(path):
    """``nrl_topk_scores`` of the library at ``path`` as a function of ``ops.topk_scores``' first three arguments"""
    from newsreclib_amd import _lib, ops
    lib = ctypes.CDLL(path)
    for name in ("nrl_topk_scores_workspace_bytes", "nrl_topk_scores"):
        getattr(lib, name).restype, getattr(lib, name).argtypes = _lib.SIGNATURES[name]
    lib.nrl_build_id.restype = ctypes.c_char_p

    def call(user, table, k):
        B, D, V = user.shape[0], user.shape[1], table.shape[0]
        idx, score, status = ops._topk_outputs(B, k, user.device)
        ws = ops.workspace(lib.nrl_topk_scores_workspace_bytes(B, V, D, k, 0), user.device)
        rc = lib.nrl_topk_scores(user.data_ptr(), table.data_ptr(), B, V, D, k, None, None, None, 0, idx.data_ptr(), score.data_ptr(),
                                 status.data_ptr(), ws.data_ptr(), ws.numel(), ops._stream())
        assert rc == 0, rc
        return idx, score, status

    return call, lib.nrl_build_id().decode()


def torch_mmr(pool_idx, pool_score, table, k, lam):
    """The definition in torch ops (every slot live: the pool of ``topk_scores`` over a table larger than N has no empty slot)."""
    B, N = pool_idx.shape
    rows = table[pool_idx]                                                    # (B, N, D)
    gram = torch.bmm(rows, rows.transpose(1, 2))
    r = torch.diagonal(gram, dim1=1, dim2=2).sqrt().reciprocal()
    sim = gram * (r.unsqueeze(2) * r.unsqueeze(1))
    lo, hi = pool_score.min(1, keepdim=True).values, pool_score.max(1, keepdim=True).values
    rel = lam * ((pool_score - lo) / (hi - lo))
    pen = torch.zeros_like(pool_score)
    taken = torch.zeros_like(pool_score, dtype=torch.bool)
    users = torch.arange(B, device=pool_idx.device)
    picks = []
    for t in range(k):
        obj = (rel - (1.0 - lam) * pen).masked_fill(taken, float("-inf"))
        c = obj.argmax(1)
        picks.append(c)
        taken[users, c] = True
        row = sim[users, c]
        pen = row if t == 0 else torch.maximum(pen, row)
    slots = torch.stack(picks, 1)
    return pool_idx.gather(1, slots), pool_score.gather(1, slots)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--users", type=int, default=512)
    ap.add_argument("--news", type=int, default=65536)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--iters", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--topics", type=int, default=256, help="topic centres the news vectors are drawn around")
    ap.add_argument("--pools", type=int, nargs="+", default=[64, 128])
    ap.add_argument("--dims", type=int, nargs="+", default=[300, 400])
    ap.add_argument("--parent-lib", default=None, help="shared library of a checkout of the parent commit")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("mmr_time: no GPU; a time measured anywhere else says nothing about this path")
    from newsreclib_amd import _lib, ops
    from newsreclib_amd.metrics import intra_list_similarity
    B, V, k = args.users, args.news, args.k
    lines = [f"mmr_time: B = {B} users, V = {V} news, k = {k}, {args.topics} topics, cosine, normalised relevance, lambda 0.5 in the timed legs; "
             f"{torch.cuda.get_device_name()} on {socket.gethostname()}; library build id {_lib.load().nrl_build_id().decode()}; torch "
             f"{torch.__version__}; warm-up {args.warmup}, {args.iters} alternating repeats of whole calls, device events"]
    parent = None
    if args.parent_lib and os.path.exists(args.parent_lib):
        parent, parent_id = parent_topk(args.parent_lib)
        lines.append(f"parent leg: nrl_topk_scores of {os.path.basename(args.parent_lib)} with build id {parent_id}, loaded beside this "
                     "build's library")
    else:
        lines.append("parent leg: NOT measured (no library of the parent commit was given with --parent-lib)")
    for D in args.dims:
        for N in args.pools:
            g = torch.Generator().manual_seed(args.seed + D + N)
            # news around --topics topic centres (half the variance each), so that similar news exist for MMR to tell apart
            centres = torch.randn(args.topics, D, generator=g)
            table = ((centres[torch.randint(0, args.topics, (V,), generator=g)] + torch.randn(V, D, generator=g)) * 0.5 ** 0.5).cuda()
            user = torch.randn(B, D, generator=g).cuda()
            pool_idx, pool_score, _ = ops.topk_scores(user, table, N)
            legs = [("mmr", lambda: ops.mmr_rerank(pool_idx, pool_score, table, k, 0.5)),
                    ("torch", lambda: torch_mmr(pool_idx, pool_score, table, k, 0.5)),
                    ("pool", lambda: ops.topk_scores(user, table, N))]
            if parent is not None:
                legs.append(("parent", lambda: parent(user, table, N)))
            for _ in range(args.warmup):
                for _, fn in legs:
                    fn()
            times, peaks, outs = {n: [] for n, _ in legs}, {}, {}
            for it in range(args.iters):
                # the pool and parent legs swap places every repeat: whichever runs second finds the table in the last-level cache
                order = legs if it % 2 == 0 or parent is None else legs[:2] + [legs[3], legs[2]]
                for name, fn in order:
                    ms, peak, out = timed(fn)
                    times[name].append(ms)
                    peaks[name] = max(peaks.get(name, 0), peak)
                    outs[name] = out
            lines.append(f"D = {D}, N = {N}: gathered pool rows {B * N * D * 4 / 2 ** 20:.1f} MiB, Gram matrices {B * N * N * 4 / 2 ** 20:.1f} "
                         f"MiB, {2.0 * B * N * N * D / 1e9:.2f} GFLOP of Gram products against {2.0 * B * V * D / 1e9:.1f} GFLOP of the pool")
            med = {}
            for name, _ in legs:
                t = sorted(times[name])
                med[name] = t[len(t) // 2]
                lines.append(f"  {name:6s} median {med[name]:8.3f} ms  min {t[0]:8.3f}  max {t[-1]:8.3f}   peak allocated above the inputs "
                             f"{peaks[name] / 2 ** 20:8.2f} MiB")
            faster = "mmr" if med["mmr"] < med["torch"] else "torch"
            ratios = f"  mmr / torch time: {med['mmr'] / med['torch']:.3f} (the faster leg: {faster})   mmr / pool time: " \
                     f"{med['mmr'] / med['pool']:.3f}"
            if parent is not None:
                same = torch.equal(outs["pool"][0], outs["parent"][0]) and \
                    torch.equal(outs["pool"][1].view(torch.int32), outs["parent"][1].view(torch.int32))
                ratios += f"   pool / parent time: {med['pool'] / med['parent']:.3f} (same rows and score bits: {same})"
            lines.append(ratios)
            fi, _, _, status = outs["mmr"]
            ti, _ = outs["torch"]
            lines.append(f"  status word {int(status)}; rows equal to torch's in {int((fi == ti).sum())} of {fi.numel()} slots, same lists for "
                         f"{int((fi == ti).all(1).sum())} of {B} users")
            lines.append(f"  first {k} of the pool:      intra-list similarity {intra_list_similarity(pool_idx[:, :k], table):.4f}   mean list "
                         f"score {float(pool_score[:, :k].mean()):.4f}")
            for lam in (0.7, 0.5):
                idx, score, _, _ = ops.mmr_rerank(pool_idx, pool_score, table, k, lam)
                lines.append(f"  mmr over {N:3d} at lambda {lam}: intra-list similarity {intra_list_similarity(idx, table):.4f}   mean list "
                             f"score {float(score.mean()):.4f}")
    report = "\n".join(lines)
    print(report)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(report + "\n")


if __name__ == "__main__":
    main()
