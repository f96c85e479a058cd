#!/usr/bin/env python3
"""Times the windowed full-catalogue top-k and rank against their neighbours, in ONE process on one GPU, the legs alternating
(A, B, C, D, A, ...) after a shared warm-up, device-event timed (nothing is read back inside the timed region).  Every leg is
timed in --rounds rounds of --iters whole calls; the report gives the median over all calls, the median of each round and the
spread between the rounds' medians.

Legs, for the top-k entry and again for the rank entry:
* window: ``ops.topk_window_scores`` / ``ops.catalogue_window_ranks``;
* plain:  ``ops.topk_scores`` / ``ops.catalogue_ranks`` of the SAME build (no window: what the walk costs without the new code);
* parent: ``nrl_topk_scores`` / ``nrl_catalogue_ranks`` of another build of the library (--parent-lib: the shared library of a
  checkout of the parent commit), called through ctypes on the same tensors, and whether plain and parent return the same bits;
  without --parent-lib the report says the leg was not measured;
* torch:  the windowed result in torch ops -- ``user @ table.T``, the three masks (window, eligible, exclusion lists),
  ``torch.topk`` / a count of the rows above each target.

Shape: --users users, --news table rows, D = 300 and 400, k = --k, exclusion lists of 0..50 rows, 3 targets per user, 2 % of the
rows ineligible.  The time column is in hours over 28 days, non-decreasing (``synthetic.news_times``).  Window sets:
  (a) all-inclusive;  (b) the 24 h before a request time drawn per user from the last 7 days;  (c) the 24 h before one request
  time shared by the batch;  (d) set (b) with the rows, and their times, randomly permuted (no tile can be skipped).
For every set the report gives the share of (workgroup, table tile) pairs whose union window meets an eligible row of the tile,
computed on the host from the inputs (``tile_share``): the part of the walk the skip cannot avoid.  Needs a GPU."""
import argparse
import ctypes
import os
import socket
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

TILE_USERS, TILE_ROWS = 64, 128                             # TK_BU, TK_BV of nrl_topk.hip
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1


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


def tile_share(row_time, eligible, lo, hi):
    """The share of (64-user workgroup, 128-row table tile) pairs the walk cannot skip: the tile holds an eligible row whose time
    is inside [min lo, max hi] over the workgroup's non-empty windows.  Host tensors."""
    V, B = int(row_time.numel()), int(lo.numel())
    pad = (-V) % TILE_ROWS
    t = torch.cat([row_time.long(), torch.zeros(pad, dtype=torch.int64)]).reshape(-1, TILE_ROWS)
    e = torch.cat([eligible.bool(), torch.zeros(pad, dtype=torch.bool)]).reshape(-1, TILE_ROWS)
    hit = total = 0
    for u0 in range(0, B, TILE_USERS):
        l, h = lo[u0:u0 + TILE_USERS].long(), hi[u0:u0 + TILE_USERS].long()
        live = l <= h
        total += t.shape[0]
        if bool(live.any()):
            ulo, uhi = int(l[live].min()), int(h[live].max())
            hit += int((e & (t >= ulo) & (t <= uhi)).any(1).sum())
    return hit / max(total, 1)


def parent_entries(path, slices=0):
    """``nrl_topk_scores`` / ``nrl_catalogue_ranks`` of the library at ``path`` as functions of the ``ops`` wrappers' arguments"""
    from newsreclib_amd import _lib, ops
    lib = ctypes.CDLL(path)
    for name in ("nrl_topk_scores_workspace_bytes", "nrl_topk_scores", "nrl_catalogue_ranks_workspace_size", "nrl_catalogue_ranks"):
        getattr(lib, name).restype, getattr(lib, name).argtypes = _lib.SIGNATURES[name]
    lib.nrl_build_id.restype = ctypes.c_char_p

    def topk(user, table, k, excl_idx, excl_off, eligible):
        B, D, V = user.shape[0], user.shape[1], table.shape[0]
        excl_idx, excl_off, eligible = ops._topk_masks(excl_idx, excl_off, eligible, B, V)      # (the device ops `ops.topk_scores` issues)
        idx, score, status = ops._topk_outputs(B, k, user.device)
        ws = ops.workspace(lib.nrl_topk_scores_workspace_bytes(B, V, D, k, slices), user.device)
        rc = lib.nrl_topk_scores(user.data_ptr(), table.data_ptr(), B, V, D, k, excl_idx.data_ptr(), excl_off.data_ptr(),
                                 eligible.data_ptr(), slices, idx.data_ptr(), score.data_ptr(), status.data_ptr(), ws.data_ptr(), ws.numel(),
                                 ops._stream())
        assert rc == 0, rc
        return idx, score, status

    def ranks(user, table, tgt_idx, tgt_off, excl_idx, excl_off, eligible):
        B, D, V = user.shape[0], user.shape[1], table.shape[0]
        tgt_idx, tgt_off, n = ops._rank_targets(tgt_idx, tgt_off, B)
        excl_idx, excl_off, eligible = ops._topk_masks(excl_idx, excl_off, eligible, B, V)
        rank, score, ranked, status = ops._rank_outputs(n, B, user.device)
        ws = ops.workspace(lib.nrl_catalogue_ranks_workspace_size(B, V, D, n, slices), user.device)
        rc = lib.nrl_catalogue_ranks(user.data_ptr(), table.data_ptr(), B, V, D, tgt_idx.data_ptr(), tgt_off.data_ptr(), n,
                                     excl_idx.data_ptr(), excl_off.data_ptr(), eligible.data_ptr(), slices, rank.data_ptr(), score.data_ptr(),
                                     ranked.data_ptr(), status.data_ptr(), ws.data_ptr(), ws.numel(), ops._stream())
        assert rc == 0, rc
        return rank, score, ranked, status

    return topk, ranks, lib.nrl_build_id().decode()


def bits_equal(a, b):
    return all(torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y)
               for x, y in zip(a, b))


def run_legs(legs, args, lines):
    """Warm-up, then --rounds rounds of --iters alternating calls -> ({leg: median ms}, {leg: last output})"""
    for _ in range(args.warmup):
        for _, fn in legs:
            fn()
    rounds, peaks, outs = {n: [] for n, _ in legs}, {}, {}
    for _ in range(args.rounds):
        times = {n: [] for n, _ in legs}
        for _ in range(args.iters):
            for name, fn in legs:
                ms, peak, out = timed(fn)
                times[name].append(ms)
                peaks[name] = max(peaks.get(name, 0), peak)
                outs[name] = out
        for n, _ in legs:
            rounds[n].append(times[n])
    med = {}
    for name, _ in legs:
        every = sorted(t for r in rounds[name] for t in r)
        per_round = [sorted(r)[len(r) // 2] for r in rounds[name]]
        med[name] = every[len(every) // 2]
        lines.append(f"    {name:7s} median {med[name]:8.3f} ms of {len(every)} calls (min {every[0]:8.3f}, max {every[-1]:8.3f}); round medians "
                     + " ".join(f"{m:.3f}" for m in per_round) + f", spread {(max(per_round) - min(per_round)) / med[name] * 100:.1f} %; "
                     f"peak above the inputs {peaks[name] / 2 ** 20:8.2f} MiB")
    return med, outs


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--users", type=int, default=512)
    ap.add_argument("--news", type=int, default=65536)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--dims", type=int, nargs="+", default=[300, 400])
    ap.add_argument("--sets", nargs="+", default=["a", "b", "c", "d"])
    ap.add_argument("--slices", type=int, default=0, help="pieces of the table walked in parallel per user tile (0: the library's plan)")
    ap.add_argument("--parent-lib", default=None, help="shared library of a checkout of the parent commit")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("topk_window_time: no GPU; a time measured anywhere else says nothing about this path")
    from newsreclib_amd import _lib, ops, synthetic
    B, V, k = args.users, args.news, args.k
    span, last = 28 * 24, 7 * 24
    plan = args.slices or "the library's plan"
    lines = [f"topk_window_time: B = {B} users, V = {V} news, k = {k}, exclusion lists of 0..50 rows, 3 targets a user, time column in "
             f"hours over 28 days; {torch.cuda.get_device_name()} on {socket.gethostname()}; library build id "
             f"{_lib.load().nrl_build_id().decode()}; torch {torch.__version__}; warm-up {args.warmup}, {args.rounds} rounds of "
             f"{args.iters} alternating calls, device events; slices = {plan}"]
    p_topk = p_ranks = None
    if args.parent_lib and os.path.exists(args.parent_lib):
        p_topk, p_ranks, parent_id = parent_entries(args.parent_lib, args.slices)
        lines.append(f"parent legs: nrl_topk_scores / nrl_catalogue_ranks of {os.path.basename(args.parent_lib)} with build id {parent_id}, "
                     "loaded beside this build's library")
    else:
        lines.append("parent legs: NOT measured (no library of the parent commit was given with --parent-lib)")
    for D in args.dims:
        g = torch.Generator().manual_seed(args.seed + D)
        user_h, table_h = torch.randn(B, D, generator=g), torch.randn(V, D, generator=g)
        time_h = synthetic.news_times(V, span, seed=args.seed + 31).to(torch.int32)
        elig_h = (torch.rand(V, generator=g) > 0.02).to(torch.uint8)
        sizes = torch.randint(0, 51, (B,), generator=g)
        excl_h = torch.randint(0, V, (int(sizes.sum()),), generator=g)
        excl_off = torch.cat([torch.zeros(1, dtype=torch.int64), sizes.cumsum(0)]).cuda()
        excl_user = torch.repeat_interleave(torch.arange(B), sizes).cuda()
        tgt_h = torch.randint(0, V, (B * 3,), generator=g)
        tgt_off = (torch.arange(B + 1) * 3).cuda()
        tgt_user = torch.repeat_interleave(torch.arange(B), 3).cuda()
        req = torch.randint(span - last, span, (B,), generator=g)
        perm = torch.randperm(V, generator=g)
        inv = torch.empty_like(perm)
        inv[perm] = torch.arange(V)
        user = user_h.cuda()
        lines.append(f"D = {D}: score matrix {B * V * 4 / 2 ** 20:.1f} MiB, {2.0 * B * V * D / 1e9:.1f} GFLOP")
        for name in args.sets:
            if name == "a":
                lo_h, hi_h = torch.full((B,), INT32_MIN, dtype=torch.int32), torch.full((B,), INT32_MAX, dtype=torch.int32)
            elif name == "c":
                lo_h, hi_h = torch.full((B,), int(req[0]) - 24, dtype=torch.int32), torch.full((B,), int(req[0]), dtype=torch.int32)
            else:
                lo_h, hi_h = (req - 24).to(torch.int32), req.to(torch.int32)
            if name == "d":                                 # row perm[i] of the sorted table becomes row i; every row index follows
                tab_h, rt_h, el_h, ex_h, tg_h = table_h[perm], time_h[perm], elig_h[perm], inv[excl_h], inv[tgt_h]
            else:
                tab_h, rt_h, el_h, ex_h, tg_h = table_h, time_h, elig_h, excl_h, tgt_h
            table, rt, elig, excl_idx, tgt_idx, lo, hi = (x.cuda() for x in (tab_h, rt_h, el_h, ex_h, tg_h, lo_h, hi_h))
            rows = torch.arange(V, device="cuda")
            share = tile_share(rt_h, el_h, lo_h, hi_h)
            inside = ((rt_h.long()[None, :] >= lo_h.long()[:, None]) & (rt_h.long()[None, :] <= hi_h.long()[:, None])).float().mean()
            lines.append(f"  set ({name}): {float(inside) * 100:.2f} % of the (user, row) pairs inside a window; the union window of a "
                         f"workgroup meets {share * 100:.2f} % of the (workgroup, table tile) pairs")

            def masked_scores():
                s = user @ table.T
                ok = (rt[None, :] >= lo[:, None]) & (rt[None, :] <= hi[:, None]) & elig.bool()[None, :]
                s.masked_fill_(~ok, float("-inf"))
                s[excl_user, excl_idx] = float("-inf")
                return s

            def torch_topk():
                score, idx = torch.topk(masked_scores(), k, dim=1)
                return idx, score

            def torch_ranks():
                s = masked_scores()
                ts = s[tgt_user, tgt_idx]
                mine = s[tgt_user]
                above = (mine > ts[:, None]) | ((mine == ts[:, None]) & (rows[None, :] < tgt_idx[:, None]))
                rank = torch.where(ts > float("-inf"), 1 + above.sum(1), torch.zeros_like(tgt_idx))
                return rank.int(), ts, (s > float("-inf")).sum(1).int()

            legs = [("window", lambda: ops.topk_window_scores(user, table, k, rt, lo, hi, excl_idx, excl_off, elig, args.slices)),
                    ("plain", lambda: ops.topk_scores(user, table, k, excl_idx, excl_off, elig, args.slices))]
            if p_topk is not None:
                legs.append(("parent", lambda: p_topk(user, table, k, excl_idx, excl_off, elig)))
            legs.append(("torch", torch_topk))
            lines.append("   top-k:")
            med, outs = run_legs(legs, args, lines)
            line = f"    window / plain {med['window'] / med['plain']:.3f}   window / torch {med['window'] / med['torch']:.3f}"
            if p_topk is not None:
                line += (f"   plain / parent {med['plain'] / med['parent']:.3f}   (plain and parent return the same rows and score bits: "
                         f"{bits_equal(outs['plain'][:2], outs['parent'][:2])})")
            lines.append(line)
            (wi, wsc, wst), (ti, _) = outs["window"], outs["torch"]
            ti = torch.where(outs["torch"][1] > float("-inf"), ti, torch.full_like(ti, -1))
            lines.append(f"    status word {int(wst)}; rows equal to torch's in {int((wi == ti).sum())} of {wi.numel()} slots; "
                         f"{int((wi >= 0).sum())} slots filled")

            legs = [("window", lambda: ops.catalogue_window_ranks(user, table, tgt_idx, tgt_off, rt, lo, hi, excl_idx, excl_off, elig,
                                                                 args.slices)),
                    ("plain", lambda: ops.catalogue_ranks(user, table, tgt_idx, tgt_off, excl_idx, excl_off, elig, args.slices))]
            if p_ranks is not None:
                legs.append(("parent", lambda: p_ranks(user, table, tgt_idx, tgt_off, excl_idx, excl_off, elig)))
            legs.append(("torch", torch_ranks))
            lines.append("   rank:")
            med, outs = run_legs(legs, args, lines)
            line = f"    window / plain {med['window'] / med['plain']:.3f}   window / torch {med['window'] / med['torch']:.3f}"
            if p_ranks is not None:
                line += (f"   plain / parent {med['plain'] / med['parent']:.3f}   (plain and parent return the same ranks, score bits and "
                         f"populations: {bits_equal(outs['plain'][:3], outs['parent'][:3])})")
            lines.append(line)
            wr, _, wn, wst = outs["window"]
            tr, _, tn = outs["torch"]
            lines.append(f"    status word {int(wst)}; ranks equal to torch's for {int((wr == tr).sum())} of {wr.numel()} targets "
                         f"({int((wr > 0).sum())} inside their window), populations for {int((wn == tn).sum())} of {B} users")
            del table, rt, elig, excl_idx, tgt_idx, lo, hi
    report = "\n".join(lines)
    print(report)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(report + "\n")


if __name__ == "__main__":
    main()
