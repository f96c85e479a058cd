#!/usr/bin/env python3
"""Times the full-catalogue rank of held-out clicks under the MINER, DKN and NPA scorers two ways, in ONE process on one GPU, the
two sides alternating (A, B, A, B, ...) after a shared warm-up, device-event timed (nothing is read back inside the timed region),
median / min / max of --iters:

* fused: ``ops.catalogue_interest_ranks`` / ``ops.catalogue_relu_ranks`` / ``ops.catalogue_pooled_ranks`` (no (B, V) matrix);
* torch: the same ranks in torch ops, in pieces of --chunk table rows because the intermediates -- (B, K, V), (B, V, Hd),
  (B, V, L) -- do not fit at once: the clicks' scores from the gathered rows first, then per piece the scores, ``-inf`` at the
  excluded positions, and per click ``(s > s_t) | (s == s_t & row < t)`` summed over the user's row (the click's own column
  left out: the piece rounds it differently from the gathered computation).

Shapes: --users users, --news table rows, 1..5 clicks per user, ragged exclusion lists of 0..50 rows per user; MINER K = 32,
D = 256, modes max / mean / weighted; DKN Hd = 16 and 64; NPA L = 30, F = 400 (the shapes ``tools/topk_interests_time.py``,
``tools/topk_dnn_time.py`` and ``tools/topk_npa_time.py`` time).  Peak allocated memory of each side is the allocator's
high-water mark above the inputs.  The two results are compared (torch rounds differently, so a rank may move where scores are
within rounding of each other; the report counts them).  Needs a GPU: there is no CPU path to time."""
import argparse
import os
import socket
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

NEG_INF = float("-inf")


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


def lists(B, V, seed):
    """Exclusion lists and clicks on the device, with the piece-wise view of the exclusions the torch side uses."""
    g = torch.Generator().manual_seed(seed)
    sizes = torch.randint(0, 51, (B,), generator=g)
    excl = torch.randint(0, V, (int(sizes.sum()),), generator=g)
    excl_user = torch.repeat_interleave(torch.arange(B), sizes)
    clicks = torch.randint(1, 6, (B,), generator=g)
    tgt = torch.randint(0, V, (int(clicks.sum()),), generator=g)
    off = lambda n: torch.cat([torch.zeros(1, dtype=torch.int64), n.cumsum(0)]).cuda()  # noqa: E731
    return dict(excl_idx=excl.cuda(), excl_off=off(sizes), excl_host=excl, excl_user_host=excl_user, tgt_idx=tgt.cuda(),
                tgt_off=off(clicks), tgt_user=torch.repeat_interleave(torch.arange(B), clicks).cuda(), n_clicks=int(clicks.sum()))


def torch_ranks(ls, V, chunk, target_scores, piece_scores):
    """The torch side: ``target_scores()`` -> (n_clicks), ``piece_scores(lo, hi)`` -> (B, hi - lo)."""
    st = target_scores()
    tgt_idx, tgt_user = ls["tgt_idx"], ls["tgt_user"]
    above = torch.zeros_like(tgt_idx)
    pop = None
    hit = torch.zeros_like(tgt_idx, dtype=torch.bool)             # the click is on its user's exclusion list
    for lo, hi, eu, ec in ls["pieces"]:
        s = piece_scores(lo, hi)
        s[eu, ec] = NEG_INF
        own = s[tgt_user]                                         # (n_clicks, Vp): every click against its user's row
        rows = torch.arange(lo, hi, device=s.device)
        mine = rows[None, :] == tgt_idx[:, None]
        hit |= (mine & (own == NEG_INF)).any(1)
        above += (((own > st[:, None]) | ((own == st[:, None]) & (rows[None, :] < tgt_idx[:, None]))) & ~mine).sum(1)
        n = (s > NEG_INF).sum(1)
        pop = n if pop is None else pop + n
    return torch.where(hit, torch.zeros_like(above), 1 + above).int(), torch.where(hit, torch.full_like(st, NEG_INF), st), pop.int()


def run(name, note, sides, ls, B, args, lines):
    for _ in range(args.warmup):
        for _, fn in sides:
            fn()
    times, peaks, outs = {n: [] for n, _ in sides}, {}, {}
    for _ in range(args.iters):
        for side, fn in sides:
            ms, peak, out = timed(fn)
            times[side].append(ms)
            peaks[side] = max(peaks.get(side, 0), peak)
            outs[side] = out
    lines.append(f"{name}: {note}")
    med = {}
    for side, _ in sides:
        t = sorted(times[side])
        med[side] = t[len(t) // 2]
        lines.append(f"  {side:6s} median {med[side]:9.3f} ms  min {t[0]:9.3f}  max {t[-1]:9.3f}   peak allocated above the inputs "
                     f"{peaks[side] / 2 ** 20:9.2f} MiB")
    fr, fs, fn_, status = outs["fused"]
    tr, ts, tn = outs["torch"]
    valid = (fr > 0) & (tr > 0)
    lines.append(f"  fused / torch time: {med['fused'] / med['torch']:.3f}   fused / torch peak memory: "
                 f"{peaks['fused'] / max(peaks['torch'], 1):.5f}")
    lines.append(f"  status word {int(status)}; {ls['n_clicks']} clicks, ranks equal for {int((fr == tr).sum())}, largest rank difference "
                 f"{int((fr - tr).abs().max())}, populations equal for {int((fn_ == tn).sum())} of {B} users, largest score difference "
                 f"{float((fs[valid] - ts[valid]).abs().max()):.3e}")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--users", type=int, default=512)
    ap.add_argument("--news", type=int, default=65536)
    ap.add_argument("--families", default="miner,dkn,npa")
    ap.add_argument("--chunk", type=int, default=4096, help="table rows per piece of the torch side")
    ap.add_argument("--iters", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("catalogue_rank_scorers_time: no GPU; a time measured anywhere else says nothing about this path")
    from newsreclib_amd import _lib, ops
    B, V = args.users, args.news
    families = args.families.split(",")
    lines = [f"catalogue_rank_scorers_time: B = {B} users, V = {V} news, 1..5 clicks per user, exclusion lists of 0..50 rows; "
             f"{torch.cuda.get_device_name()} on {socket.gethostname()}; library build id {_lib.load().nrl_build_id().decode()}; "
             f"torch {torch.__version__}; warm-up {args.warmup}, {args.iters} alternating repeats, device events, whole calls; torch in "
             f"pieces of {args.chunk} rows"]
    ls = lists(B, V, args.seed)
    ls["pieces"] = []
    for lo in range(0, V, args.chunk):
        hi = min(lo + args.chunk, V)
        inside = (ls["excl_host"] >= lo) & (ls["excl_host"] < hi)
        ls["pieces"].append((lo, hi, ls["excl_user_host"][inside].cuda(), (ls["excl_host"][inside] - lo).cuda()))
    tgt_idx, tgt_off, tgt_user, excl_idx, excl_off = ls["tgt_idx"], ls["tgt_off"], ls["tgt_user"], ls["excl_idx"], ls["excl_off"]
    g = torch.Generator(device="cuda").manual_seed(args.seed)
    rn = lambda *s: torch.randn(*s, generator=g, device="cuda")  # noqa: E731

    if "miner" in families:
        K, D = 32, 256
        E, G, T = rn(B, K, D), rn(B, K, D), rn(V, D)

        def aggregate(s, lg, mode):                               # over dim 1
            if mode == "max":
                return s.max(dim=1)[0]
            if mode == "mean":
                return s.sum(dim=1) / K
            return (torch.softmax(lg, dim=1) * s).sum(dim=1)

        for mode in ("max", "mean", "weighted"):
            def fused(mode=mode):
                return ops.catalogue_interest_ranks(E, T, tgt_idx, tgt_off, mode, G if mode == "weighted" else None, excl_idx, excl_off)

            def targets(mode=mode):
                rows = T[tgt_idx]
                s = torch.einsum("nkd,nd->nk", E[tgt_user], rows)
                return aggregate(s, torch.einsum("nkd,nd->nk", G[tgt_user], rows) if mode == "weighted" else None, mode)

            def piece(lo, hi, mode=mode):
                s = torch.einsum("bkd,vd->bkv", E, T[lo:hi])
                return aggregate(s, torch.einsum("bkd,vd->bkv", G, T[lo:hi]) if mode == "weighted" else None, mode).contiguous()

            run(f"MINER {mode}", f"K = {K}, D = {D}; (B, K, V) fp32 would be {B * K * V * 4 / 2 ** 30:.2f} GiB",
                [("fused", fused), ("torch", lambda: torch_ranks(ls, V, args.chunk, targets, piece))], ls, B, args, lines)

    if "dkn" in families:
        for Hd in (16, 64):
            q, proj, w2, b2 = rn(B, Hd), rn(V, Hd), rn(Hd) / Hd ** 0.5, 0.1 * rn(1)

            def fused(q=q, proj=proj, w2=w2, b2=b2):
                return ops.catalogue_relu_ranks(q, proj, w2, b2, tgt_idx, tgt_off, excl_idx, excl_off)

            def targets(q=q, proj=proj, w2=w2, b2=b2):
                return torch.relu(proj[tgt_idx] + q[tgt_user]) @ w2 + b2

            def piece(lo, hi, q=q, proj=proj, w2=w2, b2=b2):
                return torch.relu(proj[None, lo:hi, :] + q[:, None, :]) @ w2 + b2

            run(f"DKN Hd = {Hd}", f"(B, V, Hd) fp32 would be {B * V * Hd * 4 / 2 ** 30:.2f} GiB",
                [("fused", fused), ("torch", lambda: torch_ranks(ls, V, args.chunk, targets, piece))], ls, B, args, lines)

    if "npa" in families:
        L, F = 30, 400
        feat = torch.relu(rn(V, L, F))
        q, user = torch.tanh(0.25 * rn(B, F)), rn(B, F) / F ** 0.5
        qT, uT = q.T.contiguous(), user.T.contiguous()

        def fused():
            return ops.catalogue_pooled_ranks(q, user, feat, tgt_idx, tgt_off, excl_idx, excl_off)

        def targets():
            c = feat[tgt_idx]                                     # (n_clicks, L, F)
            w = torch.softmax(torch.einsum("nlf,nf->nl", c, q[tgt_user]), dim=1)
            return (w * torch.einsum("nlf,nf->nl", c, user[tgt_user])).sum(dim=1)

        def piece(lo, hi):
            c = feat[lo:hi]
            w = torch.softmax(c @ qT, dim=1)                      # (Vp, L, B)
            return (w * (c @ uT)).sum(dim=1).T.contiguous()

        run("NPA", f"L = {L}, F = {F}; feature maps {V * L * F * 4 / 2 ** 30:.2f} GiB, (B, V, L) fp32 would be "
            f"{B * V * L * 4 / 2 ** 30:.2f} GiB", [("fused", fused), ("torch", lambda: torch_ranks(ls, V, args.chunk, targets, piece))],
            ls, B, args, lines)

    report = "\n".join(lines)
    print(report)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(report + "\n")


if __name__ == "__main__":
    main()
