#!/usr/bin/env python3
"""Times several Gumbel top-k draws per walk (``ops.topk_sampled_draws``) against what it replaces, by the protocol of
``tools/topk_sampled_time.py`` (whose helpers it imports): ONE process on one GPU, the legs alternating after a shared warm-up, whole
calls, device events, --rounds rounds of --iters calls; the report gives the median over all calls, each round's median and the
spread between them.

Legs, per D and per number of draws R:
* multi:  ``ops.topk_sampled_draws`` with R draws (the walk with R perturbations and selections per tile, R merges, the raw scores);
* single: R calls of ``ops.topk_sampled_scores`` of the SAME build under seed + r, and whether the two return the same bits;
* torch:  the formulation both replace -- one GEMM ``user @ table.T * inv_temp``, then per draw a (B, V) matrix of Gumbel noise from
  torch's generator, ``-inf`` at the masked positions and ``torch.topk`` -- with its peak memory above the inputs.
The ratio multi / single is reported for every R as measured.
Then the gate on the existing entries, in an alternating run of its own: ``nrl_topk_scores`` and ``nrl_topk_sampled_scores`` of THIS
build's library and of the parent's (--parent-lib), all four through the same bare ctypes path: the same rows and score bits, and a
time ratio to the parent that must lie inside the parent leg's own spread between rounds.

Shape: --users users, --news table rows, D = 300 and 400, k = --k, exclusion lists of 0..50 rows, 2 % of the rows ineligible.
Needs a GPU."""
import argparse
import ctypes
import os
import socket
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from topk_window_time import bits_equal, timed  # noqa: E402


def run_legs(legs, args, lines):
    """Warm-up, then --rounds rounds of --iters alternating calls -> ({leg: median ms}, {leg: spread between the round medians as a
    fraction of the median}, {leg: last output})"""
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
    med, spread = {}, {}
    for name, _ in legs:
        every = sorted(t for r in rounds[name] for t in r)
        per_round = [sorted(r)[len(r) // 2] for r in rounds[name]]
        med[name] = every[len(every) // 2]
        spread[name] = (max(per_round) - min(per_round)) / med[name]
        lines.append(f"    {name:8s} median {med[name]:8.3f} ms of {len(every)} calls (min {every[0]:8.3f}, max {every[-1]:8.3f}); round medians "
                     + " ".join(f"{m:.3f}" for m in per_round) + f", spread {spread[name] * 100:.1f} %; "
                     f"peak above the inputs {peaks[name] / 2 ** 20:8.2f} MiB")
    return med, spread, outs


def bare_entries(path, slices=0):
    """``nrl_topk_scores`` / ``nrl_topk_sampled_scores`` of the library at ``path`` through bare ctypes, as functions of device tensors"""
    from newsreclib_amd import _lib, ops
    lib = ctypes.CDLL(path)
    for name in ("nrl_topk_scores_workspace_bytes", "nrl_topk_scores", "nrl_topk_sampled_scores"):
        getattr(lib, name).restype, getattr(lib, name).argtypes = _lib.SIGNATURES[name]
    lib.nrl_build_id.restype = ctypes.c_char_p

    def outputs(user, table, k):
        B, D, V = user.shape[0], user.shape[1], table.shape[0]
        idx, score, status = ops._topk_outputs(B, k, user.device)
        return B, D, V, idx, score, status, ops.workspace(lib.nrl_topk_scores_workspace_bytes(B, V, D, k, slices), user.device)

    def topk(user, table, k, excl_idx, excl_off, eligible):
        B, D, V, idx, score, status, ws = outputs(user, table, k)
        rc = lib.nrl_topk_scores(user.data_ptr(), table.data_ptr(), B, V, D, k, excl_idx.data_ptr(), excl_off.data_ptr(), eligible.data_ptr(),
                                 slices, idx.data_ptr(), score.data_ptr(), status.data_ptr(), ws.data_ptr(), ws.numel(), ops._stream())
        assert rc == 0, rc
        return idx, score, status

    def sampled(user, table, k, keys, seed, inv_temp, excl_idx, excl_off, eligible):
        B, D, V, idx, key, status, ws = outputs(user, table, k)
        score = torch.empty_like(key)
        rc = lib.nrl_topk_sampled_scores(user.data_ptr(), table.data_ptr(), B, V, D, k, keys.data_ptr(), seed, inv_temp, excl_idx.data_ptr(),
                                         excl_off.data_ptr(), eligible.data_ptr(), slices, idx.data_ptr(), key.data_ptr(), score.data_ptr(),
                                         status.data_ptr(), ws.data_ptr(), ws.numel(), ops._stream())
        assert rc == 0, rc
        return idx, key, score, status

    return topk, sampled, lib.nrl_build_id().decode()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--users", type=int, default=512)
    ap.add_argument("--news", type=int, default=65536)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--draws", type=int, nargs="+", default=[1, 2, 4, 8, 12])
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--inv-temp", type=float, default=1.0)
    ap.add_argument("--dims", type=int, nargs="+", default=[300, 400])
    ap.add_argument("--slices", type=int, default=0, help="pieces of the table walked in parallel per user tile (0: the library's plan)")
    ap.add_argument("--no-torch", action="store_true", help="leave the torch leg out")
    ap.add_argument("--parent-lib", default=None, help="shared library of a checkout of the parent commit")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("topk_draws_time: no GPU; a time measured anywhere else says nothing about this path")
    from newsreclib_amd import _build, _lib, ops
    own_topk, own_sampled, _ = bare_entries(_build.LIB, args.slices)
    B, V, k, inv_temp = args.users, args.news, args.k, args.inv_temp
    plan = args.slices or "the library's plan"
    lines = [f"topk_draws_time: B = {B} users, V = {V} news, k = {k}, inv_temp = {inv_temp}, exclusion lists of 0..50 rows, 2 % of the "
             f"rows ineligible; {torch.cuda.get_device_name()} on {socket.gethostname()}; library build id "
             f"{_lib.load().nrl_build_id().decode()}; torch {torch.__version__}; warm-up {args.warmup}, {args.rounds} rounds of "
             f"{args.iters} alternating calls, whole calls, device events; slices = {plan}"]
    p_topk = p_sampled = None
    if args.parent_lib and os.path.exists(args.parent_lib):
        p_topk, p_sampled, parent_id = bare_entries(args.parent_lib, args.slices)
        lines.append(f"parent legs: nrl_topk_scores / nrl_topk_sampled_scores of {os.path.basename(args.parent_lib)} with build id "
                     f"{parent_id}, loaded beside this build's library")
    else:
        lines.append("parent legs: NOT measured (no library of the parent commit was given with --parent-lib)")
    gate_ok = True
    for D in args.dims:
        g = torch.Generator().manual_seed(args.seed + D)
        user, table = torch.randn(B, D, generator=g).cuda(), torch.randn(V, D, generator=g).cuda()
        elig = (torch.rand(V, generator=g) > 0.02).to(torch.uint8).cuda()
        sizes = torch.randint(0, 51, (B,), generator=g)
        excl_idx = torch.randint(0, V, (int(sizes.sum()),), generator=g).cuda()
        excl_off = torch.cat([torch.zeros(1, dtype=torch.int64), sizes.cumsum(0)]).cuda()
        excl_user = torch.repeat_interleave(torch.arange(B), sizes).cuda()
        keys = (torch.arange(B) + 1).cuda()
        gen = torch.Generator(device="cuda").manual_seed(args.seed)
        lines.append(f"D = {D}: score matrix {B * V * 4 / 2 ** 20:.1f} MiB, {2.0 * B * V * D / 1e9:.1f} GFLOP")
        for R in args.draws:
            if not 1 <= R <= ops.TOPK_MAX_DRAWS or R * k > ops.TOPK_MAX_K:
                lines.append(f"   R = {R}: outside the entry's limits at k = {k}, not measured")
                continue

            def multi():
                return ops.topk_sampled_draws(user, table, k, R, keys, args.seed, inv_temp, excl_idx, excl_off, elig, args.slices)

            def single():
                return [ops.topk_sampled_scores(user, table, k, keys, (args.seed + r) % 2 ** 64, inv_temp, excl_idx, excl_off, elig, args.slices)
                        for r in range(R)]

            def torch_draws():
                s = user @ table.T * inv_temp
                out = []
                for _ in range(R):
                    z = s - torch.log(-torch.log(torch.rand(B, V, device="cuda", generator=gen).clamp_(2.0 ** -24, 1 - 2.0 ** -24)))
                    z.masked_fill_(~elig.bool()[None, :], float("-inf"))
                    z[excl_user, excl_idx] = float("-inf")
                    out.append(torch.topk(z, k, dim=1))
                return out

            legs = [("multi", multi), ("single", single)] + ([] if args.no_torch else [("torch", torch_draws)])
            lines.append(f"   R = {R} draws:")
            med, _, outs = run_legs(legs, args, lines)
            stacked = tuple(torch.stack([o[i] for o in outs["single"]], dim=1) for i in range(3))
            word = 0
            for o in outs["single"]:
                word |= int(o[3])
            line = (f"    multi / single {med['multi'] / med['single']:.3f}   per draw: multi {med['multi'] / R:.3f} ms, single "
                    f"{med['single'] / R:.3f} ms   (the same rows, keys, score bits and status word: "
                    f"{bits_equal(outs['multi'][:3], stacked) and int(outs['multi'][3]) == word})")
            if not args.no_torch:
                line += f"   multi / torch {med['multi'] / med['torch']:.3f}"
            lines.append(line)

        legs = [("plain", lambda: own_topk(user, table, k, excl_idx, excl_off, elig)),
                ("sampled", lambda: own_sampled(user, table, k, keys, args.seed, inv_temp, excl_idx, excl_off, elig))]
        if p_topk is not None:
            legs[1:1] = [("parent", lambda: p_topk(user, table, k, excl_idx, excl_off, elig))]
            legs.append(("parents", lambda: p_sampled(user, table, k, keys, args.seed, inv_temp, excl_idx, excl_off, elig)))
        lines.append("   gate, this build and the parent through bare ctypes: plain / parent the plain top-k, sampled / parents the "
                     "single-draw Gumbel top-k:")
        med, spread, outs = run_legs(legs, args, lines)
        if p_topk is not None:
            for own, par, n in (("plain", "parent", 2), ("sampled", "parents", 3)):
                ratio, same = med[own] / med[par], bits_equal(outs[own][:n], outs[par][:n])
                inside = abs(ratio - 1.0) <= spread[par]
                gate_ok = gate_ok and same and inside
                lines.append(f"    {own} / {par} {ratio:.3f}   (the same rows and score bits: {same}; the parent's spread between rounds "
                             f"{spread[par] * 100:.1f} %: the ratio is {'inside' if inside else 'OUTSIDE'} it)")
        del user, table, elig, excl_idx
    if p_topk is not None:
        lines.append(f"gate: {'passed' if gate_ok else 'FAILED'}")
    report = "\n".join(lines)
    print(report)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(report + "\n")


if __name__ == "__main__":
    main()
