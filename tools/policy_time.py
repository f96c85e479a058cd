#!/usr/bin/env python3
"""Times the policy entries (``ops.catalogue_logz`` / ``ops.list_logprob``) against their neighbours, by the protocol of
``tools/topk_window_time.py`` (whose timing helpers it imports): ONE process on one GPU, the legs alternating after a shared
warm-up, whole calls, device events, --rounds rounds of --iters calls; the report gives the median over all calls, each round's
median and the spread between them.

Legs:
* logz:    ``ops.catalogue_logz`` (the summing walk over the statistics chunks and its finish);
* logprob: ``ops.list_logprob`` of lists ``ops.topk_sampled_scores`` drew (the summing walk with the lists dropped, the raw scores
  of the listed rows, the list kernel);
* plain:   ``ops.topk_scores`` of the SAME build: what a walk of the table costs under the selecting consumer;
* parent:  ``nrl_topk_scores`` of another build of the library (--parent-lib: the shared library of a checkout of the parent
  commit) through bare ctypes on the same tensors, and whether plain and parent return the same bits;
* torch_z / torch_lp: the formulation the entries replace -- ``user @ table.T * inv_temp``, ``-inf`` at the masked positions,
  ``torch.logsumexp`` and the entropy from the softmax; and, for the lists, the tail form over that matrix (the listed rows set
  to ``-inf``, ``logsumexp`` of the rest, ``logcumsumexp`` backwards over the listed scores) -- with their peak memory above the
  inputs.
Then the gate on the existing entry, in an alternating run of its own: ``nrl_topk_scores`` of THIS build's library and of the
parent's, both through the same bare ctypes path, bits and times.

Shape: --users users, --news table rows, D = 300 and 400, k = --k, exclusion lists of 0..50 rows, 2 % of the rows ineligible.
Needs a GPU."""
import argparse
import os
import socket
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from topk_window_time import bits_equal, parent_entries, run_legs  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--users", type=int, default=512)
    ap.add_argument("--news", type=int, default=65536)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--inv-temp", type=float, default=0.25)
    ap.add_argument("--dims", type=int, nargs="+", default=[300, 400])
    ap.add_argument("--parent-lib", default=None, help="shared library of a checkout of the parent commit")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("policy_time: no GPU; a time measured anywhere else says nothing about this path")
    from newsreclib_amd import _build, _lib, ops
    own_topk, _, _ = parent_entries(_build.LIB)
    B, V, k, inv_temp = args.users, args.news, args.k, args.inv_temp
    lines = [f"policy_time: B = {B} users, V = {V} news, k = {k}, inv_temp = {inv_temp}, exclusion lists of 0..50 rows, 2 % of the rows "
             f"ineligible; {torch.cuda.get_device_name()} on {socket.gethostname()}; library build id "
             f"{_lib.load().nrl_build_id().decode()}; torch {torch.__version__}; warm-up {args.warmup}, {args.rounds} rounds of "
             f"{args.iters} alternating calls, whole calls, device events"]
    p_topk = None
    if args.parent_lib and os.path.exists(args.parent_lib):
        p_topk, _, parent_id = parent_entries(args.parent_lib)
        lines.append(f"parent legs: nrl_topk_scores of {os.path.basename(args.parent_lib)} with build id {parent_id}, loaded beside this "
                     "build's library")
    else:
        lines.append("parent legs: NOT measured (no library of the parent commit was given with --parent-lib)")
    for D in args.dims:
        g = torch.Generator().manual_seed(args.seed + D)
        user, table = torch.randn(B, D, generator=g).cuda(), torch.randn(V, D, generator=g).cuda()
        elig = (torch.rand(V, generator=g) > 0.02).to(torch.uint8).cuda()
        sizes = torch.randint(0, 51, (B,), generator=g)
        excl_idx = torch.randint(0, V, (int(sizes.sum()),), generator=g).cuda()
        excl_off = torch.cat([torch.zeros(1, dtype=torch.int64), sizes.cumsum(0)]).cuda()
        excl_user = torch.repeat_interleave(torch.arange(B), sizes).cuda()
        keys = (torch.arange(B) + 1).cuda()
        lists = ops.topk_sampled_scores(user, table, k, keys, args.seed, inv_temp, excl_idx, excl_off, elig)[0]
        rows = torch.arange(B, device="cuda")[:, None].expand(B, k)
        lines.append(f"D = {D}: score matrix {B * V * 4 / 2 ** 20:.1f} MiB, {2.0 * B * V * D / 1e9:.1f} GFLOP")

        def masked():
            t = user @ table.T * inv_temp
            t.masked_fill_(~elig.bool()[None, :], float("-inf"))
            t[excl_user, excl_idx] = float("-inf")
            return t

        def torch_z():
            t = masked()
            lz = torch.logsumexp(t, dim=1)
            p = torch.softmax(t, dim=1)
            ent = -(p * torch.where(p > 0, t - lz[:, None], torch.zeros_like(t))).sum(1)
            return t.max(1)[0], lz, ent

        def torch_lp():
            t = masked()
            a = t.gather(1, lists)
            t[rows, lists] = float("-inf")
            tail = torch.logsumexp(t, dim=1)
            back = torch.logcumsumexp(torch.cat([tail[:, None], a.flip(1)], dim=1), dim=1)[:, 1:].flip(1)
            return a - back

        legs = [("logz", lambda: ops.catalogue_logz(user, table, inv_temp, excl_idx, excl_off, elig)),
                ("logprob", lambda: ops.list_logprob(user, table, lists, inv_temp, excl_idx, excl_off, elig)),
                ("plain", lambda: ops.topk_scores(user, table, k, excl_idx, excl_off, elig))]
        if p_topk is not None:
            legs.append(("parent", lambda: p_topk(user, table, k, excl_idx, excl_off, elig)))
        legs += [("torch_z", torch_z), ("torch_lp", torch_lp)]
        lines.append("   the policy entries:")
        med, outs = run_legs(legs, args, lines)
        line = (f"    logz / plain {med['logz'] / med['plain']:.3f}   logz / torch_z {med['logz'] / med['torch_z']:.3f}   "
                f"logprob / torch_lp {med['logprob'] / med['torch_lp']:.3f}")
        if p_topk is not None:
            line += (f"   plain / parent {med['plain'] / med['parent']:.3f}   (plain and parent return the same rows and score bits: "
                     f"{bits_equal(outs['plain'][:2], outs['parent'][:2])})")
        lines.append(line)
        mx, ls, ent, pop, _, st = outs["logz"]
        tm, tz, te = outs["torch_z"]
        lp, total, _, lst = outs["logprob"]
        lines.append(f"    status words {int(st)} / {int(lst)}; population {int(pop.min())}..{int(pop.max())}; max |log Z - torch's| = "
                     f"{float(((mx.double() + ls.double()) - tz.double()).abs().max()):.3e} (torch: fp32 scores of its own GEMM), max |entropy - "
                     f"torch's| = {float((ent - te).abs().max()):.3e}, max |logp - torch's| = {float((lp - outs['torch_lp']).abs().max()):.3e}; "
                     f"mean entropy {float(ent.mean()):.3f} nats, mean list log-probability {float(total.mean()):.3f}")

        legs = [("plain", lambda: own_topk(user, table, k, excl_idx, excl_off, elig))]
        if p_topk is not None:
            legs.append(("parent", lambda: p_topk(user, table, k, excl_idx, excl_off, elig)))
            lines.append("   gate, this build and the parent through bare ctypes (the plain top-k):")
            med, outs = run_legs(legs, args, lines)
            lines.append(f"    plain / parent {med['plain'] / med['parent']:.3f}   (the same rows and score bits: "
                         f"{bits_equal(outs['plain'][:2], outs['parent'][:2])})")
        del user, table, elig, excl_idx, lists
    lines.append("not measured: kernel time alone (these are whole calls), hardware counters, other shapes, other inv_temp")
    report = "\n".join(lines)
    print(report)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(report + "\n")


if __name__ == "__main__":
    main()
