#!/usr/bin/env python3
"""Times Gumbel top-k (``ops.topk_sampled_scores``) against its neighbours, by the protocol of ``tools/topk_window_time.py`` (whose
timing helpers it imports): ONE process on one GPU, the legs alternating after a shared warm-up, whole calls, device events,
--rounds rounds of --iters calls; the report gives the median over all calls, each round's median and the spread between them.

Legs:
* sampled: ``ops.topk_sampled_scores`` (the walk with the perturbation, the merge, the raw scores of the selected rows);
* plain:   ``ops.topk_scores`` of the SAME build: what the walk costs without the hash and the two logs;
* parent:  ``nrl_topk_scores`` of another build of the library (--parent-lib: the shared library of a checkout of the parent
  commit) through bare ctypes on the same tensors, and whether plain and parent return the same bits;
* torch:   the formulation the entry replaces -- ``user @ table.T * inv_temp``, a (B, V) matrix of Gumbel noise from torch's
  generator, ``-inf`` at the masked positions, ``torch.topk`` -- with its peak memory above the inputs.
Then the gate on the existing entries, in an alternating run of its own: ``nrl_topk_scores`` and ``nrl_topk_window_scores`` (the 24 h
before a request time per user) of THIS build's library and of the parent's, all four through the same bare ctypes path (an
``ops`` wrapper's argument checks cost host time the parent leg would not pay), bits and times.

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

from topk_window_time import INT32_MAX, INT32_MIN, bits_equal, run_legs  # noqa: E402,F401


def parent_entries(path, slices=0):
    """``nrl_topk_scores`` / ``nrl_topk_window_scores`` of the library at ``path`` as functions of the ``ops`` wrappers' arguments"""
    from newsreclib_amd import _lib, ops
    lib = ctypes.CDLL(path)
    for name in ("nrl_topk_scores_workspace_bytes", "nrl_topk_scores", "nrl_topk_window_scores"):
        getattr(lib, name).restype, getattr(lib, name).argtypes = _lib.SIGNATURES[name]
    lib.nrl_build_id.restype = ctypes.c_char_p

    def call(entry, user, table, k, window, excl_idx, excl_off, eligible):
        B, D, V = user.shape[0], user.shape[1], table.shape[0]
        excl_idx, excl_off, eligible = ops._topk_masks(excl_idx, excl_off, eligible, B, V)      # (the device ops `ops.topk_scores` issues)
        idx, score, status = ops._topk_outputs(B, k, user.device)
        ws = ops.workspace(lib.nrl_topk_scores_workspace_bytes(B, V, D, k, slices), user.device)
        rc = entry(user.data_ptr(), table.data_ptr(), B, V, D, k, *(t.data_ptr() for t in window), excl_idx.data_ptr(),
                   excl_off.data_ptr(), eligible.data_ptr(), slices, idx.data_ptr(), score.data_ptr(), status.data_ptr(), ws.data_ptr(),
                   ws.numel(), ops._stream())
        assert rc == 0, rc
        return idx, score, status

    def topk(user, table, k, excl_idx, excl_off, eligible):
        return call(lib.nrl_topk_scores, user, table, k, (), excl_idx, excl_off, eligible)

    def window(user, table, k, rt, lo, hi, excl_idx, excl_off, eligible):
        return call(lib.nrl_topk_window_scores, user, table, k, (rt, lo, hi), excl_idx, excl_off, eligible)

    return topk, window, lib.nrl_build_id().decode()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--users", type=int, default=512)
    ap.add_argument("--news", type=int, default=65536)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--inv-temp", type=float, default=1.0)
    ap.add_argument("--dims", type=int, nargs="+", default=[300, 400])
    ap.add_argument("--slices", type=int, default=0, help="pieces of the table walked in parallel per user tile (0: the library's plan)")
    ap.add_argument("--parent-lib", default=None, help="shared library of a checkout of the parent commit")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("topk_sampled_time: no GPU; a time measured anywhere else says nothing about this path")
    from newsreclib_amd import _build, _lib, ops, synthetic
    own_topk, own_window, _ = parent_entries(_build.LIB, args.slices)
    B, V, k, inv_temp = args.users, args.news, args.k, args.inv_temp
    plan = args.slices or "the library's plan"
    lines = [f"topk_sampled_time: B = {B} users, V = {V} news, k = {k}, inv_temp = {inv_temp}, exclusion lists of 0..50 rows, 2 % of the "
             f"rows ineligible; {torch.cuda.get_device_name()} on {socket.gethostname()}; library build id "
             f"{_lib.load().nrl_build_id().decode()}; torch {torch.__version__}; warm-up {args.warmup}, {args.rounds} rounds of "
             f"{args.iters} alternating calls, whole calls, device events; slices = {plan}"]
    p_topk = p_window = None
    if args.parent_lib and os.path.exists(args.parent_lib):
        p_topk, p_window, parent_id = parent_entries(args.parent_lib, args.slices)
        lines.append(f"parent legs: nrl_topk_scores / nrl_topk_window_scores of {os.path.basename(args.parent_lib)} with build id "
                     f"{parent_id}, loaded beside this build's library")
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
        span, last = 28 * 24, 7 * 24
        rt = synthetic.news_times(V, span, seed=args.seed + 31).to(torch.int32).cuda()
        req = torch.randint(span - last, span, (B,), generator=g)
        lo, hi = (req - 24).to(torch.int32).cuda(), req.to(torch.int32).cuda()
        gen = torch.Generator(device="cuda").manual_seed(args.seed)
        lines.append(f"D = {D}: score matrix {B * V * 4 / 2 ** 20:.1f} MiB, {2.0 * B * V * D / 1e9:.1f} GFLOP")

        def torch_sampled():
            z = user @ table.T * inv_temp
            z -= torch.log(-torch.log(torch.rand(B, V, device="cuda", generator=gen).clamp_(2.0 ** -24, 1 - 2.0 ** -24)))
            z.masked_fill_(~elig.bool()[None, :], float("-inf"))
            z[excl_user, excl_idx] = float("-inf")
            key, idx = torch.topk(z, k, dim=1)
            return idx, key

        legs = [("sampled", lambda: ops.topk_sampled_scores(user, table, k, keys, args.seed, inv_temp, excl_idx, excl_off, elig, args.slices)),
                ("plain", lambda: ops.topk_scores(user, table, k, excl_idx, excl_off, elig, args.slices))]
        if p_topk is not None:
            legs.append(("parent", lambda: p_topk(user, table, k, excl_idx, excl_off, elig)))
        legs.append(("torch", torch_sampled))
        lines.append("   Gumbel top-k:")
        med, outs = run_legs(legs, args, lines)
        line = f"    sampled / plain {med['sampled'] / med['plain']:.3f}   sampled / torch {med['sampled'] / med['torch']:.3f}"
        if p_topk is not None:
            line += (f"   plain / parent {med['plain'] / med['parent']:.3f}   (plain and parent return the same rows and score bits: "
                     f"{bits_equal(outs['plain'][:2], outs['parent'][:2])})")
        lines.append(line)
        si, sk, ss, sst = outs["sampled"]
        pi, ps, _ = ops.topk_scores(user, table, min(V, ops.TOPK_MAX_K), excl_idx, excl_off, elig, args.slices)
        hit = (si[:, :, None] == pi[:, None, :])
        same = (ss[:, :, None].view(torch.int32) == ps[:, None, :].view(torch.int32)) & hit
        lines.append(f"    status word {int(sst)}; {int((si >= 0).sum())} of {si.numel()} slots filled; {int(hit.any(2).sum())} drawn rows are among "
                     f"the plain call's best {pi.shape[1]}, {int(same.any(2).sum())} of them with the plain call's score bits")

        legs = [("plain", lambda: own_topk(user, table, k, excl_idx, excl_off, elig)),
                ("window", lambda: own_window(user, table, k, rt, lo, hi, excl_idx, excl_off, elig))]
        if p_window is not None:
            legs[1:1] = [("parent", lambda: p_topk(user, table, k, excl_idx, excl_off, elig))]
            legs.append(("parentw", lambda: p_window(user, table, k, rt, lo, hi, excl_idx, excl_off, elig)))
        lines.append("   gate, this build and the parent through bare ctypes: plain / parent the plain top-k, window / parentw the windowed "
                     "top-k (the 24 h before a request time per user):")
        med, outs = run_legs(legs, args, lines)
        if p_window is not None:
            lines.append(f"    plain / parent {med['plain'] / med['parent']:.3f}   (the same rows and score bits: "
                         f"{bits_equal(outs['plain'][:2], outs['parent'][:2])})   window / parentw {med['window'] / med['parentw']:.3f}   "
                         f"(the same rows and score bits: {bits_equal(outs['window'][:2], outs['parentw'][:2])})")
        del user, table, elig, excl_idx, rt, lo, hi
    report = "\n".join(lines)
    print(report)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(report + "\n")


if __name__ == "__main__":
    main()
