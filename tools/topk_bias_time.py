#!/usr/bin/env python3
"""Times the class-biased full-catalogue top-k against its neighbours, in ONE process on one GPU, the legs alternating (A, B, C,
D, A, ...) after a shared warm-up, device-event timed (nothing is read back inside the timed region), median / min / max of
--iters:

* bias:   ``ops.topk_bias_scores`` (``nrl_topk_bias_scores``: the dot product plus bias[u, class of the row], never (B, V));
* plain:  ``ops.topk_scores`` of the SAME build: what the bias costs on top of the walk it shares;
* parent: ``nrl_topk_scores`` of another build of the library (--parent-lib: the shared library of a checkout of the parent
  commit), called through ctypes on the same tensors; without --parent-lib the report says the leg was not measured;
* torch:  the same result in torch ops -- ``user @ table.T``, the gathered bias added, ``-inf`` written at the excluded positions,
  ``torch.topk``.

Shape: --users users, --news table rows, D = 300 and 400, S = 4, 19 and 64 classes, k = --k, ragged exclusion lists of 0..50 rows
per user.  Peak allocated memory of each leg is the allocator's high-water mark above the inputs.  The bias leg's rows are
compared with the torch leg's (the torch GEMM rounds differently, so rows may swap where scores are within rounding of each
other; the report counts them).  Needs a GPU: there is no CPU path to time."""
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
    """``nrl_topk_scores`` of the library at ``path`` as a function of ``ops.topk_scores``' first five arguments"""
    from newsreclib_amd import _lib, ops
    lib = ctypes.CDLL(path)
    for name in ("nrl_topk_scores_workspace_bytes", "nrl_topk_scores"):
        getattr(lib, name).restype, getattr(lib, name).argtypes = _lib.SIGNATURES[name]
    lib.nrl_build_id.restype = ctypes.c_char_p

    def call(user, table, k, excl_idx, excl_off):
        B, D, V = user.shape[0], user.shape[1], table.shape[0]
        excl_idx, excl_off, _ = ops._topk_masks(excl_idx, excl_off, None, B, V)      # (the device ops `ops.topk_scores` issues)
        idx, score, status = ops._topk_outputs(B, k, user.device)
        ws = ops.workspace(lib.nrl_topk_scores_workspace_bytes(B, V, D, k, 0), user.device)
        rc = lib.nrl_topk_scores(user.data_ptr(), table.data_ptr(), B, V, D, k, excl_idx.data_ptr(), excl_off.data_ptr(), None, 0,
                                 idx.data_ptr(), score.data_ptr(), status.data_ptr(), ws.data_ptr(), ws.numel(), ops._stream())
        assert rc == 0, rc
        return idx, score, status

    return call, lib.nrl_build_id().decode()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--users", type=int, default=512)
    ap.add_argument("--news", type=int, default=65536)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--iters", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--classes", type=int, nargs="+", default=[4, 19, 64])
    ap.add_argument("--dims", type=int, nargs="+", default=[300, 400])
    ap.add_argument("--parent-lib", default=None, help="shared library of a checkout of the parent commit")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("topk_bias_time: no GPU; a time measured anywhere else says nothing about this path")
    from newsreclib_amd import _lib, ops
    B, V, k = args.users, args.news, args.k
    lines = [f"topk_bias_time: B = {B} users, V = {V} news, k = {k}, exclusion lists of 0..50 rows; {torch.cuda.get_device_name()} on "
             f"{socket.gethostname()}; library build id {_lib.load().nrl_build_id().decode()}; torch {torch.__version__}; "
             f"warm-up {args.warmup}, {args.iters} alternating repeats, device events"]
    parent = None
    if args.parent_lib and os.path.exists(args.parent_lib):
        parent, parent_id = parent_topk(args.parent_lib)
        lines.append(f"parent leg: nrl_topk_scores of {os.path.basename(args.parent_lib)} with build id {parent_id}, loaded beside this "
                     "build's library")
    else:
        lines.append("parent leg: NOT measured (no library of the parent commit was given with --parent-lib)")
    for D in args.dims:
        for S in args.classes:
            g = torch.Generator().manual_seed(args.seed + D + S)
            user, table = torch.randn(B, D, generator=g).cuda(), torch.randn(V, D, generator=g).cuda()
            bias = torch.randn(B, S, generator=g).cuda()
            cls = torch.randint(0, S, (V,), generator=g).to(torch.int32).cuda()
            cls64 = cls.long()
            sizes = torch.randint(0, 51, (B,), generator=g)
            excl_idx = torch.randint(0, V, (int(sizes.sum()),), generator=g).cuda()
            excl_off = torch.cat([torch.zeros(1, dtype=torch.int64), sizes.cumsum(0)]).cuda()
            excl_user = torch.repeat_interleave(torch.arange(B), sizes).cuda()

            def biased():
                return ops.topk_bias_scores(user, table, bias, cls, k, excl_idx, excl_off)

            def plain():
                return ops.topk_scores(user, table, k, excl_idx, excl_off)

            def torch_ops():
                s = user @ table.T
                s += bias[:, cls64]
                s[excl_user, excl_idx] = float("-inf")
                score, idx = torch.topk(s, k, dim=1)
                return idx, score

            legs = [("bias", biased), ("plain", plain)]
            if parent is not None:
                legs.append(("parent", lambda: parent(user, table, k, excl_idx, excl_off)))
            legs.append(("torch", torch_ops))
            for _ in range(args.warmup):
                for _, fn in legs:
                    fn()
            times, peaks, outs = {n: [] for n, _ in legs}, {}, {}
            for _ in range(args.iters):
                for name, fn in legs:
                    ms, peak, out = timed(fn)
                    times[name].append(ms)
                    peaks[name] = max(peaks.get(name, 0), peak)
                    outs[name] = out
            lines.append(f"D = {D}, S = {S}: score matrix {B * V * 4 / 2 ** 20:.1f} MiB, {2.0 * B * V * D / 1e9:.1f} GFLOP")
            med = {}
            for name, _ in legs:
                t = sorted(times[name])
                med[name] = t[len(t) // 2]
                lines.append(f"  {name:6s} median {med[name]:8.3f} ms  min {t[0]:8.3f}  max {t[-1]:8.3f}   peak allocated above the inputs "
                             f"{peaks[name] / 2 ** 20:8.2f} MiB")
            ratios = f"  bias / plain time: {med['bias'] / med['plain']:.3f}   bias / torch time: {med['bias'] / med['torch']:.3f}"
            if parent is not None:
                ratios += f"   plain / parent time: {med['plain'] / med['parent']:.3f}"
                same = torch.equal(outs["plain"][0], outs["parent"][0]) and \
                    torch.equal(outs["plain"][1].view(torch.int32), outs["parent"][1].view(torch.int32))
                ratios += f"   (plain and parent return the same rows and score bits: {same})"
            lines.append(ratios)
            fi, fs, status = outs["bias"]
            ti, ts = outs["torch"]
            same = fi == ti
            lines.append(f"  status word {int(status)}; rows equal to torch's in {int(same.sum())} of {same.numel()} slots, same row sets "
                         f"for {int((fi.sort(1).values == ti.sort(1).values).all(1).sum())} of {B} users, largest score difference "
                         f"{float((fs - ts).abs().max()):.3e}")
    report = "\n".join(lines)
    print(report)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(report + "\n")


if __name__ == "__main__":
    main()
