"""Collect the error figures of a shape sweep against float64 into a table under profiles/.

Runs one sweep file (needs the MI355X) with its output captured and keeps the ``SWEEP`` lines: per case,
engine and compared tensor the kernel's max error against the float64 oracle, the float32 CPU oracle's error at the same
case, and the tolerance.  The ratio column (kernel / max(oracle32, one fp32 ulp of 1)) is for reading only; the tests do
not assert it.  ``lstur_naml`` prints 2750 figures; its table has one row per (case, tensor) with the figures of every run of
that case side by side (``wide_rows``): each engine and, where a case runs under both visiting orders, each order.

pytest prints a test's progress character without a newline, so a test's first line arrives as ``.SWEEP ...``: lines are
searched, not matched at their start, and the tool fails when it kept fewer lines than the run printed.

    python tools/sweep_errors.py [--tests npa_dkn | sd_manner | caum_miner | lstur_naml | tests/FILE.py] [--out FILE] [--log FILE]
                                 [--timeout SECONDS]

``--tests npa_dkn`` (the default) runs tests/test_gpu_npa_dkn_sweep.py into profiles/npa_dkn_sweep_errors.txt,
``--tests sd_manner`` tests/test_gpu_sd_manner_sweep.py into profiles/sd_manner_sweep_errors.txt, ``--tests caum_miner``
tests/test_gpu_caum_miner_sweep.py into profiles/caum_miner_sweep_errors.txt, ``--tests lstur_naml``
tests/test_gpu_lstur_naml_sweep.py into profiles/lstur_naml_sweep_errors.txt; a path runs that file and needs ``--out``."""
import argparse
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWEEPS = {
    "npa_dkn": ("tests/test_gpu_npa_dkn_sweep.py", "forward 5 ftol, gradients gtol max(1, |want|_max)"),
    "sd_manner": ("tests/test_gpu_sd_manner_sweep.py", "the larger of the project's bound and 4x oracle32; MANNeR: 4x oracle32, SupCon x3 under bf16x3"),
    "caum_miner": ("tests/test_gpu_caum_miner_sweep.py", "forward 5 ftol, gradients gtol max(1, |want|_max); above a configured width the larger of that and 4x oracle32"),
    "lstur_naml": ("tests/test_gpu_lstur_naml_sweep.py", "forward 5 ftol (CNN encoder: the larger of ftol max(1, |want|_max) and 4x oracle32), gradients gtol max(1, |want|_max); above the width a bound was set at the larger of that and 4x oracle32"),
}
WIDE = {"lstur_naml"}
RUNS = [("f32", ""), ("bf16x3", ""), ("f32", "argsort"), ("bf16x3", "argsort")]
LINE = re.compile(r"SWEEP (\S+) (\S+) (.+): kernel (\S+) oracle32 (\S+) tol (\S+)( FAIL)?$")


def wide_rows(figs):
    """figs: (case, engine, tensor, kernel, oracle32, tol, fail) per printed figure -> header, one row per (case, tensor).  A case
    tag that ends in /sort or /argsort is one case under two visiting orders; oracle32 belongs to the case, tol to the engine."""
    table = {}
    for case, engine, what, kern, o32, tol, fail in figs:
        base, _, order = case.rpartition("/")
        base, order = (base, "" if order == "sort" else order) if order in ("sort", "argsort") else (case, "")
        row = table.setdefault((base, what), {"o32": o32})
        assert row["o32"] == o32 and row.setdefault("tol_" + engine, tol) == tol and (engine, order) not in row, (case, engine, what)
        row[(engine, order)] = kern + ("!" if fail else "")
    head = f"{'case':34s} {'tensor':36s} {'oracle32':>9s} {'tol f32':>9s} {'tol x3':>9s} {'f32':>9s} {'bf16x3':>9s} {'f32 args.':>9s} {'x3 args.':>9s}"
    rows = [f"{base:34s} {what:36s} {r['o32']:>9s} {r.get('tol_f32', '-'):>9s} {r.get('tol_bf16x3', '-'):>9s} "
            + " ".join(f"{r.get(run, '-'):>9s}" for run in RUNS) + (" FAIL" if any("!" in r.get(run, "") for run in RUNS) else "")
            for (base, what), r in table.items()]
    return head, rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tests", default="npa_dkn", help="npa_dkn, sd_manner, caum_miner, lstur_naml, or the path of a sweep file")
    ap.add_argument("--out", help="the table (default: profiles/<tests>_sweep_errors.txt)")
    ap.add_argument("--log", help="also keep pytest's whole output here")
    ap.add_argument("--timeout", type=float, default=300.0, help="limit of the pytest run in seconds (it takes about 10)")
    args = ap.parse_args()
    if args.tests in SWEEPS:
        tests, rule = SWEEPS[args.tests]
        out = args.out or os.path.join(ROOT, "profiles", args.tests + "_sweep_errors.txt")
    else:
        if not args.out:
            ap.error("--out is needed with the path of a sweep file")
        tests, rule, out = args.tests, "as the file states", args.out
    run = subprocess.run([sys.executable, "-m", "pytest", tests, "-m", "gpu", "-s", "-q", "--durations=10",
                          "-p", "no:cacheprovider"], cwd=ROOT, capture_output=True, text=True, timeout=args.timeout)
    if args.log:
        with open(args.log, "w") as f:
            f.write(run.stdout + run.stderr)
    rows, other, figs = [], [], []
    for line in run.stdout.splitlines():
        m = LINE.search(line)
        if m:
            case, engine, what, kern, o32, tol, fail = m.groups()
            figs.append(m.groups())
            ratio = float(kern) / max(float(o32), 1.2e-7)
            rows.append(f"{case:44s} {engine:7s} {what:58s} {kern:>10s} {o32:>10s} {tol:>10s} {ratio:8.1f}{' FAIL' if fail else ''}")
        elif "SWEEP " in line:
            other.append(line[line.index("SWEEP ") + 6:])
    head = f"{'case':44s} {'engine':7s} {'tensor':58s} {'kernel':>10s} {'oracle32':>10s} {'tol':>10s} {'ratio':>8s}"
    n_figures = len(rows)
    if args.tests in WIDE:
        head, rows = wide_rows(figs)
    with open(out, "w") as f:
        f.write(f"# {tests}: max |kernel - float64 oracle|, max |float32 CPU oracle - float64 oracle|, the\n"
                f"# asserted tolerance ({rule}), kernel / max(oracle32, 1.2e-7)\n"
                f"# pytest: {run.stdout.strip().splitlines()[-1] if run.stdout.strip() else 'no output'}\n")
        if args.tests in WIDE:
            f.write(f"# {n_figures} figures: kernel error per run (engine, visiting order 'args.' = external argsort); '!' marks a miss\n")
        f.write(head + "\n")
        f.write("\n".join(rows) + "\n")
        if other:
            f.write("\n" + "\n".join(other) + "\n")
    printed = run.stdout.count("SWEEP ")
    print(f"{n_figures} figures + {len(other)} other lines of {printed} printed -> {out}; pytest exit {run.returncode}")
    if n_figures + len(other) != printed or not rows:
        print("lines were lost between the run and the file", file=sys.stderr)
        return run.returncode or 1
    return run.returncode


if __name__ == "__main__":
    sys.exit(main())
