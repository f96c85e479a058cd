"""Collect the error figures of the NPA / DKN shape sweep into profiles/npa_dkn_sweep_errors.txt.

Runs tests/test_gpu_npa_dkn_sweep.py (needs the MI355X) with its output captured and keeps the ``SWEEP`` lines: per case,
engine and compared tensor the kernel's max error against the float64 oracle, the float32 CPU oracle's error at the same
case, and the tolerance.  The ratio column (kernel / max(oracle32, one fp32 ulp of 1)) is for reading only; the tests do
not assert it.

pytest prints a test's progress character without a newline, so a test's first line arrives as ``.SWEEP ...``: lines are
searched, not matched at their start, and the tool fails when it kept fewer lines than the run printed.

    python tools/npa_dkn_sweep_errors.py [--out profiles/npa_dkn_sweep_errors.txt] [--log FILE] [--timeout SECONDS]"""
import argparse
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINE = re.compile(r"SWEEP (\S+) (\S+) (.+): kernel (\S+) oracle32 (\S+) tol (\S+)( FAIL)?$")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "npa_dkn_sweep_errors.txt"))
    ap.add_argument("--log", help="also keep pytest's whole output here")
    ap.add_argument("--timeout", type=float, default=300.0, help="limit of the pytest run in seconds (it takes about 10)")
    args = ap.parse_args()
    run = subprocess.run([sys.executable, "-m", "pytest", "tests/test_gpu_npa_dkn_sweep.py", "-m", "gpu", "-s", "-q", "--durations=10",
                          "-p", "no:cacheprovider"], cwd=ROOT, capture_output=True, text=True, timeout=args.timeout)
    if args.log:
        with open(args.log, "w") as f:
            f.write(run.stdout + run.stderr)
    rows, other = [], []
    for line in run.stdout.splitlines():
        m = LINE.search(line)
        if m:
            case, engine, what, kern, o32, tol, fail = m.groups()
            ratio = float(kern) / max(float(o32), 1.2e-7)
            rows.append(f"{case:34s} {engine:7s} {what:44s} {kern:>10s} {o32:>10s} {tol:>10s} {ratio:8.1f}{' FAIL' if fail else ''}")
        elif "SWEEP " in line:
            other.append(line[line.index("SWEEP ") + 6:])
    with open(args.out, "w") as f:
        f.write("# tests/test_gpu_npa_dkn_sweep.py: max |kernel - float64 oracle|, max |float32 CPU oracle - float64 oracle|, the\n"
                "# asserted tolerance (forward 5 ftol, gradients gtol max(1, |want|_max)), kernel / max(oracle32, 1.2e-7)\n"
                f"# pytest: {run.stdout.strip().splitlines()[-1] if run.stdout.strip() else 'no output'}\n")
        f.write(f"{'case':34s} {'engine':7s} {'tensor':44s} {'kernel':>10s} {'oracle32':>10s} {'tol':>10s} {'ratio':>8s}\n")
        f.write("\n".join(rows) + "\n")
        if other:
            f.write("\n" + "\n".join(other) + "\n")
    printed = run.stdout.count("SWEEP ")
    print(f"{len(rows)} figures + {len(other)} other lines of {printed} printed -> {args.out}; pytest exit {run.returncode}")
    if len(rows) + len(other) != printed or not rows:
        print("lines were lost between the run and the file", file=sys.stderr)
        return run.returncode or 1
    return run.returncode


if __name__ == "__main__":
    sys.exit(main())
