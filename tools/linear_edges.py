#!/usr/bin/env python
"""The figures behind tests/test_gpu_linear_edges.py: every path of chatts_linear and the RMSNorm entry points against float64 PER ELEMENT
on the operand profiles of tests/linear_ref.py.

    python tools/linear_edges.py [--out profiles/linear_edges.txt]

It runs the test's case lists through the test's own functions (so the structural checks - finite output, NaN-filled workspace and padding,
the zero rows bit for bit - are asserted here too, and a failure ends the run) and writes one line per case: the kernel the dispatch code
sends the call to, the kernel's elem_err (the worst |got - want| / S_ij against the float64 reference), the yardstick y (the elem_err of
the fault-free float32 emulation of the family's documented arithmetic on the same inputs), the ratio err / y, MARGIN * y (what the bar
allows per unit of S; BAR_CAP = 2^-14 is its ceiling), `use` (the worst |got - want| / bar_ij, bar_ij = MARGIN y S_ij + 2^-23 |want_ij|,
plus 2^-16 |want| for plane outputs; the post-norm planes included), the element where `use` is worst, and the case.  Then the largest
ratio and the largest use per kernel.  The exit status is 1 when a case is above its bar."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from chatts_amd import _lib  # noqa: E402
from tests import linear_ref as lr  # noqa: E402
from tests import test_gpu_linear_edges as edges  # noqa: E402


def measure_all(lib):
    """every case, in the order of the test file"""
    for spec in lr.all_specs():
        yield edges.measure(lib, spec)
    for case in lr.RMSNORM:
        yield from edges.measure_rmsnorm(lib, *case)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "linear_edges.txt"))
    args = ap.parse_args()
    lib = _lib.load()
    lines = [f"# tools/linear_edges.py on {torch.cuda.get_device_name(0)}: elem_err of every case of tests/test_gpu_linear_edges.py",
             "# the emulation behind y sums in the order the kernels' comments document (tests/linear_ref.py's docstring); no kernel needed another",
             f"# {'kernel':32s} {'err':>9s} {'y':>9s} {'ratio':>6s} {'MARGIN*y':>9s} {'use':>6s} {'worst at':12s} case"]
    worst, over, n = {}, 0, 0
    for r in measure_all(lib):
        lines.append("  " + r.line())
        n += 1
        over += not r.ok
        w = worst.setdefault(r.kernel, [r, r])
        if r.ratio > w[0].ratio:
            w[0] = r
        if r.use > w[1].use:
            w[1] = r
    lines.append("")
    lines.append(f"# {n} cases, {over} above the bar; the largest MARGIN * y is {max(lr.MARGIN * lr.build(s)['y'] for s in lr.all_specs()):.3g} "
                 f"(BAR_CAP {lr.BAR_CAP:.3g})")
    lines.append("# per kernel: the largest ratio err / y, and the largest use of a bar")
    for kernel, (a, b) in worst.items():
        lines.append(f"  {kernel:32s} ratio {a.ratio:6.2f} ({a.what})")
        lines.append(f"  {'':32s} use   {b.use:6.3f} ({b.what})")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines[-(2 * len(worst) + 3):]))
    return 1 if over else 0


if __name__ == "__main__":
    sys.exit(main())
