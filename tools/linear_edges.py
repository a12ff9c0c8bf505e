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
ratio and the largest use per kernel.  The exit status is 1 when a case is above its bar.

    python tools/linear_edges.py --digests new.jsonl                            # one JSON line per case: SHA-256 of every output
    CHATTS_AMD_LIB=/path/to/another/libchatts_amd.so python tools/linear_edges.py --digests old.jsonl
    python tools/linear_edges.py --compare old.jsonl new.jsonl                  # every case equal, no tolerance; exit status 1 if not

The bitwise A/B of two builds of the linear kernels: --digests runs every spec of lr.all_specs() through the test's run_linear (c and the
post-norm planes), the lr.RMSNORM cases through both RMSNorm entry points, and chatts_linear_f16q on the forced-GEMM_SK shapes of
tests/test_gpu_f16q.py (c, the f16 hi plane, the e4m3 lo plane and the scale bytes of the post-norm output)."""
import argparse
import hashlib
import json
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


def _sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.cpu().contiguous().view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


F16Q_FORCED = [(272, 512, 1024, t, sk) for t in (2, 9, 17) for sk in (1, 2, 3, 4)] + [(17, 6272, 1024, 1, 2)]      # test_gpu_f16q.py: (M, N, K, GEMM_T, GEMM_SK)


def digest_cases(lib):
    """(case, family, digest) of every output the linear kernels write"""
    for spec in lr.all_specs():
        raw = {}
        out, _ = edges.run_linear(lib, spec, lr.make_case(spec.profile, spec.m, spec.n, spec.k, spec.epi, spec.seed, spec.fmt), raw)
        yield repr(spec), spec.kernel, _sha(out, *raw.values())
    for profile, t, hidden, seed in lr.RMSNORM:
        c = lr.rms_case(profile, t, hidden, seed)
        x, w = c["x"].to(edges.DEV), c["w"].to(edges.DEV)
        y, hi, lo = (torch.zeros((t, hidden), dtype=d, device=edges.DEV) for d in (torch.float32, torch.bfloat16, torch.bfloat16))
        _lib.check(lib.chatts_rmsnorm(x.data_ptr(), w.data_ptr(), y.data_ptr(), t, hidden, lr.EPS, edges.st()))
        _lib.check(lib.chatts_rmsnorm_planes(x.data_ptr(), w.data_ptr(), hi.data_ptr(), lo.data_ptr(), hidden, t, hidden, lr.EPS, edges.st()))
        torch.cuda.synchronize()
        yield f"rmsnorm {profile} {t}x{hidden}", "rmsnorm", _sha(y, hi, lo)
    from tests.test_gpu_strides import F16Q_DENSE, _f16q_call, _f16q_operands
    for m, n, k, t, sk in F16Q_FORCED:
        O = _f16q_operands(lib, m, n, k, seed=17 + sk, tiled=False)
        for epi in (_lib.EPI_NONE, _lib.EPI_RESID):
            for post in (False, True):
                with _lib.options(GEMM_T=t, GEMM_SK=sk):
                    rc, outs, _ = _f16q_call(lib, O, epi, F16Q_DENSE, post=post)
                _lib.check(rc)
                yield f"f16q {m}x{n}x{k} T={t} sk={sk} epi={epi} post={post}", "f16q", _sha(*(buf for buf, _ in outs.values()))


def write_digests(lib, path):
    n = 0
    with open(path, "w") as f:
        for case, family, sha in digest_cases(lib):
            f.write(json.dumps({"case": case, "family": family, "sha256": sha}) + "\n")
            n += 1
    print(f"{n} digests -> {path}")
    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "linear_edges.txt"))
    ap.add_argument("--digests", metavar="JSONL", help="write one SHA-256 per case instead of measuring")
    ap.add_argument("--compare", nargs=2, metavar="JSONL", help="compare two --digests files")
    args = ap.parse_args()
    if args.compare:
        from tools.attention_edges import compare_digests
        return compare_digests(*args.compare)
    lib = _lib.load()
    if args.digests:
        return write_digests(lib, args.digests)
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
