#!/usr/bin/env python
"""The figures behind tests/test_gpu_attention_edges.py: every attention kernel against float64 PER ROW on the score profiles and
head layouts of tests/attention_ref.py.

    python tools/attention_edges.py [--out profiles/attention_edges.txt]

It runs the test's case lists through the test's own functions (so the structural checks - finite output, intact canaries, the new K
rows, the planes kernel's two workgroup orders bit for bit - are asserted here too, and a failure ends the run) and writes one line
per case: the kernel family, the kernel's worst-row relative error against the float64 reference (row_err), the yardsticks computed
on the host from the same inputs (y32: plain float32 eager attention; y_split: float64 attention on bf16 hi + lo operands, three-pass
kernels only), the ratio err / max(yardstick), the bar max(4 y32, 1e-5) (rows, decode, verify, float32-MFMA) or
max(4 max(y32, y_split), 3e-5) (bf16x3, planes), the realised score range and the case.  Then the largest ratio per kernel, and the
sweep of the common score offset S = 0 / 30 / 120 along a spread and a one-hot direction (ar.SWEEP_DECODE, ar.SWEEP; of a decode batch
the worst sequence).  The exit status is 1 when a case is above its bar.

    python tools/attention_edges.py --digests new.jsonl                         # one JSON line per prefill case: SHA-256 of the output
    CHATTS_AMD_LIB=/path/to/another/libchatts_amd.so python tools/attention_edges.py --digests old.jsonl
    python tools/attention_edges.py --compare old.jsonl new.jsonl               # every case equal, no tolerance; exit status 1 if not

The bitwise A/B of two builds of the prefill kernels: --digests runs the test's run_attention (finite output, untouched cache, planes
written) over ROWS, PREFILL (float32-MFMA and bf16x3), PLANES, PLANES_XCD_AB under both workgroup orders, LONG_PREFILL and the prefill
cases of SWEEP - float32 output, key splits 1 / 2 / 4 / 16 through both combines, both caches, paged layouts."""
import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from chatts_amd import _lib  # noqa: E402
from tests import attention_ref as ar  # noqa: E402
from tests import test_gpu_attention_edges as edges  # noqa: E402


def measure_all(lib):
    """every case outside the sweep, in the order of the test file"""
    for batch in ar.DECODE_BATCHES + ar.DECODE_LONG:
        yield from edges.measure_decode(lib, batch)
    for spec in ar.VERIFY:
        yield edges.measure_verify(lib, spec)
    for spec in ar.ROWS + ar.PREFILL["mfma"] + ar.PREFILL["bf16x3"] + ar.PLANES + ar.LONG_PREFILL:
        yield edges.measure_attention(lib, spec)
    for spec in ar.PLANES_XCD_AB:
        yield edges.measure_xcd_ab(lib, spec)


def sweep(lib):
    """-> (every Rec of the sweep, kernel -> {(S, u kind): Rec})"""
    recs, cells = [], {}
    for batch in ar.SWEEP_DECODE:
        got = edges.measure_decode(lib, batch)
        recs += got
        cells.setdefault("decode", {})[(batch.profile, batch.u)] = max(got, key=lambda r: r.ratio)
    for spec in ar.SWEEP:
        r = (edges.measure_verify if spec.family == "verify" else edges.measure_attention)(lib, spec)
        recs.append(r)
        cells.setdefault(spec.family, {})[(spec.profile, spec.u)] = r
    return recs, cells


def digest_cases():
    """(spec, options of the call) of every prefill case"""
    for spec in ar.ROWS + ar.PREFILL["mfma"] + ar.PREFILL["bf16x3"] + ar.PLANES + ar.LONG_PREFILL:
        yield spec, edges.KERNEL_OPTIONS[spec.family]
    for spec in ar.PLANES_XCD_AB:
        for xcd in (1, 0):
            yield spec, {"ATTN_BF16X3": 1, "ATTN_XCD": xcd}
    for spec in ar.SWEEP:
        if spec.family in edges.KERNEL_OPTIONS:
            yield spec, edges.KERNEL_OPTIONS[spec.family]


def write_digests(lib, path):
    """the inputs of ar.build without its float64 truth: the digest needs none"""
    n = 0
    with open(path, "w") as f:
        for spec, options in digest_cases():
            c = ar.make_case(spec.profile, spec.u, spec.nq, spec.nkv, spec.T, spec.pos0, spec.max_ctx, spec.seed, spec.f16, spec.fused,
                             spec.qk_norm, spec.norm_seed)
            with _lib.options(**options):
                out = edges.run_attention(lib, spec, c)
            f.write(json.dumps({"case": f"{spec!r} {sorted(options.items())}", "family": spec.family,
                                "sha256": hashlib.sha256(out.contiguous().numpy().tobytes()).hexdigest()}) + "\n")
            n += 1
    print(f"{n} digests -> {path}")
    return 0


def compare_digests(old, new):
    read = lambda path: {r["case"]: r for r in map(json.loads, open(path))}          # noqa: E731
    a, b = read(old), read(new)
    bad = [k for k in a if k in b and a[k]["sha256"] != b[k]["sha256"]]
    lonely = sorted(set(a) ^ set(b))
    per = {}
    for k in a:
        per[a[k]["family"]] = per.get(a[k]["family"], 0) + 1
    print(f"{len(a)} / {len(b)} cases ({', '.join(f'{k}: {v}' for k, v in sorted(per.items()))}): {len(bad)} differ, {len(lonely)} in one file only")
    for k in bad + lonely:
        print(("DIFFERS  " if k in bad else "LONELY   ") + k)
    return 1 if bad or lonely or not a else 0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attention_edges.txt"))
    ap.add_argument("--digests", metavar="JSONL", help="write one SHA-256 per prefill case instead of measuring")
    ap.add_argument("--compare", nargs=2, metavar="JSONL", help="compare two --digests files")
    args = ap.parse_args()
    if args.compare:
        return compare_digests(*args.compare)
    lib = _lib.load()
    if args.digests:
        return write_digests(lib, args.digests)
    swept, cells = sweep(lib)
    lines = [f"# tools/attention_edges.py on {torch.cuda.get_device_name(0)}: row_err of every case of tests/test_gpu_attention_edges.py",
             f"# {'kernel':7s} {'err':>9s} {'y32':>9s} {'y_split':>9s} {'ratio':>6s} {'bar':>9s} {'s_min':>7s} {'s_max':>7s}  case"]
    worst, over = {}, 0
    for r in list(measure_all(lib)) + swept:
        lines.append("  " + r.line())
        over += not r.ok
        if r.kernel not in worst or r.ratio > worst[r.kernel].ratio:
            worst[r.kernel] = r
    lines.append("")
    lines.append(f"# {len(lines) - 3} cases, {over} above the bar")
    lines.append("# largest ratio err / max(y32, y_split) per kernel (where both are below the floor of the bar the ratio says little)")
    for kernel, r in worst.items():
        lines.append(f"  {kernel:7s} ratio {r.ratio:6.2f}  err {r.err:9.3g}  bar {r.bar:9.3g}  {r.what}")
    lines.append("")
    lines.append("# worst-row error against the common score offset S, direction u spread / one-hot (dim 5): err (y32, y_split)")
    for kernel, c in cells.items():
        for u in ar.SWEEP_U:
            row = "  ".join(f"S={S}: {c[(p, u)].err:8.3g} ({c[(p, u)].y32:8.3g}, {c[(p, u)].y_split:8.3g})" for p, S in ar.SWEEP_S)
            lines.append(f"  {kernel:7s} {'spread' if u == 'spread' else 'one-hot':8s} {row}")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines[-(len(worst) + 18):]))
    return 1 if over else 0


if __name__ == "__main__":
    sys.exit(main())
