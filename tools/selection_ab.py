#!/usr/bin/env python
"""The three selection kernels on the decoder's real row (151936 logits, rows 152064 apart), for a per-kernel A/B under the profiler:

    rocprofv3 --kernel-trace --stats -d OUT -- python tools/selection_ab.py [--calls N] [--batch B]
    CHATTS_AMD_LIB=/path/to/another/libchatts_amd.so rocprofv3 ... -- python tools/selection_ab.py      # the same calls, another build

--calls launches each of: chatts_argmax_batched_ws without workspace (argmax_kernel), with workspace (argmax_part_kernel +
argmax_final_kernel), chatts_sample_batched with temperature 0.7, top_k 20, top_p 0.9 and with temperature 1, no cuts (sample_kernel).
The logits are finite Gaussian values: the path every decode step takes.  Prints one JSON line with the tokens, so that two builds can be
compared for equality as well.  `--summarise DIR...` instead prints the per-kernel averages of the *_kernel_stats.csv files under DIRs."""
import argparse
import csv
import ctypes as C
import glob
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("argmax_kernel", "argmax_part_kernel", "argmax_final_kernel", "sample_kernel")


def summarise(dirs):
    for d in dirs:
        row = {}
        for path in glob.glob(os.path.join(d, "**", "*_kernel_stats.csv"), recursive=True):
            with open(path) as f:
                for r in csv.DictReader(f):
                    for k in KERNELS:
                        if f"chatts::{k}(" in r["Name"]:
                            row[k] = {"calls": int(r["Calls"]), "avg_us": round(float(r["AverageNs"]) / 1e3, 3), "min_us": int(r["MinNs"]) / 1e3}
        print(json.dumps({"dir": d, **row}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--summarise", nargs="+", metavar="DIR")
    args = ap.parse_args()
    if args.summarise:
        return summarise(args.summarise)
    sys.path.insert(0, ROOT)
    import torch
    from chatts_amd import _lib
    lib = _lib.load()
    V, stride, B = 151936, 152064, args.batch
    g = torch.Generator().manual_seed(1)
    logits = (torch.randn((B, stride), generator=g) * 2.5).cuda()
    tok = torch.zeros(B, dtype=torch.int64, device="cuda")
    val = torch.zeros(B, device="cuda")
    step = torch.zeros(B, dtype=torch.int32, device="cuda")
    pos = torch.zeros(B, dtype=torch.int32, device="cuda")
    out = torch.zeros((B, 8), dtype=torch.int64, device="cuda")
    ws = torch.empty(int(lib.chatts_argmax_workspace(B)), dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    tokens = {}

    def argmax(use_ws):
        _lib.check(lib.chatts_argmax_batched_ws(logits.data_ptr(), B, stride, V, 0, tok.data_ptr(), val.data_ptr(), out.data_ptr(), 8, step.data_ptr(),
                                                pos.data_ptr(), 0, ws.data_ptr() if use_ws else None, ws.numel() if use_ws else 0, st))

    def sample(T, k, p):
        sa = _lib.SamplingArgs(temperature=T, top_k=k, top_p=p, seed=99, n_kept=None, kept_mass=None)
        _lib.check(lib.chatts_sample_batched(logits.data_ptr(), B, stride, V, 0, C.byref(sa), tok.data_ptr(), val.data_ptr(), out.data_ptr(), 8,
                                             step.data_ptr(), pos.data_ptr(), 0, st))

    for name, fn in (("argmax", lambda: argmax(False)), ("argmax_ws", lambda: argmax(True)), ("sample_k20_p0.9", lambda: sample(0.7, 20, 0.9)),
                     ("sample_plain", lambda: sample(1.0, 0, 1.0))):
        for _ in range(args.calls):
            step.zero_()
            fn()
        torch.cuda.synchronize()
        tokens[name] = tok.tolist()
    print(json.dumps({"lib": _lib.lib_path(), "calls": args.calls, "batch": B, "tokens": tokens}))


if __name__ == "__main__":
    main()
