#!/usr/bin/env python
"""The decode GEMV (csrc/gemv.hip) through chatts_linear, for a bitwise A/B of two builds:

    python tools/gemv_ab.py [--seed S] > new.jsonl
    CHATTS_AMD_LIB=/path/to/another/libchatts_amd.so python tools/gemv_ab.py [--seed S] > old.jsonl      # the same calls, another build
    python tools/gemv_ab.py --compare old.jsonl new.jsonl          # every case's digest, equal or not

One JSON line per case with the SHA-256 digest of the output row (pre-filled with NaN, so an element the kernel did not write shows).
A reordered sum changes a digest: the comparison knows no tolerance.  The cases are the smallest shapes that reach each branch:
  n 96 / 1008 / 1504 (SwiGLU: rounded down to a multiple of 32), k 256 / 1600 / 5120 / 13824 = 1, 4, 10, 27 bf16 chunks with a lane tail
  (1600: 8 lanes of the last chunk) and a chunk tail (13824: an odd number of chunks), every C-ABI epilogue the GEMV serves (NONE,
  RESID, SWIGLU), fused norm and bias on and off; bf16 under the default geometry and the launch geometries of GEMV_GEOMS (tests/test_gpu_kernels.py); fp8 and int8 under the
  default and the four GEMV8_ROWS x GEMV8_UNR forms; int4 at three (n, k, group) shapes; GEMV_KS auto / 1 / 2 / 3 / 5 / 8 / 16 at three
  K-split shapes.  (The exchange-carrying epilogue needs a communicator: tests/test_gpu_tp_p2p.py compares it with the stand-alone kernels.)"""
import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GEMV_GEOMS = [{}, dict(ROWS=2, UNR=2, NW=4), dict(ROWS=4, UNR=2, NW=8), dict(ROWS=2, UNR=4, NW=16), dict(ROWS=4, UNR=4, NW=4),
              dict(ROWS=2, UNR=2, NW=7, BLOCKS=512, LDSPAD=2), dict(ROWS=2, UNR=2, NW=9, BLOCKS=768, LDSPAD=3),
              dict(ROWS=2, UNR=4, NW=5, BLOCKS=3), dict(ROWS=4, UNR=2, NW=11, BLOCKS=256, LDSPAD=1)]
GEMV8_FORMS = [{}, dict(ROWS=2, UNR=2), dict(ROWS=4, UNR=2), dict(ROWS=4, UNR=1), dict(ROWS=2, UNR=4)]
NS, KS = (96, 1008, 1504), (256, 1600, 5120, 13824)
INT4_SHAPES = ((96, 1024, 64), (160, 3072, 16), (1024, 512, 128))
KSPLIT_SHAPES, KSPLIT_WAVES = ((896, 5120), (96, 13824), (5120, 1728)), (None, 1, 2, 3, 5, 8, 16)


def tag(d):
    return ",".join(f"{k}={v}" for k, v in d.items()) or "default"


def run(seed, emit):
    import torch
    from chatts_amd import _lib
    from chatts_amd.modeling import pack_int4, quantize_fp8_rows, quantize_int4_rows, quantize_int8_rows
    lib = _lib.load()
    EPIS = {"none": _lib.EPI_NONE, "resid": _lib.EPI_RESID, "swiglu": _lib.EPI_SWIGLU}
    st = torch.cuda.current_stream().cuda_stream

    def problem(n, k, i):
        g = torch.Generator().manual_seed(seed * 1000 + i)
        P = {"a": torch.randn((1, k), generator=g), "w": (torch.randn((n, k), generator=g) * 0.05).to(torch.bfloat16),
             "bias": torch.randn(n, generator=g), "resid": torch.randn((1, n), generator=g), "norm": 1 + 0.1 * torch.randn(k, generator=g)}
        P["w"][:, 0] = torch.linspace(-1, 1, n).to(torch.bfloat16)
        P["w"][7 % n] *= 37.0                      # rows with very different scales
        return {key: v.cuda() for key, v in P.items()}

    def call(name, P, n, k, epi, norm, bias, w=None, **extra):
        ncols = n // 2 if epi == "swiglu" else n
        out = torch.full((1, ncols), float("nan"), dtype=torch.float32, device="cuda")
        la = _lib.LinearArgs(a=P["a"].data_ptr(), w=(P["w"] if w is None else w).data_ptr(), bias=P["bias"].data_ptr() if bias else None,
                             resid=P["resid"].data_ptr() if epi == "resid" else None, c=out.data_ptr(),
                             norm_w=P["norm"].data_ptr() if norm else None, norm_eps=1e-6, m=1, n=n, k=k, lda=k, ldw=k, ldc=ncols,
                             epilogue=EPIS[epi], workspace=None, workspace_bytes=0, **extra)
        _lib.check(lib.chatts_linear(la, st))
        torch.cuda.synchronize()
        emit({"case": f"{name}/n{n}/k{k}/{epi}/norm{int(norm)}/bias{int(bias)}",
              "sha256": hashlib.sha256(out.cpu().numpy().tobytes()).hexdigest()})

    def variants(n0):
        for epi in EPIS:
            yield epi, n0 // 32 * 32 if epi == "swiglu" else n0

    i = 0
    for n0 in NS:
        for k in KS:
            for epi, n in variants(n0):
                i += 1
                P = problem(n, k, i)
                w8 = [(fmt, quant(P["w"]), w8_format) for fmt, quant, w8_format in
                      (("fp8", quantize_fp8_rows, _lib.W8_FP8), ("int8", quantize_int8_rows, _lib.W8_INT8))]
                for norm in (False, True):
                    for bias in (False, True):
                        for geom in GEMV_GEOMS:
                            with _lib.options(**{"GEMV_" + key: v for key, v in geom.items()}):
                                call("bf16/" + tag(geom), P, n, k, epi, norm, bias)
                        for fmt, (q, scale, deq), w8_format in w8:
                            for form in GEMV8_FORMS:
                                with _lib.options(**{"GEMV8_" + key: v for key, v in form.items()}):
                                    call(f"{fmt}/" + tag(form), P, n, k, epi, norm, bias, w=deq, w8=q.data_ptr(), w8_scale=scale.data_ptr(),
                                         ldw8=k, w8_format=w8_format)
    for n0, k, gs in INT4_SHAPES:
        for epi, n in variants(n0):
            i += 1
            P = problem(n, k, i)
            q, sc, z, deq = quantize_int4_rows(P["w"], gs)
            w4, sz = pack_int4(q, sc, z)
            for norm in (False, True):
                for bias in (False, True):
                    call(f"int4/group{gs}", P, n, k, epi, norm, bias, w=deq, w4=w4.data_ptr(), w4_sz=sz.data_ptr(), ldw4=k // 2, w4_group=gs)
    for n, k in KSPLIT_SHAPES:
        i += 1
        P = problem(n, k, i)
        for ks in KSPLIT_WAVES:
            with _lib.options(**({} if ks is None else {"GEMV_KS": ks})):
                for epi in EPIS:
                    for norm in (False, True):
                        call(f"bf16/GEMV_KS={ks or 'auto'}", P, n, k, epi, norm, True)


def read(path):
    with open(path) as f:
        rows = [json.loads(line) for line in f if line.startswith("{")]
    return {r["case"]: r["sha256"] for r in rows if "case" in r}


def compare(a, b):
    ka, kb = read(a), read(b)
    differs = sorted(c for c in set(ka) | set(kb) if ka.get(c) != kb.get(c))
    print(json.dumps({"a": a, "b": b, "cases": [len(ka), len(kb)], "equal": not differs, "differs": differs}))
    return 1 if differs else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--compare", nargs=2, metavar="JSONL")
    args = ap.parse_args()
    if args.compare:
        return compare(*args.compare)
    from chatts_amd import _lib
    _lib.load()
    print(json.dumps({"lib": _lib.lib_path(), "seed": args.seed}), flush=True)
    cases = []
    run(args.seed, lambda row: (cases.append(row["case"]), print(json.dumps(row), flush=True)))
    assert len(set(cases)) == len(cases), "case names must be unique"
    print(json.dumps({"cases_run": len(cases)}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
