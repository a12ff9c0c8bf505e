#!/usr/bin/env python
"""A/B of the KV cache element type on the continuous-batching workload (BASELINE.json config 5 by default: ChatTS-14B fp8 weights,
16 prompts of 8 x 1024 steps): builds the model with kv_cache_dtype=None (float32) and "fp16" and times both through
bench.bench_batched, interleaved (A B A B ...), then prints the medians and spreads of step ms, tokens/s and admission ms.
--attn-only: time chatts_attention_decode_batched alone (decode attention + combine) on caches of the workload's shape instead.
--bench KV ARGS...: run bench.py's own main() with ARGS, every model it builds taking kv_cache_dtype=KV (batch-1 workloads: the
headline, config 4), so that its JSON line is comparable with the default's.

    python tools/kv_dtype_ab.py --rounds 3 --steps 32 --warmup 8 --out profiles/kv_fp16_ab_config5.json
"""
import argparse
import json
import os
import statistics
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "n": len(xs)}


def attn_only(args):
    """µs per chatts_attention_decode_batched call (attn_decode_kernel + its combine) and cache bytes per µs, both dtypes"""
    import ctypes as C
    import torch
    from chatts_amd import _lib, config as cfgmod
    lib = _lib.load()
    cfg = cfgmod.preset(args.model)
    nq, nkv, B, ctx = cfg.num_attention_heads, cfg.num_key_value_heads, args.batch, args.ctx
    max_ctx = (ctx + 256) // 256 * 256
    splits = 64
    raw = torch.randn((B, (nq + 2 * nkv) * 128), device="cuda")
    cos = torch.randn((max_ctx, 64), device="cuda")
    sin = torch.randn((max_ctx, 64), device="cuda")
    pos = torch.full((B,), ctx - 1, dtype=torch.int32, device="cuda")
    wsb = int(lib.chatts_attn_workspace(B, nq, splits))
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
    out = torch.empty((B, nq * 128), device="cuda")
    res = {}
    caches = {}
    for name, dt in (("float32", torch.float32), ("fp16", torch.float16)):
        k = torch.randn((B, nkv, max_ctx, 128), device="cuda").to(dt)
        v = torch.randn((B, nkv, max_ctx, 128), device="cuda").to(dt)
        caches[name] = (k, v, _lib.KvCache(k=k.data_ptr(), v=v.data_ptr(), max_ctx=max_ctx,
                                           dtype=_lib.KV_F16 if dt == torch.float16 else _lib.KV_F32))
        res[name] = []
    s = _lib.stream_ptr()
    for _ in range(args.rounds):
        for name, (k, v, c) in caches.items():
            def call():
                _lib.check(lib.chatts_attention_decode_batched(raw.data_ptr(), B, nq, nkv, None, None, 1e-6, cos.data_ptr(), sin.data_ptr(),
                                                               0, pos.data_ptr(), C.byref(c), nkv * max_ctx * 128, out.data_ptr(), splits,
                                                               ws.data_ptr(), wsb, s))
            for _ in range(20):
                call()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(200):
                call()
            e1.record()
            torch.cuda.synchronize()
            res[name].append(e0.elapsed_time(e1) / 200 * 1e3)
    kv_bytes = {n: B * nkv * ctx * 128 * 2 * (4 if n == "float32" else 2) for n in res}
    return {"shape": {"model": args.model, "batch": B, "ctx": ctx, "n_q": nq, "n_kv": nkv, "splits": splits},
            "us_per_call": {n: spread(v) for n, v in res.items()},
            "cache_bytes_per_call": kv_bytes,
            "cache_bytes_per_us": {n: kv_bytes[n] / statistics.median(v) for n, v in res.items()},
            "fp16_over_float32": statistics.median(res["fp16"]) / statistics.median(res["float32"])}


def bench_with_kv(kv, argv):
    """bench.main() on argv, with ChatTSForCausalLM.from_synthetic building its model with kv_cache_dtype=kv"""
    import bench
    from chatts_amd.modeling import ChatTSForCausalLM
    real = ChatTSForCausalLM.from_synthetic.__func__

    def patched(cls, config, seed=0, **kw):
        kw.setdefault("kv_cache_dtype", kv)
        return real(cls, config, seed=seed, **kw)
    ChatTSForCausalLM.from_synthetic = classmethod(patched)
    sys.argv = ["bench.py", *argv]
    bench.main()


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--bench":
        return bench_with_kv(None if sys.argv[2] == "auto" else sys.argv[2], sys.argv[3:])
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="chatts-14b")
    ap.add_argument("--weights", default="fp8", choices=["bf16", "fp8", "int8", "int4"])
    ap.add_argument("--series", type=int, default=8)
    ap.add_argument("--length", type=int, default=1024)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--max-ctx", type=int, default=2048)
    ap.add_argument("--attn-only", action="store_true")
    ap.add_argument("--ctx", type=int, default=1230, help="--attn-only: context of every sequence")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    torch.cuda.set_device(0)
    if args.attn_only:
        res = attn_only(args)
    else:
        import bench
        from chatts_amd import config as cfgmod
        from chatts_amd.modeling import ChatTSForCausalLM
        from chatts_amd.tp import LocalComm
        cfg = cfgmod.preset(args.model)
        comm = LocalComm()
        bargs = types.SimpleNamespace(batch=args.batch, series=args.series, length=args.length, steps=args.steps, warmup=args.warmup,
                                      no_pack=False, dump_outputs=None, full=False, gpus=1, layers=None, model=args.model,
                                      weights=args.weights, precision="bf16x2")
        models = {}
        for name, kv in (("float32", None), ("fp16", "fp16")):
            models[name] = ChatTSForCausalLM.from_synthetic(cfg, seed=0, device="cuda:0", comm=comm, max_ctx=args.max_ctx,
                                                            max_prefill_tokens=1024, weight_format=args.weights, max_batch=args.batch,
                                                            kv_cache_dtype=kv)
        runs = {n: [] for n in models}
        for _ in range(args.rounds):
            for name, m in models.items():
                runs[name].append(bench.bench_batched(bargs, m, cfg, comm, 1, torch.device("cuda:0")))
        res = {"workload": f"{args.model} {args.weights} weights, {args.batch} x ({args.series} x {args.length}), steps {args.steps}",
               "kv_cache_bytes": {n: m.kv_cache_bytes_local() for n, m in models.items()}}
        for name, rs in runs.items():
            res[name] = {"ms_per_step": spread([r["ms_per_step"] for r in rs]), "tokens_per_s": spread([r["value"] for r in rs]),
                         "batch_admit_ms": spread([r["batch_admit_ms_total"] for r in rs]), "ttft_ms_p50": spread([r["ttft_ms_p50"] for r in rs]),
                         "first_tokens_seq0": rs[-1]["config"]["first_tokens_seq0"]}
        res["step_ratio_fp16_over_float32"] = res["fp16"]["ms_per_step"]["median"] / res["float32"]["ms_per_step"]["median"]
    print(json.dumps(res, indent=1))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
