"""Speculative decoding by prompt lookup: what a speculative step costs against the plain step (profiles/spec_decode_ab.txt).

ChatTS-14B synthetic, the headline prompt (bench.py's 8 x 256), one MI355X, one process per weight format.  Per round, interleaved:
the plain step and the speculative step for k in --ks, each a window of --steps graph replays timed with device events after a
warm-up; the figure of a variant is the median over the rounds.  c(k) = t_spec(k) / t_plain is the break-even in mean tokens per
step: speculation pays when a step emits more than c(k) tokens on average.  The step's launches do not depend on what is accepted,
so the step time does not either.  The end-to-end tokens/s on synthetic weights says nothing about a real checkpoint: where the
synthetic continuation loops it is an UPPER BOUND (acceptance unrealistically high), where it never repeats the context it is the
floor (one token per step); the row carries tokens_per_step and the counters so that the reader sees which.

    python tools/spec_decode_ab.py --weights bf16 [--ks 1,2,4,8] [--rounds 3] [--steps 48]
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/spec_decode_ab.py --weights bf16 --trace
        (--trace: k = 4 only, one short window: the verify attention's time per layer is attn_verify_kernel + attn_verify_combine_kernel)
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="chatts-14b")
    ap.add_argument("--weights", default="bf16", choices=["bf16", "fp8"])
    ap.add_argument("--ks", default="1,2,4,8")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=48)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--layers", type=int, default=None, help="debug only: truncate depth")
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--e2e-tokens", type=int, default=256)
    args = ap.parse_args()
    import torch
    import bench
    from chatts_amd import config as cfgmod
    from chatts_amd.modeling import ChatTSForCausalLM
    if not torch.cuda.is_available():
        raise SystemExit("spec_decode_ab: needs the GPU (there is no CPU path to time)")
    ks = [4] if args.trace else [int(k) for k in args.ks.split(",")]
    steps = 8 if args.trace else args.steps
    cfg = cfgmod.preset(args.model, **({"num_hidden_layers": args.layers} if args.layers else {}))
    proc, prompt, series, lengths = bench.build_inputs(cfg)
    inputs = proc(text=[prompt], timeseries=series, padding=True, return_tensors="pt")
    ids, ser, lens = inputs["input_ids"][0].tolist(), inputs["timeseries"].cuda(), list(proc.last_lengths)
    spec = lambda k: {"k": k, "ngram_min": 1, "ngram_max": 3}
    model = ChatTSForCausalLM.from_synthetic(cfg, seed=0, max_ctx=2048, max_prefill_tokens=2048, weight_format=args.weights,
                                             speculative_config={"method": "ngram", "num_speculative_tokens": 8})
    budget = 1024                                                # never reached inside a window: every timed step does full work

    def window(k):
        """prefill the prompt, warm up, then `steps` replays of the plain (k = 0) or the speculative step -> ms per step"""
        model._spec_cfg = spec(k) if k else None
        T = model._prefill_request(ids, ser, lens, budget)
        assert model._spec_active == bool(k)
        for _ in range(args.warmup):
            model.decode_step()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(steps):
            model.decode_step()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / steps, T

    times = {k: [] for k in [0] + ks}
    for _ in range(1 if args.trace else args.rounds):
        for k in [0] + ks:
            ms, T = window(k)
            times[k].append(ms)
    med = {k: statistics.median(v) for k, v in times.items()}
    out = {"model": args.model, "weight_format": args.weights, "prompt_tokens": T, "steps_per_window": steps, "rounds": len(times[0]),
           "plain_ms": times[0], "plain_ms_median": med[0],
           "spec_ms": {str(k): times[k] for k in ks}, "spec_ms_median": {str(k): med[k] for k in ks},
           "c_k": {str(k): med[k] / med[0] for k in ks}}
    if not args.trace:
        # end to end on the synthetic model (see the module docstring for what it can and cannot say)
        e2e = {}
        for k in [0] + ks:
            model._spec_cfg = spec(k) if k else None
            model.generate_one(ids, ser, lens, 16, eos_token_id=None)             # graphs captured, caches warm
            before = model.spec_stats
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            toks = model.generate_one(ids, ser, lens, args.e2e_tokens, eos_token_id=None, sync_every=8)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            st = {n: model.spec_stats[n] - before[n] for n in before}
            e2e[str(k)] = {"tokens": len(toks), "seconds_incl_prefill": dt, "tokens_per_s_incl_prefill": len(toks) / dt,
                           "tokens_per_step": (st["emitted"] / st["steps"]) if st["steps"] else 1.0, **st}
        out["end_to_end_synthetic"] = e2e
    print(json.dumps(out))


if __name__ == "__main__":
    main()
