#!/usr/bin/env python
"""A/B of token logprobs (set_logprobs, K = max_logprobs = 20): decode step time with logprobs off vs on, interleaved (off on off on ...),
on one model, plus the two logprob launches alone (chatts_logprobs_batched on [batch, vocab] logits).

    python tools/logprobs_ab.py --model chatts-14b --batch 1 --out profiles/logprobs_ab_b1.json            # the headline's model, batch 1
    python tools/logprobs_ab.py --model chatts-14b --weight-format fp8 --batch 16 --out ...                  # config 5's shape

The prompt is a text prompt of --prompt-tokens synthetic ids (the decode step's cost depends on the context length, not on where the
prompt rows came from).  Step times are graph replays timed with device events; one --steps window per round and mode.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="chatts-14b")
    ap.add_argument("--weight-format", default="bf16")
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--prompt-tokens", type=int, default=200)
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from chatts_amd import _lib, config as cfgmod
    from chatts_amd.modeling import ChatTSForCausalLM
    cfg = cfgmod.preset(args.model)
    B = args.batch
    max_ctx = args.prompt_tokens + args.steps * (2 * args.rounds + 2) + 64
    model = ChatTSForCausalLM.from_synthetic(cfg, seed=0, max_ctx=max_ctx, max_prefill_tokens=max(args.prompt_tokens, B), max_batch=B,
                                             weight_format=args.weight_format)
    ids = [(7 * i + 11) % 1000 + 100 for i in range(args.prompt_tokens)]
    if B == 1:
        model._prefill_request(ids, None, None, max_ctx - args.prompt_tokens)
        step = model.decode_step
    else:
        model.buf["pos_all"].fill_(-1)
        for s in range(B):
            model._admit(s, ids, None, None, max_ctx - args.prompt_tokens)
        step = model.batched_step
    times = {"off": [], "on": []}
    for _ in range(args.rounds):
        for mode in ("off", "on"):
            model.set_logprobs(mode == "on")
            for _ in range(4):                       # capture + warm
                step()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.steps):
                step()
            e1.record()
            torch.cuda.synchronize()
            times[mode].append(e0.elapsed_time(e1) / args.steps)
    # the two logprob launches alone, on logits of the model's shape
    lib = _lib.load()
    V, K = cfg.vocab_size, model.max_logprobs
    lg = torch.randn((B, V), device="cuda") * 3
    tok = torch.zeros(B, dtype=torch.int64, device="cuda")
    stp = torch.ones(B, dtype=torch.int32, device="cuda")
    lp = torch.empty((B, 4), device="cuda")
    rk = torch.empty((B, 4), dtype=torch.int32, device="cuda")
    tid = torch.empty((B, 4, K), dtype=torch.int32, device="cuda")
    tlp = torch.empty((B, 4, K), device="cuda")
    wsb = int(lib.chatts_logprobs_workspace(B, K))
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
    s = _lib.stream_ptr()

    def call():
        _lib.check(lib.chatts_logprobs_batched(lg.data_ptr(), B, V, V, 0, K, tok.data_ptr(), stp.data_ptr(), 4, lp.data_ptr(),
                                               rk.data_ptr(), tid.data_ptr(), tlp.data_ptr(), ws.data_ptr(), wsb, s))
    for _ in range(20):
        call()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(200):
        call()
    e1.record()
    torch.cuda.synchronize()
    alone_us = e0.elapsed_time(e1) / 200 * 1e3
    off, on = statistics.median(times["off"]), statistics.median(times["on"])
    res = {"model": args.model, "weight_format": args.weight_format, "batch": B, "prompt_tokens": args.prompt_tokens, "k": K,
           "step_ms_off": times["off"], "step_ms_on": times["on"], "median_ms_off": off, "median_ms_on": on,
           "added_pct": 100.0 * (on - off) / off, "logprob_launches_alone_us": alone_us}
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
