#!/usr/bin/env python
"""A/B of the logit masks (allowed_token_ids, logit_bias, min_tokens) against the PARENT COMMIT: decode step time of
  parent   the parent commit's tree (--parent DIR: a checkout of it with its library built),
  off      this tree, the feature never switched on (must equal the parent within the parent's own run-to-run spread),
  on       this tree, EVERY slot constrained: 1000 allowed ids, 16 bias entries, min_tokens beyond the run with 2 end ids,
interleaved (parent off on parent off on ...), every measurement in a fresh child process under its own time limit, plus the pass
alone (chatts_logit_masks_apply on [batch, vocab] logits with the same settings) beside its yardstick, the penalty pass
(chatts_logit_controls_apply without min_p: lc_apply_kernel alone) on the same logits in the same process.

    python tools/logit_masks_ab.py --parent /path/to/parent --model chatts-14b --batch 1                       # the headline's model
    python tools/logit_masks_ab.py --parent /path/to/parent --model chatts-14b --weight-format fp8 --batch 16 --prompt-tokens 1100

The prompt is a text prompt of --prompt-tokens synthetic ids.  Step times are graph replays timed with device events, one --steps
window per round.  A child that fails or runs out of time ends the run: nothing is retried.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _timed(torch, call, n=200):
    for _ in range(20):
        call()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        call()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


def child(args):
    sys.path.insert(0, os.path.abspath(args.tree))
    import torch
    from chatts_amd import _lib, config as cfgmod
    from chatts_amd.modeling import ChatTSForCausalLM
    cfg = cfgmod.preset(args.model)
    B, V = args.batch, cfg.vocab_size
    max_ctx = args.prompt_tokens + args.steps * (args.rounds + 1) + 64
    model = ChatTSForCausalLM.from_synthetic(cfg, seed=0, max_ctx=max_ctx, max_prefill_tokens=max(args.prompt_tokens, B), max_batch=B,
                                             weight_format=args.weight_format)
    allowed = [(151 * i + 7) % V for i in range(1000)]
    bias = {(977 * i + 3) % V: 1.5 - 0.25 * i for i in range(16)}
    if args.variant == "on":
        for s in range(B):
            model.set_slot_masks(s, logit_bias=bias, allowed_token_ids=allowed, min_tokens=max_ctx, end_ids=[allowed[0], allowed[1]])
        assert model._masks_on
    ids = [(7 * i + 11) % 1000 + 100 for i in range(args.prompt_tokens)]
    if B == 1:
        model._prefill_request(ids, None, None, max_ctx - args.prompt_tokens)
        step = model.decode_step
    else:
        model.buf["pos_all"].fill_(-1)
        for s in range(B):
            model._admit(s, ids, None, None, max_ctx - args.prompt_tokens)
        step = model.batched_step
    for _ in range(6):                               # capture + warm
        step()
    times = []
    for _ in range(args.rounds):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.steps):
            step()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) / args.steps)
    res = {"variant": args.variant, "step_ms": times}
    if args.variant == "off":
        assert not any(k.startswith("lm_") for k in model.buf)
    if args.variant == "on":                         # the pass alone and its yardstick, on logits of the model's shape
        import ctypes as C
        toks = model.buf["out_tokens_all"][:, :8].tolist()
        assert all(set(t) <= set(allowed[2:]) for t in toks), toks          # every row was constrained (and min_tokens kept the end ids away)
        lib = _lib.load()
        lg = torch.randn((B, V), device="cuda") * 3
        step_dev = torch.zeros(B, dtype=torch.int32, device="cuda")
        a = model._mask_args(0)
        s = _lib.stream_ptr()
        res["pass_alone_us"] = _timed(torch, lambda: _lib.check(lib.chatts_logit_masks_apply(lg.data_ptr(), B, V, V, 0, C.byref(a),
                                                                                             step_dev.data_ptr(), s)))
        st = torch.zeros((B, V), dtype=torch.int32, device="cuda")
        st[:, ::37] = (1 << 30) + 2
        out = torch.empty((B, V), device="cuda")
        rep = torch.full((B,), 1.3, dtype=torch.float32, device="cuda")
        ws = torch.empty(int(lib.chatts_logit_controls_workspace(B)), dtype=torch.uint8, device="cuda")
        c = _lib.LogitControlArgs(state=st.data_ptr(), state_stride=V, out=out.data_ptr(), out_stride=V, repetition_rows=rep.data_ptr())
        res["lc_apply_alone_us"] = _timed(torch, lambda: _lib.check(lib.chatts_logit_controls_apply(lg.data_ptr(), B, V, V, 0, C.byref(c),
                                                                                                   ws.data_ptr(), ws.numel(), s)))
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="chatts-14b")
    ap.add_argument("--weight-format", default="bf16")
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--prompt-tokens", type=int, default=200)
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=3, help="timed windows per child process")
    ap.add_argument("--repeats", type=int, default=3, help="child processes per variant")
    ap.add_argument("--parent", default=None, help="a checkout of the parent commit with its library built")
    ap.add_argument("--child-timeout", type=int, default=240)
    ap.add_argument("--out", default=None)
    ap.add_argument("--variant", default=None, help="(child) parent / off / on")
    ap.add_argument("--tree", default=ROOT, help="(child) the tree to import chatts_amd from")
    args = ap.parse_args()
    if args.variant:
        return child(args)
    variants = (["parent"] if args.parent else []) + ["off", "on"]
    runs = {v: [] for v in variants}
    alone, yard = [], []
    for _ in range(args.repeats):
        for v in variants:
            cmd = [sys.executable, os.path.abspath(__file__), "--variant", v, "--tree", args.parent if v == "parent" else ROOT,
                   "--model", args.model, "--weight-format", args.weight_format, "--batch", str(args.batch), "--prompt-tokens",
                   str(args.prompt_tokens), "--steps", str(args.steps), "--rounds", str(args.rounds)]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.child_timeout, cwd=ROOT)
            lines = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
            if r.returncode != 0 or not lines:
                sys.exit(f"child {v} failed (rc {r.returncode}); stopping\n{r.stdout[-1500:]}\n{r.stderr[-3000:]}")
            d = json.loads(lines[-1][7:])
            runs[v].append(statistics.median(d["step_ms"]))
            print(f"{v}: {d['step_ms']}", file=sys.stderr, flush=True)
            if "pass_alone_us" in d:
                alone.append(d["pass_alone_us"])
                yard.append(d["lc_apply_alone_us"])
    med = {v: statistics.median(t) for v, t in runs.items()}
    res = {"model": args.model, "weight_format": args.weight_format, "batch": args.batch, "prompt_tokens": args.prompt_tokens,
           "step_ms_per_process": runs, "median_ms": med, "pass_alone_us": alone, "lc_apply_alone_us": yard,
           "on_vs_off_pct": 100.0 * (med["on"] - med["off"]) / med["off"]}
    if args.parent:
        p = runs["parent"]
        res["parent_spread_pct"] = 100.0 * (max(p) - min(p)) / med["parent"]
        res["off_vs_parent_pct"] = 100.0 * (med["off"] - med["parent"]) / med["parent"]
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
