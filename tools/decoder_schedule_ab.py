#!/usr/bin/env python
"""The decoder schedule (csrc/decoder.hip) end to end, for a bitwise A/B of two builds and for a pass-state check inside one:

    python tools/decoder_schedule_ab.py [--presets tiny-qwen2,tiny-qwen3] [--caches f32,f32-paged64,fp16,fp16-paged64] > new.jsonl
    CHATTS_AMD_LIB=/path/to/another/libchatts_amd.so python tools/decoder_schedule_ab.py ... > old.jsonl      # the same calls, another build
    python tools/decoder_schedule_ab.py --compare old.jsonl new.jsonl          # every digest key of round 1, equal or not
    rocprofv3 --kernel-trace -d OUT -- python tools/decoder_schedule_ab.py --presets tiny-qwen2 --caches f32      (once per build)
    python tools/decoder_schedule_ab.py --trace-diff OLD.db NEW.db             # ordered (kernel, grid, workgroup) lists, equal or not

Synthetic tiny models, every schedule entry point at the smallest shapes that reach each of its branches (STAGES below says which).
After each stage one JSON line of SHA-256 digests of x, the logits, the chosen tokens and the KV cache (zeroed when the stage starts,
so the digest covers the rows the stage touched and shows a stray write as well).  The whole list runs twice in one process on the same
model objects, with reset() between: the last line says whether round 2 equals round 1 key by key - state that one entry point leaves
behind for the next shows there.  Everything is enqueued eagerly, one C call per entry point.  run() is the importable form
(tests/test_gpu_decoder_schedule.py)."""
import argparse
import hashlib
import json
import os
import sqlite3
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CACHES = {"f32": dict(kv_block_size=None, kv_cache_dtype=None), "f32-paged64": dict(kv_block_size=64, kv_cache_dtype=None),
          "fp16": dict(kv_block_size=None, kv_cache_dtype="fp16"), "fp16-paged64": dict(kv_block_size=64, kv_cache_dtype="fp16")}
POS0 = 7                       # every chunk starts behind a 7-row chunk of the same sequence
PACKED = ((40, 0), (1, 0), (70, 5))            # (rows, pos0) of the three packed segments, cache slots 0, 1, 2
SPEC_K = 4

# model name -> constructor arguments; stage -> (model, function name, arguments).  What each shape is for:
#   prefill 1 / 5 / 16 / 97 / 260: the GEMV path, the small-M GEMM, the attention-written planes threshold, the plane path from 96 rows with
#   the fused post-norm, the >= 256 rule of the key split;  batched 3 / 16: the ping-pong and the next projection's 8-bit flag
MODELS = {
    "one": dict(max_batch=1, speculative_config={"method": "ngram", "num_speculative_tokens": SPEC_K}),
    "one-int4": dict(max_batch=1, weight_format="int4"),
    "b3": dict(max_batch=3), "b16": dict(max_batch=16),
    "b3-fp8": dict(max_batch=3, weight_format="fp8"), "b16-fp8": dict(max_batch=16, weight_format="fp8"),
    "b3-fp8speed": dict(max_batch=3, weight_format="fp8", precision="fp8"),
    "b3-f16q": dict(max_batch=3, precision="f16q"),
}
STAGES = [
    *[(f"prefill{t}", "one", "prefill", dict(t=t)) for t in (1, 5, 16, 97, 260)],
    ("prefill_last97", "one", "prefill", dict(t=97, last=True)),
    ("decode8", "one", "decode", dict(steps=8)),
    ("spec4", "one", "spec", dict(steps=4)),
    ("select", "one", "select", {}),
    ("int4.prefill_last97", "one-int4", "prefill", dict(t=97, last=True)),
    ("int4.decode8", "one-int4", "decode", dict(steps=8)),
    ("packed", "b3", "packed", {}),
    ("batched3x8", "b3", "batched", dict(steps=8)),
    ("batched16x1", "b16", "batched", dict(steps=1)),
    ("fp8.batched3x8", "b3-fp8", "batched", dict(steps=8)),
    ("fp8.batched16x1", "b16-fp8", "batched", dict(steps=1)),
    ("fp8speed.prefill_last97", "b3-fp8speed", "prefill", dict(t=97, last=True)),
    ("fp8speed.packed", "b3-fp8speed", "packed", {}),
    ("f16q.prefill97", "b3-f16q", "prefill", dict(t=97)),
    ("f16q.prefill128", "b3-f16q", "prefill", dict(t=128)),
    ("f16q.packed", "b3-f16q", "packed", {}),          # (the attention half falls back to the default kernels)
]
# the list tests/test_gpu_decoder_schedule.py runs (bf16 weights)
REDUCED = [
    ("prefill97", "one", "prefill", dict(t=97)),
    ("prefill_last97", "one", "prefill", dict(t=97, last=True)),
    ("packed", "b3", "packed", {}),
    ("decode4", "one", "decode", dict(steps=4)),
    ("batched3x4", "b3", "batched", dict(steps=4)),
    ("spec2", "one", "spec", dict(steps=2)),
    ("f16q.prefill97", "b3-f16q", "prefill", dict(t=97)),
]


def digest(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


class Driver:
    """one synthetic model and the stage functions; each returns {key: digest or token list}"""

    def __init__(self, preset, cache, request, **kw):
        import torch
        from chatts_amd import _lib
        from chatts_amd.modeling import ChatTSForCausalLM
        self.torch, self._lib = torch, _lib
        self.m = ChatTSForCausalLM.from_synthetic(preset, seed=3, max_ctx=512, max_prefill_tokens=512, use_graph=False,
                                                  enable_prefix_caching=False, max_logprobs=3, **CACHES[cache], **kw)
        self.request = request
        g = torch.Generator().manual_seed(11)
        self.emb = (torch.randn((300, self.m.config.hidden_size), generator=g) * 0.05).cuda()

    def begin(self):
        m = self.m
        m.reset()
        m.buf["pos_all"].zero_()
        m.buf["step_all"].zero_()
        m.buf["kv_k"].zero_()
        m.buf["kv_v"].zero_()
        m.select_sequence(0)

    def kv(self):
        return {"kv_k": digest(self.m.buf["kv_k"]), "kv_v": digest(self.m.buf["kv_v"])}

    def logits(self, row):
        return digest(self.m.compute_logits(row=row))

    def prefill(self, t, last=False):
        """POS0 rows, then t rows behind them: chatts_decoder_prefill, or chatts_decoder_prefill_last (the result is row 0 then)"""
        self.begin()
        self.m.prefill(self.emb[:POS0], 0)
        rows = self.m.prefill(self.emb[POS0:POS0 + t], POS0, for_next_token=last)
        assert rows == (1 if last else t)
        return {"x": digest(self.m.buf["x"][:rows]), "logits": self.logits(rows - 1), **self.kv()}

    def _admit(self, steps):
        ids, series, lengths = self.request
        self.begin()
        return self.m._prefill_request(ids, series, lengths, steps + 1)           # prefill_last + the first token

    def decode(self, steps):
        """a real prompt, its first token, then `steps` calls of chatts_decoder_decode_step"""
        m, out = self.m, {}
        self._admit(steps)
        for i in range(steps):
            m._decode_step_eager()
            out[f"logits{i}"] = digest(m.buf["logits"])
        out["tokens"] = m.buf["out_tokens"][:steps + 1].tolist()
        return {**out, "x": digest(m.buf["x"][:1]), "pos": m.buf["pos"].tolist(), **self.kv()}

    def spec(self, steps):
        """the same request, then `steps` calls of chatts_decoder_spec_step with k = SPEC_K (the proposer inside the step)"""
        m, out = self.m, {}
        self._admit(steps * (SPEC_K + 1))
        assert m._spec_active
        m.spec_stats_reset()
        for i in range(steps):
            m._spec_step_eager(propose_in_step=True)
            out[f"logits{i}"] = digest(m.buf["spec_logits"][:SPEC_K + 1])
        n = int(m.buf["step"][0])
        out["tokens"] = m.buf["out_tokens"][:n].tolist()
        return {**out, "x": digest(m.buf["x"][:SPEC_K + 1]), "pos": m.buf["pos"].tolist(), "counters": m.buf["spec_counters"].tolist(), **self.kv()}

    def select(self):
        """one logits row -> greedy, sampled, with logit controls, and the logprobs (k = 3) of the greedy choice"""
        m, B, out = self.m, self.m.buf, {}
        self.begin()
        rows = m.prefill(self.emb[:97], 0, for_next_token=True)
        m.compute_logits(row=rows - 1)

        def pick(name, sampling=None):
            B["step"].zero_()
            m._select_one(0, 0, sampling)
            out[name] = [B["token"].tolist(), digest(B["token_logit"]), B["out_tokens"][:1].tolist(), B["step"].tolist()]

        pick("greedy")
        pick("sampled", self._lib.SamplingArgs(temperature=0.7, top_k=20, top_p=0.9, seed=99))
        m.set_slot_controls(0, repetition_penalty=1.3, frequency_penalty=0.2, presence_penalty=0.1, min_p=0.05)
        m._controls_admit(0, list(range(0, 4096, 5)))
        pick("controlled")
        pick("controlled_again")          # (the state counted the first choice)
        out["control_state"] = digest(B["lc_state"])
        m.set_logit_controls(False)
        m.set_logprobs(True)
        pick("greedy_logprobs")
        R = m._logprob_rings()
        out["logprobs"] = [digest(R[k][0, :2]) for k in ("lp", "rank", "top_ids", "top_lp")]
        m.set_logprobs(False)
        return out

    def packed(self):
        """chatts_decoder_prefill_packed: three prompts in one pass, the third behind rows of an earlier chunk of its slot"""
        m = self.m
        self.begin()
        segs, row = [], 0
        for slot, (t, pos0) in enumerate(PACKED):
            if pos0:
                m.select_sequence(slot)
                m.prefill(self.emb[200:200 + pos0], 0)
            m.reserve_kv(slot, pos0 + t + 8)
            segs.append(self._lib.PrefillSegment(row0=row, t=t, pos0=pos0, slot=slot))
            row += t
        m.select_sequence(0)
        m.buf["x"][:row].copy_(self.emb[:row])
        arr = (self._lib.PrefillSegment * len(segs))(*segs)
        self._lib.check(m.lib.chatts_decoder_prefill_packed(m._decoder, arr, len(segs), self._lib.stream_ptr()))
        out = {"x": digest(m.buf["x"][:row]), **self.kv()}
        for sg in segs:
            out[f"logits_slot{sg.slot}"] = self.logits(sg.row0 + sg.t - 1)
        return out

    def batched(self, steps):
        """every slot prefilled with a prompt of its own length, then `steps` calls of chatts_decoder_decode_step_batched"""
        m, B, out = self.m, self.m.buf, {}
        self.begin()
        for slot in range(m.max_batch):
            n = 9 + slot
            m.select_sequence(slot)
            m.prefill(self.emb[slot:slot + n], 0)
            B["pos_all"][slot] = n
            B["token_all"][slot] = 17 + 3 * slot
        m.select_sequence(0)
        for i in range(steps):
            m._batched_step_eager()
            out[f"logits{i}"] = digest(B["logits_all"])
        out["tokens"] = B["out_tokens_all"][:, :steps].tolist()
        return {**out, "x": digest(B["x"][:m.max_batch]), "pos": B["pos_all"].tolist(), **self.kv()}


def build_request(preset):
    """a short chat prompt with three series -> (ids, series tensor, valid lengths, timeseries as numpy for the oracle)"""
    import bench
    from chatts_amd import config as cfgmod
    cfg = cfgmod.preset(preset)
    proc, prompt, series, _ = bench.build_inputs(cfg, n_series=3, length=64)
    inputs = proc(text=[prompt], timeseries=series, padding=True, return_tensors="pt")
    return cfg, inputs["input_ids"][0].tolist(), inputs["timeseries"], list(proc.last_lengths)


def run(preset="tiny-qwen2", cache="f32", stages=None, rounds=2, emit=None):
    """Run `stages` (default: STAGES) `rounds` times on the same model objects.  -> {"rounds": [{key: value}] per round, "differs": keys
    on which a later round is not round 1, "request": (cfg, ids, timeseries) of the decode / spec stages' prompt}"""
    stages = STAGES if stages is None else stages
    cfg, ids, ts, lengths = build_request(preset)
    drivers, results = {}, []
    for r in range(rounds):
        res = {}
        for name, model, fn, kw in stages:
            if model not in drivers:
                drivers[model] = Driver(preset, cache, (ids, ts.cuda(), lengths), **MODELS[model])
            out = getattr(drivers[model], fn)(**kw)
            res.update({f"{preset}/{cache}/{name}/{k}": v for k, v in out.items()})
            if emit:
                emit({"round": r + 1, "preset": preset, "cache": cache, "stage": name, "digests": out})
        results.append(res)
    differs = sorted(k for res in results[1:] for k in results[0] if res.get(k) != results[0][k])
    return {"rounds": results, "differs": differs, "request": (cfg, ids, ts)}


def read_round1(path):
    keys = {}
    with open(path) as f:
        for line in f:
            if not line.startswith("{"):
                continue
            row = json.loads(line)
            if row.get("round") == 1:
                keys.update({f"{row['preset']}/{row['cache']}/{row['stage']}/{k}": v for k, v in row["digests"].items()})
    return keys


def compare(a, b):
    ka, kb = read_round1(a), read_round1(b)
    differs = sorted(k for k in set(ka) | set(kb) if ka.get(k) != kb.get(k))
    print(json.dumps({"a": a, "b": b, "keys": len(ka), "equal": not differs and len(ka) == len(kb),
                      "differs": {k: [ka.get(k), kb.get(k)] for k in differs}}))
    return 1 if differs else 0


def launches(db):
    q = "select name, grid_x, grid_y, grid_z, workgroup_x, workgroup_y, workgroup_z from kernels order by start"
    return sqlite3.connect(db).cursor().execute(q).fetchall()


def trace_diff(a, b):
    la, lb = launches(a), launches(b)
    first = next((i for i, (x, y) in enumerate(zip(la, lb)) if x != y), None)
    if first is None and len(la) != len(lb):
        first = min(len(la), len(lb))
    print(json.dumps({"a": a, "b": b, "launches": [len(la), len(lb)], "equal": first is None,
                      "first_difference": None if first is None else {"index": first, "a": la[first:first + 1], "b": lb[first:first + 1]}}))
    return 0 if first is None else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--presets", default="tiny-qwen2,tiny-qwen3")
    ap.add_argument("--caches", default=",".join(CACHES))
    ap.add_argument("--reduced", action="store_true", help="the test's short list instead of STAGES")
    ap.add_argument("--compare", nargs=2, metavar="JSONL")
    ap.add_argument("--trace-diff", nargs=2, metavar="DB")
    args = ap.parse_args()
    if args.compare:
        return compare(*args.compare)
    if args.trace_diff:
        return trace_diff(*args.trace_diff)
    from chatts_amd import _lib
    _lib.load()
    print(json.dumps({"lib": _lib.lib_path()}), flush=True)
    differs, keys = [], 0
    for preset in args.presets.split(","):
        for cache in args.caches.split(","):
            res = run(preset, cache, REDUCED if args.reduced else None, emit=lambda row: print(json.dumps(row), flush=True))
            differs += res["differs"]
            keys += len(res["rounds"][0])
    print(json.dumps({"keys": keys, "round2_equals_round1": not differs, "differs": differs}), flush=True)
    return 1 if differs else 0


if __name__ == "__main__":
    sys.exit(main())
