"""GPU: token logprobs (csrc/logprobs.hip, chatts_decoder_logprobs) from the kernel up through the model, the engine, LLM and the
server.  Reference: a float64 log_softmax of the same float32 logits; order (logit desc, id asc); rank 1-based in that order."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from chatts_amd import _lib, config as cfgmod, synth
from chatts_amd.modeling import ChatTSForCausalLM
from chatts_amd.processing import ChatTSProcessor
from oracle import pipeline, synth as osynth
from tests.util import chat_prompt, random_walk_series

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _st():
    return torch.cuda.current_stream().cuda_stream


def _logits(rng, batch, V):
    """float32 logits with planted exact ties (at the top and in the middle), -inf entries and large magnitudes"""
    x = (rng.standard_normal((batch, V)) * 3.0).astype(np.float32)
    for b in range(batch):
        idx = rng.choice(V, 12, replace=False)
        x[b, idx[:3]] = 60.0 + b                        # a three-way tie of the maximum
        x[b, idx[3:6]] = x[b, idx[6]]                   # a tie in the middle
        x[b, idx[7:9]] = -np.inf
        x[b, idx[9]] = -1.0e4
        x[b, idx[10]] = 45.5
    return x


def _ref(row, tok, k):
    l = row.astype(np.float64)
    m = l.max()
    lse = m + np.log(np.exp(l - m).sum())
    lp = l - lse
    order = np.lexsort((np.arange(len(l)), -l))
    rank = 1 + int((l > l[tok]).sum()) + int((l[:tok] == l[tok]).sum())
    return lp, order[:k], rank


def _close(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    fin = np.isfinite(want)
    assert np.array_equal(np.isfinite(got), fin) and np.array_equal(got[~fin], want[~fin])
    assert np.all(np.abs(got[fin] - want[fin]) <= 1e-5 + 1e-7 * np.abs(want[fin])), np.abs(got - want).max()


def _run(lib, x, tokens, steps, k, out_stride, vocab_offset=0, graph=False):
    b, V = x.shape
    lg = torch.from_numpy(x).to(DEV)
    tok = torch.tensor(tokens, dtype=torch.int64, device=DEV)
    step = torch.tensor(steps, dtype=torch.int32, device=DEV)
    lp = torch.full((b, out_stride), float("nan"), device=DEV)
    rank = torch.full((b, out_stride), -1, dtype=torch.int32, device=DEV)
    kk = max(k, 1)
    tid = torch.full((b, out_stride, kk), -1, dtype=torch.int32, device=DEV)
    tlp = torch.full((b, out_stride, kk), float("nan"), device=DEV)
    ws = torch.zeros(int(lib.chatts_logprobs_workspace(b, k)), dtype=torch.uint8, device=DEV)
    stride = out_stride

    def call():
        _lib.check(lib.chatts_logprobs_batched(lg.data_ptr(), b, V, V, vocab_offset, k, tok.data_ptr(), step.data_ptr(), stride,
                                               lp.data_ptr(), rank.data_ptr(), tid.data_ptr() if k else None,
                                               tlp.data_ptr() if k else None, ws.data_ptr(), ws.numel(), _st()))
    if graph:
        call()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            call()
        lp.fill_(float("nan")); rank.fill_(-1); tid.fill_(-1); tlp.fill_(float("nan"))     # back to the canaries: the replay must write
        g.replay()
    else:
        call()
    torch.cuda.synchronize()
    return lp.cpu().numpy(), rank.cpu().numpy(), tid.cpu().numpy()[..., :k], tlp.cpu().numpy()[..., :k]


@pytest.mark.parametrize("V", [4096, 19008, 151936, 152064])
@pytest.mark.parametrize("batch,k", [(1, 0), (3, 5), (16, 20), (3, 1)])
def test_kernel_matches_float64_log_softmax(lib, V, batch, k):
    rng = np.random.default_rng(V + 7 * batch + k)
    x = _logits(rng, batch, V)
    out_stride = 6
    tokens, steps = [], []
    for b in range(batch):
        kind = b % 4
        if kind == 0:
            t = int(np.lexsort((np.arange(V), -x[b].astype(np.float64)))[0])     # the greedy token: rank 1
        elif kind == 1:
            t = int(np.flatnonzero(x[b] == 60.0 + b)[-1])                       # the last member of the tie at the top: rank 3
        else:
            t = int(rng.integers(V))
        tokens.append(t)
        steps.append(int(rng.integers(1, out_stride + 1)))
    if batch >= 3:
        steps[-1] = out_stride + 1        # cell == out_stride: nothing written
        steps[-2] = 0                     # a row whose counter was never bumped: nothing written
    lp, rank, tid, tlp = _run(lib, x, tokens, steps, k, out_stride)
    for b in range(batch):
        cell = steps[b] - 1
        mask = np.ones(out_stride, bool)
        if 0 <= cell < out_stride:
            mask[cell] = False
        assert np.all(np.isnan(lp[b][mask])) and np.all(rank[b][mask] == -1)
        if k:
            assert np.all(tid[b][mask] == -1) and np.all(np.isnan(tlp[b][mask]))
        if not 0 <= cell < out_stride:
            continue
        want_lp, want_ids, want_rank = _ref(x[b], tokens[b], k)
        _close([lp[b, cell]], [want_lp[tokens[b]]])
        assert rank[b, cell] == want_rank
        if b % 4 == 0:
            assert want_rank == 1
        if b % 4 == 1:
            assert want_rank == 3
        if k:
            assert tid[b, cell].tolist() == want_ids.tolist()
            _close(tlp[b, cell], want_lp[want_ids])


def test_kernel_vocab_offset_determinism_and_graph(lib):
    rng = np.random.default_rng(5)
    V, off, k = 19008, 3 * 19008, 20
    x = _logits(rng, 3, V)
    tokens = [off + int(rng.integers(V)) for _ in range(3)]
    a = _run(lib, x, tokens, [1, 2, 3], k, 4, vocab_offset=off)
    b = _run(lib, x, tokens, [1, 2, 3], k, 4, vocab_offset=off)
    g = _run(lib, x, tokens, [1, 2, 3], k, 4, vocab_offset=off, graph=True)
    for u, v, w in zip(a, b, g):
        assert np.array_equal(u.view(np.uint8), v.view(np.uint8)) and np.array_equal(u.view(np.uint8), w.view(np.uint8))
    lp, rank, tid, tlp = a
    for r in range(3):
        want_lp, want_ids, want_rank = _ref(x[r], tokens[r] - off, k)
        _close([lp[r, r]], [want_lp[tokens[r] - off]])
        assert rank[r, r] == want_rank
        assert (tid[r, r] - off).tolist() == want_ids.tolist()


# ---- model ---------------------------------------------------------------------------------------------------------------------------
def _setup(preset, lengths, seed=3, **kw):
    cfg = cfgmod.preset(preset)
    proc = ChatTSProcessor.from_pretrained(cfg)
    rng = np.random.default_rng(1234)
    series = [random_walk_series(rng, L) for L in lengths]
    inputs = proc(text=[chat_prompt(lengths)], timeseries=series, padding=True, return_tensors="pt")
    model = ChatTSForCausalLM.from_synthetic(cfg, seed=seed, max_ctx=512, max_prefill_tokens=512, **kw)
    sd = osynth.state_dict(synth.all_specs(cfg), seed)
    return cfg, proc, inputs, model, sd


def _log_softmax64(lg):
    l = np.asarray(lg, np.float64)
    m = l.max()
    return l - (m + np.log(np.exp(l - m).sum()))


def _check_vs_oracle(entries, toks, oracle_logits, k):
    for step, (tok, (lp, rank, top)) in enumerate(zip(toks, entries)):
        ref = _log_softmax64(oracle_logits[step].numpy())
        assert abs(lp - ref[tok]) <= 2e-3, (step, lp, ref[tok])
        assert len(top) == k
        order = np.lexsort((np.arange(len(ref)), -ref))
        for j, (i, v) in enumerate(top):
            assert abs(v - ref[i]) <= 2e-3
            if i != order[j]:          # ids compared exactly except among oracle logits within 1e-3 of each other
                assert abs(ref[i] - ref[order[j]]) <= 1e-3, (step, j, i, order[j])


@pytest.mark.parametrize("preset,lengths", [("tiny-qwen2", [100, 40]), ("tiny-qwen3", [64, 17])])
def test_model_greedy_logprobs_bitwise_tokens_and_oracle(preset, lengths):
    # (prefix caching off: a repeated prompt would otherwise prefill fewer rows, which changes the logits' last bits by itself)
    cfg, proc, inputs, model, sd = _setup(preset, lengths, enable_prefix_caching=False)
    ids = inputs["input_ids"][0].tolist()
    ser = inputs["timeseries"].cuda()
    new = 10
    base_toks, base_logits = model.generate_one(ids, ser, proc.last_lengths, new, return_logits=True)
    toks, logits0, entries = model.generate_one(ids, ser, proc.last_lengths, new, return_logits=True, logprobs=5)
    assert toks == base_toks and torch.equal(logits0, base_logits)
    assert model._logprobs_on and len(entries) == len(toks)
    for tok, (lp, rank, top) in zip(toks, entries):
        assert rank == 1 and top[0][0] == tok and top[0][1] == lp
        assert all(top[j][1] >= top[j + 1][1] for j in range(len(top) - 1))
    want = pipeline.generate(cfg, sd, ids, inputs["timeseries"].numpy(), new)
    assert want["tokens"] == toks
    _check_vs_oracle(entries, toks, want["logits"], 5)
    # eager and graph give the same entries; switching off restores the plain steps
    model.use_graph = False
    assert model.generate_one(ids, ser, proc.last_lengths, new, logprobs=5) == (toks, entries)
    model.use_graph = True
    model.set_logprobs(False)
    assert model.generate_one(ids, ser, proc.last_lengths, new) == base_toks


def test_model_sampled_logprobs_teacher_forced():
    cfg, proc, inputs, model, sd = _setup("tiny-qwen2", [100, 40])
    ids = inputs["input_ids"][0].tolist()
    ser = inputs["timeseries"].cuda()
    new = 12
    model.set_sampling(0.8, 0, 0.95, seed=21)
    plain = model.generate_one(ids, ser, proc.last_lengths, new)
    toks, entries = model.generate_one(ids, ser, proc.last_lengths, new, logprobs=3)
    assert toks == plain and len(entries) == new
    want = pipeline.generate(cfg, sd, ids, inputs["timeseries"].numpy(), new, forced_tokens=toks)
    _check_vs_oracle(entries, toks, want["logits"], 3)


# ---- engine / LLM --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("llm_kw", [{}, {"kv_cache_dtype": "fp16"}, {"block_size": 64}], ids=["f32", "kv_fp16", "paged"])
def test_engine_mixed_batch_logprobs(llm_kw):
    from chatts_amd import LLM, SamplingParams
    from chatts_amd.engine import Engine
    cfg = cfgmod.preset("tiny-qwen2")
    llm = LLM(cfg, max_model_len=512, seed=3, max_num_seqs=4, **llm_kw)
    rng = np.random.default_rng(9)
    shared = [random_walk_series(rng, 64).tolist()]
    prompts = [(chat_prompt([64]), shared), (chat_prompt([30]), [random_walk_series(rng, 30).tolist()]),
               (chat_prompt([17]), [random_walk_series(rng, 17).tolist()]), (chat_prompt([64]), shared),
               (chat_prompt([40]), [random_walk_series(rng, 40).tolist()])]
    # (prompt, sampling, logprobs): greedy / sampled, with / without; prompt 3 repeats prompt 0 (a prefix-reuse hit)
    plan = [(0, {}, 4), (1, {}, None), (2, dict(temperature=0.8, top_p=0.95, seed=5), 2), (3, {}, 0),
            (4, dict(temperature=0.8, top_p=0.95, seed=6), None), (1, {}, 3)]

    def run(with_lp, stop=None):
        eng = Engine(llm.model, llm.processor, sync_every=3)
        reqs = []
        for i, (p, samp, k) in enumerate(plan):
            kw = dict(samp)
            if with_lp and k is not None:
                kw["logprobs"] = k
            if i == 5 and stop is not None:
                kw["stop_token_ids"] = [stop]
            reqs.append(eng.add_request(prompts[p][0], prompts[p][1], max_tokens=8, ignore_eos=True, **kw))
        eng.run_until_done()
        assert all(r.error is None for r in reqs), [r.error for r in reqs]
        return reqs

    base = run(False)
    stop = base[5].tokens[3]                      # cut request 5 after its fourth token
    cut_at = base[5].tokens.index(stop) + 1
    reqs = run(True, stop)
    assert llm.model.prefix_stats["hits"] > 0
    for i, (r, b) in enumerate(zip(reqs, base)):
        want = b.tokens[:cut_at] if i == 5 else b.tokens
        assert r.tokens == want, i
        k = plan[i][2]
        if k is None:
            assert r.logprobs is None and r.cumulative_logprob is None
            continue
        assert len(r.logprobs) == len(r.tokens)
        assert r.cumulative_logprob == pytest.approx(sum(e[0] for e in r.logprobs), abs=1e-6)
        for tok, (lp, rank, top) in zip(r.tokens, r.logprobs):
            assert len(top) == k and lp <= 0.0 and rank >= 1
            if not plan[i][1]:
                assert rank == 1
                if k:
                    assert top[0][0] == tok
    # LLM surface: SamplingParams(logprobs=k) -> CompletionOutput.logprobs / cumulative_logprob
    outs = llm.generate([{"prompt": prompts[0][0], "multi_modal_data": {"timeseries": prompts[0][1]}}],
                        SamplingParams(max_tokens=8, ignore_eos=True, logprobs=2))
    o = outs[0].outputs[0]
    assert o.token_ids == base[0].tokens and len(o.logprobs) == len(o.token_ids)
    for tok, d, e in zip(o.token_ids, o.logprobs, reqs[0].logprobs):
        assert tok in d and d[tok].rank == 1 and abs(d[tok].logprob - e[0]) <= 2e-3
    assert o.cumulative_logprob == pytest.approx(sum(d[t].logprob for t, d in zip(o.token_ids, o.logprobs)), abs=1e-5)
    plain = llm.generate([{"prompt": prompts[0][0], "multi_modal_data": {"timeseries": prompts[0][1]}}], SamplingParams(max_tokens=8, ignore_eos=True))
    assert plain[0].outputs[0].logprobs is None and plain[0].outputs[0].token_ids == o.token_ids
    with pytest.raises(ValueError, match="max_logprobs"):
        llm.generate([prompts[0][0]], SamplingParams(max_tokens=2, logprobs=21))


# ---- server --------------------------------------------------------------------------------------------------------------------------
def _sse(resp):
    events = [line[6:] for line in resp.iter_lines() if line.startswith("data: ")]
    assert events[-1] == "[DONE]"
    return [json.loads(e) for e in events[:-1]]


def _same_entries(a, b):
    """the streamed request repeats the blocking one's prompt: it reuses its cached prefix, so values agree to rounding, tokens exactly"""
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x["token"] == y["token"] and x["bytes"] == y["bytes"] and abs(x["logprob"] - y["logprob"]) <= 1e-4
        assert [t["token"] for t in x["top_logprobs"]] == [t["token"] for t in y["top_logprobs"]]
        assert np.allclose([t["logprob"] for t in x["top_logprobs"]], [t["logprob"] for t in y["top_logprobs"]], atol=1e-4, rtol=0)


def test_server_logprobs_blocking_and_streamed():
    from starlette.testclient import TestClient
    from chatts_amd import server
    cfg = cfgmod.preset("tiny-qwen2")
    app = server.build_server(cfg, max_model_len=512, max_num_seqs=2, seed=3)
    try:
        client = TestClient(app)
        rng = np.random.default_rng(2)
        ts = random_walk_series(rng, 40).tolist()
        msgs = [{"role": "user", "content": [{"type": "text", "text": "Describe <ts><ts/>"}, {"timeseries": ts}]}]
        body = {"model": "chatts", "max_tokens": 6, "ignore_eos": True, "messages": msgs, "logprobs": True, "top_logprobs": 3}
        d = client.post("/v1/chat/completions", json=body).json()
        content = d["choices"][0]["logprobs"]["content"]
        assert len(content) == len(d["token_ids"]) == 6
        for e in content:
            assert len(e["top_logprobs"]) == 3 and e["top_logprobs"][0]["logprob"] == e["logprob"] and e["logprob"] <= 0
        with client.stream("POST", "/v1/chat/completions", json=dict(body, stream=True)) as resp:
            chunks = _sse(resp)
        streamed = [e for c in chunks for e in (c["choices"][0].get("logprobs") or {}).get("content", [])]
        _same_entries(streamed, content)
        cbody = {"model": "chatts", "prompt": "Describe <ts><ts/>", "multi_modal_data": {"timeseries": [ts]}, "max_tokens": 5,
                 "ignore_eos": True, "logprobs": 2}
        d = client.post("/v1/completions", json=cbody).json()
        lp = d["choices"][0]["logprobs"]
        assert len(lp["tokens"]) == len(lp["token_logprobs"]) == len(lp["top_logprobs"]) == len(lp["text_offset"]) == 5
        assert all(len(t) <= 2 for t in lp["top_logprobs"]) and lp["text_offset"][0] == 0
        with client.stream("POST", "/v1/completions", json=dict(cbody, stream=True)) as resp:
            chunks = _sse(resp)
        parts = [c["choices"][0]["logprobs"] for c in chunks if c["choices"][0].get("logprobs")]
        joined = {k: [x for p in parts for x in p[k]] for k in lp}
        assert joined["tokens"] == lp["tokens"] and joined["text_offset"] == lp["text_offset"]
        assert [sorted(d) for d in joined["top_logprobs"]] == [sorted(d) for d in lp["top_logprobs"]]
        assert np.allclose(joined["token_logprobs"], lp["token_logprobs"], atol=1e-4, rtol=0)
        assert client.post("/v1/completions", json=dict(cbody, logprobs=21)).status_code == 400
    finally:
        app.state.engine_thread.close()


# ---- tensor parallel -----------------------------------------------------------------------------------------------------------------
DRIVER = r"""
import json, sys
import numpy as np
sys.path.insert(0, {root!r})
sys.path.insert(0, {root!r} + "/tests")
from chatts_amd import LLM, SamplingParams
from util import chat_prompt, random_walk_series
if __name__ == "__main__":
    llm = LLM("tiny-qwen3", tensor_parallel_size={world}, max_model_len=512, seed=3)
    rng = np.random.default_rng(1234)
    lengths = [64, 30]
    series = [random_walk_series(rng, L) for L in lengths]
    req = [{{"prompt": chat_prompt(lengths), "multi_modal_data": {{"timeseries": [s.tolist() for s in series]}}}}]
    o = llm.generate(req, sampling_params=SamplingParams(max_tokens=6, ignore_eos=True, logprobs=3))[0].outputs[0]
    lps = [[(int(i), float(d[i].logprob), d[i].rank) for i in sorted(d)] for d in o.logprobs]
    llm.shutdown()
    print("RESULT " + json.dumps(dict(tokens=o.token_ids, lps=lps)), flush=True)
"""


def _tp_run(world):
    env = dict(os.environ)
    env.update(HSA_ENABLE_IPC_MODE_LEGACY="0", CHATTS_FORCE_DEVICE="0", CHATTS_DIST_BACKEND="gloo", OMP_NUM_THREADS="8")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, "-c", DRIVER.format(root=ROOT, world=world)], env=env, cwd=ROOT, capture_output=True, text=True,
                       timeout=600)
    lines = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
    assert lines, f"rc={r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-3000:]}"
    return json.loads(lines[-1][7:])


def test_tp2_logprobs_match_tp1():
    one, two = _tp_run(1), _tp_run(2)
    assert one["tokens"] == two["tokens"]
    for a, b in zip(one["lps"], two["lps"]):
        assert [x[0] for x in a] == [x[0] for x in b] and [x[2] for x in a] == [x[2] for x in b]
        assert all(abs(x[1] - y[1]) <= 2e-3 for x, y in zip(a, b))
