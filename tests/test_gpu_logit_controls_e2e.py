"""GPU: the logit controls end to end on small synthetic models: the engine's choices replayed by the float64 reference from the engine's
own raw logits, eager / captured / batched agreement, min_p = 1 as greedy decoding, defaults as today's engine, raw logprobs, slot
hygiene, LLM and server, tensor parallelism with two ranks.  Kernel level: tests/test_gpu_logit_controls.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from chatts_amd import config as cfgmod
from chatts_amd.modeling import ChatTSForCausalLM
from chatts_amd.processing import ChatTSProcessor
from tests import logit_controls_ref as ref
from tests.util import chat_prompt, random_walk_series

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PEN = dict(repetition_penalty=1.3, frequency_penalty=0.5, presence_penalty=0.5)
MODEL_SEED = 3


def _inputs(cfg, lengths, rng_seed=1234):
    proc = ChatTSProcessor.from_pretrained(cfg)
    rng = np.random.default_rng(rng_seed)
    series = [random_walk_series(rng, L) for L in lengths]
    inputs = proc(text=[chat_prompt(lengths)], timeseries=series, padding=True, return_tensors="pt")
    return inputs["input_ids"][0].tolist(), inputs["timeseries"].cuda(), list(proc.last_lengths)


def _model(preset="tiny-qwen2", **kw):
    cfg = cfgmod.preset(preset)
    kw.setdefault("enable_prefix_caching", False)      # (a repeated prompt would prefill fewer rows, which changes the logits' last bits by itself)
    return cfg, ChatTSForCausalLM.from_synthetic(cfg, seed=MODEL_SEED, max_ctx=512, max_prefill_tokens=512, **kw)


def test_replay_against_the_engines_own_raw_logits():
    """48 greedy steps with r = 1.3, f = 0.5, p = 0.5, eager: after every step the reference, given that step's raw logits row and the
    history so far, names the token the engine chose.  A step whose two best penalised reference logits are closer than the kernel's
    error bound for them may be left out (at most 1 in 48); MODEL_SEED / the prompt are such that the reference leaves out none.
    Then the same prompt through the captured step and through generate_batch at max_batch = 4 in slot 2 beside three requests with
    other settings: the same tokens."""
    cfg, model = _model(use_graph=False)
    ids, ser, lens = _inputs(cfg, [100, 40])
    V, n = cfg.vocab_size, 48
    plain = model.generate_one(ids, ser, lens, n)
    assert "lc_state" not in model.buf
    model.set_slot_controls(0, **PEN)
    model._prefill_request(ids, ser, lens, n)
    rows = [model.buf["logits"].cpu().numpy().copy()]
    for _ in range(n - 1):
        model.decode_step()
        rows.append(model.buf["logits"].cpu().numpy().copy())
    toks = model.buf["out_tokens"][:n].tolist()
    model.note_generated(0, toks)
    inp = ref.prompt_mask(ids, V)
    left_out, margins = 0, []
    for k in range(n):
        cnt = ref.counts_of(toks[:k], V)
        want, margin = ref.greedy(rows[k], inp, cnt, 1.3, 0.5, 0.5)
        pen = ref.penalise(rows[k], inp, cnt, 1.3, 0.5, 0.5)
        bound = ref.penalty_bound(rows[k], cnt, 1.3, 0.5, 0.5)
        two = np.argsort(pen)[-2:]
        slack = float(bound[two].sum())
        margins.append(margin - slack)
        print(f"step {k}: engine {toks[k]} reference {want} margin {margin:.3e} bound {slack:.3e} count of the token before {int(cnt[toks[k]])}")
        if margin <= slack:
            left_out += 1
            continue
        assert toks[k] == want, (k, toks[k], want)
    print(f"smallest margin minus bound: {min(margins):.3e}; left out {left_out}; tokens {toks}; unpenalised {plain}")
    assert left_out <= 1
    assert min(margins) > 0, min(margins)                   # (the choice of seed and prompt: the reference alone leaves out no step)
    assert toks != plain                                    # the penalties changed the text (the synthetic model repeats itself without them)
    # generate_one, eager and through the captured step
    assert model.generate_one(ids, ser, lens, n, controls=PEN) == toks
    model.use_graph = True
    assert model.generate_one(ids, ser, lens, n, controls=PEN) == toks
    assert model.generate_one(ids, ser, lens, n, controls=PEN) == toks          # replayed again: the state does not leak between requests
    assert model.generate_one(ids, ser, lens, n, controls={}) == plain          # mode on, the slot at its defaults
    assert list(model.generate_stream(ids, ser, lens, n, chunk=n, controls=PEN))[0] == toks
    del model
    # continuous batching: slot 2 of 4, beside a default request, a sampled min_p request and another penalty
    cfg, mb = _model(max_batch=4)
    others = [_inputs(cfg, [64, 17], 5), _inputs(cfg, [30], 6), _inputs(cfg, [80, 20, 10], 7)]
    reqs = [others[0], others[1], (ids, ser, lens), others[2]]
    ctl = [None, dict(repetition_penalty=2.0, presence_penalty=-1.0), PEN, dict(frequency_penalty=2.0, min_p=0.3)]
    outs = mb.generate_batch(reqs, n, eos_token_id=[], controls=ctl)
    assert outs[2] == toks
    assert mb.generate_batch(reqs[::-1], n, eos_token_id=[], controls=ctl[::-1])[1] == toks      # another slot, another order
    mb.use_graph = False
    assert mb.generate_batch(reqs, n, eos_token_id=[], controls=ctl)[2] == toks


def test_min_p_one_makes_sampling_greedy():
    cfg, model = _model()
    ids, ser, lens = _inputs(cfg, [64, 30])
    greedy = model.generate_one(ids, ser, lens, 32)
    for seed in (1, 22, 333):
        model.set_sampling(1.0, 0, 1.0, seed, min_p=0.0)
        assert model.generate_one(ids, ser, lens, 32) != greedy                   # (temperature 1 over the whole vocabulary: not the greedy text)
        model.set_sampling(1.0, 0, 1.0, seed, min_p=1.0)
        assert model.generate_one(ids, ser, lens, 32) == greedy, seed
    # HF generate: min_p only with do_sample, repetition_penalty with and without
    x = torch.tensor([ids])
    a = model.generate(input_ids=x, timeseries=ser, valid_lengths=lens, max_new_tokens=32, eos_token_id=[], do_sample=True, temperature=1.0,
                       top_k=0, seed=5, min_p=1.0)
    assert a[0, len(ids):].tolist() == greedy
    b = model.generate(input_ids=x, timeseries=ser, valid_lengths=lens, max_new_tokens=32, eos_token_id=[], min_p=1.0)
    assert b[0, len(ids):].tolist() == greedy
    c = model.generate(input_ids=x, timeseries=ser, valid_lengths=lens, max_new_tokens=32, eos_token_id=[], repetition_penalty=1.3)
    model.set_sampling(0.0)
    assert c[0, len(ids):].tolist() == model.generate_one(ids, ser, lens, 32, controls=dict(repetition_penalty=1.3)) != greedy


def test_defaults_are_todays_engine_and_logprobs_stay_raw():
    cfg, fresh = _model()
    ids, ser, lens = _inputs(cfg, [100, 40])
    n = 16
    base_toks, base_entries = fresh.generate_one(ids, ser, lens, n, logprobs=5)
    # all four at their defaults, given explicitly: the same tokens and logprobs, and nothing allocated
    toks, entries = fresh.generate_one(ids, ser, lens, n, logprobs=5, controls=dict(repetition_penalty=1.0, frequency_penalty=0.0,
                                                                                      presence_penalty=0.0, min_p=0.0))
    assert (toks, entries) == (base_toks, base_entries)
    fresh.set_sampling(0.0, repetition_penalty=1.0, min_p=0.0)
    fresh.set_slot_sampling(0, 0.0)
    assert not fresh._controls_on and not any(k.startswith("lc_") for k in fresh.buf)
    # the mode on, the slot at its defaults: still the same bits
    cfg, model = _model()
    model.set_logit_controls(True)
    assert (model.generate_one(ids, ser, lens, n, logprobs=5)) == (base_toks, base_entries)
    # logprobs stay log_softmax of the RAW logits while the selection sees the penalised ones
    model.use_graph = False
    model.set_slot_controls(0, repetition_penalty=1.5)
    model._prefill_request(ids, ser, lens, n)
    rows = [model.buf["logits"].cpu().numpy().copy()]
    for _ in range(n - 1):
        model.decode_step()
        rows.append(model.buf["logits"].cpu().numpy().copy())
    toks = model.buf["out_tokens"][:n].tolist()
    entries = model.read_logprobs(0, 0, n, 5)
    model.note_generated(0, toks)
    assert toks != base_toks
    not_first = 0
    for k, (tok, (lp, rank, top)) in enumerate(zip(toks, entries)):
        l = rows[k].astype(np.float64)
        lsm = l - (l.max() + np.log(np.exp(l - l.max()).sum()))
        assert abs(lp - lsm[tok]) <= 1e-5 + 1e-7 * abs(lsm[tok]), (k, lp, lsm[tok])       # (the kernel test's tolerance for this comparison)
        order = np.lexsort((np.arange(len(l)), -l))
        assert [i for i, _ in top] == order[:5].tolist()
        assert rank == 1 + int((l > l[tok]).sum()) + int((l[:tok] == l[tok]).sum())
        assert all(abs(v - lsm[i]) <= 1e-5 + 1e-7 * abs(lsm[i]) for i, v in top)
        not_first += rank != 1
    assert not_first > 0                                    # the penalty made the engine pass over the raw favourite at least once
    model.use_graph = True
    assert model.generate_one(ids, ser, lens, n, logprobs=5, controls=dict(repetition_penalty=1.5)) == (toks, entries)


def test_slot_hygiene_with_prefix_reuse():
    cfg, model = _model(enable_prefix_caching=True)
    ids, ser, lens = _inputs(cfg, [100, 40])
    n = 24
    first = model.generate_one(ids, ser, lens, n, controls=dict(repetition_penalty=1.8, frequency_penalty=1.0, presence_penalty=1.0))
    follow = ids + first[:6]                                # prompt + part of the answer: reuses the first request's K/V rows
    hits = model.prefix_stats["hits"]
    second = model.generate_one(follow, ser, lens, n, controls={})
    assert model.prefix_stats["hits"] == hits + 1
    third = model.generate_one(follow, ser, lens, n, controls=dict(repetition_penalty=1.8))
    cfg, fresh = _model(enable_prefix_caching=True)
    assert second == fresh.generate_one(follow, ser, lens, n)
    assert third == fresh.generate_one(follow, ser, lens, n, controls=dict(repetition_penalty=1.8)) != second
    # batched: a slot's next tenant starts from a clean row
    cfg, mb = _model(max_batch=2)
    a = mb.generate_batch([(ids, ser, lens)] * 2, n, eos_token_id=[], controls=dict(PEN))
    b = mb.generate_batch([(ids, ser, lens)] * 2, n, eos_token_id=[], controls=[None, dict(PEN)])
    c = mb.generate_batch([(ids, ser, lens)] * 2, n, eos_token_id=[])          # the slots keep their settings: slot 1 still penalised
    mb.set_sampling(0.0, repetition_penalty=1.0)
    d = mb.generate_batch([(ids, ser, lens)] * 2, n, eos_token_id=[])
    assert a[0] == a[1] == b[1] and b[0] == d[0] == d[1] != a[0]
    assert sorted(map(tuple, c)) == sorted(map(tuple, b))


def test_llm_and_server_match_the_model():
    from starlette.testclient import TestClient
    from chatts_amd import LLM, SamplingParams, server
    cfg = cfgmod.preset("tiny-qwen2")
    rng = np.random.default_rng(2)
    ts = random_walk_series(rng, 40)
    prompt = "Describe <ts><ts/>"
    n = 24
    llm = LLM(cfg, max_model_len=512, seed=MODEL_SEED)
    req = [{"prompt": prompt, "multi_modal_data": {"timeseries": [ts.tolist()]}}]
    plain = llm.generate(req, SamplingParams(max_tokens=n, ignore_eos=True))[0].outputs[0]
    out = llm.generate(req, SamplingParams(max_tokens=n, ignore_eos=True, repetition_penalty=1.3, frequency_penalty=0.5))[0].outputs[0]
    assert llm.model._controls_on and out.token_ids != plain.token_ids
    # the model-level run of the same request
    text, encs, lens = llm.processor.splice(prompt, [np.asarray(ts, dtype=np.float64)])
    ids = llm.processor.tokenizer.encode(text)
    ser = torch.from_numpy(llm.processor.pad_stack(encs))
    _, model = _model()
    assert model.generate_one(ids, ser, lens, n, controls=dict(repetition_penalty=1.3, frequency_penalty=0.5)) == out.token_ids
    again = llm.generate(req, SamplingParams(max_tokens=n, ignore_eos=True))[0].outputs[0]
    assert again.token_ids == plain.token_ids and not llm.model._controls_on     # a default call runs the plain selection
    del llm, model
    app = server.build_server(cfg, max_model_len=512, max_num_seqs=2, seed=MODEL_SEED)
    try:
        client = TestClient(app)
        body = {"model": "chatts", "prompt": prompt, "multi_modal_data": {"timeseries": [ts.tolist()]}, "max_tokens": n, "ignore_eos": True}
        d = client.post("/v1/completions", json=dict(body, repetition_penalty=1.3, frequency_penalty=0.5)).json()
        assert d["choices"][0]["text"] == out.text
        d0 = client.post("/v1/completions", json=body).json()
        assert d0["choices"][0]["text"] == plain.text != out.text
        r = client.post("/v1/completions", json=dict(body, frequency_penalty=3))
        assert r.status_code == 400 and "frequency_penalty" in r.json()["error"]["message"]
        msgs = [{"role": "user", "content": [{"type": "text", "text": prompt}, {"timeseries": ts.tolist()}]}]
        assert client.post("/v1/chat/completions", json={"messages": msgs, "max_tokens": 4, "min_p": 2}).status_code == 400
        assert client.post("/v1/chat/completions", json={"messages": msgs, "max_tokens": 4, "presence_penalty": 1.0,
                                                          "min_p": 0.1, "temperature": 0.7, "seed": 1}).status_code == 200
    finally:
        app.state.engine_thread.close()


def test_engine_mixed_batch_with_per_slot_controls():
    """Engine, four slots, per-slot sampling: a penalised greedy request, a sampled request with min_p = 1 (= its greedy text), a default
    request and a sampled one decode together; each gets what it gets alone, the mode follows the requests, and it goes off again."""
    from chatts_amd import LLM
    from chatts_amd.engine import Engine
    cfg = cfgmod.preset("tiny-qwen2")
    llm = LLM(cfg, max_model_len=512, seed=MODEL_SEED, max_num_seqs=4)
    rng = np.random.default_rng(9)
    prompts = [(chat_prompt([L]), [random_walk_series(rng, L).tolist()]) for L in (64, 30, 17, 40)]
    n = 24

    def run(plan, **engine_kw):
        eng = Engine(llm.model, llm.processor, sync_every=3, **engine_kw)
        reqs = [eng.add_request(prompts[p][0], prompts[p][1], max_tokens=n, ignore_eos=True, **kw) for p, kw in plan]
        eng.run_until_done()
        assert all(r.error is None for r in reqs), [r.error for r in reqs]
        return eng, [r.tokens for r in reqs]

    _, greedy = run([(i, {}) for i in range(4)])
    assert not llm.model._controls_on and "lc_state" not in llm.model.buf
    alone = [run([(0, PEN)])[1][0], run([(3, dict(temperature=0.8, seed=4, min_p=0.2))])[1][0]]
    assert alone[0] != greedy[0]
    eng, mixed = run([(0, PEN), (1, dict(temperature=1.0, seed=7, min_p=1.0)), (2, {}), (3, dict(temperature=0.8, seed=4, min_p=0.2))],
                     greedy_return_steps=2)
    assert llm.model._controls_on
    assert mixed[0] == alone[0] and mixed[1] == greedy[1] and mixed[2] == greedy[2] and mixed[3] == alone[1]
    for _ in range(3):                                       # iterations without a requester: the mode goes off again
        eng.add_request(prompts[2][0], prompts[2][1], max_tokens=2, ignore_eos=True)
        eng.run_until_done()
    assert not llm.model._controls_on
    with pytest.raises(ValueError, match="min_p"):
        eng.add_request(prompts[0][0], prompts[0][1], min_p=1.5)


# ---- tensor parallel: two rank processes on one GPU, every rank reports its tokens ---------------------------------------------------------
DRIVER = r"""
import json, sys
import numpy as np
sys.path.insert(0, {root!r})
sys.path.insert(0, {root!r} + "/tests")
rank, world, port = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3])
if world > 1:
    from chatts_amd.tp_spawn import init_rank
    init_rank(rank, world, port)
from chatts_amd import LLM, SamplingParams
from util import chat_prompt, random_walk_series
llm = LLM("tiny-qwen3", tensor_parallel_size=world, max_model_len=512, seed=3)
rng = np.random.default_rng(1234)
lengths = [64, 30]
series = [random_walk_series(rng, L) for L in lengths]
req = [{{"prompt": chat_prompt(lengths), "multi_modal_data": {{"timeseries": [s.tolist() for s in series]}}}}]
pen = llm.generate(req, SamplingParams(max_tokens=24, ignore_eos=True, repetition_penalty=1.3, frequency_penalty=0.5,
                                       presence_penalty=0.5))[0].outputs[0].token_ids
smp = llm.generate(req, SamplingParams(max_tokens=24, ignore_eos=True, temperature=0.8, seed=11, min_p=0.2))[0].outputs[0].token_ids
plain = llm.generate(req, SamplingParams(max_tokens=24, ignore_eos=True))[0].outputs[0].token_ids
print("RESULT " + json.dumps(dict(rank=rank, pen=pen, smp=smp, plain=plain)), flush=True)
if world > 1:
    import torch.distributed as dist
    dist.barrier()
    dist.destroy_process_group()
"""


def _ranks(world, tmp_path):
    from chatts_amd.tp_spawn import free_port
    env = dict(os.environ)
    env.update(HSA_ENABLE_IPC_MODE_LEGACY="0", CHATTS_FORCE_DEVICE="0", CHATTS_DIST_BACKEND="gloo", OMP_NUM_THREADS="8")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    script = tmp_path / f"driver_tp{world}.py"
    script.write_text(DRIVER.format(root=ROOT))
    port = free_port()
    procs = [subprocess.Popen([sys.executable, str(script), str(r), str(world), str(port)], env=env, cwd=ROOT, stdout=subprocess.PIPE,
                              stderr=subprocess.PIPE, text=True) for r in range(world)]
    res = []
    try:
        for p in procs:                                   # each child under its own time limit; a failed child ends the test
            out, err = p.communicate(timeout=300)
            lines = [l for l in out.splitlines() if l.startswith("RESULT ")]
            assert p.returncode == 0 and lines, f"rc={p.returncode}\n{out[-2000:]}\n{err[-3000:]}"
            res.append(json.loads(lines[-1][7:]))
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.wait()
    return res


def test_tp2_every_rank_picks_the_tp1_tokens(tmp_path):
    one = _ranks(1, tmp_path)[0]
    two = _ranks(2, tmp_path)
    assert sorted(r["rank"] for r in two) == [0, 1]
    assert one["pen"] != one["plain"] and one["smp"] != one["plain"]
    for r in two:
        assert r["plain"] == one["plain"], r["rank"]
        assert r["pen"] == one["pen"], r["rank"]              # greedy, penalised
        assert r["smp"] == one["smp"], r["rank"]              # sampled with min_p = 0.2
