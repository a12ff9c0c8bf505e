"""GPU: n samples per prompt from one prefill, and stop strings, on small synthetic models.

Kernel level: chatts_kv_fork / chatts_logit_state_fork against a host copy, bit for bit, with everything that must not change filled with a
NaN pattern.  End to end: sibling i of a sampled request == a stand-alone request with seed s + i (exact: the same prefill path, bitwise
equal K / V rows, batch-independent decode rows), one prefill per parent, greedy siblings == the oracle, unrelated requests undisturbed,
stop strings through LLM.generate, the engine and the server, tensor parallelism with two ranks.  Host logic: tests/test_parallel_sampling_host.py."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from chatts_amd import _lib, config as cfgmod, synth
from chatts_amd.engine import Engine
from chatts_amd.modeling import ChatTSForCausalLM
from chatts_amd.processing import ChatTSProcessor
from oracle import pipeline, synth as osynth
from tests.util import chat_prompt, random_walk_series

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODEL_SEED = 3


# ---------------------------------------------------------------------------------------------------------------------------------
# the kernels
# ---------------------------------------------------------------------------------------------------------------------------------
def _bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def _nan_pattern(shape, dtype, gen):
    """NaNs with distinct payloads (a copy is only right when it moves the bits), as `dtype`"""
    if dtype == torch.float32:
        raw = torch.randint(1, 1 << 22, shape, generator=gen, dtype=torch.int32) | 0x7FC00000
    else:
        raw = (torch.randint(1, 1 << 9, shape, generator=gen, dtype=torch.int32) | 0x7E00).to(torch.int16)
    return raw.view(dtype).cuda()


def _kv_fork(k, v, max_ctx, dtype, L, H, slots, lstride, sstride, nblocks, src, dst, t0, t1, table=None, bs=0):
    lib = _lib.load()
    kc = _lib.KvCache(k=k.data_ptr(), v=v.data_ptr(), max_ctx=max_ctx, dtype=_lib.KV_F16 if dtype == torch.float16 else _lib.KV_F32,
                      block_table=None if table is None else table.data_ptr(), block_size=bs,
                      table_stride=0 if table is None else table.shape[1])
    arr = (C.c_int32 * len(dst))(*dst)
    _lib.check(lib.chatts_kv_fork(C.byref(kc), L, H, slots, lstride, sstride, nblocks, src, arr, len(dst), t0, t1, _lib.stream_ptr()))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("m", [1, 3, 15])
def test_kv_fork_contiguous_bitwise(dtype, m):
    L, H, CTX, SLOTS, T = 3, 2, 192, 16, 101
    gen = torch.Generator().manual_seed(m)
    k, v = _nan_pattern((SLOTS, L, H, CTX, 128), dtype, gen), _nan_pattern((SLOTS, L, H, CTX, 128), dtype, gen)
    src = 5
    k[src, :, :, :T] = torch.randn((L, H, T, 128), generator=gen).to(dtype).cuda()
    v[src, :, :, :T] = torch.randn((L, H, T, 128), generator=gen).to(dtype).cuda()
    dst = [s for s in (9, 0, 15, 1, 2, 3, 4, 6, 7, 8, 10, 11, 12, 13, 14) if s != src][:m]
    want = []
    for t in (k, v):                                      # the host copy of the fork
        w = _bits(t).clone()
        w[dst, :, :, :T] = w[src, :, :, :T].clone()
        want.append(w)
    before = [_bits(k).clone(), _bits(v).clone()]
    _kv_fork(k, v, CTX, dtype, L, H, SLOTS, k.stride(1), k.stride(0), 0, src, dst, 0, T)
    torch.cuda.synchronize()
    for t, w, b in zip((k, v), want, before):
        assert torch.equal(_bits(t), w)                   # rows [0, T) of every (layer, head) arrived; rows >= T, the source and the
        assert torch.equal(_bits(t)[src], b[src])         # uninvolved slots kept their NaN pattern
        assert torch.equal(_bits(t)[dst[0], :, :, :T], b[src, :, :, :T])
    # captured in a graph and replayed == eager
    k2, v2 = before[0].clone().view(dtype), before[1].clone().view(dtype)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        _kv_fork(k2, v2, CTX, dtype, L, H, SLOTS, k2.stride(1), k2.stride(0), 0, src, dst, 0, T)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(_bits(k2), want[0]) and torch.equal(_bits(v2), want[1])


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("m", [1, 3, 15])
@pytest.mark.parametrize("T", [150, 128, 37])             # not a multiple of the block, a multiple, less than one block
def test_kv_fork_paged_bitwise(dtype, T, m):
    L, H, BS, BPS, SLOTS = 2, 2, 64, 4, 16
    NB = SLOTS * BPS
    gen = torch.Generator().manual_seed(T)
    k, v = _nan_pattern((L, NB, H, BS, 128), dtype, gen), _nan_pattern((L, NB, H, BS, 128), dtype, gen)
    perm = torch.randperm(NB, generator=gen).tolist()     # a shuffled table: every slot's blocks lie anywhere in the pool
    table = torch.tensor(perm, dtype=torch.int32).view(SLOTS, BPS).clone()
    src = 4
    dst = [1, 5, 2, 15, 0, 3, 6, 7, 8, 9, 10, 11, 12, 13, 14][:m]
    nshare = T // BS
    for d in dst:                                         # the host shares the whole prompt blocks; the trailing block stays private
        table[d, :nshare] = table[src, :nshare]
    for j in range(T):                                    # the source's prompt rows
        b = int(table[src, j // BS])
        k[:, b, :, j % BS] = torch.randn((L, H, 128), generator=gen).to(dtype).cuda()
        v[:, b, :, j % BS] = torch.randn((L, H, 128), generator=gen).to(dtype).cuda()
    want = []
    for t in (k, v):
        w = _bits(t).clone()
        if T % BS:
            sb = int(table[src, nshare])
            for d in dst:
                w[:, int(table[d, nshare]), :, :T % BS] = w[:, sb, :, :T % BS]
        want.append(w)
    tab = table.cuda()
    _kv_fork(k, v, BS * BPS, dtype, L, H, SLOTS, k.stride(0), 0, NB, src, dst, T - T % BS, T, tab, BS)
    torch.cuda.synchronize()
    assert torch.equal(_bits(k), want[0]) and torch.equal(_bits(v), want[1])
    if T % BS:
        assert torch.equal(_bits(k)[:, int(table[dst[-1], nshare]), :, :T % BS], _bits(k)[:, int(table[src, nshare]), :, :T % BS])
    # rows that span two blocks (a general caller): the same call from row 40 on, over a fresh copy
    if T == 150 and m == 3:
        k4, v4 = _nan_pattern((L, NB, H, BS, 128), dtype, gen), _nan_pattern((L, NB, H, BS, 128), dtype, gen)
        own = torch.tensor(perm, dtype=torch.int32).view(SLOTS, BPS).cuda()      # nothing shared: every row has its own blocks
        for j in range(T):
            b = perm[src * BPS + j // BS]
            k4[:, b, :, j % BS] = torch.randn((L, H, 128), generator=gen).to(dtype).cuda()
        w4 = _bits(k4).clone()
        for j in range(40, T):
            for d_ in dst:
                w4[:, perm[d_ * BPS + j // BS], :, j % BS] = w4[:, perm[src * BPS + j // BS], :, j % BS]
        _kv_fork(k4, v4, BS * BPS, dtype, L, H, SLOTS, k4.stride(0), 0, NB, src, dst, 40, T, own, BS)
        torch.cuda.synchronize()
        assert torch.equal(_bits(k4), w4)
    # captured in a graph and replayed == eager
    if T % BS:
        k5 = _bits(k).clone()
        for d_ in dst:
            k5[:, int(table[d_, nshare]), :, :T % BS] = 0
        k5, v5 = k5.view(dtype), _bits(v).clone().view(dtype)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            _kv_fork(k5, v5, BS * BPS, dtype, L, H, SLOTS, k5.stride(0), 0, NB, src, dst, T - T % BS, T, tab, BS)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(_bits(k5), want[0]) and torch.equal(_bits(v5), want[1])
    # a table entry outside the pool is skipped, never followed
    k3, v3 = want[0].clone().view(dtype), want[1].clone().view(dtype)
    bad = table.clone()
    bad[dst[0], nshare] = NB + 7
    _kv_fork(k3, v3, BS * BPS, dtype, L, H, SLOTS, k3.stride(0), 0, NB, src, dst, T - T % BS, T, bad.cuda(), BS)
    torch.cuda.synchronize()
    assert torch.equal(_bits(k3), want[0]) and torch.equal(_bits(v3), want[1])


@pytest.mark.parametrize("vocab,stride", [(4096, 4096), (1003, 1003), (1003, 1004), (152064, 152064)])   # 1003 / 1004: 16-byte units and a scalar tail
def test_logit_state_fork_bitwise(vocab, stride):
    lib = _lib.load()
    rows, src, dst = 8, 2, [0, 7, 5]
    gen = torch.Generator().manual_seed(vocab)
    state = torch.randint(-2 ** 31, 2 ** 31 - 1, (rows, stride), generator=gen, dtype=torch.int64).to(torch.int32).cuda()
    want = state.clone()
    want[dst, :vocab] = want[src, :vocab].clone()       # (cells past vocab are not the kernel's)
    arr = (C.c_int32 * len(dst))(*dst)
    _lib.check(lib.chatts_logit_state_fork(state.data_ptr(), stride, vocab, rows, src, arr, len(dst), _lib.stream_ptr()))
    torch.cuda.synchronize()
    assert torch.equal(state, want)


# ---------------------------------------------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------------------------------------------
def _prompt(lengths, rng_seed=1234):
    rng = np.random.default_rng(rng_seed)
    return chat_prompt(lengths), [random_walk_series(rng, L).tolist() for L in lengths]


def _model(preset="tiny-qwen2", **kw):
    cfg = preset if not isinstance(preset, str) else cfgmod.preset(preset)
    kw.setdefault("max_ctx", 512)
    kw.setdefault("max_prefill_tokens", 512)
    return cfg, ChatTSForCausalLM.from_synthetic(cfg, seed=MODEL_SEED, **kw)


def _run(model, cfg, plan, sync_every=4, proc=None, **engine_kw):
    eng = Engine(model, proc or ChatTSProcessor.from_pretrained(cfg), sync_every=sync_every, **engine_kw)
    reqs = [eng.add_request(p[0], p[1], **kw) for p, kw in plan]
    eng.run_until_done()
    assert all(r.error is None for r in reqs), [r.error for r in reqs]
    return reqs


SAMPLED = dict(temperature=0.8, top_p=0.95, max_tokens=24, ignore_eos=True)


@pytest.mark.parametrize("name,model_kw,req_kw", [
    ("contiguous", {}, {}),
    ("qwen3", {"preset": "tiny-qwen3"}, {}),
    ("paged", {"kv_block_size": 64}, {}),
    ("paged-oversubscribed", {"kv_block_size": 64, "kv_pool_blocks": 14}, {}),
    ("fp16", {"kv_cache_dtype": "fp16"}, {}),
    ("penalties", {}, dict(repetition_penalty=1.3, frequency_penalty=0.5, presence_penalty=0.5)),
    ("logprobs", {}, dict(logprobs=5)),
])
def test_sibling_i_is_the_stand_alone_request_with_seed_s_plus_i(name, model_kw, req_kw):
    model_kw = dict(model_kw)
    preset = model_kw.pop("preset", "tiny-qwen2")
    cfg, model = _model(preset, max_batch=4, **model_kw)
    prompt = _prompt([100, 40])                            # 196 positions: three whole blocks of 64 and 4 rows of a fourth
    s = 1000
    parent = _run(model, cfg, [(prompt, dict(SAMPLED, n=4, seed=s, **req_kw))])[0]
    kids = parent.outputs
    assert [k.index for k in kids] == [0, 1, 2, 3] and all(len(k.tokens) == 24 for k in kids)
    assert len({tuple(k.tokens) for k in kids}) > 1      # (temperature 0.8 over a synthetic model: the seeds tell the siblings apart)
    cfg, alone = _model(preset, max_batch=4, enable_prefix_caching=False, **model_kw)
    for i, k in enumerate(kids):
        one = _run(alone, cfg, [(prompt, dict(SAMPLED, seed=s + i, **req_kw))])[0]
        assert k.tokens == one.tokens, (name, i)
        if "logprobs" in req_kw:
            assert k.logprobs == one.logprobs and k.cumulative_logprob == one.cumulative_logprob and len(k.logprobs) == 24
    if "repetition_penalty" in req_kw:                     # each sibling's counts are its own: without the penalties the texts differ
        plain = _run(alone, cfg, [(prompt, dict(SAMPLED, seed=s + 1))])[0]
        assert plain.tokens != kids[1].tokens
    # ... wherever the siblings land: a second round on the used model with another request in the first slot (prefix reuse off from
    # here on, so that the prompt is prefilled in full again - the same prefill path)
    model.enable_prefix_caching = False
    for sl in range(4):
        model._slot_idents[sl] = []
    busy = _prompt([30], 5)
    again = _run(model, cfg, [(busy, dict(max_tokens=40, ignore_eos=True)), (prompt, dict(SAMPLED, n=3, seed=s, **req_kw))])[1]
    assert [k.tokens for k in again.outputs] == [k.tokens for k in kids[:3]]


def test_full_width_two_layers_identity():
    """ChatTS-14B widths (H = 5120, 40 / 8 heads, V = 152064) truncated to 2 layers"""
    cfg = cfgmod.preset("chatts-14b", num_hidden_layers=2)
    cfg, model = _model(cfg, max_batch=4, max_ctx=384, max_prefill_tokens=256)
    prompt = _prompt([64, 30])
    parent = _run(model, cfg, [(prompt, dict(SAMPLED, n=4, seed=77, max_tokens=12))])[0]
    model.enable_prefix_caching = False                    # the stand-alone runs prefill the whole prompt (nothing resident is reused)
    for sl in range(4):
        model._slot_idents[sl] = []
    for i, k in enumerate(parent.outputs):
        one = _run(model, cfg, [(prompt, dict(SAMPLED, seed=77 + i, max_tokens=12))])[0]
        assert k.tokens == one.tokens, i


@pytest.mark.parametrize("prefix_caching", [True, False])
def test_one_prefill_per_parent(prefix_caching):
    cfg, model = _model(max_batch=4, enable_prefix_caching=prefix_caching)
    calls = {"prefill": 0, "layers": 0}
    prefill, run_layers = model.prefill, model._run_layers

    def counted_prefill(*a, **kw):
        calls["prefill"] += 1
        return prefill(*a, **kw)

    def counted_layers(*a, **kw):
        calls["layers"] += 1
        return run_layers(*a, **kw)
    model.prefill, model._run_layers = counted_prefill, counted_layers
    prompt = _prompt([100, 40])
    proc = ChatTSProcessor.from_pretrained(cfg)
    text, _, lens = proc.splice(prompt[0], [np.asarray(s, dtype=np.float64) for s in prompt[1]])
    T = model.request_tokens(proc.tokenizer.encode(text), None, lens)
    assert T == 196
    parent = _run(model, cfg, [(prompt, dict(SAMPLED, n=4, seed=5))])[0]
    assert calls == {"prefill": 1, "layers": 1}            # one pass over the prompt for all four
    assert model.prefix_stats["tokens_prefilled"] == T and model.prefix_stats["forks"] == 1 and model.prefix_stats["fork_children"] == 3
    assert all(len(k.tokens) == 24 for k in parent.outputs)
    # every sibling's answer is recorded for prefix reuse like any finished request's
    if prefix_caching:
        assert all(len(model._slot_idents[sl]) == T + 23 for sl in range(4))


def test_greedy_siblings_and_unrelated_requests_match_the_oracle():
    cfg = cfgmod.preset("tiny-qwen2")
    proc = ChatTSProcessor.from_pretrained(cfg)
    model = ChatTSForCausalLM.from_synthetic(cfg, seed=5, max_ctx=512, max_prefill_tokens=256, max_batch=4)
    sd = osynth.state_dict(synth.all_specs(cfg), 5)
    rng = np.random.default_rng(77)
    specs = [[64], [17, 40], [30]]
    prompts, wants = [], []
    for lengths in specs:
        series = [random_walk_series(rng, L) for L in lengths]
        inp = proc(text=[chat_prompt(lengths)], timeseries=series, return_tensors="pt")
        prompts.append((chat_prompt(lengths), [s.tolist() for s in series]))
        wants.append(pipeline.generate(cfg, sd, inp["input_ids"][0].tolist(), inp["timeseries"].numpy(), 9)["tokens"])
    g = dict(max_tokens=9, ignore_eos=True)
    three = _run(model, cfg, [(prompts[0], dict(g, n=3))])[0]
    assert [k.tokens for k in three.outputs] == [wants[0]] * 3 and [k.index for k in three.outputs] == [0, 1, 2]
    # a sampled parent beside unrelated greedy requests, more work than slots: the unrelated ones still yield the oracle's tokens
    reqs = _run(model, cfg, [(prompts[1], g), (prompts[0], dict(SAMPLED, n=3, seed=9, max_tokens=9)), (prompts[2], g), (prompts[0], g)],
                sync_every=2)
    assert reqs[0].tokens == wants[1] and reqs[2].tokens == wants[2] and reqs[3].tokens == wants[0]
    assert len(reqs[1].outputs) == 3 and all(len(k.tokens) == 9 for k in reqs[1].outputs)
    with pytest.raises(ValueError, match="max_num_seqs"):
        Engine(model, proc).add_request(prompts[0][0], prompts[0][1], n=5)


def test_a_fork_the_pool_cannot_hold_leaves_the_counters_as_they_were():
    """admit_begin counts the admission; when the children's blocks cannot be reserved nothing of it may stay counted (the engine queues
    the request again and the retry counts it once)"""
    from chatts_amd.kv_blocks import KvPoolExhausted
    cfg, model = _model(max_batch=4, kv_block_size=64, kv_pool_blocks=5)
    proc = ChatTSProcessor.from_pretrained(cfg)
    prompt = _prompt([100, 40])
    text, encs, lens = proc.splice(prompt[0], [np.asarray(s, dtype=np.float64) for s in prompt[1]])
    ids, ser = proc.tokenizer.encode(text), torch.from_numpy(proc.pad_stack(encs))
    before = dict(model.prefix_stats)
    st = model.admit_begin(0, ids, ser, lens, 24)         # 196 + 24 positions: 4 of the 5 blocks
    assert model.prefix_stats["tokens_prefilled"] == before["tokens_prefilled"] + 196
    with pytest.raises(KvPoolExhausted):
        model.admit_fork(st, [1, 2, 3], 24)               # one block per child: the second child finds the pool empty
    assert model.prefix_stats == before and model._kv.check() and not model._kv.active
    assert all(not model._kv.rows[c] for c in (1, 2, 3))
    # the pool is as usable as before: the same prompt with n = 2 fits and runs
    parent = _run(model, cfg, [(prompt, dict(SAMPLED, n=2, seed=3))])[0]
    assert model.prefix_stats["tokens_prefilled"] == before["tokens_prefilled"] + 196 and len(parent.outputs) == 2


def test_llm_generate_seeds_with_n_and_stop():
    """What holds on the offline surface.  Calls with n > 1 or stop are served by an Engine in per-slot mode (sample i: seed s + i, a
    stream of (seed, step) alone); a call with n = 1 and no stop keeps the shared configuration of generate_batch, which with
    max_num_seqs > 1 folds the cache slot into every draw.  So: with max_num_seqs = 1 (one slot, nothing to fold) a never-matching stop
    does not change a seeded sampled call; with more slots sample 0 of n = 2 is the engine-served n = 1 call (stop given, or an Engine
    request), and the n = 1 / no-stop call still computes what model.generate_batch computes."""
    from chatts_amd import LLM, SamplingParams
    cfg = cfgmod.preset("tiny-qwen2")
    prompt, series = _prompt([64, 30])
    req = [{"prompt": prompt, "multi_modal_data": {"timeseries": series}}]
    kw = dict(max_tokens=16, ignore_eos=True, temperature=0.8, top_p=0.95, seed=21)
    one = LLM(cfg, max_model_len=512, seed=MODEL_SEED, max_num_seqs=1)
    one.model.enable_prefix_caching = False                # (every call prefills the whole prompt: the same prefill path)
    a = one.generate(req, SamplingParams(**kw))[0].outputs[0]
    b = one.generate(req, SamplingParams(stop="\x00never", **kw))[0].outputs[0]
    c = one.generate(req, SamplingParams(**kw))[0].outputs[0]
    assert a.token_ids == b.token_ids == c.token_ids and a.text == b.text and b.finish_reason == "length"
    del one
    llm = LLM(cfg, max_model_len=512, seed=MODEL_SEED, max_num_seqs=2)
    llm.model.enable_prefix_caching = False
    two = llm.generate(req, SamplingParams(n=2, **kw))[0].outputs
    single = llm.generate(req, SamplingParams(stop="\x00never", **kw))[0].outputs[0]
    assert two[0].token_ids == single.token_ids and two[1].token_ids != two[0].token_ids
    eng = _run(llm.model, cfg, [((prompt, series), dict(kw))], proc=llm.processor)[0]
    assert eng.tokens == two[0].token_ids
    # n = 1 without stop: the path and the tokens of generate_batch under the shared configuration, as before
    plain = llm.generate(req, SamplingParams(**kw))[0].outputs[0]
    text, encs, lens = llm.processor.splice(prompt, [np.asarray(s, dtype=np.float64) for s in series])
    ids, ser = llm.processor.tokenizer.encode(text), torch.from_numpy(llm.processor.pad_stack(encs))
    llm.model.set_sampling(0.8, 0, 0.95, 21)
    assert llm.model.generate_batch([(ids, ser, lens)], 16, None) == [plain.token_ids]


# ---------------------------------------------------------------------------------------------------------------------------------
# stop strings, end to end
# ---------------------------------------------------------------------------------------------------------------------------------
def _mid_token_substring(tok, toks, full):
    """a substring of the decoded text that starts inside one token's piece and ends inside a later one, and occurs there first"""
    pieces = [tok.decode([t], skip_special_tokens=True) for t in toks]
    assert "".join(pieces) == full
    off = np.cumsum([0] + [len(p) for p in pieces]).tolist()
    for i in range(2, len(pieces) - 2):
        if len(pieces[i]) >= 3 and len(pieces[i + 1]) >= 3:
            s = full[off[i] + 1:off[i + 1] + 2]
            if full.index(s) == off[i] + 1:
                return s, i + 2                            # the match completes with token i + 1: j = i + 2 tokens
    raise AssertionError("no such substring")


def test_stop_strings_llm_engine_server():
    from starlette.testclient import TestClient
    from chatts_amd import LLM, SamplingParams, server
    cfg = cfgmod.preset("tiny-qwen2")
    prompt, series = _prompt([64, 30])
    req = [{"prompt": prompt, "multi_modal_data": {"timeseries": series}}]
    n = 24
    llm = LLM(cfg, max_model_len=512, seed=MODEL_SEED, max_num_seqs=2)
    tok = llm.get_tokenizer()
    first = llm.generate(req, SamplingParams(max_tokens=n, ignore_eos=True))[0].outputs[0]
    full = first.text
    s, j = _mid_token_substring(tok, first.token_ids, full)
    cut = llm.generate(req, SamplingParams(max_tokens=n, ignore_eos=True, stop=s))[0].outputs[0]
    assert cut.text == full[:full.index(s)] and cut.finish_reason == "stop" and cut.stop_reason == s
    assert cut.token_ids == first.token_ids[:j]
    inc = llm.generate(req, SamplingParams(max_tokens=n, ignore_eos=True, stop=["\x00no", s], include_stop_str_in_output=True))[0].outputs[0]
    assert inc.text == full[:full.index(s)] + s and inc.text.endswith(s) and inc.token_ids == cut.token_ids and inc.stop_reason == s
    none = llm.generate(req, SamplingParams(max_tokens=n, ignore_eos=True, stop="\x00never"))[0].outputs[0]
    assert none.text == full and none.token_ids == first.token_ids and none.finish_reason == "length" and none.stop_reason is None
    # LLM.generate with n: sample 0 of a seeded sampled call is the engine's stand-alone request with that seed
    many = llm.generate(req, SamplingParams(max_tokens=n, ignore_eos=True, temperature=0.8, seed=21, n=2))[0].outputs
    assert [o.index for o in many] == [0, 1] and many[0].token_ids != many[1].token_ids
    for sync in (1, 8):
        rs = _run(llm.model, cfg, [((prompt, series), dict(max_tokens=n, ignore_eos=True, stop=s)),
                                   ((prompt, series), dict(max_tokens=n, ignore_eos=True, temperature=0.8, seed=22))], sync_every=sync,
                  proc=llm.processor)
        assert rs[0].tokens == cut.token_ids and rs[0].text == cut.text and rs[0].stop_reason == s and rs[0].finish_reason == "stop"
        assert rs[1].tokens == many[1].token_ids
    del llm
    app = server.build_server(cfg, max_model_len=512, max_num_seqs=2, seed=MODEL_SEED)
    try:
        client = TestClient(app)
        body = {"model": "chatts", "prompt": prompt, "multi_modal_data": {"timeseries": series}, "max_tokens": n, "ignore_eos": True}
        assert client.post("/v1/completions", json=body).json()["choices"][0]["text"] == full
        d = client.post("/v1/completions", json=dict(body, stop=s)).json()
        assert d["choices"][0]["text"] == cut.text and d["choices"][0]["finish_reason"] == "stop" and d["token_ids"] == cut.token_ids
        assert d["choices"][0]["stop_reason"] == s
        with client.stream("POST", "/v1/completions", json=dict(body, stop=[s], stream=True)) as resp:
            events = [line[6:] for line in resp.iter_lines() if line.startswith("data: ")]
        chunks = [json.loads(e) for e in events[:-1]]
        assert "".join(c["choices"][0]["text"] for c in chunks) == cut.text and chunks[-1]["choices"][0]["finish_reason"] == "stop"
        two = client.post("/v1/completions", json=dict(body, n=2, temperature=0.8, seed=21)).json()
        assert [c["token_ids"] for c in two["choices"]] == [o.token_ids for o in many] and [c["index"] for c in two["choices"]] == [0, 1]
        assert two["usage"]["completion_tokens"] == 2 * n
        assert client.post("/v1/completions", json=dict(body, n=3)).status_code == 400
    finally:
        app.state.engine_thread.close()


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
llm = LLM("tiny-qwen3", tensor_parallel_size=world, max_model_len=512, seed=3, max_num_seqs=2)
rng = np.random.default_rng(1234)
lengths = [64, 30]
series = [random_walk_series(rng, L) for L in lengths]
req = [{{"prompt": chat_prompt(lengths), "multi_modal_data": {{"timeseries": [s.tolist() for s in series]}}}}]
outs = llm.generate(req, SamplingParams(max_tokens=16, ignore_eos=True, temperature=0.8, seed=11, n=2))[0].outputs
greedy = llm.generate(req, SamplingParams(max_tokens=16, ignore_eos=True, n=2))[0].outputs
print("RESULT " + json.dumps(dict(rank=rank, sampled=[o.token_ids for o in outs], greedy=[o.token_ids for o in greedy])), flush=True)
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


def test_tp2_every_rank_returns_the_tp1_siblings(tmp_path):
    one = _ranks(1, tmp_path)[0]
    two = _ranks(2, tmp_path)
    assert sorted(r["rank"] for r in two) == [0, 1]
    assert one["sampled"][0] != one["sampled"][1] and one["greedy"][0] == one["greedy"][1]
    for r in two:
        assert r["sampled"] == one["sampled"] and r["greedy"] == one["greedy"], r["rank"]
