"""CPU: prompt-lookup speculative decoding - the references against each other, the configuration checks of every Python surface, the
C-ABI refusals (returned before anything is enqueued: the pointers below are fakes and never dereferenced), the additive ABI, and a
known answer of the proposer + accept rule on the CPU oracle's own greedy continuation."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from chatts_amd import _lib
from chatts_amd.spec import parse_speculative_config
from tests import spec_decode_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 4096          # non-null stand-in for device pointers


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


# ---- references -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alphabet", [2, 3, 4096])
def test_the_two_formulations_of_the_proposer_rule_agree(alphabet):
    rng = np.random.default_rng(alphabet)
    matched = 0
    for trial in range(120):
        n = int(rng.integers(1, 90))
        hist = rng.integers(0, alphabet, n).tolist()
        k = int(rng.choice([1, 4, 8]))
        nmin = int(rng.integers(1, 4))
        nmax = int(rng.integers(nmin, 9))
        a = ref.propose_by_match_length(hist, n - 1, k, nmin, nmax)
        b = ref.propose_by_ngram_search(hist, n - 1, k, nmin, nmax)
        assert a == b, (hist, k, nmin, nmax)
        matched += a[1] is not None
    assert (matched > 60) if alphabet <= 3 else (matched < 10)      # small alphabets: ties everywhere; 4096 symbols: (almost) no match


def test_proposer_rule_cases():
    # a match that ends at position 0
    assert ref.propose_by_match_length([7, 1, 2, 7], 3, 4, 1, 3) == ([1, 2, 7, -1], 0)
    # the continuation is cut by the end of the context: -1 fill
    assert ref.propose_by_match_length([5, 6, 5], 2, 4, 1, 3) == ([6, 5, -1, -1], 0)
    # a longer n-gram later beats a shorter one earlier; ties go to the earliest end
    hist = [9, 3, 1, 2, 3, 8, 8, 2, 3]
    assert ref.propose_by_match_length(hist, 8, 2, 1, 3) == ([8, 8], 4)
    assert ref.propose_by_match_length(hist, 8, 2, 1, 1) == ([1, 2], 1)
    # nothing matches / the match is shorter than ngram_min
    assert ref.propose_by_match_length([1, 2, 3], 2, 3, 1, 3) == ([-1, -1, -1], None)
    assert ref.propose_by_match_length(hist, 8, 2, 3, 3) == ([-1, -1], None)
    assert ref.propose_by_match_length([4], 0, 2, 1, 3) == ([-1, -1], None)


def test_verify_rule_cases():
    V = 100
    r = ref.verify([5, 6, 7, 8, 9], [5, 6, 7, 8], pos=10, step=3, out_capacity=48, max_ctx=64, vocab=V)
    assert (r["e"], r["tokens"], r["pos"], r["step"], r["token"], r["counters"]) == (5, [5, 6, 7, 8, 9], 15, 8, 9, (1, 4, 4, 5))
    r = ref.verify([5, 1, 7, 8, 9], [5, 6, 7, 8], 10, 3, 48, 64, V)            # a draft equal to the argmax AFTER a mismatch does not count
    assert (r["e"], r["tokens"], r["counters"]) == (2, [5, 1], (1, 4, 1, 2))
    r = ref.verify([5, 6, 7], [-1, 6], 10, 3, 48, 64, V)                        # -1 drafts are never accepted
    assert (r["e"], r["counters"]) == (1, (1, 1, 0, 1))
    r = ref.verify([5, 6, 7], [5, 200], 10, 3, 48, 64, V)                       # ... nor ids outside the vocabulary
    assert (r["e"], r["counters"]) == (2, (1, 1, 1, 2))
    assert ref.verify([5, 6, 7], [5, 6], 10, 47, 48, 64, V)["e"] == 1             # clamped by the output capacity
    assert ref.verify([5, 6, 7], [5, 6], 10, 48, 48, 64, V) is None
    assert ref.verify([5, 6, 7], [5, 6], 59, 3, 48, 64, V)["e"] == 2              # ... and by the context: the next step's rows must fit
    assert ref.verify([5, 6, 7], [5, 6], 61, 3, 48, 64, V) is None


def test_simulator_counts():
    prompt = [1, 2, 3, 4, 1, 2]
    toks = [3, 4, 1, 2, 3, 9]
    acc, c = ref.simulate(prompt, toks, 4, 1, 3)
    assert sum(acc) + len(acc) == len(toks) - 1 and c["emitted"] == len(toks) - 1 and c["steps"] == len(acc)
    assert acc[0] == 4 and c["accepted"] == sum(acc)
    acc1, c1 = ref.simulate([10, 11, 12], [13, 14, 15, 16, 17, 18], 4, 1, 3)     # nothing ever matches: one token per step
    assert acc1 == [0] * 5 and c1["drafted"] == 0 and c1["accepted"] == 0


# ---- configuration ----------------------------------------------------------------------------------------------------------------
def test_speculative_config_is_parsed_like_vllms():
    assert parse_speculative_config(None) is None
    assert parse_speculative_config({"method": "ngram", "num_speculative_tokens": 4}) == {"k": 4, "ngram_min": 1, "ngram_max": 3}
    assert parse_speculative_config({"num_speculative_tokens": 8, "prompt_lookup_max": 8, "prompt_lookup_min": 2}) == \
        {"k": 8, "ngram_min": 2, "ngram_max": 8}
    assert parse_speculative_config('{"method": "ngram", "num_speculative_tokens": 2}')["k"] == 2


@pytest.mark.parametrize("cfg,kw", [
    ({"method": "eagle", "num_speculative_tokens": 4}, {}),
    ({"method": "ngram"}, {}),
    ({"method": "ngram", "num_speculative_tokens": 4, "draft_model": "x"}, {}),
    ({"method": "ngram", "num_speculative_tokens": 0}, {}),
    ({"method": "ngram", "num_speculative_tokens": 9}, {}),
    ({"method": "ngram", "num_speculative_tokens": 2.5}, {}),
    ({"method": "ngram", "num_speculative_tokens": True}, {}),
    ({"method": "ngram", "num_speculative_tokens": 4, "prompt_lookup_min": 0}, {}),
    ({"method": "ngram", "num_speculative_tokens": 4, "prompt_lookup_min": 3, "prompt_lookup_max": 2}, {}),
    ({"method": "ngram", "num_speculative_tokens": 4, "prompt_lookup_max": 9}, {}),
    ({"method": "ngram", "num_speculative_tokens": 4}, {"tensor_parallel_size": 2}),
    ({"method": "ngram", "num_speculative_tokens": 4}, {"max_num_seqs": 2}),
    ("not json", {}),
    ([4], {}),
])
def test_speculative_config_refusals_name_the_argument(cfg, kw):
    with pytest.raises(ValueError, match="speculative_config"):
        parse_speculative_config(cfg, **kw)


def test_model_and_llm_refuse_a_bad_speculative_config_before_the_device_is_touched(monkeypatch):
    import torch
    from chatts_amd import config as cfgmod
    from chatts_amd.llm import LLM
    from chatts_amd.modeling import ChatTSForCausalLM
    monkeypatch.setattr(torch.cuda, "is_available", lambda: (_ for _ in ()).throw(AssertionError("the device was asked for")))
    cfg = cfgmod.preset("tiny-qwen2")
    for bad in ({"method": "medusa", "num_speculative_tokens": 2}, {"method": "ngram", "num_speculative_tokens": 40}, {"k": 3}):
        with pytest.raises(ValueError, match="speculative_config"):
            ChatTSForCausalLM(cfg, speculative_config=bad)
        with pytest.raises(ValueError, match="speculative_config"):
            LLM(cfg, speculative_config=bad)
    good = {"method": "ngram", "num_speculative_tokens": 4}
    with pytest.raises(ValueError, match="speculative_config"):
        ChatTSForCausalLM(cfg, speculative_config=good, max_batch=4)
    with pytest.raises(ValueError, match="speculative_config"):
        LLM(cfg, speculative_config=good, max_num_seqs=4)
    with pytest.raises(ValueError, match="speculative_config"):
        LLM(cfg, speculative_config=good, tensor_parallel_size=2)


def test_server_has_the_flag():
    src = open(os.path.join(ROOT, "chatts_amd", "server.py")).read()
    assert "--speculative-config" in src and "speculative_config=args.speculative_config" in src


# ---- C-ABI ------------------------------------------------------------------------------------------------------------------------
def test_abi_is_still_version_9_and_the_new_symbols_are_exported_and_declared(lib):
    assert lib.chatts_abi_version() == 9 and _lib.ABI_VERSION == 9
    assert C.sizeof(_lib.DecoderBuffers) == 176 and C.sizeof(_lib.KvCache) == 40
    header = open(os.path.join(ROOT, "include", "chatts_amd.h")).read()
    for name in ("chatts_spec_propose", "chatts_spec_verify", "chatts_attention_verify", "chatts_decoder_spec_step"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        assert re.search(r"\bint " + name + r"\(", header), name
    assert "typedef struct ChattsSpecArgs" in header and "#define CHATTS_ABI_VERSION 9" in header
    assert C.sizeof(_lib.SpecArgs) == 24 + 11 * 8 and _lib.SpecArgs.hist.offset == 24
    assert (_lib.SPEC_MAX_DRAFT, _lib.SPEC_MAX_ROWS, _lib.SPEC_MAX_NGRAM) == (8, 9, 8)


def _decoder(lib, tp_world=1):
    layers = (_lib.LayerWeights * 1)()
    for f, _ in _lib.LayerWeights._fields_:
        if f in ("input_norm", "qkv", "o", "post_norm", "gate_up", "down"):
            setattr(layers[0], f, FAKE)
    dc = _lib.DecoderConfig(hidden=256, n_layers=1, n_q=4, n_kv=2, head_dim=128, inter=512, vocab_local=1024, vocab_offset=0, rms_eps=1e-6,
                            max_ctx=256, max_pos=256, tp_world=tp_world, embed_rows=1024, embed_offset=0, w8_format=0)
    dw = _lib.DecoderWeights(layers=layers, final_norm=FAKE, lm_head=FAKE, embed=FAKE, cos_tab=FAKE, sin_tab=FAKE)
    db = _lib.DecoderBuffers(kv_k=FAKE, kv_v=FAKE, x=FAKE, xn=FAKE, qkv=FAKE, attn=FAKE, act=FAKE, delta=FAKE, logits=FAKE,
                             workspace=FAKE, workspace_bytes=1 << 26, t_max=64, max_batch=1)
    d = lib.chatts_decoder_create(C.byref(dc), C.byref(dw), C.byref(db))
    assert d
    return d, layers


def _spec_args(**over):
    kw = dict(k=4, ngram_min=1, ngram_max=3, n_splits=8, skip_propose=0, hist=FAKE, draft=FAKE, spec_tokens=FAKE, argmax=FAKE, logits=FAKE,
              pos_dev=FAKE, step_dev=FAKE, token_dev=FAKE, out_tokens=FAKE, out_capacity_dev=FAKE, counters=FAKE)
    kw.update(over)
    return _lib.SpecArgs(**kw)


def test_spec_step_refusals_return_before_anything_is_enqueued(lib):
    d, keep = _decoder(lib)
    try:
        assert lib.chatts_decoder_spec_step(None, C.byref(_spec_args()), None) == _lib.E_BADARG
        assert lib.chatts_decoder_spec_step(d, None, None) == _lib.E_BADARG
        for over in (dict(k=0), dict(k=9), dict(k=-1), dict(ngram_min=0), dict(ngram_min=3, ngram_max=2), dict(ngram_max=9),
                     dict(hist=None), dict(draft=None), dict(spec_tokens=None), dict(argmax=None), dict(logits=None), dict(pos_dev=None),
                     dict(step_dev=None), dict(token_dev=None), dict(out_tokens=None), dict(out_capacity_dev=None), dict(counters=None)):
            assert lib.chatts_decoder_spec_step(d, C.byref(_spec_args(**over)), None) == _lib.E_BADARG, over
        # a sampler on the decoder
        sa = _lib.SamplingArgs(temperature=0.7, top_k=0, top_p=1.0, seed=1)
        assert lib.chatts_decoder_set_sampling(d, C.byref(sa)) == 0
        assert lib.chatts_decoder_spec_step(d, C.byref(_spec_args()), None) == _lib.E_BADARG and b"greedy" in lib.chatts_last_error()
        assert lib.chatts_decoder_set_sampling(d, None) == 0
        # logit controls on the decoder
        lc = _lib.LogitControlArgs(state=FAKE, state_stride=1024, out=FAKE, out_stride=1024)
        assert lib.chatts_decoder_set_logit_controls(d, C.byref(lc)) == 0
        assert lib.chatts_decoder_spec_step(d, C.byref(_spec_args()), None) == _lib.E_BADARG and b"greedy" in lib.chatts_last_error()
    finally:
        lib.chatts_decoder_destroy(d)
    d2, keep2 = _decoder(lib, tp_world=2)
    try:
        assert lib.chatts_decoder_spec_step(d2, C.byref(_spec_args()), None) == _lib.E_BADARG
        assert b"tensor_parallel_size" in lib.chatts_last_error()
    finally:
        lib.chatts_decoder_destroy(d2)


def test_kernel_entry_point_refusals(lib):
    assert lib.chatts_spec_propose(None, FAKE, 64, 4, 1, 3, 100, FAKE, FAKE, None) == _lib.E_BADARG
    for k, nmin, nmax in ((0, 1, 3), (9, 1, 3), (4, 0, 3), (4, 3, 2), (4, 1, 9)):
        assert lib.chatts_spec_propose(FAKE, FAKE, 64, k, nmin, nmax, 100, FAKE, FAKE, None) == _lib.E_BADARG
    assert lib.chatts_spec_verify(FAKE, FAKE, 0, 100, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, 64, FAKE, None) == _lib.E_BADARG
    assert lib.chatts_spec_verify(FAKE, FAKE, 4, 100, FAKE, FAKE, FAKE, FAKE, None, FAKE, 64, FAKE, None) == _lib.E_BADARG
    c = _lib.KvCache(k=FAKE, v=FAKE, max_ctx=256)
    args = lambda rows, cache=c, ws=1 << 24, pos=FAKE: (FAKE, rows, 4, 2, None, None, 1e-6, FAKE, FAKE, pos, C.byref(cache), FAKE, 4, FAKE, ws, None)
    assert lib.chatts_attention_verify(*args(0)) == _lib.E_BADARG
    assert lib.chatts_attention_verify(*args(10)) == _lib.E_BADARG
    assert lib.chatts_attention_verify(*args(5, pos=None)) == _lib.E_BADARG
    assert lib.chatts_attention_verify(*args(5, cache=_lib.KvCache(k=FAKE, v=FAKE, max_ctx=256, dtype=2))) == _lib.E_BADARG
    assert b"dtype" in lib.chatts_last_error()
    assert lib.chatts_attention_verify(*args(5, ws=64)) == _lib.E_WORKSPACE


# ---- known answer on the CPU oracle ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def oracle_run():
    from chatts_amd import config as cfgmod, synth
    from chatts_amd.processing import ChatTSProcessor
    from oracle import pipeline, synth as osynth
    from tests.util import chat_prompt, random_walk_series
    cfg = cfgmod.preset("tiny-qwen2")
    proc = ChatTSProcessor.from_pretrained(cfg)
    rng = np.random.default_rng(1234)
    lengths = [100, 40]
    series = [random_walk_series(rng, L) for L in lengths]
    inputs = proc(text=[chat_prompt(lengths)], timeseries=series, padding=True, return_tensors="pt")
    sd = osynth.state_dict(synth.all_specs(cfg), 5)
    want = pipeline.generate(cfg, sd, inputs["input_ids"][0].tolist(), inputs["timeseries"].numpy(), 48)
    return [int(t) for t in want["expanded_ids"]], [int(t) for t in want["tokens"]]


def test_known_answer_accept_counts_on_the_oracles_continuation(oracle_run):
    """tiny-qwen2, weights seed 5, chat_prompt([100, 40]), series from default_rng(1234), 48 greedy tokens; context = expanded ids +
    generated tokens; k = 4, n = 3..1: 23 steps for tokens 2..48, accept counts as computed with the written rule."""
    expanded, toks = oracle_run
    assert len(toks) == 48
    acc, c = ref.simulate(expanded, toks, 4, 1, 3)
    assert acc[:20] == [0, 0, 2, 0, 0, 0, 0, 3, 3, 4, 2, 0, 0, 1, 0, 0, 0, 2, 4, 1]
    assert len(acc) == 23 and c["steps"] == 23 and c["emitted"] == 47 and c["accepted"] == 47 - 23
