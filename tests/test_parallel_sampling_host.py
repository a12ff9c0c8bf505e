"""CPU: n samples per prompt and stop strings, everything above the kernels.

* the stop rule (chatts_amd/detok.py, Engine._harvest) against its brute-force definition over random token streams, on the synthetic
  tokenizer and on a Hugging Face byte-level BPE tokenizer trained in memory, with harvests of 1, 4 and 16 tokens;
* the engine on a stub model: a parent waits for n free slots, one prefill and one fork per parent, seeds s .. s + n - 1, siblings
  retire one by one, the errors, the control-plane message;
* the server on that engine (n choices, blocking and streamed, stop parsing, 400s, streamed deltas == blocking text);
* LLMClient(sample_n=2) on a stub LLM; SamplingParams; the C-ABI's argument checks.
The GPU side: tests/test_gpu_parallel_sampling.py."""
import ctypes as C
import json
import random
import threading
import time

import pytest
import torch

from chatts_amd import _lib, config as cfgmod, detok, server
from chatts_amd.engine import Engine, EngineThread, validate_n
from chatts_amd.kv_blocks import BlockPool, KvPoolExhausted
from chatts_amd.tokenizer import SyntheticTokenizer

EOS = 7


# ---------------------------------------------------------------------------------------------------------------------------------
# a stub model with per-slot sampling settings and a fork: the token of (prompt tag, seed, step) comes from a script
# ---------------------------------------------------------------------------------------------------------------------------------
class _Cfg:
    eos_token_id = [EOS]
    ts = {"patch_size": 16}


class _OrdTok:
    """prompts are encoded character by character (the stub's tag is the first one); generated ids are decoded by `inner`"""

    def __init__(self, inner):
        self.inner = inner

    def encode(self, text):
        return [ord(c) for c in text]

    def decode(self, ids, skip_special_tokens=False):
        return self.inner.decode(ids, skip_special_tokens=skip_special_tokens)


class _Proc:
    def __init__(self, tokenizer):
        self.tokenizer = tokenizer

    def splice(self, prompt, series):
        if "BAD" in prompt:
            raise ValueError("malformed request")
        return prompt, [], []

    def pad_stack(self, encs):
        return None


class ForkStub:
    def __init__(self, max_batch, script, width=80, pool=None):
        self.max_batch, self.config, self.script, self._kv = max_batch, _Cfg(), script, pool
        self._kv_dynamic = pool is not None
        self.buf = {"pos_all": torch.zeros(max_batch, dtype=torch.int32), "out_tokens_all": torch.zeros((max_batch, width), dtype=torch.int64)}
        self.seq = [None] * max_batch                    # [tag, seed, steps produced]
        self.seed = [0] * max_batch
        self.log, self.rows_mode = [], False
        self._slot_idents = [[] for _ in range(max_batch)]

    def set_sampling(self, *a):
        self.rows_mode = False

    def set_sampling_rows(self):
        self.rows_mode = True

    def set_slot_sampling(self, slot, temperature=0.0, top_k=0, top_p=1.0, seed=0):
        self.seed[slot] = seed
        self.log.append(("settings", slot, temperature, seed))

    def _request_idents(self, ids, series, lens):
        return None

    def pick_slot(self, free, idents=None):
        return free[0]

    def request_tokens(self, ids, series=None, lens=None):
        return len(ids)

    def fork_tokens(self, T, max_new):
        return T + max_new - (T // self._kv.block_size) * self._kv.block_size

    def kv_fits(self, counts):
        return self._kv is None or self._kv.fits(counts)

    def kv_stats(self):
        return None

    def plan_pack(self, cands, free):
        return []

    def _first(self, slot, tag, T):
        self.seq[slot] = [tag, self.seed[slot], 1]
        self.buf["out_tokens_all"][slot, 0] = self.script(tag, self.seed[slot], 0)
        self.buf["pos_all"][slot] = T

    def admit_begin(self, slot, ids, series, lens, max_new):
        if self._kv is not None:
            self._kv.reserve(slot, len(ids) + max_new)
        return {"slot": slot, "T": len(ids), "done": 0, "ids": ids}

    def admit_fork(self, st, children, max_new=1):
        if self._kv is not None:
            nshare = st["T"] // self._kv.block_size
            made = []
            try:
                for c in children:
                    self._kv.release(c)
                    made.append(c)
                    self._kv.reserve(c, st["T"] + max_new - nshare * self._kv.block_size, protect={st["slot"], *children})
            except KvPoolExhausted:
                for c in made:
                    self._kv.release(c)
                self._kv.retire(st["slot"])
                raise
        st["fork"] = list(children)
        return st

    def admit_step(self, st, max_rows=None):
        a = st["done"]
        b = st["T"] if max_rows is None else min(st["T"], a + max_rows)
        self.log.append(("prefill", st["slot"], a, b))
        st["done"] = b
        if b < st["T"]:
            return False
        if st.get("fork"):
            self.log.append(("fork", st["slot"], tuple(st["fork"])))
            for c in st["fork"] if self._kv is not None else ():
                self._kv.fork(c, st["slot"], st["T"] // self._kv.block_size)
        for s in [st["slot"]] + list(st.get("fork") or []):
            self._first(s, st["ids"][0], st["T"])
        return True

    def _admit(self, slot, ids, series, lens, max_new):
        self.admit_step(self.admit_begin(slot, ids, series, lens, max_new))

    def batched_step(self):
        self.log.append(("step",))
        for s, st in enumerate(self.seq):
            if st is not None and int(self.buf["pos_all"][s]) >= 0 and st[2] < self.buf["out_tokens_all"].shape[1]:
                self.buf["out_tokens_all"][s, st[2]] = self.script(st[0], st[1], st[2])
                st[2] += 1

    def note_generated(self, slot, tokens):
        self.log.append(("retire", slot, len(tokens)))
        self.seq[slot] = None
        if self._kv is not None:
            self._kv.retire(slot)


def _engine(slots, script, tok=None, **kw):
    tok = tok or SyntheticTokenizer.for_config(cfgmod.preset("tiny-qwen2"))
    eos = kw.pop("eos", EOS)
    model = ForkStub(slots, script, pool=kw.pop("pool", None))
    model.config = type("Cfg", (_Cfg,), {"eos_token_id": [eos]})()
    return Engine(model, _Proc(_OrdTok(tok)), **kw), model


def _plain(tag, seed, step):
    return 1000 * tag + 100 * (seed % 10) + step


# ---------------------------------------------------------------------------------------------------------------------------------
# the stop rule
# ---------------------------------------------------------------------------------------------------------------------------------
def brute_force(tok, toks, stops, include, eos, stop_ids, max_tokens):
    """The definition, restated: text(j) = decode of the first j tokens without special tokens, minus one trailing U+FFFD.  j grows from 1;
    the sequence ends at the first j where token j is an EOS / stop token, or text(j) holds a stop string (the match that starts first,
    ties to the one listed first), or j == max_tokens - in that order at the same j.  -> (tokens, text, finish_reason, stop_reason)"""
    for j in range(1, len(toks) + 1):
        t = toks[j - 1]
        if t in eos or t in stop_ids:
            return toks[:j], tok.decode(toks[:j], skip_special_tokens=True), "stop", (t if t in stop_ids else None)
        text = tok.decode(toks[:j], skip_special_tokens=True)
        if text.endswith("�"):
            text = text[:-1]
        best = None
        for s in stops:
            i = text.find(s)
            if i >= 0 and (best is None or i < best[0]):
                best = (i, s)
        if best is not None:
            return toks[:j], text[:best[0] + (len(best[1]) if include else 0)], "stop", best[1]
        if j == max_tokens:
            return toks[:j], tok.decode(toks[:j], skip_special_tokens=True), "length", None
    raise AssertionError("the stream is shorter than max_tokens")


def _run_stop_case(tok, stream, stops, include, stop_ids, max_tokens, sync_every, eos=EOS):
    eng, model = _engine(2, lambda tag, seed, step: stream[step], tok, sync_every=sync_every, eos=eos)
    shown = []
    r = eng.add_request("A", max_tokens=max_tokens, stop=stops, include_stop_str_in_output=include, stop_token_ids=stop_ids,
                        on_tokens=lambda r, new, fin: shown.append(r.text))
    eng.run_until_done()
    assert r.error is None, r.error
    acc = ""
    for t in shown:                                        # what a stream shows never shrinks, and ends as the final text
        assert t.startswith(acc), (acc, t)
        acc = t
    assert acc == r.text
    return r.tokens, r.text, r.finish_reason, r.stop_reason


def _check_streams(tok, pool, rng, cases, special_eos):
    n_stop = n_eos = n_len = n_mid = 0
    for case in range(cases):
        L = rng.randint(3, 40)
        stream = [rng.choice(pool) for _ in range(64)]
        max_tokens = rng.randint(1, L)
        stop_ids = [rng.choice(pool)] if rng.random() < 0.3 else []
        if rng.random() < 0.5:
            stream[rng.randint(0, L - 1)] = special_eos
        full = tok.decode(stream[:L], skip_special_tokens=True)
        stops = []
        for _ in range(rng.randint(1, 4)):
            if len(full) >= 2:
                a = rng.randint(0, len(full) - 1)
                s = full[a:a + rng.randint(1, 7)]
                if s and "�" not in s:
                    stops.append(s)
        if stops and rng.random() < 0.5:                   # overlapping candidates: a longer string that starts earlier, a shorter inside
            a = max(0, full.find(stops[0]) - 2)
            stops.append(full[a:a + len(stops[0]) + 3] or stops[0])
            stops.append(stops[0][:max(1, len(stops[0]) // 2)])
        stops = [s for s in stops if s and "�" not in s] or ["\x00never\x00"]
        include = rng.random() < 0.5
        want = brute_force(tok, stream, stops, include, {special_eos}, set(stop_ids), max_tokens)
        got = [_run_stop_case(tok, stream, stops, include, stop_ids, max_tokens, h, special_eos) for h in (1, 4, 16)]
        for h, g in zip((1, 4, 16), got):
            assert g == want, (case, h, stops, include, max_tokens, g, want)
        n_stop += isinstance(want[3], str)
        n_eos += want[2] == "stop" and not isinstance(want[3], str)
        n_len += want[2] == "length"
        if isinstance(want[3], str):                       # the match starts inside one token's piece and ends in a later one
            j = len(want[0])
            before = tok.decode(stream[:j - 1], skip_special_tokens=True)
            n_mid += want[3] not in before and not before.endswith(want[1][-1:] if want[1] else "\x00")
    return n_stop, n_eos, n_len, n_mid


def test_stop_rule_against_brute_force_on_the_synthetic_tokenizer():
    tok = SyntheticTokenizer.for_config(cfgmod.preset("tiny-qwen2"))
    text = "The series rises, then drops sharply near point 103; a spike at t=17 stands out. Observation: none\nObservation"
    pool = sorted(set(tok.encode(text))) + [300001 % tok.word_hi, 4242]       # + ids the tokenizer has never seen: "<|id|>" pieces
    pool = [p for p in pool if p != EOS]
    n_stop, n_eos, n_len, n_mid = _check_streams(tok, pool, random.Random(5), 150, EOS)
    assert n_stop >= 30 and n_eos >= 10 and n_len >= 10 and n_mid >= 5, (n_stop, n_eos, n_len, n_mid)


@pytest.fixture(scope="module")
def hf_tok():
    from tokenizers import Tokenizer, decoders, models, pre_tokenizers, trainers
    from transformers import PreTrainedTokenizerFast
    tok = Tokenizer(models.BPE())
    tok.pre_tokenizer = pre_tokenizers.ByteLevel(add_prefix_space=False)
    tok.decoder = decoders.ByteLevel()
    corpus = ["I have 3 time series. Please analyze the local changes in these time series.\nObservation: a spike",
              "ünïcode text, 时间序列 异常 检测 ✓, numbers 0123456789 and punctuation ;:,.!?()[]|=-"] * 4
    trainer = trainers.BpeTrainer(vocab_size=420, special_tokens=["<|endoftext|>", "<|im_start|>", "<|im_end|>"],
                                  initial_alphabet=pre_tokenizers.ByteLevel.alphabet())
    tok.train_from_iterator(corpus, trainer)
    return PreTrainedTokenizerFast(tokenizer_object=tok, eos_token="<|im_end|>", pad_token="<|endoftext|>")


def test_stop_rule_against_brute_force_on_a_byte_level_bpe_tokenizer(hf_tok):
    """multi-byte characters split over tokens: the pool holds the single-byte pieces of 时间序列 ✓ ü next to merged words"""
    tok = hf_tok
    text = "Spike at t=17: ünïcode, 时间序列 异常 检测 ✓ done.\nObservation: the series rises"
    ids = tok.encode(text)
    bytes_of = [tok.convert_tokens_to_ids(c) for c in tok.backend_tokenizer.pre_tokenizer.pre_tokenize_str("时间✓ü")[0][0]]
    pool = sorted(set(ids) | set(bytes_of))
    eos = tok.convert_tokens_to_ids("<|im_end|>")
    assert eos not in pool and all(isinstance(p, int) for p in pool)
    # in order, token by token: a stop string made of a character whose bytes are split over tokens, matched only once it is whole
    toks, out, reason, why = _run_stop_case(tok, ids + [ids[0]] * 40, ["列 异"], False, [], 60, 4)
    assert out == text[:text.index("列 异")] and reason == "stop" and why == "列 异"
    assert toks == brute_force(tok, ids + [ids[0]] * 40, ["列 异"], False, {eos}, set(), 60)[0]
    n_stop, n_eos, n_len, n_mid = _check_streams(tok, pool, random.Random(11), 120, eos)
    assert n_stop >= 20 and n_eos >= 10 and n_len >= 10, (n_stop, n_eos, n_len, n_mid)


def test_stop_checker_pieces():
    assert detok.normalize_stop(None) == [] and detok.normalize_stop("x") == ["x"] and detok.normalize_stop(("a", "b")) == ["a", "b"]
    for bad in ("", [""], ["a", 3], 5, ["s"] * 17, [None]):
        with pytest.raises(ValueError):
            detok.normalize_stop(bad)
    assert detok.normalize_stop(["s%d" % i for i in range(16)])
    assert detok.find_stop("abcabc", ["ca", "bc", "b"]) == (1, "bc")           # first start wins, ties to the one listed first
    assert detok.find_stop("abc", ["x"]) is None
    assert detok.held_back("The Obs", ["\nObservation", "Observation"]) == 3
    assert detok.held_back("abc\n", ["\nObservation"]) == 1 and detok.held_back("abc", ["c"]) == 0
    assert server.IncrementalDecoder is detok.IncrementalDecoder


# ---------------------------------------------------------------------------------------------------------------------------------
# the engine with n > 1
# ---------------------------------------------------------------------------------------------------------------------------------
def test_parent_waits_for_n_slots_one_prefill_one_fork_and_seeds():
    eng, model = _engine(4, _plain, sync_every=2)
    a = eng.add_request("A" * 10, max_tokens=6, ignore_eos=True)
    b = eng.add_request("B" * 10, max_tokens=9, ignore_eos=True)
    p = eng.add_request("P" * 12, max_tokens=5, ignore_eos=True, n=3, temperature=0.8, seed=41)
    c = eng.add_request("C" * 10, max_tokens=3, ignore_eos=True)           # behind the parent: may pass it while it waits for slots
    assert p.n == 3 and [k.index for k in p.children] == [0, 1, 2] and all(k.parent is p for k in p.children)
    done = []
    while eng.has_work():
        done += eng.step()
        running = [r for r in eng.slots if r is not None]
        if any(k in running for k in p.children):          # siblings are admitted together
            assert sum(k in running or k.finished for k in p.children) == 3
    assert [r for r in done if r is p] == [p] and not any(k in done for k in p.children)      # the caller's request completes once
    order = [r.prompt[0] for r in done]
    assert order.index("A") < order.index("P") and order.index("C") < order.index("P")       # it waited for three free slots
    tag = ord("P")
    prefills = [e for e in model.log if e[0] == "prefill" and e[3] == 12]
    forks = [e for e in model.log if e[0] == "fork"]
    assert len(prefills) == 1 and len(forks) == 1 and len(forks[0][2]) == 2 and forks[0][1] == prefills[0][1]
    assert [k.sampling[3] for k in p.children] == [41, 42, 43]
    for i, k in enumerate(p.children):                     # each sibling drew with its own seed, whatever slot it landed in
        assert k.tokens == [_plain(tag, 41 + i, s) for s in range(5)] and k.finish_reason == "length" and k.finished
    assert p.finished and p.outputs == p.children and a.outputs == [a]
    assert a.tokens == [_plain(ord("A"), a.sampling[3], s) for s in range(6)] and len(b.tokens) == 9 and len(c.tokens) == 3
    # no decode step between the parent's prefill and its siblings' first tokens
    i = model.log.index(prefills[0])
    assert model.log[i + 1][0] == "fork"


def test_seed_wraps_and_default_seed_is_the_one_of_n_1():
    eng, _ = _engine(4, _plain)
    p = eng.add_request("P", n=3, seed=2 ** 32 - 1, temperature=1.0)
    assert [k.sampling[3] for k in p.children] == [2 ** 32 - 1, 0, 1]
    eng2, _ = _engine(4, _plain)
    one = eng2.add_request("P", temperature=1.0)
    eng3, _ = _engine(4, _plain)
    many = eng3.add_request("P", temperature=1.0, n=2)
    assert many.children[0].sampling == one.sampling and many.children[1].sampling[3] == (one.sampling[3] + 1) & 0xFFFFFFFF
    nxt2, nxt3 = eng2.add_request("Q", temperature=1.0), eng3.add_request("Q", temperature=1.0)
    assert nxt2.sampling == nxt3.sampling                  # a parent takes one arrival number, like any request


def test_children_retire_independently_and_the_parent_completes_with_the_last():
    ends = {50: 2, 51: 6}                                  # seed -> step at which the sibling emits EOS

    def script(tag, seed, step):
        return EOS if ends.get(seed) == step else _plain(tag, seed, step)
    eng, model = _engine(3, script, sync_every=1)
    events = []
    p = eng.add_request("P" * 8, max_tokens=12, n=3, seed=50, temperature=0.7,
                        on_tokens=lambda r, new, fin: events.append((r.index, list(new), fin)))
    late = None
    done = []
    while eng.has_work():
        done += eng.step()
        if late is None and p.children[0].finished:       # sibling 0's slot is free while its brothers still run: a newcomer takes it
            assert not p.finished and sum(r is not None for r in eng.slots) == 2
            late = eng.add_request("L" * 4, max_tokens=2, ignore_eos=True)
    assert late is not None and late.finished and p.finished
    assert [len(k.tokens) for k in p.children] == [3, 7, 12]
    assert [k.finish_reason for k in p.children] == ["stop", "stop", "length"] and [k.stop_reason for k in p.children] == [None] * 3
    assert done.index(late) < done.index(p)
    for i, k in enumerate(p.children):                     # streaming callers get each sibling's tokens under its index
        assert [t for idx, new, _ in events if idx == i for t in new] == k.tokens
        assert [fin for idx, _, fin in events if idx == i][-1] is True
    assert [e for e in model.log if e[0] == "retire"][0][2] == 3


def test_value_errors():
    eng, _ = _engine(2, _plain)
    for kw in (dict(n=3), dict(n=0), dict(n=True), dict(n=1.5), dict(n=2, best_of=3), dict(best_of=2), dict(stop=""), dict(stop=[""]),
               dict(stop=["a", 1]), dict(stop=["x"] * 17), dict(stop=7)):
        with pytest.raises(ValueError):
            eng.add_request("P", **kw)
    assert not eng.waiting
    assert eng.add_request("P", n=2, best_of=2).n == 2 and eng.add_request("P", n=1, best_of=None, stop=[]).n == 1
    assert validate_n(None) == 1 and validate_n(4, 4, 4) == 4
    noproc = Engine(ForkStub(2, _plain), type("P", (), {"tokenizer": None})())
    with pytest.raises(ValueError, match="tokenizer"):
        noproc.add_request("P", stop="x")

    class Grouped:                                         # a model with one baked-in configuration has no per-slot seeds
        max_batch, config, buf = 2, _Cfg(), {"pos_all": torch.zeros(2, dtype=torch.int32)}

        def admit_fork(self, st, children, max_new=1):
            return st
    with pytest.raises(ValueError, match="per-slot"):
        Engine(Grouped(), _Proc(_OrdTok(None))).add_request("P", n=2)


def test_paged_pool_counts_shared_prompt_blocks_once_and_waits():
    """block 64, prompt 130 (two whole blocks + 2 rows), 20 new tokens: a single sequence needs 3 blocks, each further sibling 1.
    A pool of 5 blocks holds n = 3; while another request holds 2 blocks the parent waits, then runs."""
    pool = BlockPool(5, 64, 3, 4)
    eng, model = _engine(3, _plain, pool=pool, sync_every=2)
    other = eng.add_request("O" * 100, max_tokens=8, ignore_eos=True)       # 2 blocks
    p = eng.add_request("P" * 130, max_tokens=20, ignore_eos=True, n=2)     # 3 + 1 blocks: does not fit beside `other`
    saw_waiting = False
    done = []
    while eng.has_work():
        done += eng.step()
        pool.check()
        if other in [r for r in eng.slots if r is not None] and p in eng.waiting:
            saw_waiting = True
        if p.children[0] in eng.slots:
            rows = [pool.rows[eng.slots.index(k)] for k in p.children]
            assert rows[0][:2] == rows[1][:2] and rows[0][2] != rows[1][2] and pool.shared_blocks() == 2
    assert saw_waiting and done.index(other) < done.index(p) and all(len(k.tokens) == 20 for k in p.children)
    # a request that can never fit is answered with an error instead of waiting for ever
    eng2, _ = _engine(3, _plain, pool=BlockPool(3, 64, 3, 4))
    q = eng2.add_request("Q" * 130, max_tokens=20, ignore_eos=True, n=3)
    eng2.run_until_done()
    assert q.finished and "KV positions" in str(q.error) and all(k.finished for k in q.children)


def test_chunked_prefill_of_a_parent_places_every_sibling():
    eng, model = _engine(4, _plain, sync_every=2, prefill_chunk_tokens=16)
    a = eng.add_request("A" * 8, max_tokens=30, ignore_eos=True)
    eng.step()
    p = eng.add_request("P" * 50, max_tokens=4, ignore_eos=True, n=3, seed=9, temperature=0.5)
    eng.run_until_done()
    chunks = [e for e in model.log if e[0] == "prefill" and e[1] == 1]
    assert [(e[2], e[3]) for e in chunks] == [(0, 16), (16, 32), (32, 48), (48, 50)]      # ONE prefill, in chunks, between a's steps
    assert len([e for e in model.log if e[0] == "fork"]) == 1
    assert [k.tokens for k in p.children] == [[_plain(ord("P"), 9 + i, s) for s in range(4)] for i in range(3)] and len(a.tokens) == 30


def test_control_plane_message_carries_the_new_fields():
    class Control:
        def __init__(self):
            self.sent = []

        def publish(self, new, stop=False):
            self.sent.append((json.loads(json.dumps(new)), stop))       # picklable / plain data only
    tok = SyntheticTokenizer.for_config(cfgmod.preset("tiny-qwen2"))
    words = tok.encode("alpha beta gamma delta")
    eng, _ = _engine(2, lambda tag, seed, step: words[(seed + step) % len(words)], tok, sync_every=1)
    control = Control()
    et = EngineThread(eng, control=control)
    try:
        holder, ev = [], threading.Event()
        et.submit(prompt="P", timeseries=[], holder=holder, max_tokens=6, temperature=0.9, seed=3, n=2, stop=[" gamma"],
                  include_stop_str_in_output=True, on_tokens=lambda r, new, fin: ev.set() if all(k.finished for k in r.parent.children) else None)
        bad = []
        et.submit(prompt="P", timeseries=[], holder=bad, n=3, on_tokens=lambda r, new, fin: None)      # n > slots: refused before it is announced
        assert ev.wait(10)
        t0 = time.time()
        while not bad and time.time() - t0 < 10:
            time.sleep(0.01)
    finally:
        et.close()
    msgs = [m for new, _ in control.sent for m in new]
    assert len(msgs) == 1 and msgs[0]["n"] == 2 and msgs[0]["stop"] == [" gamma"] and msgs[0]["include_stop_str_in_output"] is True
    assert msgs[0]["seed"] == 3 and "on_tokens" not in msgs[0] and "holder" not in msgs[0]
    assert isinstance(bad[0].error, ValueError) and "max_num_seqs" in str(bad[0].error)
    # a follower that replays the message makes the same decisions from the same tokens
    follower, _ = _engine(2, lambda tag, seed, step: words[(seed + step) % len(words)], tok, sync_every=1)
    f = follower.add_request(**msgs[0])
    follower.run_until_done()
    p = holder[0]
    assert [k.tokens for k in f.children] == [k.tokens for k in p.children] and [k.text for k in f.children] == [k.text for k in p.children]
    assert any(k.stop_reason == " gamma" and k.text.endswith(" gamma") for k in p.children)


def test_engine_thread_answers_what_the_engine_cannot_serve_and_lives_on():
    """stop without a tokenizer, n > 1 on a model without a fork: refused before the request is announced to follower ranks, answered
    with an error, and the thread keeps serving"""
    class Control:
        sent = []

        def publish(self, new, stop=False):
            self.sent.append(list(new))
    model = ForkStub(2, _plain)
    eng = Engine(model, type("P", (_Proc,), {})(None))         # a processor without a tokenizer
    eng.processor.tokenizer = None
    et = EngineThread(eng, control=Control())
    try:
        bad1, bad2 = [], []
        et.submit(prompt="P", timeseries=[], holder=bad1, stop="x", on_tokens=lambda r, new, fin: None)
        et.submit(prompt="P", timeseries=[], holder=bad2, n=3, on_tokens=lambda r, new, fin: None)
        t0 = time.time()
        while not (bad1 and bad2) and time.time() - t0 < 10:
            time.sleep(0.01)
        assert isinstance(bad1[0].error, ValueError) and "tokenizer" in str(bad1[0].error) and isinstance(bad2[0].error, ValueError)
        assert et.error is None and et.thread.is_alive() and not any(Control.sent)
    finally:
        et.close()


def test_engine_thread_answers_controls_and_logprobs_the_model_lacks_and_lives_on():
    """ForkStub has neither set_slot_controls nor set_logprobs: Engine.add_request raises for such a request, so the engine thread must
    refuse it BEFORE it is announced (after the publish every rank would go down) - an error on that request, nothing published for
    it, and the next valid request is served."""
    class Control:
        def __init__(self):
            self.sent = []

        def publish(self, new, stop=False):
            self.sent.append(list(new))
    eng, model = _engine(2, _plain)
    assert not hasattr(model, "set_slot_controls") and not hasattr(model, "set_logprobs")
    for kw in (dict(min_p=0.1), dict(logprobs=1)):
        with pytest.raises(ValueError):
            eng.add_request("P", **kw)
    control = Control()
    et = EngineThread(eng, control=control)
    try:
        bad1, bad2, good, ev = [], [], [], threading.Event()
        et.submit(prompt="P", timeseries=[], holder=bad1, frequency_penalty=0.5, on_tokens=lambda r, new, fin: None)
        et.submit(prompt="P", timeseries=[], holder=bad2, logprobs=2, on_tokens=lambda r, new, fin: None)
        et.submit(prompt="Q", timeseries=[], holder=good, max_tokens=3, ignore_eos=True, on_tokens=lambda r, new, fin: fin and ev.set())
        assert ev.wait(10)
        assert isinstance(bad1[0].error, ValueError) and "does not apply" in str(bad1[0].error) and bad1[0].finish_reason == "error"
        assert isinstance(bad2[0].error, ValueError) and "does not compute logprobs" in str(bad2[0].error)
        assert good[0].error is None and good[0].tokens == [_plain(ord("Q"), good[0].sampling[3], s) for s in range(3)]
        assert et.error is None and et.thread.is_alive()
        assert [m["prompt"] for new in control.sent for m in new] == ["Q"]        # the refused ones never reached a follower
    finally:
        et.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# the server on the engine (stub model), the offline surfaces
# ---------------------------------------------------------------------------------------------------------------------------------
ANSWERS = ["The series rises.\nObservation: it drops near point 103 and recovers later on",
           "A spike at t=17 stands out; nothing else.\nObservation: none at all, really nothing",
           "Flat, then noisy, then flat again for a long while and so on and on"]


@pytest.fixture()
def app_client():
    from starlette.testclient import TestClient
    tok = SyntheticTokenizer.for_config(cfgmod.preset("tiny-qwen2"))
    eos = tok.special["<|im_end|>"]
    streams = [tok.encode(a) + [eos] * 80 for a in ANSWERS]
    eng, model = _engine(4, lambda tag, seed, step: streams[seed % 3][step], tok, sync_every=3, eos=eos)
    et = EngineThread(eng)
    client = TestClient(server.create_app(et, _OrdTok(tok), "chatts", limit_timeseries=3))
    yield client, model
    et.close()


def _stream(client, url, body):
    with client.stream("POST", url, json=dict(body, stream=True)) as resp:
        assert resp.status_code == 200
        events = [line[6:] for line in resp.iter_lines() if line.startswith("data: ")]
    assert events[-1] == "[DONE]"
    return [json.loads(e) for e in events[:-1]]


def test_server_n_choices_blocking_and_streamed(app_client):
    client, model = app_client
    body = {"prompt": "P", "max_tokens": 60, "n": 3, "seed": 0, "temperature": 0.7}
    d = client.post("/v1/completions", json=body).json()
    assert [c["index"] for c in d["choices"]] == [0, 1, 2] and [c["text"] for c in d["choices"]] == ANSWERS
    assert all(c["finish_reason"] == "stop" for c in d["choices"]) and "token_ids" not in d
    assert d["usage"]["prompt_tokens"] == 1 and d["usage"]["completion_tokens"] == sum(len(c["token_ids"]) for c in d["choices"])
    assert len([e for e in model.log if e[0] == "prefill"]) == 1 and len([e for e in model.log if e[0] == "fork"]) == 1
    one = client.post("/v1/completions", json=dict(body, n=1)).json()
    assert len(one["choices"]) == 1 and one["choices"][0]["text"] == ANSWERS[0] and len(one["token_ids"]) == one["usage"]["completion_tokens"]
    chunks = _stream(client, "/v1/completions", body)
    for i in range(3):
        mine = [c["choices"][0] for c in chunks if c["choices"][0]["index"] == i]
        assert "".join(c["text"] for c in mine) == ANSWERS[i] and mine[-1]["finish_reason"] == "stop"
        assert [c["finish_reason"] for c in mine[:-1]] == [None] * (len(mine) - 1)
    msgs = [{"role": "user", "content": "hello"}]
    chat = client.post("/v1/chat/completions", json={"messages": msgs, "max_tokens": 60, "n": 2, "seed": 1, "temperature": 0.7}).json()
    assert [c["message"]["content"] for c in chat["choices"]] == ANSWERS[1:3] and [c["index"] for c in chat["choices"]] == [0, 1]
    cc = _stream(client, "/v1/chat/completions", {"messages": msgs, "max_tokens": 60, "n": 2, "seed": 1, "temperature": 0.7})
    for i in range(2):
        mine = [c["choices"][0] for c in cc if c["choices"][0]["index"] == i]
        assert mine[0]["delta"]["role"] == "assistant" and "".join(c["delta"].get("content", "") for c in mine) == ANSWERS[1 + i]


def test_server_stop_strings_and_400s(app_client):
    client, model = app_client
    body = {"prompt": "P", "max_tokens": 60, "seed": 0, "temperature": 0.7}
    # the ReAct agent's stop (a string); it ends in the middle of a harvest of three tokens and in the middle of a delta
    d = client.post("/v1/completions", json=dict(body, stop="\nObservation")).json()
    c = d["choices"][0]
    assert c["text"] == "The series rises." and c["finish_reason"] == "stop" and c["stop_reason"] == "\nObservation"
    tok_ids = d["token_ids"]
    full = client.post("/v1/completions", json=body).json()
    assert tok_ids == full["token_ids"][:len(tok_ids)] and len(tok_ids) < len(full["token_ids"])
    inc = client.post("/v1/completions", json=dict(body, stop=["zzz", "ops near"], include_stop_str_in_output=True)).json()["choices"][0]
    assert inc["text"] == ANSWERS[0][:ANSWERS[0].index("ops near")] + "ops near" and inc["stop_reason"] == "ops near"
    for stop, extra in (("\nObservation", {}), (["zzz", "ops near"], {"include_stop_str_in_output": True}), ("t dr", {}), (["never"], {})):
        blocking = client.post("/v1/completions", json=dict(body, stop=stop, n=3, **extra)).json()
        chunks = _stream(client, "/v1/completions", dict(body, stop=stop, n=3, **extra))
        for i in range(3):
            mine = [ch["choices"][0] for ch in chunks if ch["choices"][0]["index"] == i]
            assert "".join(ch["text"] for ch in mine) == blocking["choices"][i]["text"], (stop, i)
            assert mine[-1]["finish_reason"] == blocking["choices"][i]["finish_reason"]
    chat = client.post("/v1/chat/completions", json={"messages": [{"role": "user", "content": "x"}], "max_tokens": 60, "seed": 1,
                                                      "temperature": 0.5, "stop": ["Observation"]}).json()
    assert chat["choices"][0]["message"]["content"] == ANSWERS[1][:ANSWERS[1].index("Observation")]
    n_seen = len([e for e in model.log if e[0] == "prefill"])
    for bad in ({"n": 0}, {"n": 5}, {"n": "2"}, {"n": 1.5}, {"n": True}, {"n": 2, "best_of": 3}, {"stop": ""}, {"stop": [""]}, {"stop": 3},
                {"stop": ["a", 2]}, {"stop": ["s"] * 17}, {"include_stop_str_in_output": "yes"}):
        for url, base in (("/v1/completions", {"prompt": "P"}), ("/v1/chat/completions", {"messages": [{"role": "user", "content": "x"}]})):
            r = client.post(url, json=dict(base, **bad))
            assert r.status_code == 400 and r.json()["error"]["message"], (url, bad)
    assert len([e for e in model.log if e[0] == "prefill"]) == n_seen


def test_sampling_from_body_passes_the_new_fields_only_when_set():
    assert not {"n", "stop", "include_stop_str_in_output", "best_of"} & set(server.sampling_from_body({"max_tokens": 4}))
    sp = server.sampling_from_body({"n": 2, "stop": ["a", "b"], "include_stop_str_in_output": True}, max_num_seqs=2)
    assert sp["n"] == 2 and sp["stop"] == ["a", "b"] and sp["include_stop_str_in_output"] is True
    assert server.sampling_from_body({"stop": "x"})["stop"] == "x"
    with pytest.raises(ValueError, match="max_num_seqs"):
        server.sampling_from_body({"n": 3}, max_num_seqs=2)


def test_sampling_params_and_llm_client_sample_n():
    from chatts_amd.inference import LLMClient
    from chatts_amd.llm import CompletionOutput, RequestOutput, SamplingParams
    sp = SamplingParams(n=3, stop="\nObservation", include_stop_str_in_output=True, best_of=3)
    assert sp.n == 3 and sp.stop == ["\nObservation"] and sp.include_stop_str_in_output is True
    d = SamplingParams()
    assert d.n == 1 and d.stop == [] and d.include_stop_str_in_output is False and d.best_of is None
    for kw in (dict(n=0), dict(n=2, best_of=4), dict(stop=[""]), dict(stop=["x"] * 17), dict(n="2")):
        with pytest.raises(ValueError):
            SamplingParams(**kw)
    c = CompletionOutput("t", [1], index=2, finish_reason="stop", stop_reason="x")
    assert (c.index, c.finish_reason, c.stop_reason) == (2, "stop", "x") and CompletionOutput("t", [1]).index == 0

    class StubLLM:
        def __init__(self):
            self.calls = []

        def generate(self, reqs, sp, use_tqdm=False):
            self.calls.append((reqs, sp))
            return [RequestOutput(r["prompt"], [1], [CompletionOutput(f"{r['prompt'][-3:]}#{i}", [i], index=i) for i in range(sp.n)])
                    for r in reqs]
    llm = StubLLM()
    client = LLMClient(llm=llm, sample_n=2, batch_size=2)
    assert client.default_sampling_params().n == 2
    ans = client.llm_batch_generate(["q one", "q two", "q 3"], use_chat_template=False)
    assert ans == [["one#0", "one#1"], ["two#0", "two#1"], ["q 3#0", "q 3#1"]] and llm.calls[0][1].n == 2
    single = LLMClient(llm=StubLLM(), batch_size=2)
    assert single.default_sampling_params().n == 1
    assert single.llm_batch_generate(["q one"], use_chat_template=False) == ["one#0"]
    with pytest.raises(ValueError):
        LLMClient(llm=llm, sample_n=0)


# ---------------------------------------------------------------------------------------------------------------------------------
# the C-ABI: exported, declared, and refusing bad arguments before anything touches a device
# ---------------------------------------------------------------------------------------------------------------------------------
def test_fork_entry_points_are_declared_and_validate_their_arguments():
    import os
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "chatts_amd.h")).read()
    for name in ("chatts_kv_fork", "chatts_logit_state_fork"):
        assert name in _lib.SIGNATURES and f"int {name}(" in header
    assert f"#define CHATTS_FORK_MAX_DST {_lib.FORK_MAX_DST}" in header
    lib = _lib.load()
    assert lib.chatts_abi_version() == 9
    fake = 0x10000                                         # never dereferenced on the host: every call below ends in its checks
    L, H, CTX, SLOTS = 2, 2, 256, 4
    ls, ss = H * CTX * 128, L * H * CTX * 128

    def cache(**kw):
        f = dict(k=fake, v=fake, max_ctx=CTX, dtype=_lib.KV_F32, block_table=None, block_size=0, table_stride=0)
        f.update(kw)
        return _lib.KvCache(**f)

    def fork(c, dst, src=0, t0=0, t1=100, layers=L, heads=H, slots=SLOTS, lstride=ls, sstride=ss, blocks=0):
        arr = (C.c_int32 * max(len(dst), 1))(*dst)
        return lib.chatts_kv_fork(C.byref(c) if c is not None else None, layers, heads, slots, lstride, sstride, blocks, src, arr, len(dst),
                                  t0, t1, None)
    assert fork(cache(), [1, 2], t0=64, t1=64) == _lib.OK                # nothing to copy: valid, nothing enqueued
    assert fork(cache(), [1, 2], t0=64, t1=64, lstride=ls + 2, sstride=L * (ls + 2)) == _lib.E_BADARG      # ... but checked like any call
    assert fork(cache(), [1, 2], t0=64, t1=64, layers=40000, sstride=40000 * ls) == _lib.E_BADARG
    bad = [fork(None, [1]), fork(cache(k=None), [1]), fork(cache(dtype=7), [1]), fork(cache(), []), fork(cache(), list(range(1, 66)), slots=80),
           fork(cache(), [0]), fork(cache(), [1, 1]), fork(cache(), [4]), fork(cache(), [-1]), fork(cache(), [1], src=4),
           fork(cache(), [1], t1=CTX + 1), fork(cache(), [1], t0=5, t1=4), fork(cache(), [1], t0=-1), fork(cache(), [1], layers=0),
           fork(cache(), [1], lstride=ls - 128), fork(cache(), [1], sstride=ss - 128), fork(cache(k=fake + 4), [1]),
           fork(cache(block_table=fake, block_size=48, table_stride=8), [1], blocks=8, lstride=8 * H * 48 * 128),
           fork(cache(block_table=fake, block_size=64, table_stride=3), [1], blocks=8, lstride=8 * H * 64 * 128),
           fork(cache(block_table=fake, block_size=64, table_stride=4), [1], blocks=8, lstride=8 * H * 64 * 128 - 128),
           fork(cache(block_table=fake, block_size=64, table_stride=4), [1], blocks=0, lstride=8 * H * 64 * 128)]
    assert bad == [_lib.E_BADARG] * len(bad), bad
    assert b"kv_fork" in lib.chatts_last_error()

    def sfork(state, dst, src=0, stride=1000, vocab=1000, rows=4):
        arr = (C.c_int32 * max(len(dst), 1))(*dst)
        return lib.chatts_logit_state_fork(state, stride, vocab, rows, src, arr, len(dst), None)
    bad = [sfork(None, [1]), sfork(fake, []), sfork(fake, [0]), sfork(fake, [4]), sfork(fake, [1, 2, 1]), sfork(fake, [1], src=-1),
           sfork(fake, [1], stride=999), sfork(fake, [1], vocab=0), sfork(fake, list(range(1, 66)), rows=80)]
    assert bad == [_lib.E_BADARG] * len(bad), bad
