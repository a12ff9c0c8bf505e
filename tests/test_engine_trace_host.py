"""CPU: the scheduler's behaviour, pinned call by call.

Every scenario below is one deterministic script of add_request / step calls on a stub model behind a `Recorder`; the trace - every
method the engine calls on the model with its arguments, every on_tokens callback, the list every step() returns - is compared with
tests/golden/engine_trace.json exactly (it is a pure function of the script: no tolerance).  The golden file was written once, by
`python tests/test_engine_trace_host.py --write`, and is not regenerated: a refactor of chatts_amd/engine.py passes only if the model
sees the same calls in the same order and every caller the same tokens at the same iteration."""
import json
import os
import sys

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from chatts_amd.engine import Engine
from chatts_amd.kv_blocks import BlockPool
from tests.test_engine_host import StubModel, _Proc
from tests.test_parallel_sampling_host import EOS, ForkStub, _plain

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "engine_trace.json")


# ---- the recorder -----------------------------------------------------------------------------------------------------------------
def _value(v):
    if v is None or isinstance(v, (bool, int, float, str)):
        return v
    if isinstance(v, (list, tuple)):
        return [_value(x) for x in v]
    if isinstance(v, dict) and "slot" in v and "T" in v:             # an admission state
        return {"slot": v["slot"], "T": v["T"], "done": v["done"], "fork": _value(v.get("fork"))}
    return type(v).__name__


class Recorder:
    """the model as the engine sees it: attributes pass through (hasattr probes answer as on the bare stub), calls are recorded"""

    def __init__(self, model, trace):
        self.__dict__["_model"], self.__dict__["_trace"] = model, trace

    def __getattr__(self, name):
        v = getattr(self.__dict__["_model"], name)
        if not callable(v):
            return v

        def call(*a, **k):
            self._trace.append([name, [_value(x) for x in a] + [[key, _value(k[key])] for key in sorted(k)]])
            return v(*a, **k)
        return call


class Session:
    """one engine on a recorded stub; `add` is add_request with the recording callback, `steps` a fixed number of step() calls"""

    def __init__(self, model, processor=None, max_bypass=None, **kw):
        self.trace, self.model = [], model
        self.eng = Engine(Recorder(model, self.trace), processor or _Proc(), **kw)
        if max_bypass is not None:
            self.eng.max_bypass = max_bypass
        step = self.eng.step

        def recorded_step():
            done = step()
            self.trace.append(["done", [r.rid for r in done]])
            return done
        self.eng.step = recorded_step                # run_until_done goes through it too

    def _emit(self, r, new, finished):
        self.trace.append(["emit", r.rid, r.index, list(new), finished, r.finish_reason, r.stop_reason,
                           None if r.error is None else type(r.error).__name__])

    def add(self, prompt, **kw):
        return self.eng.add_request(prompt, on_tokens=self._emit, **kw)

    def steps(self, n):
        for _ in range(n):
            self.eng.step()

    def finish(self):
        self.eng.run_until_done()
        assert not self.eng.has_work() and all(s is None for s in self.eng.slots) and self.eng.prefilling is None
        return self.trace


# ---- the stubs: what StubModel / ForkStub lack ---------------------------------------------------------------------------------------
class _Extras:
    """logprobs and logit controls as the real model exposes them to the engine (the mode flags included)"""
    _logprobs_on = False
    _controls_on = False

    def set_logprobs(self, on):
        self._logprobs_on = bool(on)

    def read_logprobs(self, slot, a, b, k):
        return [(-0.25 * (i + 1), 1 + i % 3, [(100 + j, -0.5 * (j + 1)) for j in range(k)]) for i in range(a, b)]

    def set_logit_controls(self, on):
        self._controls_on = bool(on)

    def set_slot_controls(self, slot, repetition_penalty=1.0, frequency_penalty=0.0, presence_penalty=0.0, min_p=0.0):
        pass


class RowsModel(_Extras, StubModel):
    """per-slot sampling settings ("mixed" mode)"""

    def set_slot_sampling(self, slot, temperature=0.0, top_k=0, top_p=1.0, seed=0):
        pass

    def set_sampling_rows(self):
        pass


class GroupedModel(StubModel):
    """one baked-in configuration; the library refuses temperature 0.123"""

    def set_sampling(self, *a):
        if a and a[0] == 0.123:
            raise ValueError("refused by the library")
        super().set_sampling(*a)


class ChunkFailModel(StubModel):
    """the prompt whose first character is `fail_tag` loses the device on its second chunk"""
    fail_tag = None

    def admit_step(self, st, max_rows=None):
        if st["ids"][0] == self.fail_tag and st["done"] > 0:
            raise RuntimeError("device lost")
        return super().admit_step(st, max_rows)


class ForkModel(_Extras, ForkStub):
    pass


class _CharTok:
    """token id = code point; the EOS id decodes to nothing"""

    def encode(self, text):
        return [ord(c) for c in text]

    def decode(self, ids, skip_special_tokens=False):
        return "".join(chr(i) for i in ids if not (skip_special_tokens and i == EOS))


class _CharProc(_Proc):
    tokenizer = _CharTok()


# ---- the scenarios ------------------------------------------------------------------------------------------------------------------
def _modes(greedy_return_steps):
    """greedy, sampled, greedy again on a per-slot model: the rows mode is entered, idles for fewer than 3 iterations, is re-armed by a
    late sampled arrival and finally left; a logprobs and a controls request with other lifetimes switch their modes on their own."""
    s = Session(RowsModel(4, pack=False), sync_every=2, greedy_return_steps=greedy_return_steps)
    s.add("G" * 10, max_tokens=40, ignore_eos=True)                               # greedy, keeps the engine stepping throughout
    s.steps(2)
    s.add("S" * 10, max_tokens=2, temperature=0.7, top_p=0.9, seed=5)
    s.add("L" * 10, max_tokens=3, logprobs=2)
    s.steps(4)                                                                    # nobody has sampled for two iterations ...
    s.add("T" * 10, max_tokens=2, temperature=0.2, top_k=40)                      # ... and a sampled request re-arms the rows mode
    s.add("C" * 10, max_tokens=3, repetition_penalty=1.3, frequency_penalty=0.5)
    s.steps(1)
    s.add("M" * 10, max_tokens=5, logprobs=0)                                     # re-arms logprobs
    s.steps(4)
    s.add("K" * 10, max_tokens=6, presence_penalty=0.5)                           # re-arms the controls
    s.steps(3)
    s.add("H" * 10, max_tokens=3)                                                 # greedy again
    return s.finish()


MODES_TAGS = "GSLTCMKH"                                                           # request ids 1 .. 8 of the script above


def _grouped():
    """three sampling keys interleaved on a grouped model: the head with another key is overtaken max_bypass = 2 times, then blocks;
    the key the library refuses fails that request only"""
    s = Session(GroupedModel(2, pack=False), sync_every=1, max_bypass=2)
    s.add("A" * 10, max_tokens=3)
    s.steps(1)
    s.add("B" * 10, max_tokens=2, temperature=0.5, seed=4)                        # another key: waits for the greedy batch to drain
    s.add("C" * 10, max_tokens=3)
    s.add("D" * 10, max_tokens=2)
    s.add("E" * 10, max_tokens=2)                                                 # the third latecomer: B is not overtaken again
    s.add("F" * 10, max_tokens=2, temperature=0.123)
    s.steps(3)
    s.add("I" * 10, max_tokens=2, temperature=0.5, seed=4)                        # B's key
    s.add("J" * 10, max_tokens=2)
    return s.finish()


def _single_slot():
    s = Session(StubModel(1), sync_every=2)
    s.model.stop_at[66] = 2
    s.add("A" * 10, max_tokens=3)
    s.add("B" * 10, max_tokens=9)
    return s.finish()


def _packed():
    """four arrivals for four slots, one of them malformed: plan_pack takes two of the three that are left"""
    s = Session(StubModel(4, pack=True, t_max=25))
    s.add("A" * 10, max_tokens=2)
    s.add("BAD" * 3, max_tokens=2)
    s.add("C" * 10, max_tokens=3)
    s.add("D" * 10, max_tokens=2)
    return s.finish()


def _pool_waits():
    s = Session(StubModel(3, pool=BlockPool(3, 64, 3, 4), pack=True, t_max=64), sync_every=1)
    s.add("A" * 10, max_tokens=6, ignore_eos=True)                                # 1 block
    s.add("B" * 10, max_tokens=3, ignore_eos=True)                                # 1 block
    s.add("D" * 30, max_tokens=40, ignore_eos=True)                               # 2 blocks: waits until B's becomes evictable
    s.add("C" * 10, max_tokens=2, ignore_eos=True)
    return s.finish()


def _pool_never_fits():
    s = Session(StubModel(2, pool=BlockPool(2, 64, 2, 4), pack=False))
    s.add("Z" * 20, max_tokens=15, ignore_eos=True)
    s.add("Y" * 130, max_tokens=10, ignore_eos=True)                              # 3 blocks of 2: an error once nothing runs
    return s.finish()


def _pool_requeue():
    m = StubModel(2, pool=BlockPool(2, 64, 2, 2), pack=False)
    m.kv_fits = lambda counts: True                                               # the optimistic pre-check lets everything through
    s = Session(m, sync_every=1)
    s.add("A" * 70, max_tokens=10, ignore_eos=True)
    s.add("B" * 70, max_tokens=10, ignore_eos=True)                               # KvPoolExhausted while A runs: back to the head
    s.add("C" * 10, max_tokens=2, ignore_eos=True)
    return s.finish()


def _chunked():
    m = ChunkFailModel(3, pack=False)
    m.fail_tag = ord("F")
    s = Session(m, sync_every=1, prefill_chunk_tokens=16)
    s.add("A" * 10, max_tokens=14, ignore_eos=True)
    s.steps(1)
    s.add("B" * 40, max_tokens=3, ignore_eos=True)                                # 16 + 16 + 8 rows between A's steps
    s.add("F" * 40, max_tokens=3, ignore_eos=True)                                # fails on its second chunk
    s.add("C" * 10, max_tokens=2, ignore_eos=True)
    return s.finish()


def _sibling_script(ends):
    return lambda tag, seed, step: EOS if ends.get(seed) == step else _plain(tag, seed, step)


def _parent_waits():
    """n = 3, seeds 2^32 - 2, 2^32 - 1, 0: the parent waits for three free slots while two later single requests pass it, then one
    prefill + fork beside the long-running A; the siblings end after 3, 6 (length) and 5 tokens"""
    s = Session(ForkModel(4, _sibling_script({2 ** 32 - 2: 2, 0: 4})), _CharProc(), sync_every=2)
    s.add("A" * 10, max_tokens=24, ignore_eos=True)
    s.add("B" * 10, max_tokens=3, ignore_eos=True)
    s.steps(1)
    s.add("P" * 12, max_tokens=6, n=3, temperature=0.8, seed=2 ** 32 - 2, logprobs=1, presence_penalty=0.5)
    s.add("C" * 10, max_tokens=2, ignore_eos=True)
    s.add("D" * 10, max_tokens=4, ignore_eos=True)
    return s.finish()


def _parent_chunked():
    s = Session(ForkModel(4, _plain), _CharProc(), sync_every=2, prefill_chunk_tokens=16)
    s.add("A" * 8, max_tokens=16, ignore_eos=True)
    s.steps(1)
    s.add("P" * 40, max_tokens=4, ignore_eos=True, n=2, seed=9, temperature=0.5)
    s.add("C" * 8, max_tokens=2, ignore_eos=True)
    return s.finish()


def _parent_pool_waits():
    s = Session(ForkModel(3, _plain, pool=BlockPool(5, 64, 3, 4)), _CharProc(), sync_every=2)
    s.add("O" * 100, max_tokens=8, ignore_eos=True)                               # 2 blocks
    s.add("P" * 130, max_tokens=20, ignore_eos=True, n=2)                         # 3 + 1 blocks: not beside O
    return s.finish()


def _parent_pool_never_fits():
    s = Session(ForkModel(3, _plain, pool=BlockPool(3, 64, 3, 4)), _CharProc())
    s.add("Q" * 130, max_tokens=20, ignore_eos=True, n=3)                         # 3 + 1 + 1 blocks of 3
    return s.finish()


def _parent_pool_requeue():
    m = ForkModel(3, _plain, pool=BlockPool(5, 64, 3, 4))
    m.kv_fits = lambda counts: True
    s = Session(m, _CharProc(), sync_every=2)
    s.add("O" * 100, max_tokens=8, ignore_eos=True)
    s.steps(1)
    s.add("P" * 130, max_tokens=20, ignore_eos=True, n=2)                         # the fork's block does not exist while O runs
    s.add("C" * 10, max_tokens=2, ignore_eos=True)                                # behind the parent, and stays there
    return s.finish()


STOP_TEXT = "one two\nObs: three four five" + "x" * 40


def _stop_strings(sync_every):
    streams = {c: [ord(ch) for ch in STOP_TEXT] for c in "abcdef"}
    for c in "ef":
        streams[c][10] = EOS                                                      # an EOS before "four"
    s = Session(ForkModel(2, lambda tag, seed, step: streams[chr(tag)][step]), _CharProc(), sync_every=sync_every)
    s.add("a", max_tokens=40, stop="\nObs")                                       # ends inside a harvest of four
    s.add("b", max_tokens=40, stop=["zzz", "two"], include_stop_str_in_output=True)
    s.add("c", max_tokens=40, stop=["tw"], stop_token_ids=[ord("w")])             # the stop token completes the stop string: the token wins
    s.add("d", max_tokens=40, stop_token_ids=[ord("\n")])
    s.add("e", max_tokens=40, stop=["four"], ignore_eos=True)
    s.add("f", max_tokens=40, stop=["four"])                                      # the EOS comes first
    s.add("aa", max_tokens=5, stop=["never"])                                 # max_tokens with a stop string that never matches
    return s.finish()


SCENARIOS = {
    "01_modes_return_after_3": lambda: _modes(3),
    "02_modes_never_return": lambda: _modes(0),
    "03_grouped_keys": _grouped,
    "04_single_slot": _single_slot,
    "05_packed": _packed,
    "06a_pool_waits": _pool_waits,
    "06b_pool_never_fits": _pool_never_fits,
    "06c_pool_requeue": _pool_requeue,
    "07_chunked_prefill": _chunked,
    "08_parent_waits_and_is_overtaken": _parent_waits,
    "09_parent_chunked": _parent_chunked,
    "10a_parent_pool_waits": _parent_pool_waits,
    "10b_parent_pool_never_fits": _parent_pool_never_fits,
    "10c_parent_pool_requeue": _parent_pool_requeue,
    "11a_stop_sync_1": lambda: _stop_strings(1),
    "11b_stop_sync_4": lambda: _stop_strings(4),
}


def run_all():
    return {name: json.loads(json.dumps(fn())) for name, fn in SCENARIOS.items()}


def dumps(traces):
    """one event per line: a difference reads as a diff"""
    parts = []
    for name, trace in traces.items():
        parts.append(json.dumps(name) + ": [\n" + ",\n".join("  " + json.dumps(e) for e in trace) + "\n]")
    return "{\n" + ",\n".join(parts) + "\n}\n"


# ---- the tests ----------------------------------------------------------------------------------------------------------------------
def test_trace_matches_the_golden_file():
    with open(GOLDEN) as f:
        want = json.load(f)
    got = run_all()
    assert sorted(got) == sorted(want)
    for name in got:
        for i, (g, w) in enumerate(zip(got[name], want[name])):
            assert g == w, f"{name}: event {i}: got {g}, golden {w}"
        assert len(got[name]) == len(want[name]), f"{name}: {len(got[name])} events, golden {len(want[name])}"


def _calls(trace, name):
    return [i for i, e in enumerate(trace) if e[0] == name]


def _errors(trace):
    return [e for e in trace if e[0] == "emit" and e[7] is not None]


def test_trace_reaches_every_branch():
    t = run_all()
    everything = [e for trace in t.values() for e in trace]
    for name in ("admit_fork", "_admit_packed", "_prefill_request", "decode_step", "_admit", "batched_step", "read_logprobs",
                 "set_slot_sampling", "set_slot_controls", "note_generated"):
        assert _calls(everything, name), name
    assert any(e[0] == "admit_step" and len(e[1]) == 2 and e[1][1] == 16 for e in everything)        # a row limit
    assert any(e[0] == "admit_step" and len(e[1]) == 1 for e in everything)
    def iteration(tr, i):
        return sum(1 for e in tr[:i] if e[0] == "done")

    def idle(tr, gone, arrived):
        """iterations between the end of request `gone` and the admission of request `arrived` (tags of MODES_TAGS)"""
        end = next(i for i, e in enumerate(tr) if e[0] == "emit" and e[4] and e[1] == MODES_TAGS.index(gone) + 1)
        start = next(i for i, e in enumerate(tr) if e[0] == "_admit" and e[1][1][0] == ord(arrived))
        return iteration(tr, start) - iteration(tr, end) - 1
    for name in ("01_modes_return_after_3", "02_modes_never_return"):
        tr = t[name]
        # each mode idled for one or two iterations - fewer than greedy_return_steps = 3 - and was re-armed, not re-entered
        assert 1 <= idle(tr, "S", "T") < 3 and 1 <= idle(tr, "L", "M") < 3 and 1 <= idle(tr, "C", "K") < 3
        assert len(_calls(tr, "set_sampling_rows")) == 1
        off = [] if name.startswith("02") else [[False]]
        assert [e[1] for e in tr if e[0] == "set_logprobs"] == [[True]] + off
        assert [e[1] for e in tr if e[0] == "set_logit_controls"] == [[True]] + off
    tr = t["01_modes_return_after_3"]
    rows, greedy = _calls(tr, "set_sampling_rows")[0], _calls(tr, "set_sampling")
    assert len(greedy) == 1 and greedy[0] > rows and tr[greedy[0]][1] == [0.0]
    offs = [greedy[0]] + [i for n in ("set_logprobs", "set_logit_controls") for i in _calls(tr, n) if tr[i][1] == [False]]
    assert len({iteration(tr, i) for i in offs}) == 3                    # the three modes are left at different iterations
    assert not _calls(t["02_modes_never_return"], "set_sampling")
    # the failures: one error each, of the expected kind
    assert [e[7] for e in _errors(t["03_grouped_keys"])] == ["ValueError"]
    assert [e[7] for e in _errors(t["05_packed"])] == ["ValueError"]
    assert [e[7] for e in _errors(t["06b_pool_never_fits"])] == ["RuntimeError"]
    assert [e[7] for e in _errors(t["07_chunked_prefill"])] == ["RuntimeError"]
    assert [e[7] for e in _errors(t["10b_parent_pool_never_fits"])] == ["RuntimeError"]
    for name in ("06a_pool_waits", "06c_pool_requeue", "08_parent_waits_and_is_overtaken", "09_parent_chunked", "10a_parent_pool_waits",
                 "10c_parent_pool_requeue", "11a_stop_sync_1", "11b_stop_sync_4"):
        assert not _errors(t[name]), name
    # the grouped head was overtaken exactly twice: C and D ran before B, E after it
    order = "".join(chr(e[1][1][0]) for e in t["03_grouped_keys"] if e[0] == "_admit")
    assert order.index("C") < order.index("D") < order.index("B") < order.index("E") and "F" not in order, order
    # a requeued admission was attempted more than once and succeeded in the end
    assert len(_calls(t["10c_parent_pool_requeue"], "admit_fork")) > 1 and len(_calls(t["06c_pool_requeue"], "_admit")) > 3
    # the stop cases end the same way whatever the harvest length
    ends = lambda tr: sorted((e[1], e[5], e[6]) for e in tr if e[0] == "emit" and e[4])
    assert ends(t["11a_stop_sync_1"]) == ends(t["11b_stop_sync_4"])
    assert {(e[5], e[6]) for e in t["11b_stop_sync_4"] if e[0] == "emit" and e[4]} == {
        ("stop", "\nObs"), ("stop", "two"), ("stop", ord("w")), ("stop", ord("\n")), ("stop", "four"), ("stop", None), ("length", None)}


if __name__ == "__main__":
    if sys.argv[1:] == ["--write"]:
        with open(GOLDEN, "w") as f:
            f.write(dumps(run_all()))
        print(f"wrote {GOLDEN}")
    else:
        sys.exit("usage: python tests/test_engine_trace_host.py --write   (on the commit whose behaviour is to be pinned)")
