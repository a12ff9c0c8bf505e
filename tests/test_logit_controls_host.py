"""CPU: the host side of the logit controls (repetition / frequency / presence penalties, min_p): SamplingParams, validate_sampling,
the server's request parsing, the C ABI's new symbols and unchanged struct sizes, and the numpy reference of
tests/logit_controls_ref.py against hand-computed cases.  The kernels and the model run in tests/test_gpu_logit_controls.py."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from chatts_amd import _lib, server
from chatts_amd.engine import validate_controls, validate_sampling
from chatts_amd.llm import SamplingParams
from tests import logit_controls_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("repetition_penalty", "frequency_penalty", "presence_penalty", "min_p")
BAD = [("repetition_penalty", 0.0), ("repetition_penalty", -1.0), ("repetition_penalty", math.inf), ("repetition_penalty", math.nan),
       ("frequency_penalty", 2.5), ("frequency_penalty", -2.5), ("frequency_penalty", math.nan), ("frequency_penalty", math.inf),
       ("presence_penalty", 3.0), ("presence_penalty", -2.01), ("presence_penalty", math.nan), ("presence_penalty", -math.inf),
       ("min_p", -0.1), ("min_p", 1.5), ("min_p", math.nan), ("min_p", math.inf)]


def test_sampling_params_keep_the_four_fields():
    sp = SamplingParams(max_tokens=4, repetition_penalty=1.3, frequency_penalty=0.5, presence_penalty=-0.25, min_p=0.2, some_vllm_field=1)
    assert (sp.repetition_penalty, sp.frequency_penalty, sp.presence_penalty, sp.min_p) == (1.3, 0.5, -0.25, 0.2)
    d = SamplingParams()
    assert (d.repetition_penalty, d.frequency_penalty, d.presence_penalty, d.min_p) == (1.0, 0.0, 0.0, 0.0)
    # the edges of the ranges are inside
    SamplingParams(frequency_penalty=2.0, presence_penalty=-2.0, min_p=1.0, repetition_penalty=1e-3)


@pytest.mark.parametrize("name,value", BAD)
def test_out_of_range_values_raise(name, value):
    with pytest.raises(ValueError, match=name):
        SamplingParams(**{name: value})
    with pytest.raises(ValueError, match=name):
        validate_sampling(**{name: value})
    with pytest.raises(ValueError, match=name):
        validate_controls(**{name: value})


def test_validate_sampling_accepts_the_ranges():
    validate_sampling(max_tokens=3, temperature=0.7, repetition_penalty=1.05, frequency_penalty=-2, presence_penalty=2, min_p=0.05)
    assert validate_controls() == (1.0, 0.0, 0.0, 0.0)
    assert validate_controls(1.3, 0.5, None, 1) == (1.3, 0.5, 0.0, 1.0)
    with pytest.raises(ValueError, match="min_p"):
        validate_sampling(min_p="0.1")
    with pytest.raises(ValueError, match="presence_penalty"):
        validate_sampling(presence_penalty=True)


def test_sampling_from_body_reads_the_four_fields():
    sp = server.sampling_from_body({"max_tokens": 7, "presence_penalty": 0.5, "frequency_penalty": 1, "repetition_penalty": 1.3, "min_p": 0.1})
    assert (sp["presence_penalty"], sp["frequency_penalty"], sp["repetition_penalty"], sp["min_p"]) == (0.5, 1.0, 1.3, 0.1)
    assert not set(FIELDS) & set(server.sampling_from_body({"max_tokens": 7}))       # not sent: an engine without them never sees them
    for name, value in BAD:
        with pytest.raises(ValueError, match=name):
            server.sampling_from_body({name: value})
    for name in FIELDS:
        with pytest.raises(ValueError, match=name):
            server.sampling_from_body({name: "1.0"})
        with pytest.raises(ValueError, match=name):
            server.sampling_from_body({name: [1.0]})


def test_server_answers_400_and_passes_the_fields_on():
    from tests.test_server_host import _client
    for path, extra in (("/v1/chat/completions", {"messages": [{"role": "user", "content": "Hello"}]}), ("/v1/completions", {"prompt": "Hello"})):
        client, et, _ = _client()
        for bad in ({"frequency_penalty": 3}, {"presence_penalty": -2.5}, {"repetition_penalty": 0}, {"min_p": 1.5}, {"min_p": "x"},
                    {"frequency_penalty": [1]}):
            r = client.post(path, json={"max_tokens": 4, **extra, **bad})
            assert r.status_code == 400, (path, bad, r.text)
            assert list(bad)[0] in r.json()["error"]["message"]
        assert et.seen == []                                  # refused before the engine thread
        r = client.post(path, json={"max_tokens": 4, **extra, "frequency_penalty": 1.0, "presence_penalty": 0.5, "repetition_penalty": 1.3,
                                    "min_p": 0.2})
        assert r.status_code == 200, r.text
        kw = et.seen[0][3]
        assert (kw["frequency_penalty"], kw["presence_penalty"], kw["repetition_penalty"], kw["min_p"]) == (1.0, 0.5, 1.3, 0.2)


def test_engine_carries_the_controls_and_switches_the_mode():
    """Engine: Request.controls, the per-slot settings written at admission, the mode on while a request needs it and off again after
    greedy_return_steps iterations without one."""
    from chatts_amd.engine import NO_CONTROLS, Engine
    from tests.test_engine_host import StubModel, _Proc          # the scripted model of the engine's own host tests

    class Model(StubModel):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            self._controls_on, self.switches, self.slot_controls = False, [], {}

        def set_slot_sampling(self, slot, *a):
            pass

        def set_sampling_rows(self):
            pass

        def set_logit_controls(self, on):
            if on != self._controls_on:
                self.switches.append(on)
            self._controls_on = on

        def set_slot_controls(self, slot, r=1.0, f=0.0, p=0.0, m=0.0):
            self.slot_controls[slot] = (r, f, p, m)

    model = Model(2)
    eng = Engine(model, _Proc(), greedy_return_steps=3)
    a = eng.add_request("a" * 10, max_tokens=3, repetition_penalty=1.3, frequency_penalty=0.5)
    b = eng.add_request("b" * 10, max_tokens=3)
    assert a.controls == (1.3, 0.5, 0.0, 0.0) and b.controls == NO_CONTROLS
    with pytest.raises(ValueError, match="frequency_penalty"):
        eng.add_request("c", frequency_penalty=3)
    eng.run_until_done()
    assert model.switches == [True]
    assert sorted(model.slot_controls.values()) == [(1.0, 0.0, 0.0, 0.0), (1.3, 0.5, 0.0, 0.0)]
    for _ in range(3):
        eng.add_request("d" * 10, max_tokens=4)
        eng.run_until_done()
    assert model.switches == [True, False]                       # ... after greedy_return_steps iterations without a requester
    # a model without the feature refuses the request instead of ignoring the field
    plain = Engine(StubModel(2), _Proc())
    with pytest.raises(ValueError, match="does not apply"):
        plain.add_request("e" * 10, min_p=0.1)
    plain.add_request("e" * 10, min_p=0.0)


def test_abi_new_symbols_and_unchanged_layouts():
    hdr = open(os.path.join(ROOT, "include", "chatts_amd.h")).read()
    lib = _lib.load()
    for name in ("chatts_logit_controls_workspace", "chatts_logit_controls_apply", "chatts_logit_state_reset", "chatts_logit_state_update",
                 "chatts_decoder_set_logit_controls", "chatts_decoder_select_tokens_controlled"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert lib.chatts_abi_version() == 9 and _lib.ABI_VERSION == 9
    assert re.search(r"#define\s+CHATTS_ABI_VERSION\s+9\b", hdr)
    # the sizes of the parent commit: no existing struct grew
    assert C.sizeof(_lib.SamplingArgs) == 64
    assert C.sizeof(_lib.KvCache) == 40
    assert C.sizeof(_lib.DecoderBuffers) == 176
    assert C.sizeof(_lib.LogitControlArgs) == 72
    assert lib.chatts_logit_controls_workspace(16) >= 16 * 64 * 4 and lib.chatts_logit_controls_workspace(0) == 0
    # host-only validation: refused before any launch
    assert lib.chatts_logit_controls_apply(None, 1, 8, 8, 0, None, None, 0, None) == _lib.E_BADARG
    assert lib.chatts_logit_state_reset(None, 8, 0, None, 0, None) == _lib.E_BADARG
    assert lib.chatts_logit_state_update(None, 8, 1, 8, 0, None, None) == _lib.E_BADARG
    assert lib.chatts_decoder_set_logit_controls(None, None) == _lib.E_BADARG


# ---- the numpy reference against hand-computed cases -----------------------------------------------------------------------------------
def test_reference_repetition_on_positive_and_negative_logits():
    l = np.array([2.0, -2.0, 3.0, -3.0, 0.0], dtype=np.float32)
    out = ref.penalise(l, ref.prompt_mask([0, 1], 5), ref.counts_of([], 5), r=2.0)
    assert out.tolist() == [1.0, -4.0, 3.0, -3.0, 0.0]                   # l / r above zero, l * r below, the others untouched


def test_reference_prompt_only_id_gets_r_but_not_f_or_p():
    l = np.array([4.0, 4.0, 4.0], dtype=np.float32)
    out = ref.penalise(l, ref.prompt_mask([0, 0, 0], 3), ref.counts_of([1], 3), r=2.0, f=0.5, p=0.25)
    # id 0: prompt only (multiplicity is irrelevant) -> 4 / 2; id 1: generated once -> 4 / 2 - 0.5 - 0.25; id 2: unseen
    assert out.tolist() == [2.0, 1.25, 4.0]


def test_reference_count_of_three():
    l = np.array([1.0, -1.0, 5.0], dtype=np.float32)
    counts = ref.counts_of([0, 1, 0, 0, 1, 1], 3)
    assert counts.tolist() == [3, 3, 0]
    out = ref.penalise(l, ref.prompt_mask([], 3), counts, r=1.0, f=0.5, p=1.0)
    assert out.tolist() == [1.0 - 1.5 - 1.0, -1.0 - 1.5 - 1.0, 5.0]
    out = ref.penalise(l, ref.prompt_mask([], 3), counts, r=4.0, f=-0.5, p=0.0)
    assert out.tolist() == [0.25 + 1.5, -4.0 + 1.5, 5.0]
    assert ref.counts_of([7, 9, 9, 3], 4, vocab_offset=6).tolist() == [0, 1, 0, 2]     # a vocabulary slice: ids 6..9


def test_reference_min_p_cut_with_a_tie_at_the_cut():
    # T = 2, min_p = 0.25: cut = 8 + 2 * log(0.25) = 8 - 4 log 2.  Two ids sit exactly on the (float64) cut: both are kept
    cut = 8.0 + 2.0 * math.log(0.25)
    l = np.array([8.0, cut, cut, np.nextafter(cut, -np.inf), 0.0, cut + 1.0])
    sel, c = ref.apply(l, np.zeros(6, bool), np.zeros(6, int), min_p=0.25, temperature=2.0)
    assert c == cut
    assert np.isfinite(sel).tolist() == [True, True, True, False, False, True]
    assert sel[3] == -np.inf and sel[1] == cut
    # the cut follows the PENALISED maximum: the raw maximum 8 is halved first
    sel, c = ref.apply(np.array([8.0, 3.9, 1.0]), ref.prompt_mask([0], 3), np.zeros(3, int), r=2.0, min_p=0.5, temperature=1.0)
    assert c == 4.0 + math.log(0.5) and np.isfinite(sel).tolist() == [True, True, False]
    # inert on greedy rows and at min_p == 0
    assert ref.apply(l, np.zeros(6, bool), np.zeros(6, int), min_p=0.25, temperature=0.0)[1] is None
    assert ref.apply(l, np.zeros(6, bool), np.zeros(6, int), min_p=0.0, temperature=1.0)[1] is None


def test_reference_min_p_one_keeps_exactly_the_maxima():
    l = np.array([1.0, 7.5, 7.5, 7.4999, -3.0])
    sel, c = ref.apply(l, np.zeros(5, bool), np.zeros(5, int), min_p=1.0, temperature=0.7)
    assert c == 7.5 and np.isfinite(sel).tolist() == [False, True, True, False, False]
    for seed in range(4):                                               # whatever the variate, a maximum is drawn
        assert ref.sample(l, np.zeros(5, bool), np.zeros(5, int), 0.7, 0, 1.0, seed, 0, min_p=1.0) in (1, 2)


def test_reference_greedy_token_and_margin():
    l = np.array([5.0, 4.0, 1.0], dtype=np.float32)
    tok, margin = ref.greedy(l, ref.prompt_mask([0], 3), ref.counts_of([], 3), r=2.0)
    assert tok == 1 and margin == 1.5                                    # 5 / 2 = 2.5 < 4
    b = ref.penalty_bound(l, np.array([0, 2, 0]), r=2.0, f=0.5, p=0.25)
    assert np.allclose(b, 4 * 2.0 ** -24 * np.array([10.0 + 0.25, 8.0 + 1.0 + 0.25, 2.0 + 0.25]))
