"""CPU: logit_bias / allowed_token_ids / min_tokens - the value ranges on every Python surface (SamplingParams, request_settings, the
server's body parsing: a 400 naming the field), the additive C ABI, the entry points' refusals (returned before anything is enqueued:
the pointers below are fakes and never dereferenced), the request fields, the engine's mode switch and slot hygiene on a scripted
model, the stop-string rule under min_tokens, and the numpy reference on hand-computed cases.  The kernels: tests/test_gpu_logit_masks.py."""
import ctypes as C
import json
import os
import re
import types

import numpy as np
import pytest

from chatts_amd import _lib
from chatts_amd.sampling import NO_MASKS, REQUEST_FIELDS, SamplingParams, request_settings, validate_masks
from tests import logit_masks_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 4096          # non-null stand-in for device pointers
FAKE2 = 8192
VOCAB = 1000

# (the field the message must name, the offending settings); ids are checked against VOCAB where the surface knows a vocabulary
VIOLATIONS = [
    ("allowed_token_ids", dict(allowed_token_ids=[])),
    ("allowed_token_ids", dict(allowed_token_ids=[5, 9, 5])),
    ("allowed_token_ids", dict(allowed_token_ids=[3, -1])),
    ("allowed_token_ids", dict(allowed_token_ids=[3, 2 ** 31])),
    ("allowed_token_ids", dict(allowed_token_ids=[1.5])),
    ("logit_bias", dict(logit_bias={"7": float("inf")})),
    ("logit_bias", dict(logit_bias={"7": float("nan")})),
    ("logit_bias", dict(logit_bias={"7": "high"})),
    ("logit_bias", dict(logit_bias={str(i): 0.5 for i in range(1025)})),
    ("logit_bias", dict(logit_bias={"-3": 1.0})),
    ("logit_bias", dict(logit_bias={"seven": 1.0})),
    ("logit_bias", dict(logit_bias=[1, 2])),
    ("logit_bias", dict(logit_bias={"++3": 1.0})),
    ("logit_bias", dict(logit_bias={"+3": 1.0})),
    ("allowed_token_ids", dict(allowed_token_ids=["12"])),           # decimal strings are logit_bias keys only
    ("min_tokens", dict(min_tokens=9, max_tokens=8)),
    ("min_tokens", dict(min_tokens=-1)),
    ("min_tokens", dict(min_tokens=1.5)),
    ("min_tokens", dict(min_tokens=2, max_tokens=8, stop_token_ids=list(range(65)))),
]
IN_VOCAB_ONLY = [("allowed_token_ids", dict(allowed_token_ids=[3, VOCAB])), ("logit_bias", dict(logit_bias={str(VOCAB): 1.0}))]


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


# ---- validation -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field,bad", VIOLATIONS)
def test_every_surface_refuses_the_value_and_names_the_field(field, bad):
    with pytest.raises(ValueError, match=field):
        SamplingParams(**bad)
    with pytest.raises(ValueError, match=field):
        request_settings(**bad)
    from chatts_amd.server import sampling_from_body
    with pytest.raises(ValueError, match=field):
        sampling_from_body(dict(bad))


@pytest.mark.parametrize("field,bad", IN_VOCAB_ONLY)
def test_ids_are_checked_against_the_vocabulary_where_it_is_known(field, bad):
    SamplingParams(**bad)                                     # (SamplingParams knows no model: LLM.generate checks)
    with pytest.raises(ValueError, match=field):
        request_settings(**bad, vocab_size=VOCAB)
    from chatts_amd.server import sampling_from_body
    with pytest.raises(ValueError, match=field):
        sampling_from_body(dict(bad), vocab_size=VOCAB)


def test_accepted_values_are_normalised():
    assert request_settings()["masks"] == NO_MASKS
    assert request_settings(logit_bias={}, min_tokens=0)["masks"] == NO_MASKS            # the empty dict counts as off
    s = request_settings(logit_bias={"12": -3, 7: 1.5}, allowed_token_ids=(4, 2), min_tokens=3, max_tokens=3, vocab_size=VOCAB)
    assert s["masks"] == ({12: -3.0, 7: 1.5}, [4, 2], 3)
    with pytest.raises(ValueError, match="logit_bias"):
        validate_masks(logit_bias={"12": 1.0, 12: 2.0})       # distinct after conversion
    sp = SamplingParams(logit_bias={"5": 1000.0}, allowed_token_ids=[1], min_tokens=2, max_tokens=4)
    assert (sp.logit_bias, sp.allowed_token_ids, sp.min_tokens) == ({5: 1000.0}, [1], 2)      # any finite bias here
    sp = SamplingParams()
    assert (sp.logit_bias, sp.allowed_token_ids, sp.min_tokens) == NO_MASKS
    assert request_settings(min_tokens=2, stop_token_ids=list(range(64)))["masks"][2] == 2
    assert request_settings(min_tokens=0, stop_token_ids=list(range(65)))["masks"][2] == 0     # (the limit belongs to min_tokens)


def test_request_fields_carry_the_three_names():
    for name in ("logit_bias", "allowed_token_ids", "min_tokens"):
        assert name in REQUEST_FIELDS
        assert hasattr(SamplingParams(), name)                # LLM builds add_request's keywords from REQUEST_FIELDS


def test_server_answers_400_clamps_the_bias_and_passes_the_fields_on():
    from tests.test_server_host import _client
    for path, extra in (("/v1/chat/completions", {"messages": [{"role": "user", "content": "Hello"}]}), ("/v1/completions", {"prompt": "Hello"})):
        client, et, _ = _client()
        et.engine = types.SimpleNamespace(nslots=1, vocab_size=VOCAB)
        for field, bad in VIOLATIONS + IN_VOCAB_ONLY:
            # (sent as text: Python's JSON writes inf / nan as Infinity / NaN, and the server's parser reads them)
            r = client.post(path, content=json.dumps({"max_tokens": 8, **extra, **bad}), headers={"content-type": "application/json"})
            assert r.status_code == 400, (path, bad, r.text)
            assert field in r.json()["error"]["message"], (bad, r.text)
        assert et.seen == []                                  # refused before the engine thread
        r = client.post(path, json={"max_tokens": 8, **extra, "logit_bias": {"12": -250, "13": 42.5, "14": 1e9}, "allowed_token_ids": [12, 13, 14],
                                    "min_tokens": 2})
        assert r.status_code == 200, r.text
        kw = et.seen[0][3]
        assert kw["logit_bias"] == {"12": -100.0, "13": 42.5, "14": 100.0}      # clamped to [-100, 100] like vLLM's OpenAI layer
        assert kw["allowed_token_ids"] == [12, 13, 14] and kw["min_tokens"] == 2
        r = client.post(path, json={"max_tokens": 8, **extra})
        assert r.status_code == 200 and not {"logit_bias", "allowed_token_ids", "min_tokens"} & set(et.seen[1][3])


# ---- C ABI ------------------------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("chatts_logit_masks_apply", "chatts_decoder_set_logit_masks", "chatts_decoder_select_tokens_masked")


def test_abi_is_still_version_9_the_layouts_are_unchanged_and_the_new_symbols_exist(lib):
    hdr = open(os.path.join(ROOT, "include", "chatts_amd.h")).read()
    assert lib.chatts_abi_version() == 9 and _lib.ABI_VERSION == 9
    assert re.search(r"#define\s+CHATTS_ABI_VERSION\s+9\b", hdr)
    assert C.sizeof(_lib.LogitControlArgs) == 72
    assert C.sizeof(_lib.SamplingArgs) == 64
    assert C.sizeof(_lib.KvCache) == 40
    assert C.sizeof(_lib.DecoderBuffers) == 176
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint %s\s*\(" % name, hdr), name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    # chatts_decoder_select_tokens_controlled keeps its signature: 14 arguments, the controls last before the stream
    m = re.search(r"int chatts_decoder_select_tokens_controlled\((.*?)\);", hdr, re.S)
    assert m and len(m.group(1).split(",")) == 14 == len(_lib.SIGNATURES["chatts_decoder_select_tokens_controlled"][1])
    assert (_lib.LOGIT_BIAS_MAX, _lib.LOGIT_END_IDS_MAX) == (1024, 64)
    assert re.search(r"#define\s+CHATTS_LOGIT_BIAS_MAX\s+1024\b", hdr) and re.search(r"#define\s+CHATTS_LOGIT_END_IDS_MAX\s+64\b", hdr)


def test_the_new_structs_ctypes_layout_equals_the_headers():
    hdr = open(os.path.join(ROOT, "include", "chatts_amd.h")).read()
    body = re.search(r"typedef struct ChattsLogitMaskArgs \{(.*?)\} ChattsLogitMaskArgs;", hdr, re.S).group(1)
    fields = []
    for line in body.split(";"):
        line = re.sub(r"/\*.*?\*/", "", line, flags=re.S).strip()
        if line:
            m = re.match(r"(.*?)(\w+)$", line)
            fields.append((m.group(2), m.group(1).strip()))
    assert [f for f, _ in fields] == [f for f, _ in _lib.LogitMaskArgs._fields_]
    for (name, ctype), (_, py) in zip(fields, _lib.LogitMaskArgs._fields_):
        assert (py is C.c_void_p) == ctype.endswith("*"), name
        assert (py is C.c_int64) == (ctype == "int64_t"), name
    # thirteen 8-byte members, no padding
    assert C.sizeof(_lib.LogitMaskArgs) == 13 * 8
    assert [getattr(_lib.LogitMaskArgs, f).offset for f, _ in _lib.LogitMaskArgs._fields_] == list(range(0, 104, 8))


def _args(**over):
    kw = dict(out=FAKE2, out_stride=64, allow_bits=FAKE, allow_stride=2, allow_on=FAKE, bias_ids=FAKE, bias_val=FAKE, bias_n=FAKE,
              bias_stride=1024, end_ids=FAKE, end_n=FAKE, min_tokens=FAKE, end_stride=64)
    kw.update(over)
    return _lib.LogitMaskArgs(**kw)


def test_apply_refusals_return_before_anything_is_enqueued(lib):
    call = lambda a, logits=FAKE, batch=2, stride=64, vocab=64, off=0, step=FAKE: lib.chatts_logit_masks_apply(
        logits, batch, stride, vocab, off, None if a is None else C.byref(a), step, None)
    assert call(None) == _lib.E_BADARG
    assert call(_args(), logits=None) == _lib.E_BADARG
    assert call(_args(out=None)) == _lib.E_BADARG
    assert call(_args(out=FAKE)) == _lib.E_BADARG and b"another buffer" in lib.chatts_last_error()       # out == logits
    assert call(_args(), batch=0) == _lib.E_BADARG
    assert call(_args(), vocab=0) == _lib.E_BADARG
    assert call(_args(), stride=63) == _lib.E_BADARG
    assert call(_args(out_stride=63)) == _lib.E_BADARG
    assert call(_args(), off=-4) == _lib.E_BADARG
    assert call(_args(), off=2 ** 31 - 64) == _lib.E_BADARG and b"int32" in lib.chatts_last_error()
    assert call(_args(), vocab=2 ** 31, stride=2 ** 31) == _lib.E_BADARG
    assert call(_args(allow_stride=1)) == _lib.E_BADARG and b"allow_stride" in lib.chatts_last_error()   # 64 ids need 2 words
    assert call(_args(allow_stride=2), off=32) == _lib.E_BADARG                                           # ids 32 .. 95 need 3
    assert call(_args(bias_stride=0)) == _lib.E_BADARG
    assert call(_args(bias_stride=1025)) == _lib.E_BADARG and b"bias_stride" in lib.chatts_last_error()
    assert call(_args(end_stride=65)) == _lib.E_BADARG and b"end_stride" in lib.chatts_last_error()
    assert call(_args(), step=None) == _lib.E_BADARG and b"step" in lib.chatts_last_error()              # min_tokens needs the counters


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


def test_decoder_entry_point_refusals_return_before_anything_is_enqueued(lib):
    assert lib.chatts_decoder_set_logit_masks(None, None) == _lib.E_BADARG
    d, keep = _decoder(lib)
    try:
        assert lib.chatts_decoder_set_logit_masks(d, C.byref(_args(out=None))) == _lib.E_BADARG
        sel = lambda lm, lc=None, logits=FAKE, step=FAKE, dec=d: lib.chatts_decoder_select_tokens_masked(
            dec, logits, 1, 1024, FAKE, FAKE, FAKE, 0, step, None, 0, None, None if lc is None else C.byref(lc), C.byref(lm), None)
        ok = dict(out=FAKE2, out_stride=1024, allow_stride=32)
        assert sel(_args(**ok), dec=None) == _lib.E_BADARG
        assert sel(_args(**ok), logits=None) == _lib.E_BADARG
        assert sel(_args(**dict(ok, out_stride=1000))) == _lib.E_BADARG                       # rows shorter than the vocabulary
        assert sel(_args(**dict(ok, out=FAKE))) == _lib.E_BADARG                              # out == logits
        assert sel(_args(**dict(ok, allow_stride=31))) == _lib.E_BADARG
        assert sel(_args(**dict(ok, bias_stride=2000))) == _lib.E_BADARG
        assert sel(_args(**dict(ok, end_stride=0))) == _lib.E_BADARG
        assert sel(_args(**ok), step=None) == _lib.E_BADARG and b"step" in lib.chatts_last_error()
        lc = _lib.LogitControlArgs(state=FAKE, state_stride=1024, out=FAKE2, out_stride=1024)
        assert sel(_args(**ok), lc=lc) == _lib.E_BADARG                                       # masks and controls share an output buffer
        # the setter: masks on the decoder keep the speculative step away, NULL turns them off again
        assert lib.chatts_decoder_set_logit_masks(d, C.byref(_args(**ok))) == 0
        spec = _lib.SpecArgs(k=4, ngram_min=1, ngram_max=3, n_splits=8, skip_propose=0, hist=FAKE, draft=FAKE, spec_tokens=FAKE, argmax=FAKE,
                             logits=FAKE, pos_dev=FAKE, step_dev=FAKE, token_dev=FAKE, out_tokens=FAKE, out_capacity_dev=FAKE, counters=FAKE)
        assert lib.chatts_decoder_spec_step(d, C.byref(spec), None) == _lib.E_BADARG and b"greedy" in lib.chatts_last_error()
        assert lib.chatts_decoder_set_logit_masks(d, None) == 0
    finally:
        lib.chatts_decoder_destroy(d)
    d2, keep2 = _decoder(lib, tp_world=2)
    try:                                                      # tensor parallel without an exchange: refused ahead of the gather
        lm = _args(out=FAKE2, out_stride=2048, allow_stride=64)
        assert lib.chatts_decoder_select_tokens_masked(d2, FAKE, 1, 1024, FAKE, FAKE, FAKE, 0, FAKE, None, 0, None, None, C.byref(lm),
                                                       None) == _lib.E_BADARG
        assert b"exchange" in lib.chatts_last_error()
    finally:
        lib.chatts_decoder_destroy(d2)


# ---- the engine on a scripted model -------------------------------------------------------------------------------------------------
def _stub_model():
    from tests.test_engine_host import StubModel

    class Model(StubModel):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            self._masks_on, self.switches, self.slot_masks = False, [], []
            self.plan = types.SimpleNamespace(vocab=VOCAB // 2, world=2)

        def set_slot_sampling(self, slot, *a):
            pass

        def set_sampling_rows(self):
            pass

        def set_logit_masks(self, on):
            if on != self._masks_on:
                self.switches.append(on)
            self._masks_on = on

        def set_slot_masks(self, slot, logit_bias=None, allowed_token_ids=None, min_tokens=0, end_ids=()):
            self.slot_masks.append((slot, logit_bias, allowed_token_ids, min_tokens, list(end_ids)))
    return Model, StubModel


def test_engine_carries_the_masks_and_switches_the_mode():
    from chatts_amd.engine import Engine
    from tests.test_engine_host import _Proc
    Model, StubModel = _stub_model()
    model = Model(2)
    eng = Engine(model, _Proc(), greedy_return_steps=8)
    assert eng.vocab_size == VOCAB
    a = eng.add_request("a" * 10, max_tokens=3, allowed_token_ids=[4, 5], min_tokens=2, stop_token_ids=[11])
    b = eng.add_request("b" * 10, max_tokens=3, logit_bias={"9": -100})
    c = eng.add_request("c" * 10, max_tokens=3)
    assert a.masks == (None, [4, 5], 2) and b.masks == ({9: -100.0}, None, 0) and c.masks == NO_MASKS
    for field, bad in VIOLATIONS + IN_VOCAB_ONLY:             # Engine.check knows the vocabulary: before the request is announced
        with pytest.raises(ValueError, match=field):
            eng.check(**bad)
    with pytest.raises(ValueError, match="min_tokens"):      # 64 stop ids + the model's EOS id: 65 ids to keep away
        eng.check(min_tokens=1, max_tokens=4, stop_token_ids=list(range(100, 164)))
    eng.check(min_tokens=1, max_tokens=4, stop_token_ids=list(range(100, 164)), ignore_eos=True)
    eng.run_until_done()
    assert model.switches == [True]
    # every admission writes its slot: the plain tenant's defaults reset whatever the slot held (end ids: EOS 7 + stop ids)
    assert (0, None, [4, 5], 2, [7, 11]) in model.slot_masks and (1, {9: -100.0}, None, 0, [7]) in model.slot_masks
    assert [m[1:4] for m in model.slot_masks if m[1:4] == (None, None, 0)] == [(None, None, 0)]
    for _ in range(3):
        eng.add_request("d" * 10, max_tokens=4)
        eng.run_until_done()
    assert model.switches == [True, False]                   # ... after greedy_return_steps iterations without a requester
    plain = Engine(StubModel(2), _Proc())                    # a model without the feature refuses instead of ignoring the field
    for kw in (dict(logit_bias={"3": 1.0}), dict(allowed_token_ids=[3]), dict(min_tokens=1)):
        with pytest.raises(ValueError, match="does not apply"):
            plain.add_request("e" * 10, **kw)
    plain.add_request("e" * 10, logit_bias={}, min_tokens=0)


def test_a_stop_string_is_not_searched_in_the_first_min_tokens_tokens():
    from chatts_amd.detok import StopChecker

    class Tok:
        def decode(self, ids, **kw):
            return "".join(chr(i) for i in ids)
    ids = [ord(c) for c in "abXYcdXYef"]
    assert StopChecker(Tok(), ["XY"]).push(ids)[0] == 4                       # without min_tokens: the first match
    ch = StopChecker(Tok(), ["XY"], min_tokens=4)
    assert ch.push(ids) == (8, "abXYcd", "XY")                                # the text of the first 4 tokens is not searched
    assert StopChecker(Tok(), ["XY"], min_tokens=3).push(ids)[0] == 8         # nor a match that begins inside it
    assert StopChecker(Tok(), ["XY"], min_tokens=2).push(ids)[0] == 4
    assert StopChecker(Tok(), ["XY"], min_tokens=10).push(ids) is None
    assert StopChecker(Tok(), ["XY"], True, min_tokens=4).push(ids) == (8, "abXYcdXY", "XY")


# ---- the numpy reference on hand-computed cases ---------------------------------------------------------------------------------------
def test_reference_order_and_exactness():
    inf = np.inf
    l = np.array([1.0, 2.0, 3.0, 4.0, 5.0], dtype=np.float32)
    assert ref.apply(l).tolist() == l.tolist()
    assert ref.apply(l, allowed=[1, 3]).tolist() == [-inf, 2.0, -inf, 4.0, -inf]
    assert ref.apply(l, allowed=[1, 3], bias={3: -2.5, 0: 100.0}).tolist() == [-inf, 2.0, -inf, 1.5, -inf]     # -inf + b stays -inf
    assert ref.apply(l, bias={4: 1.0}, min_tokens=2, end_ids=[4, 0], step=1).tolist() == [-inf, 2.0, 3.0, 4.0, -inf]
    assert ref.apply(l, bias={4: 1.0}, min_tokens=2, end_ids=[4, 0], step=2).tolist() == [1.0, 2.0, 3.0, 4.0, 6.0]
    assert ref.apply(l, allowed=[2, 7, 8, 9, 40], bias={9: 1.0, 3: 1.0}, min_tokens=1, end_ids=[5, 0], vocab_offset=5).tolist() == [-inf, -inf, 3.0, 4.0, 6.0]
    odd = np.array([0x7FC12345, 0xFFC00001, 0x7F800000, 0xFF800000, 0x7F812345], dtype=np.uint32).view(np.float32)
    assert ref.apply(odd).view(np.uint32).tolist() == odd.view(np.uint32).tolist()                             # NaN payloads are copied
    assert ref.bitset([0, 31, 32, 70], 3).tolist() == [0x80000001, 1, 0x40]
    assert ref.argmax(np.array([1.0, np.nan, 3.0, 3.0, -inf], dtype=np.float32)) == 2


# ---- stop_token_ids outside the vocabulary: inert as before, refused only where min_tokens would need them -----------------------------
def test_stop_ids_outside_the_vocabulary_stay_inert_and_one_bad_admission_fails_alone():
    from chatts_amd.engine import Engine
    from chatts_amd.modeling import ChatTSForCausalLM
    from tests.test_engine_host import _Proc
    Model, _ = _stub_model()

    class Checked(Model):
        """set_slot_masks with the real model's checks (check_masks reads nothing but the shard plan)"""

        def set_slot_masks(self, slot, logit_bias=None, allowed_token_ids=None, min_tokens=0, end_ids=()):
            if allowed_token_ids == [13]:
                raise NotImplementedError("refused at admission")
            bias, allowed, m, ends = ChatTSForCausalLM.check_masks(self, logit_bias, allowed_token_ids, min_tokens, end_ids)
            self.slot_masks.append((slot, bias, allowed, m, ends))

    model = Checked(2)
    eng = Engine(model, _Proc())
    plain = eng.add_request("a" * 10, max_tokens=3, stop_token_ids=[VOCAB + 5, -4, 11])        # what the engine accepted before
    held = eng.add_request("b" * 10, max_tokens=3, stop_token_ids=[11], min_tokens=2)
    for bad in ([VOCAB + 5], [-4]):                          # min_tokens would have to keep them away: a ValueError before the request is announced
        with pytest.raises(ValueError, match="min_tokens.*stop_token_ids"):
            eng.check(max_tokens=3, stop_token_ids=bad, min_tokens=2)
    eng.check(max_tokens=3, stop_token_ids=[VOCAB + 5], min_tokens=0)
    eng.run_until_done()
    assert plain.error is None and held.error is None and len(plain.tokens) == 3
    assert (0, None, None, 0, [7, 11]) in model.slot_masks    # the ids outside the vocabulary are dropped: nothing to keep away
    # an admission the model refuses fails that request alone; its neighbour and the engine go on
    bad = eng.add_request("c" * 10, max_tokens=3, allowed_token_ids=[13])
    good = eng.add_request("d" * 10, max_tokens=3)
    eng.run_until_done()
    assert isinstance(bad.error, NotImplementedError) and bad.finish_reason == "error"
    assert good.error is None and len(good.tokens) == 3 and not eng.has_work()
    # the server: a 400 naming the fields, and the plain body as before
    from chatts_amd.server import sampling_from_body
    with pytest.raises(ValueError, match="min_tokens.*stop_token_ids"):
        sampling_from_body({"max_tokens": 4, "min_tokens": 2, "stop_token_ids": [VOCAB + 5]}, vocab_size=VOCAB)
    assert sampling_from_body({"max_tokens": 4, "stop_token_ids": [VOCAB + 5]}, vocab_size=VOCAB)["stop_token_ids"] == [VOCAB + 5]
