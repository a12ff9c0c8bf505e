"""CPU: token logprobs on the host side - the C-ABI's new symbols and its argument refusals (nothing here reaches a device: every call
below is refused before a kernel could be enqueued), the SamplingParams / validate_sampling limits, and the server's OpenAI formatting
and validation through a scripted engine that returns known entries (chat and completions, blocking and streamed)."""
import ctypes as C
import json
import os
import threading

import pytest

from chatts_amd import _lib, config as cfgmod, server
from chatts_amd.engine import validate_sampling
from chatts_amd.tokenizer import SyntheticTokenizer

NEW = ("chatts_logprobs_workspace", "chatts_logprobs_batched", "chatts_decoder_logprobs")
FAKE = 4096          # non-null stand-in for device pointers


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_symbols_declared_and_exported(lib):
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "chatts_amd.h")).read()
    for name in NEW:
        assert name in _lib.SIGNATURES and f"{name}(" in hdr
        assert hasattr(lib, name)
    assert "#define CHATTS_LOGPROBS_MAX_K 64" in hdr and _lib.LOGPROBS_MAX_K == 64
    assert lib.chatts_logprobs_workspace(16, 20) >= 16 * 64 * 20 * 8
    assert lib.chatts_logprobs_workspace(0, 5) == 0


def _call(lib, **over):
    a = dict(logits=FAKE, batch=2, stride=4096, vocab=4096, off=0, k=5, token=FAKE, step=FAKE, out_stride=8, lp=FAKE, rank=FAKE,
             ids=FAKE, tlp=FAKE, ws=FAKE, ws_bytes=1 << 20)
    a.update(over)
    rc = lib.chatts_logprobs_batched(a["logits"], a["batch"], a["stride"], a["vocab"], a["off"], a["k"], a["token"], a["step"],
                                     a["out_stride"], a["lp"], a["rank"], a["ids"], a["tlp"], a["ws"], a["ws_bytes"], None)
    return rc, lib.chatts_last_error()


@pytest.mark.parametrize("over,code,msg", [
    (dict(logits=None), "E_BADARG", b"required"),
    (dict(token=None), "E_BADARG", b"required"),
    (dict(lp=None), "E_BADARG", b"required"),
    (dict(k=-1), "E_BADARG", b"k = -1"),
    (dict(k=65), "E_BADARG", b"k = 65"),
    (dict(ids=None), "E_BADARG", b"out_top_ids"),
    (dict(tlp=None), "E_BADARG", b"out_top_ids"),
    (dict(stride=100), "E_BADARG", b"bad sizes"),
    (dict(batch=0), "E_BADARG", b"bad sizes"),
    (dict(out_stride=0), "E_BADARG", b"out_stride"),
    (dict(vocab=300000, stride=300000), "E_SHAPE", b"exceeds"),
    (dict(ws=None), "E_WORKSPACE", b"workspace"),
    (dict(ws_bytes=16), "E_WORKSPACE", b"workspace"),
])
def test_host_refusals(lib, over, code, msg):
    rc, err = _call(lib, **over)
    assert rc == getattr(_lib, code) and msg in err, (rc, err)


def test_decoder_level_refusal(lib):
    rc = lib.chatts_decoder_logprobs(None, FAKE, 1, 4096, 5, FAKE, FAKE, 8, FAKE, FAKE, FAKE, FAKE, None)
    assert rc == _lib.E_BADARG and b"decoder_logprobs" in lib.chatts_last_error()


def test_sampling_params_and_validate_sampling_limits():
    from chatts_amd import SamplingParams
    from chatts_amd.llm import CompletionOutput, Logprob
    assert SamplingParams(logprobs=5).logprobs == 5 and SamplingParams().logprobs is None
    for bad in (-1, 1.5, True, "3"):
        with pytest.raises(ValueError, match="logprobs"):
            SamplingParams(logprobs=bad)
    with pytest.raises(ValueError, match="prompt_logprobs"):
        SamplingParams(prompt_logprobs=1)
    validate_sampling(8, logprobs=0)
    validate_sampling(8, logprobs=20)
    for bad in (21, -1, True, 2.0, "5"):
        with pytest.raises(ValueError, match="logprobs"):
            validate_sampling(8, logprobs=bad)
    validate_sampling(8, logprobs=30, max_logprobs=30)
    with pytest.raises(ValueError, match="prompt_logprobs"):
        validate_sampling(8, prompt_logprobs=0)
    assert CompletionOutput("x", [1]).logprobs is None and CompletionOutput("x", [1]).cumulative_logprob is None
    lp = Logprob(-0.5, 1, "a")
    assert lp.logprob == -0.5 and lp.rank == 1 and lp.decoded_token == "a"


def test_logprobs_from_body():
    f = server.logprobs_from_body
    assert f({}, True) is None and f({"logprobs": False}, True) is None
    assert f({"logprobs": True}, True) == 0 and f({"logprobs": True, "top_logprobs": 20}, True) == 20
    assert f({}, False) is None and f({"logprobs": 0}, False) == 0 and f({"logprobs": 5}, False) == 5
    for body, chat in [({"top_logprobs": 2}, True), ({"logprobs": False, "top_logprobs": 2}, True),
                       ({"logprobs": True, "top_logprobs": 21}, True), ({"logprobs": True, "top_logprobs": -1}, True),
                       ({"logprobs": 1}, True), ({"logprobs": "yes"}, True), ({"logprobs": True, "top_logprobs": 1.5}, True),
                       ({"logprobs": 21}, False), ({"logprobs": True}, False), ({"logprobs": -2}, False),
                       ({"logprobs": "2"}, False), ({"prompt_logprobs": 1}, False)]:
        with pytest.raises(ValueError):
            f(body, chat)


# ---- server through a scripted engine ------------------------------------------------------------------------------------------------
class LogprobEngineThread:
    """stands in for EngineThread: answers with a fixed sentence, two tokens at a time, and known entries when logprobs are asked"""

    def __init__(self, tok, answer):
        self.tok, self.answer, self.seen = tok, answer, []

    def submit(self, prompt, timeseries, on_tokens, holder, max_tokens, **kw):
        self.seen.append(kw)
        ids = self.tok.encode(self.answer)[:max_tokens]
        k = kw.get("logprobs")
        entries = [(-0.25 * (i + 1), 1 + i % 3, [(ids[(i + j) % len(ids)], -0.25 * (i + 1) - 0.5 * j) for j in range(k or 0)])
                   for i in range(len(ids))]

        class R:
            error, prompt_tokens, tokens, finish_reason = None, 3, [], "stop"
            logprobs = [] if k is not None else None
        r = R()

        def run():
            for i in range(0, len(ids), 2):
                r.tokens = ids[:i + 2]
                if k is not None:
                    r.logprobs = entries[:len(r.tokens)]
                on_tokens(r, ids[i:i + 2], i + 2 >= len(ids))
        threading.Thread(target=run).start()


def _client():
    from starlette.testclient import TestClient
    answer = "The series rises, then drops sharply near point 103."
    tok = SyntheticTokenizer.for_config(cfgmod.preset("tiny-qwen2"))
    tok.encode(answer)
    et = LogprobEngineThread(tok, answer)
    return TestClient(server.create_app(et, tok, "chatts", limit_timeseries=3)), et, tok, answer


def _sse(resp):
    events = [line[6:] for line in resp.iter_lines() if line.startswith("data: ")]
    assert events[-1] == "[DONE]"
    return [json.loads(e) for e in events[:-1]]


def test_chat_logprobs_blocking_and_streamed():
    client, et, tok, answer = _client()
    ids = tok.encode(answer)
    body = {"model": "chatts", "max_tokens": 64, "messages": [{"role": "user", "content": "hi"}], "logprobs": True, "top_logprobs": 3}
    r = client.post("/v1/chat/completions", json=body)
    assert r.status_code == 200, r.text
    assert et.seen[-1]["logprobs"] == 3
    content = r.json()["choices"][0]["logprobs"]["content"]
    assert len(content) == len(ids)
    for i, (tid, e) in enumerate(zip(ids, content)):
        piece = tok.decode([tid], skip_special_tokens=False)
        assert e["token"] == piece and e["logprob"] == -0.25 * (i + 1) and e["bytes"] == list(piece.encode())
        assert [t["logprob"] for t in e["top_logprobs"]] == [-0.25 * (i + 1) - 0.5 * j for j in range(3)]
        assert e["top_logprobs"][1]["token"] == tok.decode([ids[(i + 1) % len(ids)]], skip_special_tokens=False)
    with client.stream("POST", "/v1/chat/completions", json=dict(body, stream=True)) as resp:
        chunks = _sse(resp)
    streamed = [e for c in chunks for e in (c["choices"][0].get("logprobs") or {}).get("content", [])]
    assert streamed == content
    # logprobs without top_logprobs: the chosen token only
    d = client.post("/v1/chat/completions", json=dict(body, top_logprobs=None)).json()
    assert all(e["top_logprobs"] == [] for e in d["choices"][0]["logprobs"]["content"])
    # not asked: no keyword to the engine, no field in the answer
    d = client.post("/v1/chat/completions", json={"messages": [{"role": "user", "content": "hi"}]}).json()
    assert "logprobs" not in et.seen[-1] and "logprobs" not in d["choices"][0]


def test_completions_logprobs_blocking_and_streamed():
    client, et, tok, answer = _client()
    ids = tok.encode(answer)
    body = {"model": "chatts", "prompt": "Describe", "max_tokens": 64, "logprobs": 2}
    d = client.post("/v1/completions", json=body).json()
    lp = d["choices"][0]["logprobs"]
    pieces = [tok.decode([t], skip_special_tokens=False) for t in ids]
    assert lp["tokens"] == pieces and lp["token_logprobs"] == [-0.25 * (i + 1) for i in range(len(ids))]
    assert all(len(t) <= 2 for t in lp["top_logprobs"])
    assert lp["text_offset"] == [sum(len(p) for p in pieces[:i]) for i in range(len(pieces))]
    with client.stream("POST", "/v1/completions", json=dict(body, stream=True)) as resp:
        chunks = _sse(resp)
    parts = [c["choices"][0]["logprobs"] for c in chunks if c["choices"][0].get("logprobs")]
    assert {k: [x for p in parts for x in p[k]] for k in lp} == lp


@pytest.mark.parametrize("path,extra", [
    ("/v1/chat/completions", {"top_logprobs": 2}),
    ("/v1/chat/completions", {"logprobs": True, "top_logprobs": 21}),
    ("/v1/chat/completions", {"logprobs": 3}),
    ("/v1/completions", {"logprobs": 21}),
    ("/v1/completions", {"logprobs": "x"}),
    ("/v1/completions", {"prompt_logprobs": 1}),
])
def test_logprobs_400(path, extra):
    client, et, tok, answer = _client()
    body = {"messages": [{"role": "user", "content": "hi"}]} if "chat" in path else {"prompt": "hi"}
    r = client.post(path, json=dict(body, **extra))
    assert r.status_code == 400, r.text
    assert not et.seen
