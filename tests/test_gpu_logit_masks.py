"""GPU: logit_bias / allowed_token_ids / min_tokens (csrc/logit_masks.hip).  Kernel level: the pass against the numpy restatement of
tests/logit_masks_ref.py, bitwise (copy, -inf and one float32 add are exact), and inside a replayed graph.  Model, engine, LLM, server
and tensor parallelism: every token is judged against the raw logits of its own step, read back from the GPU."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from chatts_amd import _lib
from chatts_amd import config as cfgmod
from chatts_amd.modeling import ChatTSForCausalLM
from chatts_amd.processing import ChatTSProcessor
from tests import logit_controls_ref as lc_ref
from tests import logit_masks_ref as ref
from tests.util import chat_prompt, random_walk_series

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 20261019
MODEL_SEED = 3
CANARY = np.uint32(0x7FC0BEEF)               # a NaN with a payload: what the padding of every buffer holds
ODD = np.array([0x7FC12345, 0xFFC00001, 0x7F812345, 0x7F800000, 0xFF800000], dtype=np.uint32)      # NaNs (quiet, negative, signalling), +inf, -inf


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _st():
    return torch.cuda.current_stream().cuda_stream


# ---- kernel level -----------------------------------------------------------------------------------------------------------------
def _rows(batch, V, off, rng):
    """per row (allowed or None, bias or None, min_tokens, end ids, step), global ids.  The kinds cycle: everything set with step =
    min_tokens - 1; nothing set; a single allowed id with step = min_tokens; bias only; min_tokens only; allowed only."""
    first, last = off, off + V - 1
    pick = lambda n: (off + rng.choice(V, size=min(n, V), replace=False)).tolist()
    rows = []
    for b in range(batch):
        kind = b % 6
        if kind == 0:
            allowed = sorted(set(pick(max(2, V // 3)) + [first, last]))             # the last id of a part-filled word among them
            banned = np.setdiff1d(np.arange(off, off + V), allowed)[:1].tolist()
            ends = pick(5) + [last]
            bias = {first: 3.25, last: -7.5, ends[0]: 1.5}                           # ids 0 and V - 1; an end id that carries a bias
            if banned:
                bias[banned[0]] = 50.0                                               # a bias on a disallowed id: stays -inf
            bias.update({off - 1: 9.0, off + V: 9.0})                               # outside the slice: skipped
            rows.append((allowed, bias, 4, ends + [off + V + 3], 3))
        elif kind == 1:
            rows.append((None, None, 0, [], 7))
        elif kind == 2:
            one = pick(1)
            rows.append((one, {one[0]: -2.0, last: 1.0} if one[0] != last else {last: 1.0}, 4, [one[0], first], 4))
        elif kind == 3:
            ids = pick(1024)                                                         # (as many as the vocabulary has, up to the limit)
            rows.append((None, {t: float(np.float32(rng.standard_normal() * 20)) for t in ids}, 0, [], 0))
        elif kind == 4:
            rows.append((None, None, 1, pick(64), 0))
        else:
            rows.append((sorted(set(pick(V // 2 + 1) + [last])), None, 0, [], 2))
    return rows


def _logits(batch, V, stride, rows, off, rng):
    """float32 [batch, stride]: NaN / +-inf among the logits (never under a bias: a NaN's payload through an add is not defined), a
    canary in the padding"""
    x = np.empty((batch, stride), dtype=np.uint32)
    x[:] = CANARY
    x[:, :V] = (rng.standard_normal((batch, V)) * 3.0).astype(np.float32).view(np.uint32)
    for b in range(batch):
        biased = {t - off for t in (rows[b][1] or {})}
        free = np.setdiff1d(np.arange(V), sorted(biased))
        for j, i in enumerate(rng.choice(free, size=min(len(ODD), len(free)), replace=False)):
            x[b, i] = ODD[j]
        inf_at = sorted(biased & set(range(V)))
        if len(inf_at) > 3:
            x[b, inf_at[3]] = ODD[3]                                                 # +inf under a bias stays +inf
    return x.view(np.float32)


class Pass:
    """the device arrays of one chatts_logit_masks_apply call"""

    def __init__(self, x, V, off, rows, out_stride):
        batch = x.shape[0]
        self.batch, self.V, self.off, self.stride = batch, V, off, x.shape[1]
        self.lg = torch.from_numpy(x.copy()).to(DEV)
        self.out = torch.from_numpy(np.full((batch, out_stride), CANARY, dtype=np.uint32).view(np.float32)).to(DEV)
        W = (off + V + 31) // 32 + 1
        i32 = dict(dtype=torch.int32, device=DEV)
        self.allow, self.allow_on = torch.zeros((batch, W), **i32), torch.zeros(batch, **i32)
        self.bias_ids, self.bias_val = torch.zeros((batch, 1024), **i32), torch.zeros((batch, 1024), dtype=torch.float32, device=DEV)
        self.bias_n, self.end_ids, self.end_n = torch.zeros(batch, **i32), torch.zeros((batch, 64), **i32), torch.zeros(batch, **i32)
        self.min_tokens, self.step = torch.zeros(batch, **i32), torch.zeros(batch, **i32)
        for b, r in enumerate(rows):
            self.write(b, *r)
        self.args = _lib.LogitMaskArgs(out=self.out.data_ptr(), out_stride=out_stride, allow_bits=self.allow.data_ptr(), allow_stride=W,
                                       allow_on=self.allow_on.data_ptr(), bias_ids=self.bias_ids.data_ptr(), bias_val=self.bias_val.data_ptr(),
                                       bias_n=self.bias_n.data_ptr(), bias_stride=1024, end_ids=self.end_ids.data_ptr(),
                                       end_n=self.end_n.data_ptr(), min_tokens=self.min_tokens.data_ptr(), end_stride=64)

    def write(self, b, allowed, bias, min_tokens, ends, step):
        """row b's settings: plain device copies"""
        self.allow_on[b] = int(allowed is not None)
        if allowed is not None:
            self.allow[b].copy_(torch.from_numpy(ref.bitset(allowed, self.allow.shape[1]).view(np.int32)))
        ids = list(bias or {})
        self.bias_n[b] = len(ids)
        if ids:
            self.bias_ids[b, :len(ids)] = torch.tensor(ids, dtype=torch.int32)
            self.bias_val[b, :len(ids)] = torch.tensor([bias[t] for t in ids], dtype=torch.float32)
        self.end_n[b] = len(ends)
        if ends:
            self.end_ids[b, :len(ends)] = torch.tensor(ends, dtype=torch.int32)
        self.min_tokens[b], self.step[b] = min_tokens, step

    def call(self, lib):
        _lib.check(lib.chatts_logit_masks_apply(self.lg.data_ptr(), self.batch, self.stride, self.V, self.off, C.byref(self.args),
                                                self.step.data_ptr(), _st()))

    def result(self):
        torch.cuda.synchronize()
        return self.out.cpu().numpy(), self.lg.cpu().numpy()


def _check(x, V, off, rows, got, after):
    assert np.array_equal(after.view(np.uint32), x.view(np.uint32))                  # the raw logits (and their padding) are unchanged
    assert (got[:, V:].view(np.uint32) == CANARY).all()                              # the output padding past vocab is untouched
    for b, (allowed, bias, m, ends, step) in enumerate(rows):
        want = ref.apply(x[b, :V], allowed, bias, m, ends, step, off)
        same = got[b, :V].view(np.uint32) == want.view(np.uint32)
        assert same.all(), (b, np.nonzero(~same)[0][:8].tolist(), got[b, :V][~same][:4], want[~same][:4])
        if allowed is None and not bias and not (step < m and ends):
            assert np.array_equal(got[b, :V].view(np.uint32), x[b, :V].view(np.uint32))      # nothing set: every bit, NaN payloads included


@pytest.mark.parametrize("V", [31, 32, 33, 1023, 1024, 1025, 4099, 152064])
@pytest.mark.parametrize("batch", [1, 3, 16])
@pytest.mark.parametrize("aligned", [True, False])
def test_the_pass_equals_the_numpy_restatement_bit_for_bit(lib, V, batch, aligned):
    """aligned: the row strides of logits and output are multiples of 4, every row starts 16-byte aligned and the pass takes the 16-byte
    path (with a scalar tail where V is no multiple of 4); otherwise a stride that is none: the scalar path (batch 1 takes the
    vector path whatever the stride: only row 0 has to be aligned)."""
    rng = np.random.default_rng([SEED, V, batch, int(aligned)])
    rows = _rows(batch, V, 0, rng)
    stride = (V + 4) // 4 * 4 + (0 if aligned else 1)        # at least one cell of padding behind every row
    x = _logits(batch, V, stride, rows, 0, rng)
    p = Pass(x, V, 0, rows, stride + (4 if aligned else 2))
    p.call(lib)
    got, after = p.result()
    _check(x, V, 0, rows, got, after)


@pytest.mark.parametrize("off", [4100, 4099])
def test_a_vocabulary_slice_skips_the_ids_outside_it(lib, off):
    """vocab_offset = the first id of the slice (a multiple of 4: vector path; otherwise the scalar path): the bitset is indexed by global
    id, bias and end ids outside the slice are skipped"""
    V, batch = 4099, 3
    rng = np.random.default_rng([SEED, off])
    rows = _rows(batch, V, off, rng)
    x = _logits(batch, V, V + 1, rows, off, rng)
    p = Pass(x, V, off, rows, V + 1)
    p.call(lib)
    got, after = p.result()
    _check(x, V, off, rows, got, after)


def test_null_arrays_mean_off_and_the_pass_is_a_copy(lib):
    V, batch = 1025, 3
    rng = np.random.default_rng(SEED)
    rows = _rows(batch, V, 0, rng)
    x = _logits(batch, V, V + 3, rows, 0, rng)
    p = Pass(x, V, 0, rows, V + 3)
    p.args = _lib.LogitMaskArgs(out=p.out.data_ptr(), out_stride=V + 3)
    _lib.check(lib.chatts_logit_masks_apply(p.lg.data_ptr(), batch, V + 3, V, 0, C.byref(p.args), None, _st()))
    got, after = p.result()
    _check(x, V, 0, [(None, None, 0, [], 0)] * batch, got, after)


def test_a_replayed_graph_obeys_settings_rewritten_between_two_replays(lib):
    V, batch = 4099, 3
    rng = np.random.default_rng([SEED, 7])
    rows = _rows(batch, V, 0, rng)
    x = _logits(batch, V, V + 1, rows, 0, rng)
    p = Pass(x, V, 0, rows, V + 1)
    p.call(lib)
    eager, _ = p.result()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        p.call(lib)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        p.call(lib)
    p.out.copy_(torch.from_numpy(np.full(tuple(p.out.shape), CANARY, dtype=np.uint32).view(np.float32)))
    g.replay()
    got, after = p.result()
    _check(x, V, 0, rows, got, after)
    assert np.array_equal(got.view(np.uint32), eager.view(np.uint32))                # eager and replayed: the same bits
    # slot 1 (nothing set) gets a tenant, slot 0 loses its allow list and reaches min_tokens: plain device writes, then the same graph
    rows2 = [(None, rows[0][1], rows[0][2], rows[0][3], rows[0][2]), ([5, V - 1, 77], {77: -1.0}, 2, [5], 1), rows[2]]
    p.write(0, *rows2[0])
    p.write(1, *rows2[1])
    g.replay()
    got2, after2 = p.result()
    _check(x, V, 0, rows2, got2, after2)
    assert np.isfinite(got2[1, :V]).sum() <= 2                                       # the new tenant's three ids, one of them an end id


# ---- model: every token against the raw logits of its own step ---------------------------------------------------------------------------
PEN = dict(repetition_penalty=1.3, frequency_penalty=0.5, presence_penalty=0.5)
N_PLAIN = 12
# (series lengths, series seed) of each preset's prompt: one whose plain greedy run has a third token that differs from its first two
# (the min_tokens case stops on it); the synthetic models repeat themselves early on most prompts
PROMPTS = {"tiny-qwen2": ([50], 8), "tiny-qwen3": ([100, 40], 1234)}


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


def _steps(model, ids, ser, lens, n):
    """n tokens on the eager single-sequence path, one step at a time -> (tokens, the raw logits row each token was chosen from)"""
    assert not model.use_graph
    model._prefill_request(ids, ser, lens, n)
    rows = [model.buf["logits"].cpu().numpy().copy()]
    for _ in range(n - 1):
        model.decode_step()
        rows.append(model.buf["logits"].cpu().numpy().copy())
    toks = model.buf["out_tokens"][:n].tolist()
    model.note_generated(0, toks)
    return toks, rows


class Ctx:
    """one eager model per preset, its prompt, and the plain greedy run (computed once, before the mode was ever on)"""

    def __init__(self, preset):
        self.preset = preset
        self.cfg, self.model = _model(preset, use_graph=False)
        self.ids, self.ser, self.lens = _inputs(self.cfg, *PROMPTS[preset])
        self.V = self.cfg.vocab_size
        self.plain, self.plain_rows = _steps(self.model, self.ids, self.ser, self.lens, N_PLAIN)
        assert not self.model._masks_on and not any(k.startswith("lm_") for k in self.model.buf)

    def run(self, n, masks, end_ids=()):
        self.model.set_slot_masks(0, **masks, end_ids=end_ids)
        return _steps(self.model, self.ids, self.ser, self.lens, n)

    def captured(self, n, masks, eos=None):
        """the same request through generate_one and the captured step"""
        self.model.use_graph = True
        try:
            return self.model.generate_one(self.ids, self.ser, self.lens, n, eos_token_id=eos, masks=masks)
        finally:
            self.model.use_graph = False


_CTX = {}


@pytest.fixture(params=["tiny-qwen2", "tiny-qwen3"])
def ctx(request):
    if request.param not in _CTX:
        _CTX[request.param] = Ctx(request.param)
    c = _CTX[request.param]
    yield c
    c.model.set_slot_masks(0)                                 # every test leaves slot 0 at its defaults, greedy
    c.model.set_slot_controls(0)
    c.model.set_logit_controls(False)
    c.model.set_logprobs(False)
    c.model.set_sampling(0.0)
    c.model.use_graph = False


def test_allowed_token_ids_every_token_is_the_argmax_over_the_three(ctx):
    allowed = [ctx.plain[0], 11, ctx.V - 1]
    assert len(set(allowed)) == 3
    toks, rows = ctx.run(10, dict(allowed_token_ids=allowed))
    for k, (t, row) in enumerate(zip(toks, rows)):
        assert t == ref.argmax(ref.apply(row, allowed=allowed)) == allowed[int(np.argmax(row[allowed]))], (k, t)
    # token_logit is the logit the selection read (an allowed id's logit is the raw one)
    assert ctx.model.buf["token_logit"].cpu().numpy().view(np.uint32)[0] == rows[-1][toks[-1:]].view(np.uint32)[0]
    assert ctx.captured(10, dict(allowed_token_ids=allowed)) == toks
    assert ctx.captured(10, dict(allowed_token_ids=allowed[:1])) == allowed[:1] * 10          # a single allowed id


def test_logit_bias_minus_100_on_the_first_token_gives_the_runner_up(ctx):
    bias = {ctx.plain[0]: -100.0}
    toks, rows = ctx.run(4, dict(logit_bias=bias))
    order = np.argsort(-rows[0].astype(np.float64), kind="stable")
    assert order[0] == ctx.plain[0] and np.array_equal(rows[0].view(np.uint32), ctx.plain_rows[0].view(np.uint32))
    assert toks[0] == order[1] == ref.argmax(ref.apply(rows[0], bias=bias))
    for k, (t, row) in enumerate(zip(toks, rows)):
        assert t == ref.argmax(ref.apply(row, bias=bias)), k
    assert ctx.captured(4, dict(logit_bias=bias)) == toks


def test_logit_bias_plus_100_on_one_id_makes_every_token_that_id(ctx):
    tid = 4321 % ctx.V
    bias = {str(tid): 100.0}                                  # (a decimal string key, as the OpenAI JSON carries it)
    toks, rows = ctx.run(8, dict(logit_bias=bias))
    assert toks == [tid] * 8
    for k, row in enumerate(rows):
        assert ref.argmax(ref.apply(row, bias={tid: 100.0})) == tid, k
    want = np.float32(rows[-1][tid]) + np.float32(100.0)      # token_logit: the biased logit, one float32 add
    assert ctx.model.buf["token_logit"].cpu().numpy().view(np.uint32)[0] == np.array([want], dtype=np.float32).view(np.uint32)[0]
    assert ctx.captured(8, dict(logit_bias=bias)) == toks


def test_min_tokens_keeps_the_stop_id_away_for_six_tokens(ctx):
    stop = ctx.plain[2]
    assert stop not in ctx.plain[:2]                          # (a property of the model seed and the prompt)
    m = ctx.model
    assert len(m.generate_one(ctx.ids, ctx.ser, ctx.lens, N_PLAIN, eos_token_id=[stop], masks={})) == 3       # the plain run ends after 3
    out = m.generate_one(ctx.ids, ctx.ser, ctx.lens, N_PLAIN, eos_token_id=[stop], masks=dict(min_tokens=6))
    assert len(out) >= 6 and stop not in out[:6]
    assert ctx.captured(N_PLAIN, dict(min_tokens=6), eos=[stop]) == out
    toks, rows = ctx.run(N_PLAIN, dict(min_tokens=6), end_ids=[stop])
    assert toks[:len(out)] == out and toks[2] != stop
    for k, (t, row) in enumerate(zip(toks, rows)):
        assert t == ref.argmax(ref.apply(row, min_tokens=6, end_ids=[stop], step=k)), k
        if k >= 6:
            assert t == ref.argmax(row), k                    # from the seventh token on the raw argmax again
    # HF's name: min_new_tokens
    x = torch.tensor([ctx.ids])
    hf = m.generate(input_ids=x, timeseries=ctx.ser, valid_lengths=ctx.lens, max_new_tokens=N_PLAIN, eos_token_id=[stop], min_new_tokens=6)
    assert hf[0, len(ctx.ids):].tolist() == out
    hf0 = m.generate(input_ids=x, timeseries=ctx.ser, valid_lengths=ctx.lens, max_new_tokens=N_PLAIN, eos_token_id=[stop])
    assert hf0[0, len(ctx.ids):].tolist() == ctx.plain[:3] and not m._masks_on


def test_penalties_read_the_biased_logits(ctx):
    """order: raw -> logit_bias -> repetition -> frequency and presence -> argmax.  The float64 restatement of the penalties on the
    (exact) biased row names the engine's token; its two best candidates are further apart than the penalty kernel's error bound for
    them at every step (a property of seed and prompt that is asserted, not a reason to leave a step out)."""
    n = 24
    bias = {ctx.plain[0]: -100.0, ctx.plain[1]: 2.0, 77: 6.0}
    ctx.model.set_slot_controls(0, **PEN)
    toks, rows = ctx.run(n, dict(logit_bias=bias))
    inp = lc_ref.prompt_mask(ctx.ids, ctx.V)
    r, f, p = PEN["repetition_penalty"], PEN["frequency_penalty"], PEN["presence_penalty"]
    for k in range(n):
        masked = ref.apply(rows[k], bias=bias)
        cnt = lc_ref.counts_of(toks[:k], ctx.V)
        want, margin = lc_ref.greedy(masked, inp, cnt, r, f, p)
        pen = lc_ref.penalise(masked, inp, cnt, r, f, p)
        slack = float(lc_ref.penalty_bound(masked, cnt, r, f, p)[np.argsort(pen)[-2:]].sum())
        print(f"step {k}: engine {toks[k]} restatement {want} margin {margin:.3e} bound {slack:.3e}")
        assert margin > slack, (k, margin, slack)
        assert toks[k] == want, (k, toks[k], want)
    assert toks[0] != ctx.plain[0]
    ctx.model.use_graph = True
    assert ctx.model.generate_one(ctx.ids, ctx.ser, ctx.lens, n, controls=PEN, masks=dict(logit_bias=bias)) == toks


def test_logprobs_stay_those_of_the_raw_logits(ctx):
    n = 8
    allowed = [5, 11, ctx.V - 1]
    ctx.model.set_logprobs(True)
    toks, rows = ctx.run(n, dict(allowed_token_ids=allowed))
    entries = ctx.model.read_logprobs(0, 0, n, 5)
    passed_over = 0
    for k, (tok, (lp, rank, top)) in enumerate(zip(toks, entries)):
        l = rows[k].astype(np.float64)
        lsm = l - (l.max() + np.log(np.exp(l - l.max()).sum()))
        assert abs(lp - lsm[tok]) <= 1e-5 + 1e-7 * abs(lsm[tok]), (k, lp, lsm[tok])       # (the logprobs kernel test's tolerance)
        assert [i for i, _ in top] == np.lexsort((np.arange(len(l)), -l))[:5].tolist()
        assert rank == 1 + int((l > l[tok]).sum()) + int((l[:tok] == l[tok]).sum())
        passed_over += rank != 1
    assert passed_over > 0 and set(toks) <= set(allowed)


def test_sampled_tokens_stay_in_the_set_and_repeat_with_the_seed(ctx):
    m = ctx.model
    allowed = np.argsort(-ctx.plain_rows[0])[:3].tolist()     # the three raw favourites of the first step
    m.set_sampling_rows()
    m.set_slot_sampling(0, 1.0, 0, 1.0, 5)
    a = m.generate_one(ctx.ids, ctx.ser, ctx.lens, 64, masks=dict(allowed_token_ids=allowed))
    assert len(a) == 64 and set(a) <= set(allowed)
    assert m.generate_one(ctx.ids, ctx.ser, ctx.lens, 64, masks=dict(allowed_token_ids=allowed)) == a
    assert ctx.captured(64, dict(allowed_token_ids=allowed)) == a
    m.set_slot_sampling(0, 1.0, 0, 1.0, 6)
    b = m.generate_one(ctx.ids, ctx.ser, ctx.lens, 64, masks=dict(allowed_token_ids=allowed))
    assert set(b) <= set(allowed)
    print(f"seed 5: {a[:16]} seed 6: {b[:16]}")
    # the same seed in another slot: two cache slots, the sampled request once in slot 0 and once in slot 1 beside a plain greedy one
    cfg, mb = _model(ctx.preset, max_batch=2)
    other = _inputs(cfg, [30], 6)
    mb.set_sampling_rows()
    runs = []
    for slot in (0, 1):
        mb.set_slot_sampling(slot, 1.0, 0, 1.0, 5)
        mb.set_slot_sampling(1 - slot, 0.0)
        reqs, msk = [(ctx.ids, ctx.ser, ctx.lens), other], [dict(allowed_token_ids=allowed), None]
        outs = mb.generate_batch(reqs[::-1] if slot else reqs, 64, eos_token_id=[], masks=msk[::-1] if slot else msk)
        runs.append(outs[slot])
        assert len(outs[slot]) == 64 and set(outs[slot]) <= set(allowed), slot
        assert len(set(outs[1 - slot]) - set(allowed)) > 0           # the neighbour is not constrained
    assert runs[0] == runs[1]


def test_slot_reuse_leaves_nothing_behind():
    cfg, model = _model(enable_prefix_caching=True)
    ids, ser, lens = _inputs(cfg, [100, 40])
    n = 12
    first = model.generate_one(ids, ser, lens, n, masks=dict(allowed_token_ids=[5, 6, 7], logit_bias={5: 3.0}, min_tokens=4), eos_token_id=[6])
    assert set(first) <= {5, 6, 7} and model._masks_on
    hits = model.prefix_stats["hits"]
    second = model.generate_one(ids, ser, lens, n, masks={})              # the same slot, the same prompt (its K/V rows are reused)
    assert model.prefix_stats["hits"] == hits + 1
    cfg, fresh = _model(enable_prefix_caching=True)
    fresh.generate_one(ids, ser, lens, n)
    assert second == fresh.generate_one(ids, ser, lens, n) and not fresh._masks_on
    # batched: a slot's next tenant starts from clean rows
    cfg, mb = _model(max_batch=2)
    req = [(ids, ser, lens)] * 2
    plain = mb.generate_batch(req, n, eos_token_id=[])
    a = mb.generate_batch(req, n, eos_token_id=[], masks=[dict(allowed_token_ids=[9]), None])
    assert a[0] == [9] * n and a[1] == plain[1]
    b = mb.generate_batch(req, n, eos_token_id=[], masks=[None, dict(logit_bias={"9": 100})])
    assert b[0] == plain[0] and b[1] == [9] * n
    with pytest.raises(ValueError, match="allowed_token_ids"):
        mb.generate_batch(req, n, masks=dict(allowed_token_ids=[cfg.vocab_size]))
    with pytest.raises(ValueError, match="min_tokens"):
        mb.generate_one(ids, ser, lens, 4, masks=dict(min_tokens=5))


def test_a_model_that_gets_no_such_request_never_calls_a_new_entry_point(lib, monkeypatch):
    calls = []
    for name in ("chatts_logit_masks_apply", "chatts_decoder_set_logit_masks", "chatts_decoder_select_tokens_masked"):
        real = getattr(lib, name)
        monkeypatch.setattr(lib, name, lambda *a, _n=name, _r=real: (calls.append(_n), _r(*a))[1])
    cfg, model = _model(max_batch=2)
    ids, ser, lens = _inputs(cfg, [64, 30])
    model.generate_one(ids, ser, lens, 8)
    model.generate_batch([(ids, ser, lens)] * 3, 8, eos_token_id=[], controls=[None, dict(repetition_penalty=1.2), None])
    model.generate_one(ids, ser, lens, 8, masks={})           # all-default values never allocate
    model.set_slot_masks(1, logit_bias={}, allowed_token_ids=None, min_tokens=0, end_ids=[3])
    model.set_slot_masks(0, min_tokens=4)                     # nothing could end the sequence: nothing to keep away
    x = torch.tensor([ids])
    model.generate(input_ids=x, timeseries=ser, valid_lengths=lens, max_new_tokens=4, eos_token_id=[])
    assert calls == [] and not model._masks_on
    assert not any(k.startswith("lm_") for k in model.buf)
    model.generate_one(ids, ser, lens, 4, masks=dict(logit_bias={3: 1.0}))
    assert "chatts_decoder_set_logit_masks" in calls and "chatts_decoder_select_tokens_masked" in calls


# ---- engine -----------------------------------------------------------------------------------------------------------------------
def _engine_setup(max_num_seqs=4, **kw):
    from chatts_amd import LLM
    cfg = cfgmod.preset("tiny-qwen2")
    llm = LLM(cfg, max_model_len=512, seed=MODEL_SEED, max_num_seqs=max_num_seqs, **kw)
    rng = np.random.default_rng(9)
    prompts = [(chat_prompt([L]), [random_walk_series(rng, L).tolist()]) for L in (64, 30, 17, 40)]
    return cfg, llm, prompts


def _run(llm, prompts, plan, n=16, **engine_kw):
    from chatts_amd.engine import Engine
    eng = Engine(llm.model, llm.processor, sync_every=3, **engine_kw)
    reqs = [eng.add_request(prompts[p][0], prompts[p][1], max_tokens=n, ignore_eos=True, **kw) for p, kw in plan]
    eng.run_until_done()
    assert all(r.error is None for r in reqs), [r.error for r in reqs]
    return eng, reqs


def test_engine_three_requests_share_one_batched_step():
    cfg, llm, prompts = _engine_setup()
    m, V = llm.model, cfg.vocab_size
    _, solo = _run(llm, prompts, [(2, {})])                   # the plain request alone, on a model that never turned the mode on
    assert not m._masks_on and not any(k.startswith("lm_") for k in m.buf)
    allowed = [3, 30, V - 1]
    eng, (a, b, c) = _run(llm, prompts, [(0, dict(allowed_token_ids=allowed)), (1, dict(logit_bias={"77": 100})), (2, {})],
                          greedy_return_steps=2)
    assert m._masks_on and m._graph_batched is not None       # one captured batched step served the three
    assert set(a.tokens) <= set(allowed) and len(a.tokens) == 16
    assert b.tokens == [77] * 16
    assert c.tokens == solo[0].tokens
    for _ in range(3):                                        # iterations without a requester: the mode goes off again
        eng.add_request(prompts[2][0], prompts[2][1], max_tokens=2, ignore_eos=True)
        eng.run_until_done()
    assert not m._masks_on
    # n = 2, sampled: both samples stay in the set; sample 0 is the n = 1 answer of the same seed, in whatever slot it runs
    _, (par,) = _run(llm, prompts, [(3, dict(allowed_token_ids=allowed, n=2, temperature=1.0, seed=5))])
    assert len(par.children) == 2 and all(set(ch.tokens) <= set(allowed) and len(ch.tokens) == 16 for ch in par.children)
    _, (one,) = _run(llm, prompts, [(3, dict(allowed_token_ids=allowed, temperature=1.0, seed=5))])
    _, (_, other) = _run(llm, prompts, [(2, {}), (3, dict(allowed_token_ids=allowed, temperature=1.0, seed=5))])
    assert one.tokens == par.children[0].tokens == other.tokens
    with pytest.raises(ValueError, match="allowed_token_ids"):
        eng.add_request(prompts[0][0], prompts[0][1], allowed_token_ids=[V])
    with pytest.raises(ValueError, match="logit_bias"):
        eng.add_request(prompts[0][0], prompts[0][1], logit_bias={str(V): 1.0})


def test_engine_min_tokens_and_stop_strings_and_slot_reuse():
    cfg, llm, _ = _engine_setup(max_num_seqs=1)
    m = llm.model
    lengths, seed = PROMPTS["tiny-qwen2"]                     # (the prompt whose third plain token differs from its first two)
    rng = np.random.default_rng(seed)
    prompts = [(chat_prompt(lengths), [random_walk_series(rng, L).tolist() for L in lengths])]
    _, (plain,) = _run(llm, prompts, [(0, {})], n=10)
    stop = plain.tokens[2]
    assert stop not in plain.tokens[:2]
    from chatts_amd.engine import Engine
    eng = Engine(m, llm.processor, sync_every=3)
    kw = dict(max_tokens=10, stop_token_ids=[stop], ignore_eos=True)
    short = eng.add_request(*prompts[0], **kw)
    held = eng.add_request(*prompts[0], min_tokens=6, **kw)
    after = eng.add_request(*prompts[0], **kw)                # the same slot, after the constrained tenant
    eng.run_until_done()
    assert short.tokens == plain.tokens[:3] == after.tokens and short.finish_reason == "stop"
    assert len(held.tokens) >= 6 and stop not in held.tokens[:6] and held.tokens[:2] == plain.tokens[:2]


def test_speculation_steps_aside_for_a_biased_request_and_comes_back():
    from chatts_amd import LLM, SamplingParams
    cfg = cfgmod.preset("tiny-qwen2")
    llm = LLM(cfg, max_model_len=512, seed=MODEL_SEED, speculative_config={"method": "ngram", "num_speculative_tokens": 4})
    rng = np.random.default_rng(2)
    req = [{"prompt": "Describe <ts><ts/>", "multi_modal_data": {"timeseries": [random_walk_series(rng, 40).tolist()]}}]
    n = 24
    plain = llm.generate(req, SamplingParams(max_tokens=n, ignore_eos=True))[0].outputs[0].token_ids
    assert llm.model.spec_stats["steps"] > 0
    llm.model.spec_stats_reset()
    out = llm.generate(req, SamplingParams(max_tokens=n, ignore_eos=True, logit_bias={plain[0]: -100}))[0].outputs[0].token_ids
    assert llm.model.spec_stats["steps"] == 0 and out[0] != plain[0] and len(out) == n        # the plain step
    again = llm.generate(req, SamplingParams(max_tokens=n, ignore_eos=True))[0].outputs[0].token_ids
    assert llm.model.spec_stats["steps"] > 0 and again == plain and not llm.model._masks_on
    with pytest.raises(ValueError, match="logit_bias"):
        llm.generate(req, SamplingParams(max_tokens=4, logit_bias={cfg.vocab_size: 1.0}))


# ---- server -----------------------------------------------------------------------------------------------------------------------
def test_server_streamed_and_blocking_completions_are_constrained():
    from starlette.testclient import TestClient
    from chatts_amd import server
    cfg = cfgmod.preset("tiny-qwen2")
    rng = np.random.default_rng(2)
    ts = random_walk_series(rng, 40)
    n, V = 12, cfg.vocab_size
    app = server.build_server(cfg, max_model_len=512, max_num_seqs=2, seed=MODEL_SEED)
    try:
        client = TestClient(app)
        body = {"model": "chatts", "prompt": "Describe <ts><ts/>", "multi_modal_data": {"timeseries": [ts.tolist()]}, "max_tokens": n,
                "ignore_eos": True}
        plain = client.post("/v1/completions", json=body).json()["token_ids"]
        d = client.post("/v1/completions", json=dict(body, allowed_token_ids=[400, 401, 402], logit_bias={"401": 250})).json()
        assert d["token_ids"] == [401] * n                     # (250 is clamped to 100: still decisive)
        d = client.post("/v1/completions", json=dict(body, logit_bias={str(plain[0]): -100})).json()
        assert d["token_ids"][0] != plain[0] and len(d["token_ids"]) == n
        msgs = [{"role": "user", "content": [{"type": "text", "text": "Describe <ts><ts/>"}, {"timeseries": ts.tolist()}]}]
        chat = {"messages": msgs, "max_tokens": n, "ignore_eos": True, "allowed_token_ids": [400, 401, 402], "logit_bias": {"402": 100},
                "logprobs": True, "stream": True}
        with client.stream("POST", "/v1/chat/completions", json=chat) as resp:
            assert resp.status_code == 200
            events = [line[6:] for line in resp.iter_lines() if line.startswith("data: ")]
        assert events[-1] == "[DONE]"
        tok = app.state.llm.processor.tokenizer
        pieces = [e["token"] for ev in events[:-1] for ch in json.loads(ev)["choices"] for e in ((ch.get("logprobs") or {}).get("content") or [])]
        assert pieces == [tok.decode([402], skip_special_tokens=False)] * n
        assert client.post("/v1/completions", json=body).json()["token_ids"] == plain
        for bad, field in ((dict(logit_bias={str(V): 1.0}), "logit_bias"), (dict(allowed_token_ids=[V + 5]), "allowed_token_ids"),
                           (dict(min_tokens=n + 1), "min_tokens")):
            r = client.post("/v1/completions", json=dict(body, **bad))
            assert r.status_code == 400 and field in r.json()["error"]["message"], (bad, r.text)
            r = client.post("/v1/chat/completions", json=dict(chat, stream=False, **bad))
            assert r.status_code == 400 and field in r.json()["error"]["message"], (bad, r.text)
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
llm = LLM("tiny-qwen3", tensor_parallel_size=world, max_model_len=512, seed=3)
V = llm.config.vocab_size
rng = np.random.default_rng(1234)
lengths = [64, 30]
series = [random_walk_series(rng, L) for L in lengths]
req = [{{"prompt": chat_prompt(lengths), "multi_modal_data": {{"timeseries": [s.tolist() for s in series]}}}}]
gen = lambda **kw: llm.generate(req, SamplingParams(max_tokens=16, ignore_eos=True, **kw))[0].outputs[0].token_ids
plain = gen()
allowed = [plain[0], 7, V // 2 + 3, V - 1]
alw = gen(allowed_token_ids=allowed)
bias = gen(logit_bias={{plain[0]: -100.0, V - 2: 3.0}})
smp = gen(allowed_token_ids=allowed, temperature=1.0, seed=11)
again = gen()
print("RESULT " + json.dumps(dict(rank=rank, plain=plain, alw=alw, bias=bias, smp=smp, again=again, allowed=allowed)), flush=True)
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
    assert set(one["alw"]) <= set(one["allowed"]) and set(one["smp"]) <= set(one["allowed"])
    assert one["bias"][0] != one["plain"][0] and one["again"] == one["plain"]
    for r in two:
        for key in ("plain", "alw", "bias", "smp", "again"):
            assert r[key] == one[key], (r["rank"], key)
