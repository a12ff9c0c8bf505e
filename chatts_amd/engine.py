"""Request-level engine: incremental continuous batching over the model's KV-cache slots.

The role vLLM's LLMEngine / AsyncLLMEngine plays for the reference (NetManAIOps/ChatTS demo/demo_vllm.py:49-63 offline,
scripts/start_vllm_server.sh + chatts/utils/vllm_stream_qa.py:41-52 streaming): requests arrive at any time, are admitted
into free cache slots between decode steps, advance together in one batched step, and hand their new tokens back as
they are produced.  One engine owns one model (= one GPU, or one TP rank group); it is driven by a single thread
(`EngineThread`) because the HIP stream, the captured graphs and the slot state are not re-entrant.

Sampling: with a model that keeps per-slot sampling settings on the device (`set_slot_sampling`, ChattsSamplingArgs.*_rows) requests
with DIFFERENT temperature / top-k / top-p / seed decode together in one captured step - each slot's settings are written when the
request is admitted; the step selects greedily as long as nobody samples.  With a model that only has one baked-in configuration
(`set_sampling`) the requests decoded together share it: a request with a different one waits until the running batch has drained.
"""
import queue
import threading
import time
from collections import deque

import numpy as np


def validate_controls(repetition_penalty=None, frequency_penalty=None, presence_penalty=None, min_p=None):
    """The four logit controls with vLLM's defaults and ranges -> (r, f, p, min_p) as floats (None = the default); ValueError otherwise."""
    import math
    vals = []
    for name, v, default in (("repetition_penalty", repetition_penalty, 1.0), ("frequency_penalty", frequency_penalty, 0.0),
                             ("presence_penalty", presence_penalty, 0.0), ("min_p", min_p, 0.0)):
        v = default if v is None else v
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not math.isfinite(v):
            raise ValueError(f"{name} must be a finite number, got {v!r}")
        vals.append(float(v))
    r, f, p, m = vals
    if not r > 0.0:
        raise ValueError(f"repetition_penalty must be > 0, got {repetition_penalty}")
    if not -2.0 <= f <= 2.0:
        raise ValueError(f"frequency_penalty must be in [-2, 2], got {frequency_penalty}")
    if not -2.0 <= p <= 2.0:
        raise ValueError(f"presence_penalty must be in [-2, 2], got {presence_penalty}")
    if not 0.0 <= m <= 1.0:
        raise ValueError(f"min_p must be in [0, 1], got {min_p}")
    return r, f, p, m


NO_CONTROLS = (1.0, 0.0, 0.0, 0.0)


def validate_n(n=None, best_of=None, max_num_seqs=None):
    """n (samples per prompt, vLLM's name) -> int >= 1; best_of only as None or equal to n (vLLM V1 removed it); siblings are admitted
    together, so n may not exceed max_num_seqs (checked when given).  ValueError otherwise."""
    n = 1 if n is None else n
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or int(n) < 1:
        raise ValueError(f"n must be an integer >= 1, got {n!r}")
    if best_of is not None and (isinstance(best_of, bool) or not isinstance(best_of, (int, np.integer)) or int(best_of) != int(n)):
        raise ValueError(f"best_of is accepted only as None or equal to n={n}, got {best_of!r}")
    if max_num_seqs is not None and int(n) > int(max_num_seqs):
        raise ValueError(f"n={n} exceeds max_num_seqs={max_num_seqs}: the samples of one prompt are admitted together")
    return int(n)


def validate_sampling(max_tokens=64, temperature=0.0, top_p=1.0, top_k=0, logprobs=None, max_logprobs=20, prompt_logprobs=None,
                      repetition_penalty=None, frequency_penalty=None, presence_penalty=None, min_p=None, n=None, best_of=None,
                      stop=None, **_):
    """The ranges vLLM's SamplingParams accepts (what the reference's drivers pass: inference_tsmllm_vllm.py:43-46,
    llm_utils.py:153).  Raises ValueError - the server turns it into a 400 - BEFORE the request can reach the engine thread, where
    an out-of-range value would otherwise surface inside set_sampling / chatts_decoder_set_sampling."""
    import math
    from .detok import normalize_stop
    validate_controls(repetition_penalty, frequency_penalty, presence_penalty, min_p)
    validate_n(n, best_of)
    normalize_stop(stop)
    t = 0.0 if temperature is None else float(temperature)
    if not math.isfinite(t) or t < 0.0:
        raise ValueError(f"temperature must be a finite number >= 0, got {temperature}")
    p = 1.0 if top_p is None else float(top_p)
    if not math.isfinite(p) or not (0.0 < p <= 1.0):
        raise ValueError(f"top_p must be in (0, 1], got {top_p}")
    if int(top_k or 0) < -1:
        raise ValueError(f"top_k must be -1 / 0 (off) or positive, got {top_k}")
    if int(max_tokens) < 1:
        raise ValueError(f"max_tokens must be at least 1, got {max_tokens}")
    if prompt_logprobs is not None:
        raise ValueError("prompt_logprobs is not supported (only the logprobs of generated tokens)")
    if logprobs is not None and (isinstance(logprobs, bool) or not isinstance(logprobs, (int, np.integer))
                                 or not 0 <= int(logprobs) <= int(max_logprobs)):
        raise ValueError(f"logprobs must be an integer in 0..{max_logprobs} (max_logprobs), got {logprobs!r}")


class ExchangeBroken(RuntimeError):
    """The tensor-parallel exchange timed out on THIS rank.  Fatal for the whole rank group: the ranks can no longer be assumed to hold
    the same engine state (a peer that arrived late saw no timeout and kept decoding), so the engine stops instead of serving
    on - EngineThread fails every request, releases the followers, and a supervisor restarts all ranks."""


class Request:
    def __init__(self, rid, prompt, timeseries, max_tokens, sampling_key, eos, on_tokens):
        self.rid, self.prompt, self.timeseries, self.max_tokens = rid, prompt, timeseries, int(max_tokens)
        self.sampling_key, self.eos, self.on_tokens = sampling_key, set(eos or ()), on_tokens
        self.tokens, self.sent, self.finished, self.finish_reason = [], 0, False, None
        self.prompt_tokens = 0
        # logprobs=k: one (logprob, rank, [(id, logprob)] * k) entry per token of `tokens`, grown with it; None when not asked
        self.logprob_k, self.logprobs, self.cumulative_logprob = None, None, None
        self.t_arrival, self.t_first = time.perf_counter(), None
        self.error = None
        self.controls = NO_CONTROLS          # (repetition_penalty, frequency_penalty, presence_penalty, min_p): Engine.add_request
        self.bypassed = 0                    # later arrivals admitted past this request while it waited for its sampling group
        # n > 1 (parallel sampling): the request the caller holds is the PARENT - it never occupies a slot; `children` are the n
        # sequences (index 0 .. n-1, each with the fields of a request of its own), `remaining` those still running
        self.n, self.index, self.parent, self.children, self.remaining = 1, 0, None, None, 0
        # stop strings: `text` is then the engine's own decode (what a stream may show so far; the final text once finished)
        self.stop, self.include_stop, self.checker, self.text = [], False, None, None
        self.stop_reason = None              # the matched stop string, the id of a stop_token_ids hit, None for EOS / length
        self.stop_ids = set()

    @property
    def outputs(self):
        """the n sequences of this request in index order (the request itself when n == 1)"""
        return list(self.children) if self.children else [self]


class Engine:
    """add_request() / step() like vLLM's LLMEngine.  `on_tokens(request, new_token_ids, finished)` is called from step()."""

    def __init__(self, model, processor, sync_every=4, prefill_chunk_tokens=None, greedy_return_steps=256):
        self.model, self.processor = model, processor
        # per-slot sampling: scheduler iterations without any sampling request (running or waiting) after which the step goes back from the
        # per-row sampler to the plain argmax tail (a graph re-capture); 0 = stay in per-row mode once entered.  Every rank of a
        # tensor-parallel group counts the same iterations (followers replay the leader's), so all of them switch together.
        self.greedy_return_steps = max(0, int(greedy_return_steps))
        self._greedy_iters = 0
        self._no_logprob_iters = 0
        self._no_control_iters = 0
        self.sync_every = max(1, int(sync_every))       # decode steps between device->host token reads
        # chunked-prefill scheduling (vLLM: enable_chunked_prefill / max_num_batched_tokens): while other sequences are decoding, a
        # long prompt is prefilled this many rows per scheduler iteration, each followed by one decode step of the running batch,
        # instead of stalling them for the whole prefill.  None: a prompt is always prefilled in one go.
        self.prefill_chunk_tokens = None if not prefill_chunk_tokens else max(16, int(prefill_chunk_tokens))
        self.prefilling = None                          # (request, slot, admission state) of the prompt being prefilled in chunks
        self.max_bypass = 8                             # admissions that may overtake a request waiting for another sampling group
        self.waiting = deque()
        self.nslots = max(1, model.max_batch)
        self.slots = [None] * self.nslots
        self.produced = [0] * self.nslots
        self.active_key = None
        self.mixed = hasattr(model, "set_slot_sampling")   # per-slot sampling settings on the device: no sampling groups
        self._since_sync = 0
        self._rid = 0
        if self.nslots > 1:
            model.buf["pos_all"].fill_(-1)            # every slot starts parked

    # ---- requests ---------------------------------------------------------------------------------
    def add_request(self, prompt, timeseries=None, max_tokens=64, temperature=0.0, top_p=1.0, top_k=0, seed=None,
                    stop_token_ids=None, ignore_eos=False, on_tokens=None, logprobs=None, repetition_penalty=None,
                    frequency_penalty=None, presence_penalty=None, min_p=None, n=1, best_of=None, stop=None,
                    include_stop_str_in_output=False):
        """seed None: per-slot mode gives every request its own stream (a hash of its arrival number - vLLM's seed=None means "not
        reproducible across requests"; here two identical prompts still differ, and a rerun of the same arrival order repeats);
        grouped mode uses 0 (requests that decode together must share ONE configuration there).
        n > 1: -> the parent request; its `children` are n sequences of the one prompt, child i drawing with seed + i (mod 2^32), all
        admitted together from ONE prefill (step()).  on_tokens is called per child (`r.index`, `r.parent`).
        stop: strings that end a sequence when they appear in its decoded text (chatts_amd/detok.py: the rule)."""
        validate_sampling(max_tokens, temperature, top_p, top_k, logprobs=logprobs, max_logprobs=self.max_logprobs)
        n, stop = self.check_request(n, best_of, stop)
        controls = validate_controls(repetition_penalty, frequency_penalty, presence_penalty, min_p)
        if controls != NO_CONTROLS and not hasattr(self.model, "set_slot_controls"):
            raise ValueError("this model does not apply repetition / frequency / presence penalties or min_p")
        if logprobs is not None and not hasattr(self.model, "set_logprobs"):
            raise ValueError("this model does not compute logprobs")
        if seed is None:
            seed = ((self._rid + 1) * 2654435761) & 0xFFFFFFFF if self.mixed else 0
        e = self.model.config.eos_token_id
        eos = [] if ignore_eos else (list(e) if isinstance(e, (list, tuple)) else [e])
        eos += list(stop_token_ids or [])
        key = None if not temperature else (float(temperature), max(int(top_k or 0), 0), float(top_p), int(seed))
        self._rid += 1
        r = Request(self._rid, prompt, list(timeseries or []), max_tokens, key, eos, on_tokens)
        r.sampling = (0.0, 0, 1.0, 0) if key is None else key
        r.controls = controls                # (repetition_penalty, frequency_penalty, presence_penalty, min_p)
        if logprobs is not None:
            r.logprob_k, r.logprobs, r.cumulative_logprob = int(logprobs), [], 0.0
        if self.mixed:
            r.sampling_key = "rows" if key is not None else None     # one group: who samples is a per-slot matter
        r.stop, r.include_stop, r.stop_ids = stop, bool(include_stop_str_in_output), {int(t) for t in (stop_token_ids or [])}
        if n > 1:
            r.n, r.remaining, r.children = n, n, []
            for i in range(n):
                c = Request(r.rid, prompt, r.timeseries, max_tokens, r.sampling_key, eos, on_tokens)
                c.index, c.parent, c.controls, c.t_arrival = i, r, controls, r.t_arrival
                c.sampling = r.sampling[:3] + ((int(seed) + i) & 0xFFFFFFFF,)
                c.stop, c.include_stop, c.stop_ids = stop, r.include_stop, r.stop_ids
                if logprobs is not None:
                    c.logprob_k, c.logprobs, c.cumulative_logprob = int(logprobs), [], 0.0
                r.children.append(c)
        self.waiting.append(r)
        return r

    def check_request(self, n=None, best_of=None, stop=None, **_):
        """What this engine refuses about n and stop beyond their value ranges (ValueError): n > max_num_seqs, n > 1 on a model without
        per-slot sampling settings or without a fork, stop strings without a tokenizer.  -> (n, list of stop strings).  add_request
        calls it; EngineThread calls it BEFORE a request is announced to the follower ranks."""
        from .detok import normalize_stop
        n = validate_n(n, best_of, self.nslots)
        stop = normalize_stop(stop)
        if n > 1 and not self.mixed:
            raise ValueError("n > 1 needs a model with per-slot sampling settings (set_slot_sampling)")
        if n > 1 and not hasattr(self.model, "admit_fork"):
            raise ValueError("this model cannot fork a prompt into several samples (n > 1)")
        if stop and getattr(self.processor, "tokenizer", None) is None:
            raise ValueError("stop strings need a tokenizer (the engine's processor has none)")
        return n, stop

    @property
    def max_logprobs(self):
        return int(getattr(self.model, "max_logprobs", 20))

    def _logprobs_mode(self):
        """Logprobs on while any running, prefilling or waiting request asks for them; off again after `greedy_return_steps`
        consecutive iterations without one (the sampling mode's hysteresis, for the same reason: a switch re-captures the graphs;
        0 = stay on once on).  Followers replay the leader's requests and count the same iterations: all ranks switch together."""
        if not hasattr(self.model, "set_logprobs"):
            return
        want = (any(r is not None and r.logprob_k is not None for r in self.slots) or
                (self.prefilling is not None and self.prefilling[0].logprob_k is not None) or
                any(q.logprob_k is not None for q in self.waiting))
        on = bool(getattr(self.model, "_logprobs_on", False))
        if want:
            self._no_logprob_iters = 0
            if not on:
                self.model.set_logprobs(True)
        elif on:
            self._no_logprob_iters += 1
            if self.greedy_return_steps and self._no_logprob_iters >= self.greedy_return_steps:
                self.model.set_logprobs(False)

    def _controls_mode(self):
        """The model's logit-controls mode on while any running, prefilling or waiting request has a penalty or min_p; off again after
        `greedy_return_steps` consecutive iterations without one (the hysteresis of _logprobs_mode, for the same reason)."""
        if not hasattr(self.model, "set_logit_controls"):
            return
        want = (any(r is not None and r.controls != NO_CONTROLS for r in self.slots) or
                (self.prefilling is not None and self.prefilling[0].controls != NO_CONTROLS) or
                any(q.controls != NO_CONTROLS for q in self.waiting))
        on = bool(getattr(self.model, "_controls_on", False))
        if want:
            self._no_control_iters = 0
            if not on:
                self.model.set_logit_controls(True)
        elif on:
            self._no_control_iters += 1
            if self.greedy_return_steps and self._no_control_iters >= self.greedy_return_steps:
                self.model.set_logit_controls(False)

    def has_work(self):
        return bool(self.waiting) or self.prefilling is not None or any(s is not None for s in self.slots)

    def _encode(self, r):
        import torch
        text, encs, lens = self.processor.splice(r.prompt, [np.asarray(s, dtype=np.float64) for s in r.timeseries])
        ids = self.processor.tokenizer.encode(text)
        ser = torch.from_numpy(self.processor.pad_stack(encs)) if encs else None
        return ids, ser, lens

    def _apply_sampling(self, key):
        if key is None:
            self.model.set_sampling(0.0)
        elif key == "rows":
            self.model.set_sampling_rows()
        else:
            self.model.set_sampling(key[0], key[1], key[2], key[3])
        self.active_key = key

    def _mixed_mode(self):
        """Per-slot mode: the step draws per row (greedy rows included) while any running or waiting request samples, and goes back
        to the plain argmax tail when nobody does.  Every slot's settings are current at all times, so the switch is safe whenever."""
        want = "rows" if (any(r is not None and r.sampling_key for r in self.slots) or
                          (self.prefilling is not None and self.prefilling[0].sampling_key) or
                          any(q.sampling_key for q in self.waiting)) else None
        if want is None and self.active_key == "rows":
            # Hysteresis instead of either extreme.  Every switch drops both captured hipGraphs (re-capture + a warm eager step on all
            # ranks), so alternating traffic must not flip the mode per request; but staying in per-row mode for good would leave later
            # greedy traffic on the sampler path (under TP: a full-vocabulary all-gather + the sampler kernel per step instead of the
            # 2-word tp_argmax).  So: back to the argmax tail after `greedy_return_steps` consecutive iterations without any sampling
            # request running or waiting (0 = never switch back).
            self._greedy_iters = getattr(self, "_greedy_iters", 0) + 1
            if not self.greedy_return_steps or self._greedy_iters < self.greedy_return_steps:
                return
        if want == "rows":
            self._greedy_iters = 0
        if want != self.active_key:
            self._apply_sampling(want)

    def _emit(self, r, finished, reason=None):
        new = r.tokens[r.sent:]
        r.sent = len(r.tokens)
        if finished:
            r.finished, r.finish_reason = True, reason
        if r.on_tokens is not None and (new or finished):
            r.on_tokens(r, new, finished)

    def _fail(self, r, e, done):
        r.error = e
        for c in (r.children or ()):
            c.error, c.finished, c.finish_reason = e, True, "error"
        self._emit(r, True, "error")
        done.append(r)

    def _place(self, r, s, st=None):
        """the admission of r into slot s is complete: it runs from now on (n > 1: its children, in s and the forked slots)"""
        if r.n > 1:
            for c, sl in zip(r.children, [s] + list(st["fork"])):
                c.prompt_tokens = r.prompt_tokens
                self.slots[sl], self.produced[sl] = c, 1
        else:
            self.slots[s], self.produced[s] = r, 1

    def _admit_parent(self, r, free, done):
        """Admission of a request with n > 1 (the head of the queue; n slots are free): ONE preparation and ONE prefill into the slot
        child 0 takes, the other n - 1 slots are forked from it (model.admit_fork / admit_step).  -> "ok", "failed" (the request was
        answered with an error) or "wait" (the block pool cannot hold it yet, or its prompt is now being prefilled in chunks)."""
        m = self.model
        if getattr(r, "_enc", None) is None:
            try:
                r._enc = self._encode(r)
                r.prompt_tokens = len(r._enc[0])
            except Exception as e:
                self.waiting.remove(r)
                self._fail(r, e, done)
                return "failed"
        ids, ser, lens = r._enc
        if getattr(m, "_kv_dynamic", False):
            T = m.request_tokens(ids, ser, lens)
            need = [T + r.max_tokens] + [m.fork_tokens(T, r.max_tokens)] * (r.n - 1)      # shared prompt blocks counted once
            if not m.kv_fits(need):
                if any(v is not None for v in self.slots):
                    return "wait"
                self.waiting.remove(r)
                self._fail(r, RuntimeError(f"request needs {sum(need)} KV positions for its {r.n} samples, more than the block pool "
                                           f"can hold ({m.kv_stats()})"), done)
                return "failed"
        s = m.pick_slot(list(free), m._request_idents(ids, ser, lens)) if hasattr(m, "pick_slot") else free[0]
        kids = [f for f in free if f != s][:r.n - 1]
        self.waiting.remove(r)
        for c, sl in zip(r.children, [s] + kids):        # every sibling's own settings, before its first token is drawn
            m.set_slot_sampling(sl, *c.sampling)
            if hasattr(m, "set_slot_controls"):
                m.set_slot_controls(sl, *c.controls)
        try:
            st = m.admit_fork(m.admit_begin(s, ids, ser, lens, r.max_tokens), kids, r.max_tokens)
            if (self.prefill_chunk_tokens and any(v is not None for v in self.slots)
                    and st["T"] - st["done"] > self.prefill_chunk_tokens):
                self.prefilling = (r, s, st)             # others are decoding: the one prefill goes in chunks between their steps
                m.admit_step(st, self.prefill_chunk_tokens)
                return "wait"
            m.admit_step(st)
        except Exception as e:
            self.prefilling = None
            if type(e).__name__ == "KvPoolExhausted" and any(v is not None for v in self.slots):
                self.waiting.appendleft(r)
                return "wait"
            self._fail(r, e, done)
            return "failed"
        self._place(r, s, st)
        self._since_sync = self.sync_every               # read the first tokens right away
        return "ok"

    # ---- one scheduler iteration ---------------------------------------------------------------------
    def step(self):
        """Admit what fits, advance every running sequence by one token, deliver finished / newly read tokens.
        Returns the requests that finished in this call."""
        m = self.model
        done = []
        # (a prompt that is being prefilled in chunks draws its first token with the CURRENT configuration: it counts as running)
        running = any(s is not None for s in self.slots) or self.prefilling is not None
        if self.mixed:
            self._mixed_mode()
        self._logprobs_mode()
        self._controls_mode()
        while not self.mixed and not running and self.waiting and self.waiting[0].sampling_key != self.active_key:
            try:
                self._apply_sampling(self.waiting[0].sampling_key)
            except Exception as e:                       # a configuration the library refuses fails THAT request, not the engine
                r = self.waiting.popleft()
                r.error = e
                self._emit(r, True, "error")
                done.append(r)
        if self.prefilling is not None:                  # a long prompt is on its way in: its next chunk, no other admission meanwhile
            r, s, st = self.prefilling
            try:
                if m.admit_step(st, self.prefill_chunk_tokens):
                    self.prefilling = None
                    self._place(r, s, st)
                    self._since_sync = self.sync_every   # read the first token right away
            except Exception as e:
                self.prefilling = None
                self._fail(r, e, done)
        # admission: free slots take waiting requests that share the running batch's sampling configuration
        while self.prefilling is None and self.waiting and any(v is None for v in self.slots):
            free = [i for i, v in enumerate(self.slots) if v is None]
            # requests that share the running batch's sampling configuration may overtake a head of the queue that waits for ANOTHER
            # one (it joins when the batch has drained) - but only `max_bypass` times, or a steady stream of same-key arrivals
            # would starve it
            head = self.waiting[0]
            if head.n > 1:                               # n samples of one prompt: admitted together, from one prefill
                if head.n <= len(free):
                    if self._admit_parent(head, free, done) == "wait":
                        break
                    continue
                if head.bypassed >= self.max_bypass:     # it waits for n free slots; later single requests may pass it, a few times
                    break
            if self.mixed:
                cands = []
                for q in self.waiting:                   # arrival order; a later request with n > 1 ends the run (it goes first then)
                    if q.n > 1:
                        if q is head:
                            continue
                        break
                    cands.append(q)
                cands = cands[:len(free)]
                if not cands:
                    break
                if head.n > 1:
                    head.bypassed += len(cands)
            else:
                if head.sampling_key != self.active_key and head.bypassed >= self.max_bypass:
                    break
                cands = [q for q in self.waiting if q.sampling_key == self.active_key][:len(free)]
                if not cands:
                    break
                if head.sampling_key != self.active_key:
                    head.bypassed += len(cands)
            ready = []
            for r in cands:                              # tokenise / sp-encode once per request
                if getattr(r, "_enc", None) is None:
                    try:
                        r._enc = self._encode(r)
                        r.prompt_tokens = len(r._enc[0])
                    except Exception as e:               # a bad request must not take the engine down
                        self.waiting.remove(r)
                        r.error = e
                        self._emit(r, True, "error")
                        done.append(r)
                        continue
                ready.append(r)
            if not ready:
                continue
            pack = m.plan_pack([r._enc + (r.max_tokens,) for r in ready], free) if self.nslots > 1 else []
            group = [ready[j] for j in pack] if pack else ready[:1]
            if getattr(m, "_kv_dynamic", False):         # block-paged cache with an oversubscribed pool: admit only what it can hold
                def need(q):
                    return m.request_tokens(*q._enc) + q.max_tokens
                if len(group) > 1 and not m.kv_fits([need(q) for q in group]):
                    group = group[:1]
                if not m.kv_fits([need(group[0])]):
                    if any(v is not None for v in self.slots):
                        break                            # wait until a running sequence finishes: its blocks become evictable
                    r = group[0]                         # nothing is running: this request can never fit
                    self.waiting.remove(r)
                    r.error = RuntimeError(f"request needs {need(r)} KV positions, more than the block pool can hold ({m.kv_stats()})")
                    self._emit(r, True, "error")
                    done.append(r)
                    continue
            items = []
            for r in group:
                ids, ser, lens = r._enc
                s = m.pick_slot(free, m._request_idents(ids, ser, lens))      # the slot whose resident prefix matches best
                free.remove(s)
                items.append((s, ids, ser, lens, r.max_tokens))
                self.waiting.remove(r)
                if self.mixed:                           # the slot's settings, before its first token is drawn
                    m.set_slot_sampling(s, *r.sampling)
                    if hasattr(m, "set_slot_controls"):
                        m.set_slot_controls(s, *r.controls)
            try:
                if len(items) > 1:
                    m._admit_packed(items)               # several short prompts: one packed prefill pass
                elif self.nslots == 1:
                    m._prefill_request(*items[0][1:])
                elif self.prefill_chunk_tokens and any(v is not None for v in self.slots):
                    st = m.admit_begin(*items[0])         # others are decoding: feed a long prompt in chunks between their steps
                    if st["T"] - st["done"] > self.prefill_chunk_tokens:
                        self.prefilling = (group[0], items[0][0], st)
                        m.admit_step(st, self.prefill_chunk_tokens)
                        break
                    m.admit_step(st)
                else:
                    m._admit(*items[0])
            except Exception as e:
                self.prefilling = None
                if type(e).__name__ == "KvPoolExhausted" and any(v is not None for v in self.slots):
                    self.waiting.extendleft(reversed(group))      # the block pool is full (resident-prefix claims of the touched slots were dropped): back to the head
                    break                                         # of the queue until a running sequence finishes
                for r in group:
                    r.error = e
                    self._emit(r, True, "error")
                    done.append(r)
                continue
            for r, it in zip(group, items):
                self.slots[it[0]], self.produced[it[0]] = r, 1
            self._since_sync = self.sync_every          # read the first token right away (time to first token)
        live = [s for s in range(self.nslots) if self.slots[s] is not None]
        if not live:
            return done
        if self._since_sync >= self.sync_every or any(self.produced[s] >= self.slots[s].max_tokens for s in live):
            done += self._harvest()
            live = [s for s in range(self.nslots) if self.slots[s] is not None]
            if not live:
                return done
        if self.nslots == 1:
            m.decode_step()
        else:
            m.batched_step()
        for s in live:
            if self.produced[s] < self.slots[s].max_tokens:
                self.produced[s] += 1
        self._since_sync += 1
        return done

    def _harvest(self):
        """One device->host read of every slot's tokens; deliver the new ones; retire finished sequences."""
        m, B = self.model, self.model.buf
        done = []
        self._since_sync = 0
        toks_all = B["out_tokens_all"].cpu() if self.nslots > 1 else B["out_tokens"][None].cpu()
        tp = getattr(m, "_tp", None)
        if tp is not None and tp.status():
            # a peer's contribution did not arrive (csrc/tp.hip sets a sticky bit and every later collective sums garbage): the
            # tokens read above are worthless - fail what is running instead of serving them, and reset the exchange
            err = RuntimeError("tensor-parallel exchange timed out (a peer rank did not reach a collective): tokens discarded")
            for s in range(self.nslots):
                r = self.slots[s]
                if r is None:
                    continue
                self.slots[s] = None
                if self.nslots > 1:
                    B["pos_all"][s] = -1
                m._slot_idents[s] = []
                r.error = err
                self._emit(r, True, "error")
                done.append(r)
            # Each rank reads only ITS OWN sticky status: a peer that arrived late saw no timeout and would keep decoding these
            # slots while this rank hands them to other requests - slot choice and packing would differ between the ranks and every
            # later collective would be mismatched.  So this is fatal for the rank group, not for the running requests only: raise
            # out of step() (EngineThread._run fails everything, publishes stop to the followers; a follower's loop ends with the
            # exception) and let the supervisor restart all ranks.
            raise ExchangeBroken(str(err))
        for s in range(self.nslots):
            r = self.slots[s]
            if r is None:
                continue
            toks = toks_all[s, :self.produced[s]].tolist()
            cut = next((i + 1 for i, t in enumerate(toks) if t in r.eos), None) if r.eos else None
            if r.t_first is None:
                r.t_first = time.perf_counter()
                if r.parent is not None and r.parent.t_first is None:
                    r.parent.t_first = r.t_first
            if r.stop and self._check_stop(s, r, toks, cut, done):
                continue
            if cut is not None:
                r.tokens = toks[:cut]
                if r.tokens[-1] in r.stop_ids:
                    r.stop_reason = r.tokens[-1]
                self._read_logprobs(s, r)
                self._retire(s, "stop", done)
            elif self.produced[s] >= r.max_tokens:
                r.tokens = toks[:r.max_tokens]
                self._read_logprobs(s, r)
                self._retire(s, "length", done)
            else:
                r.tokens = toks
                self._read_logprobs(s, r)
                self._emit(r, False)
        return done

    def _check_stop(self, s, r, toks, cut, done):
        """Stop strings of the sequence in slot s over the tokens this harvest read, in generation order: only the tokens before an
        EOS / stop token or the max_tokens limit can match (a sequence ends at the smallest j).  -> True when the sequence was retired
        here (a stop string matched: the tokens generated past the match are dropped); otherwise r.text is what a stream may show."""
        from .detok import StopChecker
        if r.checker is None:
            r.checker = StopChecker(self.processor.tokenizer, r.stop, r.include_stop)
        limit = min(len(toks), r.max_tokens) if cut is None else cut
        seen = len(r.checker.ids)
        hit = r.checker.push(toks[seen:limit])
        if hit is not None and not (cut is not None and hit[0] == cut):      # (at the same j the EOS / stop token ends it)
            r.tokens, r.text, r.stop_reason = toks[:hit[0]], hit[1], hit[2]
            self._read_logprobs(s, r)
            self._retire(s, "stop", done)
            return True
        if cut is not None or self.produced[s] >= r.max_tokens:
            r.text = r.checker.finish(toks[:limit])
        else:
            r.text = r.checker.released
        return False

    def _read_logprobs(self, s, r):
        """the entries of the tokens read in this harvest (requests that asked only)"""
        if r.logprob_k is None or len(r.logprobs) >= len(r.tokens):
            return
        new = self.model.read_logprobs(s, len(r.logprobs), len(r.tokens), r.logprob_k)
        r.logprobs.extend(new)
        r.cumulative_logprob = float(sum(e[0] for e in r.logprobs))

    def _retire(self, s, reason, done):
        r = self.slots[s]
        self.slots[s] = None
        if self.nslots > 1:
            self.model.buf["pos_all"][s] = -1         # parked: the batched step neither attends nor writes this slot's cache
        self.model.note_generated(s, r.tokens)
        self._emit(r, True, reason)
        p = r.parent
        if p is None:
            done.append(r)
            return
        p.remaining -= 1                              # a sibling: its slot is free now; the parent completes with the last one
        if p.remaining == 0:
            p.finished, p.finish_reason = True, reason
            done.append(p)

    def run_until_done(self):
        out = []
        while self.has_work():
            out += self.step()
        return out


class ControlPlane:
    """Tensor-parallel serving: rank 0 owns the HTTP front end, the other ranks follow.  Every rank's Engine must see the SAME
    sequence of add_request() / step() calls (slot choice, packing and harvest points are deterministic functions of it, and the
    decode steps rendezvous inside the exchange kernels), so before every engine iteration the leader publishes what it is about
    to do - the requests it admits now (usually none) or a shutdown - over a CPU (gloo) group: followers block there without
    spinning a GPU.  One small broadcast per iteration (a count), a pickled list only when there is something to say."""

    def __init__(self, rank, world, group=None, dist=None):
        self.rank, self.world, self.group = rank, world, group
        if dist is None:
            import torch.distributed as dist
        self.dist = dist

    @classmethod
    def create(cls):
        """collective: a gloo group over all ranks of the default process group"""
        import torch.distributed as dist
        group = dist.new_group(backend="gloo")
        return cls(dist.get_rank(), dist.get_world_size(), group, dist)

    def publish(self, new_requests, stop=False):
        """leader: new_requests = list of add_request kwargs (picklable: no callbacks)"""
        import torch
        head = torch.tensor([-1 if stop else len(new_requests)], dtype=torch.int64)
        self.dist.broadcast(head, src=0, group=self.group)
        if new_requests and not stop:
            self.dist.broadcast_object_list([new_requests], src=0, group=self.group)

    def receive(self):
        """follower: -> (list of add_request kwargs, stop)"""
        import torch
        head = torch.zeros(1, dtype=torch.int64)
        self.dist.broadcast(head, src=0, group=self.group)
        n = int(head.item())
        if n < 0:
            return [], True
        if n == 0:
            return [], False
        box = [None]
        self.dist.broadcast_object_list(box, src=0, group=self.group)
        return box[0], False


def follow(engine, control):
    """The loop of a non-zero TP rank: replay the leader's admissions and step whenever it steps."""
    while True:
        new, stop = control.receive()
        if stop:
            return
        for kw in new:
            engine.add_request(**kw)
        if engine.has_work():
            engine.step()


class EngineThread:
    """Owns an Engine on one thread; other threads (the HTTP server's event loop) submit requests through a queue and get
    their tokens through the per-request callback.  With a ControlPlane (tensor parallel) this is the LEADER: every iteration is
    announced to the follower ranks first."""

    def __init__(self, engine, device=None, control=None):
        self.engine, self.device, self.control = engine, device, control
        self.inbox = queue.Queue()
        self.error = None
        self._stop = threading.Event()
        self.thread = threading.Thread(target=self._run, name="chatts-engine", daemon=True)
        self.thread.start()

    def submit(self, **kw):
        """Queue a request for the engine thread (kw: Engine.add_request arguments + `holder`, a list that receives the Request)."""
        if self.error is not None or not self.thread.is_alive():
            raise RuntimeError(f"engine thread is not running: {self.error}")
        self.inbox.put(kw)

    def _run(self):
        try:
            self._loop()
        except BaseException as e:           # the engine must never die silently: every waiting / later request is failed
            self.error = e
            import traceback
            traceback.print_exc()
            self._fail_all(e)
            if self.control is not None:     # the follower ranks block in control.receive(): release them
                try:
                    self.control.publish([], stop=True)
                except Exception:
                    pass

    def _fail_all(self, e):
        eng = self.engine
        pending = list(eng.waiting) + [r for r in eng.slots if r is not None]
        if getattr(eng, "prefilling", None) is not None:
            pending.append(eng.prefilling[0])
            eng.prefilling = None
        eng.waiting.clear()
        eng.slots = [None] * eng.nslots
        while True:
            try:
                kw = self.inbox.get_nowait()
            except queue.Empty:
                break
            holder = kw.pop("holder", None)
            r = eng.add_request(**kw)
            eng.waiting.clear()
            pending.append(r)
            if holder is not None:
                holder.append(r)
        for r in pending:
            r.error = RuntimeError(f"engine thread died: {type(e).__name__}: {e}")
            if r.on_tokens is not None:
                r.finished = True
                r.on_tokens(r, [], True)

    def _reject_invalid(self, new):
        """validate_sampling on every queued request; the offending ones are answered with an error here and never reach the engine
        (nor, under tensor parallelism, the followers - add_request raising after control.publish would take every rank down)."""
        ok = []
        for kw in new:
            try:
                validate_sampling(**{k: kw[k] for k in ("max_tokens", "temperature", "top_p", "top_k", "logprobs", "repetition_penalty",
                                                          "frequency_penalty", "presence_penalty", "min_p", "n", "best_of", "stop")
                                     if k in kw}, max_logprobs=getattr(self.engine, "max_logprobs", 20))
                if hasattr(self.engine, "check_request"):       # n > slots, n > 1 / stop on an engine that cannot serve them
                    self.engine.check_request(kw.get("n"), kw.get("best_of"), kw.get("stop"))
                ok.append(kw)
            except (ValueError, TypeError) as e:
                r = Request(-1, kw.get("prompt"), list(kw.get("timeseries") or []), 1, None, [], kw.get("on_tokens"))
                r.error, r.finished, r.finish_reason = e, True, "error"
                holder = kw.get("holder")
                if holder is not None:
                    holder.append(r)
                if r.on_tokens is not None:
                    r.on_tokens(r, [], True)
        return ok

    def _loop(self):
        import torch
        idx = getattr(self.device, "index", self.device) if self.device is not None else None
        if isinstance(idx, int):
            torch.cuda.set_device(idx)
        while not self._stop.is_set():
            new = []
            try:
                block = not self.engine.has_work()
                while True:
                    kw = self.inbox.get(timeout=0.05) if block else self.inbox.get_nowait()
                    new.append(kw)
                    block = False
            except queue.Empty:
                pass
            new = self._reject_invalid(new)        # BEFORE anything is announced: a bad value fails that request only, on no rank
            if self.control is not None:
                if not new and not self.engine.has_work():
                    continue                       # idle: nothing to announce, the followers keep waiting
                self.control.publish([{k: v for k, v in kw.items() if k not in ("holder", "on_tokens")} for kw in new])
            for kw in new:
                holder = kw.pop("holder", None)
                r = self.engine.add_request(**kw)
                if holder is not None:
                    holder.append(r)
            if self.engine.has_work():
                self.engine.step()
        if self.control is not None:
            self.control.publish([], stop=True)

    def close(self):
        self._stop.set()
        self.thread.join(timeout=5)
