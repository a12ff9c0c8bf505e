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

from .sampling import (END_IDS_MAX, NO_CONTROLS, NO_MASKS, REQUEST_FIELDS, request_settings, validate_controls, validate_n,  # noqa: F401  (re-exported)
                       validate_sampling)


class ExchangeBroken(RuntimeError):
    """The tensor-parallel exchange timed out on THIS rank.  Fatal for the whole rank group: the ranks can no longer be assumed to hold
    the same engine state (a peer that arrived late saw no timeout and kept decoding), so the engine stops instead of serving
    on - EngineThread fails every request, releases the followers, and a supervisor restarts all ranks."""


_DEFAULT_SETTINGS = {**request_settings(max_tokens=1), "seed": 0}


class Request:
    """One request and its settings (sampling.request_settings: Engine.check made them).  `mixed`: the model keeps per-slot sampling
    settings, so requests do not form sampling groups - `sampling_key` then only says whether this one samples."""

    def __init__(self, rid, prompt, timeseries, on_tokens=None, model_eos=(), mixed=False, **settings):
        s = self.settings = {**_DEFAULT_SETTINGS, **settings}
        self.rid, self.prompt, self.timeseries, self.on_tokens, self.max_tokens = rid, prompt, timeseries, on_tokens, s["max_tokens"]
        self._model_eos, self._mixed = model_eos, mixed
        self.eos = set(() if s["ignore_eos"] else model_eos) | set(s["stop_token_ids"])
        self.stop_ids = {int(t) for t in s["stop_token_ids"]}
        key = (s["temperature"], s["top_k"], s["top_p"], s["seed"]) if s["temperature"] else None
        self.sampling = (0.0, 0, 1.0, 0) if key is None else key       # (temperature, top_k, top_p, seed): the slot's settings
        self.sampling_key = key if not mixed else "rows" if key else None
        self.controls = s["controls"]        # (repetition_penalty, frequency_penalty, presence_penalty, min_p)
        self.masks = tuple(s["masks"])       # (logit_bias {id: bias} or None, allowed_token_ids or None, min_tokens)
        self.tokens, self.sent, self.finished, self.finish_reason = [], 0, False, None
        self.prompt_tokens = 0
        # logprobs=k: one (logprob, rank, [(id, logprob)] * k) entry per token of `tokens`, grown with it; None when not asked
        self.logprob_k = s["logprobs"]
        self.logprobs, self.cumulative_logprob = (None, None) if self.logprob_k is None else ([], 0.0)
        self.t_arrival, self.t_first = time.perf_counter(), None
        self.error = None
        self.bypassed = 0                    # later arrivals admitted past this request while it waited for its sampling group
        # stop strings: `text` is then the engine's own decode (what a stream may show so far; the final text once finished)
        self.stop, self.include_stop, self.checker, self.text = s["stop"], s["include_stop"], None, None
        self.stop_reason = None              # the matched stop string, the id of a stop_token_ids hit, None for EOS / length
        # n > 1 (parallel sampling): the request the caller holds is the PARENT - it never occupies a slot; `children` are the n
        # sequences (index 0 .. n-1, each with the fields of a request of its own), `remaining` those still running
        self.n, self.index, self.parent, self.children, self.remaining = s["n"], 0, None, None, 0
        if self.n > 1:
            self.remaining, self.children = self.n, [self.child(i) for i in range(self.n)]

    def child(self, i):
        """sibling i of a request with n > 1: every setting of the parent, its own seed (+ i mod 2^32), the parent's arrival time"""
        c = Request(self.rid, self.prompt, self.timeseries, self.on_tokens, self._model_eos, self._mixed,
                    **{**self.settings, "n": 1, "seed": (self.settings["seed"] + i) & 0xFFFFFFFF})
        c.sampling = self.sampling[:3] + (c.settings["seed"],)         # (a greedy row keeps its seed too)
        c.index, c.parent, c.t_arrival = i, self, self.t_arrival
        return c

    @property
    def outputs(self):
        """the n sequences of this request in index order (the request itself when n == 1)"""
        return list(self.children) if self.children else [self]


class Engine:
    """add_request() / step() like vLLM's LLMEngine.  `on_tokens(request, new_token_ids, finished)` is called from step()."""

    def __init__(self, model, processor, sync_every=4, prefill_chunk_tokens=None, greedy_return_steps=256):
        self.model, self.processor = model, processor
        # the modes of the decode step (per-row sampling, logprobs, logit controls): scheduler iterations without any request that needs
        # one (running or waiting) after which it is switched off again (a graph re-capture); 0 = stay in a mode once entered.  Every rank
        # of a tensor-parallel group counts the same iterations (followers replay the leader's), so all of them switch together.
        self.greedy_return_steps = max(0, int(greedy_return_steps))
        self._idle = {}                                 # mode -> consecutive iterations nobody needed it (_mode)
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
    def check(self, **settings):
        """The one check of a request's settings (sampling.REQUEST_FIELDS): their value ranges, and what THIS engine cannot serve - n >
        max_num_seqs, n > 1 on a model without per-slot sampling settings or without a fork, stop strings without a tokenizer, logit
        controls, logit masks or logprobs on a model without them, ids of logit_bias / allowed_token_ids outside the model's vocabulary,
        more than 64 ids for min_tokens to keep away.  ValueError, or -> the normalised settings (sampling.request_settings).
        add_request calls it; EngineThread calls it BEFORE a request is announced to the follower ranks."""
        s = request_settings(**settings, max_logprobs=self.max_logprobs, max_num_seqs=self.nslots, vocab_size=self.vocab_size)
        if s["n"] > 1 and not self.mixed:
            raise ValueError("n > 1 needs a model with per-slot sampling settings (set_slot_sampling)")
        if s["n"] > 1 and not hasattr(self.model, "admit_fork"):
            raise ValueError("this model cannot fork a prompt into several samples (n > 1)")
        if s["stop"] and getattr(self.processor, "tokenizer", None) is None:
            raise ValueError("stop strings need a tokenizer (the engine's processor has none)")
        if s["controls"] != NO_CONTROLS and not hasattr(self.model, "set_slot_controls"):
            raise ValueError("this model does not apply repetition / frequency / presence penalties or min_p")
        if tuple(s["masks"]) != NO_MASKS:
            if not hasattr(self.model, "set_slot_masks"):
                raise ValueError("this model does not apply logit_bias, allowed_token_ids or min_tokens")
            ends = {t for t in set(() if s["ignore_eos"] else self._model_eos()) | set(s["stop_token_ids"]) if t is not None}
            V = self.vocab_size                      # (request_settings refused stop_token_ids outside it when min_tokens > 0)
            ends = {t for t in ends if V is None or 0 <= t < V}       # (an EOS id the logits do not cover can never be chosen)
            if s["masks"][2] and len(ends) > END_IDS_MAX:
                raise ValueError(f"min_tokens: {len(ends)} ids would end the sequence (stop_token_ids and the EOS ids), at most "
                                 f"{END_IDS_MAX} are accepted")
        if s["logprobs"] is not None and not hasattr(self.model, "set_logprobs"):
            raise ValueError("this model does not compute logprobs")
        return s

    def add_request(self, prompt, timeseries=None, on_tokens=None, **settings):
        """settings: sampling.REQUEST_FIELDS (max_tokens=64, temperature=0.0, top_p=1.0, top_k=0, seed=None, stop_token_ids, ignore_eos,
        logprobs, the four logit controls, n=1, best_of, stop, include_stop_str_in_output), checked by check().
        seed None: per-slot mode gives every request its own stream (a hash of its arrival number - vLLM's seed=None means "not
        reproducible across requests"; here two identical prompts still differ, and a rerun of the same arrival order repeats);
        grouped mode uses 0 (requests that decode together must share ONE configuration there).
        n > 1: -> the parent request; its `children` are n sequences of the one prompt, child i drawing with seed + i (mod 2^32), all
        admitted together from ONE prefill (step()).  on_tokens is called per child (`r.index`, `r.parent`).
        stop: strings that end a sequence when they appear in its decoded text (chatts_amd/detok.py: the rule)."""
        s = self.check(**settings)
        if s["seed"] is None:
            s["seed"] = ((self._rid + 1) * 2654435761) & 0xFFFFFFFF if self.mixed else 0
        self._rid += 1
        r = Request(self._rid, prompt, list(timeseries or []), on_tokens, self._model_eos(), self.mixed, **s)
        self.waiting.append(r)
        return r

    def _model_eos(self):
        e = self.model.config.eos_token_id
        return list(e) if isinstance(e, (list, tuple)) else [e]

    @property
    def vocab_size(self):
        """the ids the model's logits cover (None for a stand-in model without a shard plan: the ids are then checked as int32 only)"""
        plan = getattr(self.model, "plan", None)
        return None if plan is None else int(plan.vocab) * int(plan.world)

    @property
    def max_logprobs(self):
        return int(getattr(self.model, "max_logprobs", 20))

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

    def _requests_in_flight(self):
        """every request that will still draw a token: running, being prefilled, waiting"""
        yield from (r for r in self.slots if r is not None)
        if self.prefilling is not None:
            yield self.prefilling[0]
        yield from self.waiting

    def _mode(self, name, wanted, on, switch):
        """One mode of the decode step (per-row sampling, logprobs, logit controls): on while any request in flight wants it
        (`wanted(request)`), off again when nobody has for a while.  `on`: the model's current state; `switch(bool)` changes it.
        The per-row sampler draws greedy rows too and every slot's settings are current at all times, so a switch is safe whenever.
        Hysteresis instead of either extreme.  Every switch drops both captured hipGraphs (re-capture + a warm eager step on all
        ranks), so alternating traffic must not flip the mode per request; but staying in per-row mode for good would leave later
        greedy traffic on the sampler path (under TP: a full-vocabulary all-gather + the sampler kernel per step instead of the
        2-word tp_argmax).  So: back to the plain step after `greedy_return_steps` consecutive iterations without any request that
        wants the mode running or waiting (0 = never switch back).  Followers replay the leader's requests and count the same
        iterations: all ranks switch together."""
        if any(wanted(r) for r in self._requests_in_flight()):
            self._idle[name] = 0
            if not on:
                switch(True)
        elif on:
            self._idle[name] = self._idle.get(name, 0) + 1
            if self.greedy_return_steps and self._idle[name] >= self.greedy_return_steps:
                switch(False)

    def _emit(self, r, finished, reason=None):
        new = r.tokens[r.sent:]
        r.sent = len(r.tokens)
        if finished:
            r.finished, r.finish_reason = True, reason
        if r.on_tokens is not None and (new or finished):
            r.on_tokens(r, new, finished)

    def _fail(self, r, e, done):
        """the one way a request ends with an error (a bad request must not take the engine down); n > 1: its samples with it"""
        r.error = e
        for c in (r.children or ()):
            c.error, c.finished, c.finish_reason = e, True, "error"
        self._emit(r, True, "error")
        done.append(r)

    def _running(self):
        return any(v is not None for v in self.slots)

    # ---- admission --------------------------------------------------------------------------------
    def _candidates(self, free):
        """The waiting requests that may be admitted into the `free` slots now, in arrival order ([]: nobody).  A request with n > 1
        at the head goes alone, once n slots are free.  Requests that share the running batch's sampling configuration may overtake
        a head of the queue that waits for ANOTHER one (it joins when the batch has drained), and single requests a head that waits
        for n slots - but only `max_bypass` times, or a steady stream of such arrivals would starve it."""
        head = self.waiting[0]
        if head.n > 1:
            if head.n <= len(free):
                return [head]
            blocked = True
        else:
            blocked = not self.mixed and head.sampling_key != self.active_key
        if blocked and head.bypassed >= self.max_bypass:
            return []
        if self.mixed:
            cands = []
            for q in self.waiting:                       # a later request with n > 1 ends the run (it goes first then)
                if q.n > 1:
                    if q is head:
                        continue
                    break
                cands.append(q)
        else:
            cands = [q for q in self.waiting if q.sampling_key == self.active_key]
        cands = cands[:len(free)]
        if blocked:
            head.bypassed += len(cands)
        return cands

    def _encoded(self, r, done):
        """tokenise / sp-encode once per request -> True; a request that cannot be encoded is failed (and no longer waits)"""
        if getattr(r, "_enc", None) is None:
            try:
                r._enc = self._encode(r)
                r.prompt_tokens = len(r._enc[0])
            except Exception as e:
                self.waiting.remove(r)
                self._fail(r, e, done)
                return False
        return True

    def _needs(self, r):
        """KV positions of r's sequences (n > 1: the shared whole prompt blocks are counted once, with sample 0)"""
        m = self.model
        T = m.request_tokens(*r._enc)
        spec = getattr(m, "spec_reserve", None)          # a speculating request reserves k more positions (modeling._prefill_request)
        extra = spec(T, r.max_tokens) if spec is not None and self.nslots == 1 else 0
        return [T + r.max_tokens + extra] + ([m.fork_tokens(T, r.max_tokens)] * (r.n - 1) if r.n > 1 else [])

    def _pool_gate(self, needs):
        """block-paged cache with an oversubscribed pool -> "admit"; "wait" until a running sequence finishes (its blocks become
        evictable); "never" when nothing is running: the request can never fit"""
        if self.model.kv_fits(needs):
            return "admit"
        return "wait" if self._running() else "never"

    def _write_settings(self, slot, r):
        """the slot's sampling settings, logit controls and logit masks, before its first token is drawn (per-slot mode)"""
        self.model.set_slot_sampling(slot, *r.sampling)
        if hasattr(self.model, "set_slot_controls"):
            self.model.set_slot_controls(slot, *r.controls)
        if hasattr(self.model, "set_slot_masks"):        # (a tenant with none of the three resets the slot's rows)
            self.model.set_slot_masks(slot, *r.masks, end_ids=sorted(i for i in r.eos if i is not None))

    def _place(self, r, s, st=None):
        """the admission of r into slot s is complete: it runs from now on (n > 1: its children, in s and the forked slots)"""
        if r.n > 1:
            for c, sl in zip(r.children, [s] + list(st["fork"])):
                c.prompt_tokens = r.prompt_tokens
                self.slots[sl], self.produced[sl] = c, 1
        else:
            self.slots[s], self.produced[s] = r, 1

    def _start(self, group, items, kids):
        """Prefill what was picked: several short prompts in one packed pass, otherwise one request (n > 1: ONE prefill into the slot
        sample 0 takes, the slots `kids` are forked from it) - in chunks between the others' decode steps when it is long and others
        are decoding.  -> False when the prompt is now `self.prefilling`: no other admission until it is in."""
        m, r, chunk, st = self.model, group[0], self.prefill_chunk_tokens, None
        if len(items) > 1:
            m._admit_packed(items)
        elif self.nslots == 1:
            m._prefill_request(*items[0][1:])
        elif r.n > 1 or (chunk and self._running()):
            st = m.admit_begin(*items[0])
            if r.n > 1:
                st = m.admit_fork(st, kids, r.max_tokens)
            if chunk and self._running() and st["T"] - st["done"] > chunk:
                self.prefilling = (r, items[0][0], st)
                m.admit_step(st, chunk)
                return False
            m.admit_step(st)
        else:
            m._admit(*items[0])
        for q, it in zip(group, items):
            self._place(q, it[0], st)
        self._since_sync = self.sync_every               # read the first token right away (time to first token)
        return True

    def _admit_waiting(self, done):
        """free slots take waiting requests (that share the running batch's sampling configuration, on a model with one)"""
        m = self.model
        while self.prefilling is None and self.waiting and any(v is None for v in self.slots):
            free = [i for i, v in enumerate(self.slots) if v is None]
            cands = self._candidates(free)
            if not cands:
                return
            ready = [r for r in cands if self._encoded(r, done)]
            if not ready:
                continue
            pack = m.plan_pack([r._enc + (r.max_tokens,) for r in ready], free) if self.nslots > 1 and ready[0].n == 1 else []
            group = [ready[j] for j in pack] if pack else ready[:1]
            if getattr(m, "_kv_dynamic", False):         # admit only what the block pool can hold
                if len(group) > 1 and self._pool_gate([c for q in group for c in self._needs(q)]) != "admit":
                    group = group[:1]
                r = group[0]
                needs = self._needs(r)
                verdict = self._pool_gate(needs)
                if verdict == "wait":
                    return
                if verdict == "never":
                    self.waiting.remove(r)
                    # (a single request's count is asked for again, as it always was: the model sees the same calls)
                    self._fail(r, RuntimeError(f"request needs {sum(needs)} KV positions for its {r.n} samples, more than the block pool "
                                               f"can hold ({m.kv_stats()})" if r.n > 1 else
                                               f"request needs {sum(self._needs(r))} KV positions, more than the block pool can hold "
                                               f"({m.kv_stats()})"), done)
                    continue
            items, kids, admitted = [], [], []
            for r in group:
                ids, ser, lens = r._enc
                s = m.pick_slot(free, m._request_idents(ids, ser, lens))      # the slot whose resident prefix matches best
                free.remove(s)
                kids = free[:r.n - 1]
                self.waiting.remove(r)
                if self.mixed:                           # every sequence's own settings
                    try:
                        for c, sl in zip(r.outputs, [s] + kids):
                            self._write_settings(sl, c)
                    except Exception as e:               # settings the model refuses fail THAT request: its slot is free again
                        free.append(s)
                        free.sort()
                        kids = []
                        self._fail(r, e, done)
                        continue
                items.append((s, ids, ser, lens, r.max_tokens))
                admitted.append(r)
            group = admitted
            if not group:
                continue
            try:
                if not self._start(group, items, kids):
                    return
            except Exception as e:
                self.prefilling = None
                if type(e).__name__ == "KvPoolExhausted" and self._running():
                    # the block pool is full (resident-prefix claims of the touched slots were dropped): back to the head of the
                    # queue, in order, until a running sequence finishes
                    self.waiting.extendleft(reversed(group))
                    return
                for r in group:
                    self._fail(r, e, done)

    # ---- one scheduler iteration ---------------------------------------------------------------------
    def step(self):
        """Admit what fits, advance every running sequence by one token, deliver finished / newly read tokens.
        Returns the requests that finished in this call."""
        m = self.model
        done = []
        # (a prompt that is being prefilled in chunks draws its first token with the CURRENT configuration: it counts as running)
        running = self._running() or self.prefilling is not None
        if self.mixed:
            self._mode("rows", lambda r: r.sampling_key, self.active_key == "rows", lambda on: self._apply_sampling("rows" if on else None))
        if hasattr(m, "set_logprobs"):
            self._mode("logprobs", lambda r: r.logprob_k is not None, bool(getattr(m, "_logprobs_on", False)), m.set_logprobs)
        if hasattr(m, "set_logit_controls"):
            self._mode("controls", lambda r: r.controls != NO_CONTROLS, bool(getattr(m, "_controls_on", False)), m.set_logit_controls)
        if hasattr(m, "set_logit_masks"):
            self._mode("masks", lambda r: r.masks != NO_MASKS, bool(getattr(m, "_masks_on", False)), m.set_logit_masks)
        while not self.mixed and not running and self.waiting and self.waiting[0].sampling_key != self.active_key:
            try:
                self._apply_sampling(self.waiting[0].sampling_key)
            except Exception as e:                       # a configuration the library refuses fails THAT request, not the engine
                self._fail(self.waiting.popleft(), e, done)
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
        self._admit_waiting(done)
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
            if getattr(m, "_spec_request", False):
                # upper bound of the tokens on the device (a speculative step emits at most k + 1): once the request MAY be complete,
                # read the device before the next step - a step after the last token would be a pass over the weights for nothing
                self._spec_most = max(getattr(self, "_spec_most", 0), self.produced[0]) + m._spec_now["k"] + 1
                if self._spec_most >= self.slots[0].max_tokens:
                    self._since_sync = self.sync_every
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
        if self.nslots == 1 and self.slots[0] is not None and getattr(m, "_spec_request", False):
            # speculative steps emit 1 .. k + 1 tokens: the count kept here (one per step) is a lower bound, the device's counter rules
            self.produced[0] = m._spec_produced(self.produced[0], self.slots[0].max_tokens)
            self._spec_most = self.produced[0]
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
                self._fail(r, err, done)
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
            r.checker = StopChecker(self.processor.tokenizer, r.stop, r.include_stop, r.masks[2])
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
        """Engine.check on every queued request; the offending ones are answered with an error here and never reach the engine
        (nor, under tensor parallelism, the followers - add_request raising after control.publish would take every rank down)."""
        ok = []
        check = getattr(self.engine, "check", validate_sampling)        # (a stand-in engine without check(): the value ranges)
        for kw in new:
            try:
                check(**{k: kw[k] for k in REQUEST_FIELDS if k in kw})
                ok.append(kw)
            except (ValueError, TypeError) as e:
                r = Request(-1, kw.get("prompt"), list(kw.get("timeseries") or []), kw.get("on_tokens"))
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
                self.control.publish([{k: kw[k] for k in ("prompt", "timeseries") + REQUEST_FIELDS if k in kw} for kw in new])
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
