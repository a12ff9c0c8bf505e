"""vLLM-style offline surface: ``LLM(...).generate([{"prompt", "multi_modal_data": {"timeseries": [...]}}], SamplingParams)``.

Mirrors how the reference drives vLLM (NetManAIOps/ChatTS demo/demo_vllm.py:30-63, chatts/utils/llm_utils.py:154-182):
same constructor keywords, same dict input schema, results expose ``.outputs[0].text``.  vLLM itself is not a
dependency; requests are served one after another on the HIP engine (continuous batching: SURVEY.md section 8f).
"""
import os

import numpy as np


from .sampling import REQUEST_FIELDS, SamplingParams, validate_n  # noqa: F401  (SamplingParams: importable from here as before)


class Logprob:
    """vLLM's Logprob: log-probability of a token under the raw logits of its step, its 1-based rank, its text"""

    def __init__(self, logprob, rank=None, decoded_token=None):
        self.logprob, self.rank, self.decoded_token = logprob, rank, decoded_token

    def __repr__(self):
        return f"Logprob(logprob={self.logprob}, rank={self.rank}, decoded_token={self.decoded_token!r})"


class CompletionOutput:
    def __init__(self, text, token_ids, logprobs=None, cumulative_logprob=None, index=0, finish_reason=None, stop_reason=None):
        self.text, self.token_ids, self.index = text, token_ids, index
        # finish_reason: "stop" (EOS, a stop token, a stop string) / "length"; stop_reason: the matched stop string, the id of a
        # stop_token_ids hit, None otherwise (vLLM's convention)
        self.finish_reason, self.stop_reason = finish_reason, stop_reason
        # logprobs: one {token_id: Logprob} per generated token (its top-k + the chosen token); None when not requested
        self.logprobs, self.cumulative_logprob = logprobs, cumulative_logprob


def _logprob_dicts(tokenizer, token_ids, entries):
    out = []
    for tid, (lp, rank, top) in zip(token_ids, entries):
        d = {}
        for r, (i, v) in enumerate(top):
            d[int(i)] = Logprob(v, r + 1, tokenizer.decode([int(i)], skip_special_tokens=False))
        if int(tid) not in d:
            d[int(tid)] = Logprob(lp, rank, tokenizer.decode([int(tid)], skip_special_tokens=False))
        else:
            d[int(tid)] = Logprob(lp, rank, d[int(tid)].decoded_token)
        out.append(d)
    return out


class RequestOutput:
    def __init__(self, prompt, prompt_token_ids, outputs):
        self.prompt, self.prompt_token_ids, self.outputs = prompt, prompt_token_ids, outputs


def _load_checkpoint_tokenizer(path):
    """The HF tokenizer stored in a checkpoint directory (demo/demo_vllm.py builds prompts with it).  A directory written
    by ChatTSConfig.save_pretrained for the synthetic-weight tests marks itself with `synthetic_tokenizer` in config.json."""
    import json
    with open(os.path.join(path, "config.json")) as f:
        if json.load(f).get("synthetic_tokenizer"):
            return None
    has_files = any(os.path.exists(os.path.join(path, f)) for f in ("tokenizer.json", "vocab.json", "tokenizer.model"))
    if not has_files:
        raise ValueError(f"{path} holds no tokenizer files (tokenizer.json / vocab.json): pass tokenizer=... explicitly; "
                         "the synthetic stand-in tokenizer would feed meaningless ids to real weights")
    from transformers import AutoTokenizer
    return AutoTokenizer.from_pretrained(path, trust_remote_code=False)


def _build_llm(model, kw):
    """factory of chatts_amd.tp_spawn.TpGroup: every spawned rank (and the leader) builds the same LLM"""
    return LLM(model, **kw)


class LLM:
    def __init__(self, model, tensor_parallel_size=1, max_model_len=6000, limit_mm_per_prompt=None,
                 trust_remote_code=True, gpu_memory_utilization=None, seed=0, tokenizer=None, comm=None,
                 max_num_seqs=1, block_size=None, num_gpu_blocks_override=None, kv_cache_dtype=None, max_logprobs=20,
                 speculative_config=None, **kw):
        from .config import PRESETS, ChatTSConfig, preset
        from .modeling import ChatTSForCausalLM
        from .processing import ChatTSProcessor
        from .tp import Comm, LocalComm
        self._tp_group = None
        # speculative_config (vLLM's name and dict): {"method": "ngram", "num_speculative_tokens": k, "prompt_lookup_max": 3,
        # "prompt_lookup_min": 1} - prompt-lookup speculative decoding for greedy requests; needs tensor_parallel_size 1, max_num_seqs 1
        from .spec import parse_speculative_config
        parse_speculative_config(speculative_config, tensor_parallel_size, max_num_seqs)      # ValueError before any device / worker
        if tensor_parallel_size > 1 and comm is None and "WORLD_SIZE" not in os.environ:
            import torch.distributed as dist
            if not dist.is_initialized():
                # the reference's call shape (demo/demo_vllm.py:30, llm_utils.py:154): ONE plain process asks for k GPUs and the
                # engine spawns its own workers, like vLLM does.  This process becomes rank 0; the followers replay every generate()
                from .tp_spawn import TpGroup
                args = dict(tensor_parallel_size=tensor_parallel_size, max_model_len=max_model_len,
                            limit_mm_per_prompt=limit_mm_per_prompt, trust_remote_code=trust_remote_code,
                            gpu_memory_utilization=gpu_memory_utilization, seed=seed, tokenizer=tokenizer,
                            max_num_seqs=max_num_seqs, block_size=block_size, num_gpu_blocks_override=num_gpu_blocks_override,
                            kv_cache_dtype=kv_cache_dtype, max_logprobs=max_logprobs, **kw)
                group, inner = TpGroup.launch(tensor_parallel_size, _build_llm, (model, args))
                self.__dict__.update(inner.__dict__)
                self._tp_group = group
                return
        self._seed = int(seed)              # also the default seed of sampled generation (SamplingParams.seed overrides)
        if comm is None:
            comm = Comm() if tensor_parallel_size > 1 else LocalComm()
        if comm.world != tensor_parallel_size:
            raise ValueError(f"tensor_parallel_size={tensor_parallel_size} needs {tensor_parallel_size} ranks launched "
                             f"one per GPU (torchrun); this process group has {comm.world}")
        # max_num_seqs (vLLM's name): cache slots decoded together (continuous batching); 1 = one request at a time
        # block_size / num_gpu_blocks_override (vLLM's names): block-paged KV cache; fewer blocks than
        # max_num_seqs x max_model_len / block_size oversubscribes the slots (requests then wait for blocks at admission)
        # kv_cache_dtype (vLLM's name): None / "auto" = the float32 KV cache, "fp16" = the half-size speed mode (ChatTSForCausalLM)
        mk = dict(comm=comm, max_ctx=max_model_len, max_prefill_tokens=min(2048, max_model_len),
                  max_batch=max(1, int(max_num_seqs)), kv_block_size=block_size, kv_pool_blocks=num_gpu_blocks_override,
                  kv_cache_dtype=kv_cache_dtype, max_logprobs=max_logprobs, speculative_config=speculative_config)
        if isinstance(model, ChatTSConfig):
            self.model = ChatTSForCausalLM.from_synthetic(model, seed=seed, **mk)
        elif isinstance(model, str) and model in PRESETS:
            self.model = ChatTSForCausalLM.from_synthetic(preset(model), seed=seed, **mk)
        elif isinstance(model, str) and os.path.isdir(model):
            self.model = ChatTSForCausalLM.from_pretrained(model, **mk)
            if tokenizer is None:           # real weights need the checkpoint's own tokenizer, never the synthetic stand-in
                tokenizer = _load_checkpoint_tokenizer(model)
        else:
            raise ValueError(f"model must be a checkpoint directory, a ChatTSConfig or one of {sorted(PRESETS)}")
        self.config = self.model.config
        self.processor = ChatTSProcessor.from_pretrained(self.config, tokenizer=tokenizer)
        self.limit = (limit_mm_per_prompt or {}).get("timeseries", 50)      # chatts_vllm.py:220 caps at 50

    def get_tokenizer(self):
        return self.processor.tokenizer

    def shutdown(self):
        """stop the tensor-parallel workers this object spawned (no-op otherwise)"""
        if self._tp_group is not None:
            self._tp_group.shutdown()
            self._tp_group = None

    def __del__(self):
        try:
            self.shutdown()
        except Exception:
            pass

    def _requests(self, prompts):
        """what generate() accepts (a str, a {"prompt", "multi_modal_data": {"timeseries": [...]}} dict, a list of them) ->
        [(prompt text, list of series)]; ValueError past the limit_mm_per_prompt cap"""
        out = []
        for req in [prompts] if isinstance(prompts, (str, dict)) else prompts:
            if isinstance(req, str):
                req = {"prompt": req}
            series = list((req.get("multi_modal_data") or {}).get("timeseries", []))
            if len(series) > self.limit:
                raise ValueError(f"At most {self.limit} timeseries may be provided in one prompt, got {len(series)}")
            out.append((req["prompt"], series))
        return out

    def generate(self, prompts, sampling_params=None, use_tqdm=False):
        if self._tp_group is not None:      # spawned followers run the same call now; all ranks meet inside the exchange kernels
            self._tp_group.call("generate", prompts, sampling_params)
        sp = sampling_params or SamplingParams()
        if sp.logprobs is not None and sp.logprobs > self.model.max_logprobs:
            raise ValueError(f"logprobs={sp.logprobs} exceeds max_logprobs={self.model.max_logprobs} (LLM(max_logprobs=...))")
        masked = bool(getattr(sp, "logit_bias", None) or getattr(sp, "allowed_token_ids", None) or getattr(sp, "min_tokens", 0))
        if getattr(sp, "n", 1) > 1 or getattr(sp, "stop", None) or masked:
            return self._generate_engine(prompts, sp)         # per-slot seeds / stop strings / logit masks: through an Engine on this model
        self.model.set_logit_masks(False)                     # per call, like the modes below: a plain call runs the plain selection
        self.model.set_logprobs(sp.logprobs is not None)      # per call, like the sampling mode (a switch re-captures the graphs)
        controls = (sp.repetition_penalty, sp.frequency_penalty, sp.presence_penalty, sp.min_p)
        if controls == (1.0, 0.0, 0.0, 0.0):
            self.model.set_logit_controls(False)              # per call too: a default call runs the plain selection
        self.model.set_sampling(sp.temperature or 0.0, max(int(sp.top_k or 0), 0), sp.top_p,
                                self._seed if sp.seed is None else sp.seed, *controls)
        import torch
        reqs, metas = [], []
        for prompt, series in self._requests(prompts):
            text, encs, lens = self.processor.splice(prompt, [np.asarray(s, dtype=np.float64) for s in series])
            ids = self.processor.tokenizer.encode(text)
            ser = torch.from_numpy(self.processor.pad_stack(encs)) if encs else None
            reqs.append((ids, ser, lens))
            metas.append((prompt, ids))
        e = self.config.eos_token_id
        eos = None if sp.ignore_eos else ((list(e) if isinstance(e, (list, tuple)) else [e]) + sp.stop_token_ids)
        tok = self.processor.tokenizer
        if sp.logprobs is None:
            toks_all = self.model.generate_batch(reqs, sp.max_tokens, eos)      # sequential when max_num_seqs == 1
            return [RequestOutput(p, ids, [CompletionOutput(tok.decode(t, skip_special_tokens=True), t)])
                    for (p, ids), t in zip(metas, toks_all)]
        toks_all, entries_all = self.model.generate_batch(reqs, sp.max_tokens, eos, logprobs=sp.logprobs)
        return [RequestOutput(p, ids, [CompletionOutput(tok.decode(t, skip_special_tokens=True), t, _logprob_dicts(tok, t, e),
                                                        float(sum(x[0] for x in e)))])
                for (p, ids), t, e in zip(metas, toks_all, entries_all)]

    def _generate_engine(self, prompts, sp):
        """generate() for n > 1 and / or stop strings: the requests go through a chatts_amd.engine.Engine on this model (per-slot
        sampling settings and seeds, one prefill + fork per prompt, the stop rule at every harvest).  Sample i of a prompt draws with
        seed + i, seed = SamplingParams.seed or this LLM's, from the per-slot stream hash(seed, step).
        The n = 1 / no-stop path is left exactly as it was, and it draws differently when max_num_seqs > 1: generate_batch's one shared
        configuration hashes (seed, cache slot, step) and folds the slot into the first token's seed, so that requests sharing ONE seed
        do not draw alike.  Hence on such an LLM a sampled call changes its tokens when n > 1 or stop is added (greedy calls do not,
        and neither does any call with max_num_seqs = 1, where there is no slot to fold); Engine and server requests always use the
        per-slot stream, for n = 1 too."""
        from .engine import Engine
        m = self.model
        validate_n(sp.n, sp.best_of, max(1, m.max_batch))
        requests = self._requests(prompts)
        if getattr(m, "_sampling_key", None) not in (None, "rows"):
            m.set_sampling(0.0)                    # the engine works with per-slot settings: leave the baked-in configuration
        eng = Engine(m, self.processor, sync_every=8)
        eng.active_key = getattr(m, "_sampling_key", None)
        kw = {k: getattr(sp, k) for k in REQUEST_FIELDS}
        if sp.seed is None:
            kw["seed"] = self._seed
        eng.check(**kw)                            # (the ids of logit_bias / allowed_token_ids against this model's vocabulary) before anything runs
        reqs = [eng.add_request(prompt, timeseries=series, **kw) for prompt, series in requests]
        eng.run_until_done()
        tok = self.processor.tokenizer
        outs = []
        for r in reqs:
            if r.error is not None:
                raise r.error
            cs = []
            for c in r.outputs:
                text = c.text if c.stop and c.text is not None else tok.decode(c.tokens, skip_special_tokens=True)
                lps = _logprob_dicts(tok, c.tokens, c.logprobs) if c.logprob_k is not None else None
                cs.append(CompletionOutput(text, c.tokens, lps, c.cumulative_logprob, c.index, c.finish_reason, c.stop_reason))
            outs.append(RequestOutput(r.prompt, list(r._enc[0]), cs))
        return outs
