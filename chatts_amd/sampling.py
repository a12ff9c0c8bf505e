"""A request's sampling settings, named and checked in one place: the validators every surface shares (SamplingParams, the server's
request parsing, Engine.check), the names of the settings that travel from a caller to Engine.add_request, and SamplingParams itself.
Depends on nothing above it (no engine, model, LLM or server import): the model and the scheduler both check with these."""
import math

import numpy as np

from .detok import normalize_stop

# the per-request settings a caller hands to Engine.add_request (next to prompt / timeseries / on_tokens): what LLM builds from a
# SamplingParams, what EngineThread checks before a request is announced, what the control plane sends to the follower ranks
REQUEST_FIELDS = ("max_tokens", "temperature", "top_p", "top_k", "seed", "stop_token_ids", "ignore_eos", "logprobs", "repetition_penalty",
                  "frequency_penalty", "presence_penalty", "min_p", "n", "best_of", "stop", "include_stop_str_in_output", "logit_bias",
                  "allowed_token_ids", "min_tokens")


def validate_controls(repetition_penalty=None, frequency_penalty=None, presence_penalty=None, min_p=None):
    """The four logit controls with vLLM's defaults and ranges -> (r, f, p, min_p) as floats (None = the default); ValueError otherwise."""
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

LOGIT_BIAS_MAX = 1024       # CHATTS_LOGIT_BIAS_MAX: entries of one request's logit_bias
END_IDS_MAX = 64            # CHATTS_LOGIT_END_IDS_MAX: ids min_tokens keeps away (stop_token_ids + the model's EOS ids)
NO_MASKS = (None, None, 0)


def _token_id(name, t, vocab_size):
    """an id of `name` as it arrives (an int, or for logit_bias the decimal string the OpenAI JSON carries) -> int; ValueError"""
    if name == "logit_bias" and isinstance(t, str) and t.strip().isdigit():
        t = int(t.strip())
    if isinstance(t, bool) or not isinstance(t, (int, np.integer)):
        raise ValueError(f"{name}: token ids must be integers, got {t!r}")
    t = int(t)
    if t < 0 or t > 0x7FFFFFFF or (vocab_size is not None and t >= int(vocab_size)):
        raise ValueError(f"{name}: token id {t} is outside the vocabulary [0, {vocab_size if vocab_size is not None else 2 ** 31})")
    return t


def validate_masks(logit_bias=None, allowed_token_ids=None, min_tokens=None, max_tokens=None, vocab_size=None, end_ids=None):
    """logit_bias / allowed_token_ids / min_tokens with vLLM's meaning -> (bias {id: float} or None, allowed [ids] or None, min_tokens);
    ValueError naming the field otherwise.  logit_bias: None or a dict of at most 1024 entries, keys ints or decimal strings, distinct
    after conversion, values finite (the empty dict counts as off).  allowed_token_ids: None or a non-empty list of distinct ids.
    min_tokens: an integer >= 0, at most max_tokens (when given).  Ids lie in [0, vocab_size) where the caller knows the vocabulary.
    end_ids (when given): the ids min_tokens keeps away - at most 64."""
    bias = None
    if logit_bias is not None:
        if not isinstance(logit_bias, dict):
            raise ValueError(f"logit_bias must be a dict of token id -> bias, got {type(logit_bias).__name__}")
        if len(logit_bias) > LOGIT_BIAS_MAX:
            raise ValueError(f"logit_bias holds {len(logit_bias)} entries, at most {LOGIT_BIAS_MAX} are accepted")
        bias = {}
        for k, v in logit_bias.items():
            t = _token_id("logit_bias", k, vocab_size)
            if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not math.isfinite(v):
                raise ValueError(f"logit_bias: the bias of token {t} must be a finite number, got {v!r}")
            if t in bias:
                raise ValueError(f"logit_bias: token id {t} occurs twice")
            bias[t] = float(v)
        bias = bias or None
    allowed = None
    if allowed_token_ids is not None:
        if isinstance(allowed_token_ids, (str, bytes, dict)) or not hasattr(allowed_token_ids, "__iter__"):
            raise ValueError(f"allowed_token_ids must be a list of token ids, got {allowed_token_ids!r}")
        allowed = [_token_id("allowed_token_ids", t, vocab_size) for t in allowed_token_ids]
        if not allowed:
            raise ValueError("allowed_token_ids must not be empty (None = every token is allowed)")
        if len(set(allowed)) != len(allowed):
            raise ValueError("allowed_token_ids: the ids must be distinct")
    m = 0 if min_tokens is None else min_tokens
    if isinstance(m, bool) or not isinstance(m, (int, np.integer)) or int(m) < 0:
        raise ValueError(f"min_tokens must be an integer >= 0, got {min_tokens!r}")
    m = int(m)
    if max_tokens is not None and m > int(max_tokens):
        raise ValueError(f"min_tokens={m} must not exceed max_tokens={max_tokens}")
    if m and end_ids is not None and vocab_size is not None and any(not 0 <= int(t) < int(vocab_size) for t in end_ids):
        raise ValueError(f"min_tokens: stop_token_ids {sorted(int(t) for t in end_ids if not 0 <= int(t) < int(vocab_size))} lie outside the "
                         f"vocabulary [0, {vocab_size})")
    if m and end_ids is not None and len(set(end_ids)) > END_IDS_MAX:
        raise ValueError(f"min_tokens: {len(set(end_ids))} ids would end the sequence (stop_token_ids and the EOS ids), at most "
                         f"{END_IDS_MAX} are accepted")
    return bias, allowed, m


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


def validate_logprobs(logprobs=None, prompt_logprobs=None, max_logprobs=None):
    """logprobs=k: None or an integer in 0..max_logprobs (no upper limit when that is None); prompt_logprobs only as None"""
    if prompt_logprobs is not None:
        raise ValueError("prompt_logprobs is not supported (only the logprobs of generated tokens)")
    if logprobs is not None and (isinstance(logprobs, bool) or not isinstance(logprobs, (int, np.integer)) or int(logprobs) < 0
                                 or (max_logprobs is not None and int(logprobs) > int(max_logprobs))):
        raise ValueError(f"logprobs must be a non-negative integer, got {logprobs!r}" if max_logprobs is None else
                         f"logprobs must be an integer in 0..{max_logprobs} (max_logprobs), got {logprobs!r}")
    return logprobs


def validate_sampling(max_tokens=64, temperature=0.0, top_p=1.0, top_k=0, logprobs=None, max_logprobs=20, prompt_logprobs=None,
                      repetition_penalty=None, frequency_penalty=None, presence_penalty=None, min_p=None, n=None, best_of=None,
                      stop=None, logit_bias=None, allowed_token_ids=None, min_tokens=None, stop_token_ids=None, vocab_size=None, **_):
    """The ranges vLLM's SamplingParams accepts (what the reference's drivers pass: inference_tsmllm_vllm.py:43-46,
    llm_utils.py:153).  Raises ValueError - the server turns it into a 400 - BEFORE the request can reach the engine thread, where
    an out-of-range value would otherwise surface inside set_sampling / chatts_decoder_set_sampling."""
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
    validate_logprobs(logprobs, prompt_logprobs, max_logprobs)
    validate_masks(logit_bias, allowed_token_ids, min_tokens, int(max_tokens), vocab_size, stop_token_ids or ())


def request_settings(max_tokens=64, temperature=0.0, top_p=1.0, top_k=0, seed=None, stop_token_ids=None, ignore_eos=False, logprobs=None,
                     repetition_penalty=None, frequency_penalty=None, presence_penalty=None, min_p=None, n=1, best_of=None, stop=None,
                     include_stop_str_in_output=False, logit_bias=None, allowed_token_ids=None, min_tokens=0, max_logprobs=20,
                     max_num_seqs=None, vocab_size=None):
    """REQUEST_FIELDS as a caller passes them -> checked (ValueError) and normalised: the settings an engine.Request is made of.
    seed stays None when the caller gave none (the engine chooses one)."""
    validate_sampling(max_tokens, temperature, top_p, top_k, logprobs=logprobs, max_logprobs=max_logprobs)
    stop_token_ids = [int(t) for t in (stop_token_ids or [])]
    masks = validate_masks(logit_bias, allowed_token_ids, min_tokens, int(max_tokens), vocab_size, stop_token_ids)
    return dict(masks=masks, n=validate_n(n, best_of, max_num_seqs), stop=normalize_stop(stop), include_stop=bool(include_stop_str_in_output),
                controls=validate_controls(repetition_penalty, frequency_penalty, presence_penalty, min_p),
                max_tokens=int(max_tokens), temperature=float(temperature or 0.0), top_k=max(int(top_k or 0), 0),
                top_p=1.0 if top_p is None else float(top_p), seed=None if seed is None else int(seed),
                logprobs=None if logprobs is None else int(logprobs), ignore_eos=bool(ignore_eos),
                stop_token_ids=stop_token_ids)


class SamplingParams:
    def __init__(self, max_tokens=16, temperature=0.0, top_p=1.0, top_k=-1, seed=None, stop_token_ids=None,
                 ignore_eos=False, logprobs=None, prompt_logprobs=None, repetition_penalty=1.0, frequency_penalty=0.0,
                 presence_penalty=0.0, min_p=0.0, n=1, best_of=None, stop=None, include_stop_str_in_output=False, logit_bias=None,
                 allowed_token_ids=None, min_tokens=0, **kw):
        # n: samples per prompt (RequestOutput.outputs[i], i = 0 .. n-1).  Sample i draws with seed + i from a stream of (seed, step)
        # alone, so it is what an Engine / server request with seed + i generates, and sample 0 is that surface's n = 1 answer.
        # (LLM.generate serves n = 1 without stop through generate_batch's shared configuration, which with max_num_seqs > 1 folds
        # the cache slot into the draws: there a sampled n = 1 call is not sample 0 of the n = 2 call - LLM._generate_engine.)
        # best_of only as None or n.  stop: strings that end a sequence where they appear in its decoded text - the text ends before
        # the match, or after it with include_stop_str_in_output (chatts_amd/detok.py: the rule)
        self.n = validate_n(n, best_of)
        self.best_of = best_of
        self.stop = normalize_stop(stop)
        self.include_stop_str_in_output = bool(include_stop_str_in_output)
        # k: the chosen token + its k best alternatives per generated token (raw logits); any k >= 0 here, LLM.generate knows max_logprobs
        self.logprobs = validate_logprobs(logprobs, prompt_logprobs)
        self.max_tokens = int(max_tokens)
        self.temperature = temperature          # 0 = greedy (this engine's default; the reference's drivers pass 0.2 / 0.5)
        self.top_p = top_p
        self.top_k = top_k                      # -1 / 0 = off, like vLLM
        self.seed = seed
        self.stop_token_ids = list(stop_token_ids or [])
        self.ignore_eos = ignore_eos
        # vLLM's names, defaults and ranges: l / r (l > 0) or l * r for ids of the prompt or the output; l -= f * count and l -= p for
        # ids of the output; min_p drops ids less probable than min_p x the most probable one (sampled requests only)
        self.repetition_penalty, self.frequency_penalty, self.presence_penalty, self.min_p = validate_controls(
            repetition_penalty, frequency_penalty, presence_penalty, min_p)
        # vLLM's names again: logit_bias {id: bias} (any finite value; the server clamps to [-100, 100]), allowed_token_ids (every other
        # id becomes -inf), min_tokens (no EOS / stop token before that many tokens, no stop string searched in them); the ids are
        # checked against the vocabulary where the model is known (LLM.generate)
        self.logit_bias, self.allowed_token_ids, self.min_tokens = validate_masks(logit_bias, allowed_token_ids, min_tokens, self.max_tokens,
                                                                                  end_ids=self.stop_token_ids)
