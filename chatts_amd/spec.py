"""Speculative decoding by prompt lookup: the configuration (vLLM's speculative_config dict, HF generate's names).  Host-only, no device
work: the checks run before a model touches the GPU.  The kernels are csrc/spec_decode.hip, the step is chatts_decoder_spec_step."""

MAX_DRAFT = 8          # CHATTS_SPEC_MAX_DRAFT
MAX_NGRAM = 8          # CHATTS_SPEC_MAX_NGRAM
_KEYS = ("method", "num_speculative_tokens", "prompt_lookup_max", "prompt_lookup_min")


def _int(name, v):
    if isinstance(v, bool) or not isinstance(v, int):
        raise ValueError(f"speculative_config: {name}={v!r} must be an integer")
    return v


def parse_speculative_config(cfg, tensor_parallel_size=1, max_num_seqs=1):
    """vLLM's {"method": "ngram", "num_speculative_tokens": k, "prompt_lookup_max": 3, "prompt_lookup_min": 1} (or its JSON text) ->
    None (speculation off) or {"k", "ngram_min", "ngram_max"}.  ValueError naming speculative_config: not a dict, an unknown method
    or key, num_speculative_tokens missing or outside 1..8, n-gram sizes outside 1 <= min <= max <= 8, tensor_parallel_size > 1,
    max_num_seqs > 1 (greedy requests of ONE sequence on ONE GPU are what the speculative step serves)."""
    if cfg is None:
        return None
    if isinstance(cfg, str):
        import json
        try:
            cfg = json.loads(cfg)
        except ValueError as e:
            raise ValueError(f"speculative_config is not valid JSON: {e}") from None
        if cfg is None:
            return None
    if not isinstance(cfg, dict):
        raise ValueError(f"speculative_config must be a dict like {{'method': 'ngram', 'num_speculative_tokens': 4}}, got {type(cfg).__name__}")
    unknown = sorted(set(cfg) - set(_KEYS))
    if unknown:
        raise ValueError(f"speculative_config: unknown keys {unknown} (known: {list(_KEYS)})")
    method = cfg.get("method", "ngram")
    if method != "ngram":
        raise ValueError(f"speculative_config: method={method!r} is not available (only 'ngram', prompt lookup)")
    if "num_speculative_tokens" not in cfg:
        raise ValueError("speculative_config: num_speculative_tokens is required")
    k = _int("num_speculative_tokens", cfg["num_speculative_tokens"])
    nmax = _int("prompt_lookup_max", cfg.get("prompt_lookup_max", 3))
    nmin = _int("prompt_lookup_min", cfg.get("prompt_lookup_min", 1))
    if not 1 <= k <= MAX_DRAFT:
        raise ValueError(f"speculative_config: num_speculative_tokens={k} must be in 1..{MAX_DRAFT}")
    if not 1 <= nmin <= nmax <= MAX_NGRAM:
        raise ValueError(f"speculative_config: prompt_lookup_min={nmin} / prompt_lookup_max={nmax} must satisfy 1 <= min <= max <= {MAX_NGRAM}")
    if int(tensor_parallel_size) > 1:
        raise ValueError(f"speculative_config: speculative decoding runs with tensor_parallel_size 1 only (got {tensor_parallel_size})")
    if int(max_num_seqs) > 1:
        raise ValueError(f"speculative_config: speculative decoding serves one sequence at a time, max_num_seqs 1 (got {max_num_seqs})")
    return {"k": k, "ngram_min": nmin, "ngram_max": nmax}
