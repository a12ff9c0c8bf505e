"""ChatTSForCausalLM - the MI355X-native model behind the reference's two call surfaces.

Mirrors (NetManAIOps/ChatTS):
  HF surface      AutoModelForCausalLM.from_pretrained(...); model.generate(**inputs, max_new_tokens=...)
                  README.md:88-103, demo/demo_hf.ipynb cells 3-5, chatts/utils/inference_tsmllm_deepspeed.py:89-105
                  (returned ids begin with the UN-expanded input_ids; model.config.ts['patch_size'] readable)
  vLLM plugin     Qwen2TSForCausalLM / Qwen3TSForCausalLM hooks, chatts/vllm/chatts_vllm.py:
                  get_multimodal_embeddings :538-562, get_input_embeddings :564-574, forward :576-599,
                  compute_logits :601-610, load_weights :612-625, packed_modules_mapping :454-464
All arithmetic runs in libchatts_amd.so (hand-written HIP, gfx950); torch only owns device memory,
streams and the RCCL process group.  There is no CPU/PyTorch fallback.
"""
import ctypes as C
import math
import os

import numpy as np
import torch

from . import _lib, prefix_cache, synth
from .config import ChatTSConfig, preset
from .spec import parse_speculative_config
from .tp import Comm, LocalComm, ShardPlan
from .ts_encoder import TimeSeriesEmbedding

packed_modules_mapping = {"qkv_proj": ["q_proj", "k_proj", "v_proj"], "gate_up_proj": ["gate_proj", "up_proj"]}
PROJECTIONS = ("qkv", "o", "gate_up", "down")          # the four weight matrices of a layer, as packed (q|k|v, gate/up interleaved)


def interleave_gate_up(gate, up):
    """[I,H],[I,H] -> [2I,H] with gate/up alternating in blocks of 16 rows (CHATTS_EPI_SWIGLU layout)."""
    I, H = gate.shape
    out = torch.empty((2 * I, H), dtype=gate.dtype, device=gate.device)
    v = out.view(I // 16, 2, 16, H)
    v[:, 0] = gate.view(I // 16, 16, H)
    v[:, 1] = up.view(I // 16, 16, H)
    return out


def quantize_int8_rows(w):
    """[N,K] bf16 -> (q uint8 view of int8 [N,K], scale f32 [N] (powers of two), deq bf16 [N,K]).

    w ~= scale[n] * q[n,k], q in [-127, 127], scale a power of two: the dequantised value has <= 7 significant bits and is EXACTLY
    representable in bf16 - the same lossless-re-encoding argument as quantize_fp8_rows, on a uniform grid (the weight-only 8-bit
    format in the role of the HF demo's `load_in_8bit`, demo/demo_hf.ipynb:78-80)."""
    wf = w.float()
    amax = wf.abs().amax(dim=1).clamp_min(1e-30)
    scale = torch.exp2(torch.ceil(torch.log2(amax / 127.0)))
    scale = torch.where(amax / scale > 127.0, scale * 2.0, scale)          # guard log2 rounding: never overflow int8
    q = torch.clamp(torch.round(wf / scale[:, None]), -127, 127).to(torch.int8)
    deq = (q.float() * scale[:, None]).to(torch.bfloat16)
    return q.view(torch.uint8).contiguous(), scale.contiguous(), deq.contiguous()


def quantize_fp8_rows(w):
    """[N,K] bf16 -> (q uint8 view of float8_e4m3fn [N,K], scale f32 [N] (powers of two), deq bf16 [N,K]).

    w ~= scale[n] * float(q[n,k]) with scale a power of two, so the dequantised value has <= 4 significant bits and is
    EXACTLY representable in bf16: `deq` replaces the bf16 weight and both copies describe the same matrix."""
    wf = w.float()
    amax = wf.abs().amax(dim=1).clamp_min(1e-30)
    scale = torch.exp2(torch.ceil(torch.log2(amax / 448.0)))
    scale = torch.where(amax / scale > 448.0, scale * 2.0, scale)          # guard log2 rounding: never overflow e4m3
    q = (wf / scale[:, None]).to(torch.float8_e4m3fn)
    deq = (q.float() * scale[:, None]).to(torch.bfloat16)
    return q.view(torch.uint8).contiguous(), scale.contiguous(), deq.contiguous()


def quantize_int4_rows(w, group_size=128):
    """[N,K] bf16 -> (codes uint8 [N,K] in 0..15, scale f32 [N,G] (fp16-representable, like GPTQ's), zero f32 [N,G], deq bf16 [N,K]).
    Round-to-nearest asymmetric 4-bit per group of `group_size` weights of a row (NOT the GPTQ solver: that runs offline and its
    checkpoints are loaded as they are, chatts_amd/gptq.py).  deq = bf16_rne(scale * (code - zero)) REPLACES the bf16 weight, so
    every kernel and the oracle see one matrix; the int4 decode GEMV rebuilds exactly these values from the codes."""
    N, K = w.shape
    assert K % group_size == 0 and group_size % 16 == 0
    wf = w.float().view(N, K // group_size, group_size)
    lo, hi = wf.amin(2), wf.amax(2)
    scale = ((hi - lo) / 15.0).clamp_min(1e-8).to(torch.float16).float()
    zero = torch.clamp(torch.round(-lo / scale), 0, 15)
    q = torch.clamp(torch.round(wf / scale[:, :, None]) + zero[:, :, None], 0, 15)
    deq = (q * scale[:, :, None] - (scale * zero)[:, :, None]).to(torch.bfloat16).view(N, K)
    return q.to(torch.uint8).view(N, K).contiguous(), scale.contiguous(), zero.contiguous(), deq.contiguous()


def pack_int4(codes, scale, zero):
    """codes uint8 [N,K] -> (row-major nibbles uint8 [N,K/2]: byte j = code 2j | code 2j+1 << 4;  (scale, scale*zero) f32 [N,G,2])."""
    packed = (codes[:, 0::2] | (codes[:, 1::2] << 4)).contiguous()
    return packed, torch.stack([scale, scale * zero], dim=-1).contiguous()


def rope_tables(cfg, max_pos, device):
    """float32 cos/sin [max_pos, d/2], computed like Qwen2RotaryEmbedding (inv_freq = theta^(-2i/d), f32)."""
    d = cfg.head_dim
    inv = 1.0 / (cfg.rope_theta ** (torch.arange(0, d, 2, dtype=torch.float32) / d))
    fr = torch.arange(max_pos, dtype=torch.float32)[:, None] * inv[None, :]
    return fr.cos().contiguous().to(device), fr.sin().contiguous().to(device)


KV_CACHE_DTYPES = {None: "float32", "auto": "float32", "float32": "float32", "fp16": "float16", "float16": "float16", "half": "float16"}


def _eos_set(eos_token_id):
    """eos_token_id: one id, a list / tuple / set of ids, or None -> set of ids"""
    return set(eos_token_id if isinstance(eos_token_id, (list, tuple, set)) else ([] if eos_token_id is None else [eos_token_id]))


def _eos_end(toks, eos):
    """length of toks up to and including its first EOS token; None without one"""
    return next((i + 1 for i, t in enumerate(toks) if t in eos), None)


def kv_cache_dtype_name(kv_cache_dtype):
    """kv_cache_dtype (vLLM's name) -> "float32" or "float16"; ValueError for anything else (fp8 included)."""
    try:
        return KV_CACHE_DTYPES[kv_cache_dtype]
    except (KeyError, TypeError):
        raise ValueError(f"kv_cache_dtype={kv_cache_dtype!r}: accepted are None / 'auto' / 'float32' (the float32 cache) and "
                         "'fp16' / 'float16' / 'half'") from None


class ChatTSForCausalLM:
    packed_modules_mapping = packed_modules_mapping

    def __init__(self, config, device="cuda", comm=None, max_ctx=2048, max_prefill_tokens=2048, use_graph=True,
                 max_batch=1, weight_format="bf16", use_p2p=True, enable_prefix_caching=True, kv_block_size=None,
                 kv_pool_blocks=None, precision=None, prefill_tiled_weights=None, kv_cache_dtype=None, max_logprobs=20,
                 speculative_config=None):
        kv_name = kv_cache_dtype_name(kv_cache_dtype)       # (checked before anything touches the device)
        # speculative_config (vLLM's dict, {"method": "ngram", "num_speculative_tokens": k, "prompt_lookup_max": 3, "prompt_lookup_min": 1}):
        # prompt-lookup speculative decoding for greedy requests of the single-sequence path (chatts_amd/spec.py, csrc/spec_decode.hip).
        # None = off: no buffer, no launch and no graph of the feature exists.
        self._spec_cfg = parse_speculative_config(speculative_config, 1 if comm is None else comm.world, max_batch)
        self._spec_call = None                   # the configuration of ONE generate() call (HF's prompt_lookup_num_tokens)
        self._spec_active = False                # the running request takes the speculative step
        self._spec_request = False               # ... or did when it started: host token counts are lower bounds, the device step counter rules
        self._spec_graphs = {}                   # (k, ngram_min, ngram_max) -> captured speculative step
        if not 0 <= int(max_logprobs) <= _lib.LOGPROBS_MAX_K:
            raise ValueError(f"max_logprobs={max_logprobs} must be in 0..{_lib.LOGPROBS_MAX_K}")
        if not torch.cuda.is_available():
            raise RuntimeError("chatts_amd needs a ROCm GPU: there is no CPU fallback for the model")
        self.lib = _lib.load()
        self.config = config
        # precision: None / "bf16x2" = the parity-grade default (float32 activations carried as bf16 hi + lo planes, two MFMA passes
        # in the prefill GEMMs: logits ~5e-5 of the float32 oracle).  "bf16" = SPEED mode: the prefill GEMMs
        # multiply the bf16-rounded activations only - half the matrix work, logits ~1e-2, what a bf16 HF / vLLM run computes.
        # PROCESS-WIDE (the library's GEMM_PRECISION option, chatts_set_option): every model of this process follows the last setting.
        # "fp8" = SPEED mode on the CDNA4 fp8 matrix pipe (needs weight_format="fp8", BASELINE.json config 5): prefill chunks and the
        # TS encoder quantise their activations per row to e4m3 and multiply fp8 x fp8 (v_mfma_scale_f32_16x16x128_f8f6f4: 4x less
        # matrix time than bf16x2), logits ~1e-2 from the default; decode steps are unchanged.  Per model, not process-wide.
        # "f16q" = PARITY GRADE like the default, on other matrix pipes: prefill chunks of >= 96 rows multiply an f16 high part
        # on the f16 MFMA and an e4m3 residual x e4m3 weights on the CDNA4 block-scaled fp8 MFMA (1.5 instead of 2 pass-equivalents per
        # product; logits ~1.3e-4 of the float32 oracle against ~5e-5).  Measured SLOWER than the default (the kernel is paced by its
        # operand feed, which the split does not shrink) and costs 3 more bytes per weight: opt-in, never the default.  Per model.
        # kv_cache_dtype: None / "auto" / "float32" = the float32 KV cache (parity grade, the default).  "fp16" / "float16" / "half" =
        # SPEED mode: K / V rows stored as IEEE fp16 ((_Float16)x, round to nearest even; |x| > 65504 becomes inf, as in the reference's
        # fp16 run), half the cache bytes - twice the slots, context or paged pool in the same memory, half the decode attention's
        # stream (config 5: 5.62 -> 5.26 ms per step).  Logits 1.86e-3 of the float32 oracle at full depth, tokens equal (the float32
        # cache under option KV_ROUND=3 computes the same values; profiles/kv_fp16_ab.txt): NOT parity grade against the 1e-3 bar.
        # Scores, softmax and P.V stay float32.  Per model.
        if precision not in (None, "bf16x2", "bf16", "fp8", "f16q"):
            raise ValueError("precision must be None / 'bf16x2' or 'f16q' (parity grade), 'bf16' or 'fp8' (speed modes)")
        if precision == "fp8" and weight_format != "fp8":
            raise ValueError("precision='fp8' multiplies the fp8 weight copies: it needs weight_format='fp8'")
        if precision is not None:
            _lib.set_option("GEMM_PRECISION", 1 if precision == "bf16" else None)
        self.precision = precision or "bf16x2"
        self.kv_cache_dtype = getattr(torch, kv_name)
        self.device = torch.device(device)
        self.comm = comm or LocalComm()
        self.plan = ShardPlan(config, self.comm.rank, self.comm.world)
        self.max_ctx = int(max_ctx)
        # block-paged KV cache (vLLM's block_size / num_gpu_blocks): kv_block_size = positions per block (power of two >= 64),
        # None = one contiguous cache per slot.  kv_pool_blocks < max_batch * max_ctx / block oversubscribes the slots: requests
        # reserve blocks for prompt + max_new_tokens at admission and wait while the pool cannot cover them (chatts_amd/kv_blocks.py)
        self.kv_block_size = int(kv_block_size or 0)
        if self.kv_block_size:
            if self.kv_block_size < 64 or self.kv_block_size & (self.kv_block_size - 1):
                raise ValueError(f"kv_block_size={kv_block_size} must be a power of two >= 64")
            self.max_ctx = -(-self.max_ctx // self.kv_block_size) * self.kv_block_size      # whole blocks
        self._kv_pool_blocks = None if kv_pool_blocks is None else int(kv_pool_blocks)
        self._kv = None                          # kv_blocks.BlockPool once the buffers exist
        self._kv_replaced = {}                   # slot -> logical blocks swapped for private ones since its last prefix decision
        self._kv_dynamic = False
        self._cur_slot = 0
        if weight_format not in ("bf16", "fp8", "int8", "int4"):
            raise ValueError("weight_format must be 'bf16', 'fp8', 'int8' or 'int4'")
        # "fp8": decode GEMVs stream an e4m3 copy (BASELINE.json config 5); "int4": they stream 4-bit codes + group scales (what a
        # GPTQ-Int4 checkpoint brings along; a bf16 checkpoint is quantised round-to-nearest at load)
        self.weight_format = weight_format
        self.int4_group = 128
        self._gptq_codes = {}                    # HF module name -> (codes, scale, zero) of a GPTQ checkpoint, consumed by _load_with
        self.max_batch = int(max_batch)          # KV-cache slots for batched decode (continuous batching)
        self.t_max = int(max(min(max_prefill_tokens, self.max_ctx), self.max_batch))
        # a second copy of the four projection matrices of every layer in the prefill kernel's tiled layout (chatts_tile_bf16: its LDS-DMA
        # pieces then read consecutive memory; bit-identical results, prefill projections -4 %, profiles/r6_tiled_check.txt).  None = when
        # a prefill chunk can reach that kernel (>= 96 rows) and CHATTS_TILED_WEIGHTS != 0; costs the bf16 weight bytes once more.
        if prefill_tiled_weights is None:
            prefill_tiled_weights = self.t_max >= 96 and os.environ.get("CHATTS_TILED_WEIGHTS", "1") != "0" and self.precision != "f16q"
        self.prefill_tiled_weights = bool(prefill_tiled_weights)
        self._tiled = []                         # per layer: {projection: tiled copy}
        self.use_graph = use_graph
        self.use_p2p = use_p2p                   # TP: decode-sized exchanges through csrc/tp.hip instead of RCCL (chatts_amd/tp.py)
        self._tp = None                          # P2PExchange of this rank once attached
        # prefix reuse (vLLM's enable_prefix_caching; demo/demo_vllm.py:55 submits 100 identical prompts, multi-turn chats
        # re-send their history): per cache slot, the identity of every token whose K/V rows are resident
        self.enable_prefix_caching = bool(enable_prefix_caching)
        self._slot_idents = [[] for _ in range(max(1, int(max_batch)))]
        self.prefix_stats = {"requests": 0, "hits": 0, "tokens_reused": 0, "tokens_prefilled": 0}
        self.ts_encoder = TimeSeriesEmbedding(config.ts, device=self.device)
        self._tensors = {}            # keeps every device tensor alive (the C side borrows pointers)
        self._decoder = None
        self._graph = None
        # token logprobs (set_logprobs): every selection is followed by chatts_decoder_logprobs with K = max_logprobs into per-slot
        # rings [max_batch, out_stride(, K)] allocated on first use; a request reads the first k <= max_logprobs of its cells
        self.max_logprobs = int(max_logprobs)
        self._logprobs_on = False
        # logit controls (set_logit_controls): repetition / frequency / presence penalties and min_p ahead of every selection, from
        # per-slot arrays and a per-slot state [max_batch, vocab] allocated on first use
        self._controls_on = False
        # logit masks (set_logit_masks): allowed_token_ids / logit_bias / min_tokens ahead of the controls, from per-slot arrays
        # allocated on first use
        self._masks_on = False
        self.layers = []
        self.loaded = set()

    # ---------------------------------------------------------------------------------------------
    # weights
    # ---------------------------------------------------------------------------------------------
    @classmethod
    def from_synthetic(cls, config, seed=0, **kw):
        """Random-init model whose weights are the counter-hash of chatts_amd/synth.py (bf16-exact)."""
        if isinstance(config, str):
            config = preset(config)
        m = cls(config, **kw)
        dev, plan, cfg = m.device, m.plan, config
        specs = {s.name: s for s in synth.all_specs(cfg)}

        def block(name, row0=0, rows=None, col0=0, cols=None, f32=False):
            s = specs[name]
            rows = s.rows - row0 if rows is None else rows
            cols = s.cols - col0 if cols is None else cols
            t = torch.empty((rows, cols), dtype=torch.float32 if f32 else torch.bfloat16, device=dev)
            synth.fill_device(t, s, seed, row0=row0, col0=col0, rows=rows, cols=cols)
            return t[0] if s.is_1d else t

        m._load_with(block, tied=cfg.tie_word_embeddings)
        m.ts_encoder.load_synthetic(synth.ts_encoder_specs(cfg), seed)
        m.seed = seed
        m._finalize()
        return m

    @classmethod
    def register_for_auto_class(cls, auto_class="AutoModelForCausalLM"):
        """transformers calls this on a class resolved through config.json's auto_map (trust_remote_code); nothing to register."""

    @classmethod
    def from_pretrained(cls, path, *model_args, trust_remote_code=True, device_map=None, torch_dtype=None, dtype=None,
                        lora_adapter=None, config=None, **kw):
        """HF checkpoint directory (config.json + *.safetensors with the names of SURVEY.md section 5).
        Also the target of ``AutoModelForCausalLM.from_pretrained(path, trust_remote_code=True, device_map=..., torch_dtype=...)``
        (README.md:88) through the auto_map ChatTSConfig.save_pretrained writes: transformers' own keywords are accepted and
        ignored (`config` is re-read from config.json; activations are float32 whatever torch_dtype says).
        lora_adapter: a peft LoRA adapter directory merged into the weights while loading (chatts_amd/lora.py)."""
        import glob
        import os
        from safetensors import safe_open
        cfg = ChatTSConfig.from_pretrained(path)
        for hf_only in ("cache_dir", "force_download", "local_files_only", "token", "revision", "use_safetensors", "subfolder",
                        "low_cpu_mem_usage", "attn_implementation", "code_revision", "_from_auto", "adapter_kwargs", "use_auth_token",
                        "proxies", "resume_download", "_commit_hash", "_from_pipeline", "quantization_config", "weights_only"):
            kw.pop(hf_only, None)
        if isinstance(device_map, int):
            device_map = f"cuda:{device_map}"
        if isinstance(device_map, dict):
            device_map = "cuda"
        if device_map not in (None, "auto") and "device" not in kw:
            kw["device"] = device_map if isinstance(device_map, str) else "cuda"
        m = cls(cfg, **kw)
        handles, index = [], {}
        for f in sorted(glob.glob(os.path.join(path, "*.safetensors"))):
            h = safe_open(f, framework="pt", device="cpu")
            handles.append(h)
            for k in h.keys():
                index[k] = h
        pairs = ((k, h.get_tensor(k)) for k, h in index.items())
        from . import gptq
        if gptq.is_gptq_config(cfg.extra):          # ChatTS-14B-GPTQ-Int4: unpack qweight / qzeros / scales / g_idx to bf16 weights
            pairs = gptq.dequantized_pairs(pairs, cfg.extra["quantization_config"], has_g_idx=any(k.endswith(".g_idx") for k in index))
        if lora_adapter is not None:
            from . import lora
            pairs = lora.merged(pairs, lora_adapter)
        m.load_weights(pairs)
        m._checkpoint_path, m._checkpoint_kw = path, dict(kw)
        return m

    def load_weights(self, weights):
        """chatts_vllm.py:612-625: consume (name, tensor) pairs with HF names; q/k/v and gate/up are packed,
        a missing lm_head means tied embeddings (:619-623).  Returns the set of loaded names."""
        sd = {}
        for name, t in weights:
            if name.endswith(".gptq_codes"):          # (codes, scale, zero) of a GPTQ module (chatts_amd/gptq.py)
                self._gptq_codes[name[:-len(".gptq_codes")]] = t
                continue
            if name.startswith("ts_encoder."):
                self.ts_encoder.load_tensor(name[len("ts_encoder."):], t)
                self.loaded.add(name)
            else:
                sd[name] = t
        dev = self.device

        def block(name, row0=0, rows=None, col0=0, cols=None, f32=False):
            t = sd[name]
            if t.dim() == 1:
                t = t[col0:(None if cols is None else col0 + cols)]
            else:
                t = t[row0:(None if rows is None else row0 + rows), col0:(None if cols is None else col0 + cols)]
            self.loaded.add(name)
            return t.to(dev).to(torch.float32 if f32 else torch.bfloat16).contiguous()

        self._load_with(block, tied="lm_head.weight" not in sd)
        self._finalize()
        return self.loaded

    def _load_with(self, block, tied):
        cfg, plan = self.config, self.plan
        d = cfg.head_dim
        T = self._tensors
        T["embed"] = block("model.embed_tokens.weight")
        if tied:
            T["lm_head"] = T["embed"][plan.v0:plan.v0 + plan.vocab].contiguous() if plan.world > 1 else T["embed"]
        else:
            T["lm_head"] = block("lm_head.weight", row0=plan.v0, rows=plan.vocab)
        T["final_norm"] = block("model.norm.weight", f32=True)
        for l in range(cfg.num_hidden_layers):
            p = f"model.layers.{l}."
            q = block(p + "self_attn.q_proj.weight", row0=plan.q0 * d, rows=plan.nq * d)
            k = block(p + "self_attn.k_proj.weight", row0=plan.kv0 * d, rows=plan.nkv * d)
            v = block(p + "self_attn.v_proj.weight", row0=plan.kv0 * d, rows=plan.nkv * d)
            L = {"qkv": torch.cat([q, k, v], dim=0).contiguous()}
            del q, k, v
            if cfg.attention_bias:
                L["qkv_bias"] = torch.cat([
                    block(p + "self_attn.q_proj.bias", col0=plan.q0 * d, cols=plan.nq * d, f32=True),
                    block(p + "self_attn.k_proj.bias", col0=plan.kv0 * d, cols=plan.nkv * d, f32=True),
                    block(p + "self_attn.v_proj.bias", col0=plan.kv0 * d, cols=plan.nkv * d, f32=True)]).contiguous()
            if cfg.qk_norm:
                L["q_norm"] = block(p + "self_attn.q_norm.weight", f32=True)
                L["k_norm"] = block(p + "self_attn.k_norm.weight", f32=True)
            L["o"] = block(p + "self_attn.o_proj.weight", col0=plan.q0 * d, cols=plan.nq * d)
            g = block(p + "mlp.gate_proj.weight", row0=plan.i0, rows=plan.inter)
            u = block(p + "mlp.up_proj.weight", row0=plan.i0, rows=plan.inter)
            L["gate_up"] = interleave_gate_up(g, u)
            del g, u
            L["down"] = block(p + "mlp.down_proj.weight", col0=plan.i0, cols=plan.inter)
            L["input_norm"] = block(p + "input_layernorm.weight", f32=True)
            L["post_norm"] = block(p + "post_attention_layernorm.weight", f32=True)
            self._fuse_gptq_codes(L, p)
            self.layers.append(L)

    def _fuse_gptq_codes(self, L, p):
        """GPTQ checkpoint: pack the per-module 4-bit codes the way the weights were packed (q|k|v rows, gate/up interleaved) so
        that the decode GEMV can stream them.  Only for tensor_parallel_size 1 (a K-slice of down_proj is not group aligned)."""
        G = self._gptq_codes
        names = ["self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj", "mlp.gate_proj", "mlp.up_proj",
                 "mlp.down_proj"]
        if self.plan.world != 1 or not all(p + n in G for n in names):
            return
        dev = self.device
        c = {n: tuple(t.to(dev) for t in G.pop(p + n)) for n in names}
        cat = lambda ns: tuple(torch.cat([c[n][i] for n in ns], dim=0).contiguous() for i in range(3))
        fused = {"qkv": cat(names[:3]), "o": c[names[3]], "down": c[names[6]],
                 "gate_up": tuple(interleave_gate_up(c[names[4]][i], c[names[5]][i]) for i in range(3))}
        for k, (q, sc, z) in fused.items():
            self.int4_group = q.shape[1] // sc.shape[1]
            L[k + "4"], L[k + "4_sz"] = pack_int4(q, sc, z)

    def _finalize(self):
        """Allocate activations / KV cache and create the C-side decoder handle (borrowing all pointers)."""
        cfg, plan = self.config, self.plan
        max_pos = max(self.max_ctx, 64)
        self._tensors["cos"], self._tensors["sin"] = rope_tables(cfg, max_pos, self.device)
        self._quantize_projections()
        # decode attention: one wave per 16-key tile; slots beyond the live context exit immediately
        self.n_splits = max(1, min(64, (self.max_ctx + 15) // 16))
        dc = _lib.DecoderConfig(hidden=cfg.hidden_size, n_layers=cfg.num_hidden_layers, n_q=plan.nq, n_kv=plan.nkv, head_dim=cfg.head_dim,
                                inter=plan.inter, vocab_local=plan.vocab, vocab_offset=plan.v0,
                                rms_eps=cfg.rms_norm_eps, max_ctx=self.max_ctx, max_pos=max_pos, tp_world=plan.world,
                                embed_rows=cfg.vocab_size, embed_offset=0,       # the embedding table is replicated
                                w8_format=_lib.W8_INT8 if self.weight_format == "int8" else _lib.W8_FP8)
        ws_bytes = self._workspace_bytes(dc)
        self._alloc_buffers(ws_bytes)
        self._tiled = self._tiled_copies()
        self._f16q = self._f16q_copies()
        self._layer_arr = self._layer_weights()
        self._create_decoder(dc, ws_bytes)
        if plan.world > 1 and self.use_p2p and getattr(self.comm, "dist", None) is not None and self._tp is None:
            self._attach_p2p()

    def _quantize_projections(self):
        T = self._tensors
        if self.weight_format in ("fp8", "int8") and "lm_head8" not in T:
            # quantise every decoder projection once; the bf16 tensors are REPLACED by the (bf16-exact) dequantised
            # values so prefill (bf16 MFMA GEMM), batched decode and the 8-bit decode GEMV all see the same weights
            quant = quantize_fp8_rows if self.weight_format == "fp8" else quantize_int8_rows
            for lw in self.layers:
                for name in PROJECTIONS:
                    lw[name + "8"], lw[name + "8_scale"], lw[name] = quant(lw[name])
            tied = T["lm_head"].data_ptr() == T["embed"].data_ptr()
            T["lm_head8"], T["lm_head8_scale"], deq = quant(T["lm_head"])
            T["lm_head"] = deq
            if tied:
                T["embed"] = deq
        if self.weight_format == "int4" and self.layers and "qkv4" not in self.layers[0]:
            # round-to-nearest 4-bit codes of every decoder projection; the bf16 tensors are REPLACED by the dequantised values
            for lw in self.layers:
                for name in PROJECTIONS:
                    q, sc, z, lw[name] = quantize_int4_rows(lw[name], self.int4_group)
                    lw[name + "4"], lw[name + "4_sz"] = pack_int4(q, sc, z)

    def _workspace_bytes(self, dc):
        lib, plan, H = self.lib, self.plan, self.config.hidden_size
        ws_bytes = int(lib.chatts_decoder_workspace(C.byref(dc), self.t_max, self.n_splits))
        ws_bytes = max(ws_bytes, int(lib.chatts_linear_workspace(self.t_max, plan.vocab, H)))
        for m in range(2, self.max_batch + 1):     # batched lm_head
            ws_bytes = max(ws_bytes, int(lib.chatts_linear_workspace(m, plan.vocab, H)))
        ws_bytes = max(ws_bytes, int(lib.chatts_attn_workspace(self.max_batch, plan.nq, self.n_splits)) + 256)
        ws_bytes = max(ws_bytes, int(lib.chatts_logprobs_workspace(max(1, self.max_batch), self.max_logprobs)))
        if self._spec_cfg is not None:           # the speculative step: lm_head for 2 .. 9 rows, attention partials of 9 rows
            ws_bytes = max(ws_bytes, self._spec_workspace_bytes())
        # the prefill attention's K / V planes (kv_planes_kernel: 32 KB per (kv head, 32-key tile)) for a sequence of max_ctx positions:
        # with the workspace sized for them the planes kernel is taken at EVERY chunk position, so the same prompt never changes
        # kernel (and summation order) with where a chunk starts
        return max(ws_bytes, ((self.max_ctx + 31) // 32) * plan.nkv * 4 * 32 * self.config.head_dim * 2 + 256)

    def _spec_workspace_bytes(self):
        lib, plan, H = self.lib, self.plan, self.config.hidden_size
        need = max(int(lib.chatts_linear_workspace(m, plan.vocab, H)) for m in range(2, _lib.SPEC_MAX_ROWS + 1))
        return max(need, int(lib.chatts_attn_workspace(_lib.SPEC_MAX_ROWS, plan.nq, min(self.n_splits, 16))) + 256)

    def _alloc_buffers(self, ws_bytes):
        cfg, plan, dev = self.config, self.plan, self.device
        H, d = cfg.hidden_size, cfg.head_dim
        MB = self.max_batch
        f32 = dict(dtype=torch.float32, device=dev)
        qkv_n = (plan.nq + 2 * plan.nkv) * d
        L = cfg.num_hidden_layers
        if self.kv_block_size:
            from .kv_blocks import BlockPool
            bps = self.max_ctx // self.kv_block_size
            nblk = MB * bps if self._kv_pool_blocks is None else self._kv_pool_blocks
            if nblk < 1 or nblk > MB * bps:
                raise ValueError(f"kv_pool_blocks={nblk} must lie in 1..{MB * bps} (max_batch x max_ctx / kv_block_size)")
            kv_shape = (L, nblk, plan.nkv, self.kv_block_size, d)             # layer-major block pools
            self._kv = BlockPool(nblk, self.kv_block_size, MB, bps)
            self._kv_dynamic = nblk < MB * bps
        else:
            kv_shape = (MB, L, plan.nkv, self.max_ctx, d)                     # slot-major: one contiguous cache per sequence
        B = {
            "kv_k": torch.zeros(kv_shape, dtype=self.kv_cache_dtype, device=dev),
            "kv_v": torch.zeros(kv_shape, dtype=self.kv_cache_dtype, device=dev),
            "kv_table": torch.zeros((MB, self.max_ctx // self.kv_block_size), dtype=torch.int32, device=dev) if self.kv_block_size else None,
            "x": torch.zeros((self.t_max, H), **f32), "xn": torch.zeros((self.t_max, H), **f32),
            "qkv": torch.zeros((self.t_max, qkv_n), **f32), "attn": torch.zeros((self.t_max, plan.nq * d), **f32),
            "act": torch.zeros((self.t_max, plan.inter), **f32), "delta": torch.zeros((self.t_max, H), **f32),
            "logits": torch.zeros(plan.vocab, **f32),
            # two pairs of bf16 hi / lo planes (prefill: LDS-DMA GEMM operands; pair 0 = projection input, pair 1 = SwiGLU out)
            "planes": torch.zeros((4, (self.t_max + 31) // 32 * 32, max(H, plan.nq * d, plan.inter)), dtype=torch.bfloat16, device=dev),   # (rows: whole 16-row blocks for the tiled f16q planes)
            "ws": torch.zeros(ws_bytes, dtype=torch.uint8, device=dev),
            # decode-loop state lives on the device so a captured step can be replayed
            "pos_all": torch.zeros(MB, dtype=torch.int32, device=dev), "step_all": torch.zeros(MB, dtype=torch.int32, device=dev),
            "token_all": torch.zeros(MB, dtype=torch.int64, device=dev), "token_logit_all": torch.zeros(MB, **f32),
            "out_tokens_all": torch.zeros((MB, self.max_ctx + 8), dtype=torch.int64, device=dev),
            "logits_all": torch.zeros((MB, plan.vocab), **f32) if MB > 1 else None,
            "scan": torch.zeros(self.t_max + 8, dtype=torch.int32, device=dev),
            "status": torch.zeros(1, dtype=torch.int32, device=dev),
            # tensor parallel: scratch of the token agreement (chatts_decoder_select_tokens)
            "tp_pair_logit": torch.zeros(MB, **f32) if plan.world > 1 else None,
            "tp_pair_token": torch.zeros(MB, dtype=torch.int64, device=dev) if plan.world > 1 else None,
            "logits_full": torch.zeros((MB, plan.vocab * plan.world), **f32) if plan.world > 1 else None,
        }
        # single-sequence views (slot 0): the batch-1 fast path and its hipGraph use these
        B["pos"], B["step"], B["token"], B["token_logit"] = B["pos_all"][:1], B["step_all"][:1], B["token_all"][:1], B["token_logit_all"][:1]
        B["out_tokens"] = B["out_tokens_all"][0]
        self.buf = B
        if self._kv is not None and not self._kv_dynamic:       # a full pool: every slot owns max_ctx positions for good
            for sl in range(MB):
                self._kv.reserve(sl, self.max_ctx)
                self._kv.retire(sl)
                self._push_kv_row(sl)

    def _tiled_copies(self):
        """per layer {projection: copy in the prefill kernel's tiled layout} (prefill_tiled_weights)"""
        lib, dev = self.lib, self.device
        out, tile_ok = [], self.prefill_tiled_weights
        for lw in self.layers:
            tiled = {}
            if tile_ok:
                # the copies are an optimisation: never let them take the memory the KV cache / activations of a large configuration need
                need = sum(lw[n].numel() * 2 for n in PROJECTIONS)
                free = torch.cuda.mem_get_info(dev)[0]
                if free < need + (8 << 30):
                    import warnings
                    warnings.warn(f"prefill_tiled_weights: {free / 2**30:.1f} GiB free - layers {len(out)}.. keep the row-major weights only")
                    tile_ok = False
            if tile_ok:
                for name in PROJECTIONS:
                    w = lw[name]
                    rows, k = w.shape
                    if k % 64 == 0 and w.is_contiguous():
                        t = torch.empty(int(lib.chatts_tile_bf16_elems(rows, k)), dtype=torch.bfloat16, device=dev)
                        _lib.check(lib.chatts_tile_bf16(w.data_ptr(), rows, k, k, t.data_ptr(), _lib.stream_ptr()))
                        tiled[name] = t
            out.append(tiled)
        return out

    def _f16q_copies(self):
        """per layer {projection: (w16, w8, w8e)} of precision='f16q' (empty dicts otherwise)"""
        lib, dev = self.lib, self.device
        out = []
        for lw in self.layers:
            qd = {}
            if self.precision == "f16q":
                for name in PROJECTIONS:
                    w = lw[name]
                    rows, k = w.shape
                    if k % 128 or not w.is_contiguous():
                        raise ValueError(f"precision='f16q' needs K % 128 == 0 for every projection ({name}: K={k})")
                    w16 = torch.empty((rows, k), dtype=torch.float16, device=dev)
                    w8 = torch.empty((rows, k), dtype=torch.uint8, device=dev)
                    w8e = torch.empty((rows,), dtype=torch.uint8, device=dev)
                    _lib.check(lib.chatts_weights_f16q(w.data_ptr(), rows, k, k, w16.data_ptr(), w8.data_ptr(), w8e.data_ptr(), k, _lib.stream_ptr()))
                    # ... stored in the kernel's own block order: an LDS-DMA piece is 1 KB of consecutive memory
                    w16t = torch.empty(int(lib.chatts_tile_bf16_elems(rows, k)), dtype=torch.float16, device=dev)
                    w8t = torch.empty(int(lib.chatts_tile_e4m3_bytes(rows, k)), dtype=torch.uint8, device=dev)
                    _lib.check(lib.chatts_tile_bf16(w16.data_ptr(), rows, k, k, w16t.data_ptr(), _lib.stream_ptr()))
                    _lib.check(lib.chatts_tile_e4m3(w8.data_ptr(), rows, k, k, w8t.data_ptr(), _lib.stream_ptr()))
                    qd[name] = (w16t, w8t, w8e)
            out.append(qd)
        return out

    def _layer_weights(self):
        """the C side's per-layer pointer array: every weight format and copy present (NULL for the absent ones)"""
        arr = (_lib.LayerWeights * self.config.num_hidden_layers)()
        for i, lw in enumerate(self.layers):
            tl, fq = self._tiled[i], self._f16q[i]
            ts = {n: lw.get(n) for n in ("input_norm", "qkv_bias", "q_norm", "k_norm", "post_norm")}
            for n in PROJECTIONS:
                ts.update({n: lw[n], n + "_t": tl.get(n)})
                ts.update({n + suf: lw.get(n + suf) for suf in ("8", "8_scale", "4", "4_sz")})
                ts.update(zip((n + "16", n + "_q8", n + "_q8e"), fq.get(n, (None, None, None))))
            arr[i] = _lib.LayerWeights(**{k: _lib.ptr(t) for k, t in ts.items()}, w4_group=self.int4_group)
        return arr

    def _create_decoder(self, dc, ws_bytes):
        lib, T, B = self.lib, self._tensors, self.buf
        dw = _lib.DecoderWeights(layers=self._layer_arr, final_norm=_lib.ptr(T["final_norm"]), lm_head=_lib.ptr(T["lm_head"]),
                                 lm_head8=_lib.ptr(T.get("lm_head8")), lm_head8_scale=_lib.ptr(T.get("lm_head8_scale")),
                                 embed=_lib.ptr(T["embed"]), cos_tab=_lib.ptr(T["cos"]), sin_tab=_lib.ptr(T["sin"]))
        db = _lib.DecoderBuffers(kv_k=_lib.ptr(B["kv_k"]), kv_v=_lib.ptr(B["kv_v"]), x=_lib.ptr(B["x"]),
                                 xn=_lib.ptr(B["xn"]), qkv=_lib.ptr(B["qkv"]), attn=_lib.ptr(B["attn"]),
                                 act=_lib.ptr(B["act"]), delta=_lib.ptr(B["delta"]), logits=_lib.ptr(B["logits"]),
                                 workspace=_lib.ptr(B["ws"]), workspace_bytes=ws_bytes, t_max=self.t_max,
                                 max_batch=self.max_batch, planes_hi=_lib.ptr(B["planes"][0]),
                                 planes_lo=_lib.ptr(B["planes"][1]), planes2_hi=_lib.ptr(B["planes"][2]),
                                 planes2_lo=_lib.ptr(B["planes"][3]), tp_pair_logit=_lib.ptr(B["tp_pair_logit"]),
                                 tp_pair_token=_lib.ptr(B["tp_pair_token"]), logits_full=_lib.ptr(B["logits_full"]),
                                 kv_block_table=_lib.ptr(B["kv_table"]), kv_block_size=self.kv_block_size,
                                 kv_table_stride=(self.max_ctx // self.kv_block_size) if self.kv_block_size else 0,
                                 kv_pool_blocks=self._kv.n_blocks if self._kv is not None else 0,
                                 kv_dtype=_lib.KV_F16 if self.kv_cache_dtype == torch.float16 else _lib.KV_F32)
        h = lib.chatts_decoder_create(C.byref(dc), C.byref(dw), C.byref(db))
        if not h:
            raise _lib.ChattsError(-1, lib.chatts_last_error().decode())
        self._decoder = C.c_void_p(h)
        self._drop_graphs()
        if self.precision == "fp8":              # speed mode: prefill chunks and the TS encoder on the fp8 matrix pipe
            _lib.check(lib.chatts_decoder_set_prefill_fp8(self._decoder, 1))
            self.ts_encoder.set_precision("fp8")
        if self.precision == "f16q":             # parity-grade prefill on the f16 + fp8 matrix pipes (the TS encoder keeps bf16x2)
            _lib.check(lib.chatts_decoder_set_prefill_f16q(self._decoder, 1))

    def _attach_p2p(self):
        """TP: set up the peer-to-peer exchange on every rank, or on none (then batch-1 decode falls back to host-driven RCCL)"""
        from .tp import P2PExchange
        world = self.plan.world
        ex, err = None, None
        try:
            ex = P2PExchange.create(self.comm, self.exchange_elems(), self.exchange_bulk_elems())
        except Exception as e:               # e.g. no IPC mapping between these two devices
            err = e
        # every rank must take the same path: agree before anyone attaches
        oks = [None] * world
        self.comm.dist.all_gather_object(oks, err is None, group=self.comm.group)
        if all(oks):
            self.attach_exchange(ex)
        else:
            if ex is not None:
                ex.close()
            if self.max_batch > 1:
                raise RuntimeError(f"the peer-to-peer exchange could not be set up on ranks {[r for r, ok in enumerate(oks) if not ok]} "
                                   f"({err}); batched decode under tensor parallelism needs it")
            import warnings
            warnings.warn(f"peer-to-peer exchange unavailable on ranks {[r for r, ok in enumerate(oks) if not ok]} ({err}): "
                          "decode-sized sums go through RCCL from the host (slower, no hipGraph)")
            self.use_p2p = False

    def exchange_bulk_elems(self):
        """float32 elements of the largest prefill-sized sum: one chunk of partial [t_max, H] rows (chatts_allreduce_bulk)"""
        return self.t_max * self.config.hidden_size

    def exchange_elems(self):
        """float32 elements per rank the largest in-step collective moves: [max_batch, H] partial sums, or the logits gather."""
        return max(self.max_batch * self.config.hidden_size, self.max_batch * self.plan.vocab, 2 * self.max_batch)

    def attach_exchange(self, exchange):
        """Bind this rank's P2PExchange (chatts_amd/tp.py): the whole TP decode step then runs behind one C call / one hipGraph."""
        _lib.check(self.lib.chatts_decoder_set_tp(self._decoder, exchange.handle if exchange is not None else None))
        self._tp = exchange
        self._drop_graphs()

    def __del__(self):
        try:
            if self._decoder:
                self.lib.chatts_decoder_destroy(self._decoder)
            if self._tp is not None:
                self._tp.close()
        except Exception:
            pass

    def weight_bytes_local(self):
        """Bytes one batch-1 decode step streams on this rank (fp8 copies replace their bf16 twins when present)."""
        n = 0
        for lw in self.layers:
            for k, t in lw.items():
                if k + "8" in lw or k + "4" in lw:
                    continue                       # the fp8 / 4-bit copy is the one the decode GEMV reads
                n += t.numel() * t.element_size()
        T = self._tensors
        head = (T["lm_head8"].numel() + T["lm_head8_scale"].numel() * 4) if "lm_head8" in T else T["lm_head"].numel() * 2
        return n + head + T["final_norm"].numel() * 4

    def kv_cache_bytes_local(self):
        """Bytes of this rank's K and V caches (every slot, or the paged pool): halved by kv_cache_dtype="fp16"."""
        return sum(self.buf[k].numel() * self.buf[k].element_size() for k in ("kv_k", "kv_v"))

    def tiled_weight_bytes_local(self):
        """Bytes of the prefill kernel's tiled weight copies on this rank (resident beside the tensors weight_bytes_local() counts)."""
        return sum(t.numel() * t.element_size() for tl in self._tiled for t in tl.values())

    def f16q_weight_bytes_local(self):
        """Bytes of the f16q weight copies (precision='f16q' only)"""
        return sum(t.numel() * t.element_size() for qd in self._f16q for t3 in qd.values() for t in t3)

    # ---------------------------------------------------------------------------------------------
    # vLLM-plugin-shaped hooks (same names/order as chatts_vllm.py:538-610)
    # ---------------------------------------------------------------------------------------------
    def get_multimodal_embeddings(self, timeseries=None, valid_lengths=None, **kw):
        """-> list of [patch_cnt_i, H] tensors (empty [0,H] for zero-length series), or None."""
        if timeseries is None:
            return None
        ts = self._parse_and_validate_ts_input(timeseries)
        feats, patch_cnt = self.ts_encoder(ts, valid_lengths=valid_lengths)
        if valid_lengths is not None:
            counts = self._patch_counts(valid_lengths)
        else:
            counts = patch_cnt.tolist()
        out, s = [], 0
        for c in counts:
            out.append(feats[s:s + c])
            s += c
        return out

    def _parse_and_validate_ts_input(self, timeseries):
        """chatts_vllm.py:493-536: accept the padded tensor, or a list of (ts_tokens, encoded [1,2L,1]) items."""
        if isinstance(timeseries, torch.Tensor):
            return timeseries.to(self.device, dtype=torch.float32)
        if isinstance(timeseries, (list, tuple)):
            encs = []
            for item in timeseries:
                if isinstance(item, (list, tuple)) and len(item) == 2 and not np.isscalar(item[1]):
                    encs.append(np.asarray(item[1], dtype=np.float32).reshape(1, -1, 1))
                else:
                    encs.append(np.asarray(item, dtype=np.float32).reshape(1, -1, 1))
            lmax = max(e.shape[1] for e in encs)
            out = np.zeros((len(encs), lmax, 1), dtype=np.float32)
            for i, e in enumerate(encs):
                out[i, :e.shape[1]] = e[0]
            return torch.from_numpy(out).to(self.device)
        raise ValueError(f"Incorrect type of ts input features. Got type: {type(timeseries)}")

    def get_input_embeddings(self, input_ids, multimodal_embeddings=None, out=None):
        """embed_tokens(ids) with rows at ts_token_start_index overwritten in order by the TS rows (:564-574).
        input_ids: 1-D (already expanded) ids, host list / CPU tensor / device tensor."""
        ids_host = None
        if not isinstance(input_ids, torch.Tensor):
            input_ids = torch.tensor(list(input_ids), dtype=torch.int64)
        if not input_ids.is_cuda:
            ids_host = input_ids.to(torch.int64).contiguous()
            ids_dev = ids_host.to(self.device, non_blocking=True)
        else:
            ids_dev = input_ids.to(torch.int64).contiguous()
        t = ids_dev.numel()
        H = self.config.hidden_size
        rows, n_rows = None, 0
        if multimodal_embeddings is not None:
            rows = (multimodal_embeddings if isinstance(multimodal_embeddings, torch.Tensor)
                    else (torch.cat(list(multimodal_embeddings), dim=0) if len(multimodal_embeddings) else
                          torch.empty((0, H), dtype=torch.float32, device=self.device)))
            rows = rows.contiguous()
            n_rows = rows.shape[0]
        if out is None:
            out = torch.empty((t, H), dtype=torch.float32, device=self.device)
        scan = self.buf["scan"] if t + 1 <= self.buf["scan"].numel() else torch.empty(t + 1, dtype=torch.int32, device=self.device)
        if ids_host is None:
            self.buf["status"].zero_()
        _lib.check(self.lib.chatts_embed_merge(
            _lib.ptr(ids_dev), _lib.ptr(ids_host) if ids_host is not None else None, t, _lib.ptr(self._tensors["embed"]),
            self.config.vocab_size, H, _lib.ptr(rows) if n_rows else None, n_rows, self.config.ts_token_start_index,
            _lib.ptr(out), _lib.ptr(scan), _lib.ptr(self.buf["status"]), _lib.stream_ptr()))
        if ids_host is None and int(self.buf["status"].item()) & 1:
            # device-resident ids: the count check ran on the GPU (one D2H sync, as vLLM's merge_multimodal_embeddings does)
            raise ValueError(f"Attempted to assign {n_rows} multimodal tokens to a different number of <ts> placeholders")
        return out

    def forward(self, input_ids=None, positions=None, intermediate_tensors=None, inputs_embeds=None, **kw):
        """Prefill `inputs_embeds` [T,H] (or embed input_ids [+ timeseries kw]) at positions pos0..pos0+T-1;
        returns the residual-stream hidden states [T,H] BEFORE the final norm (compute_logits applies it)."""
        if inputs_embeds is None:
            mm = self.get_multimodal_embeddings(**kw)
            inputs_embeds = self.get_input_embeddings(input_ids, mm)
        pos0 = 0 if positions is None else int(positions[0])
        T = inputs_embeds.shape[0]
        if T > self.t_max:
            raise ValueError(f"{T} tokens exceed max_prefill_tokens={self.t_max}; use prefill() for chunking")
        self.buf["x"][:T].copy_(inputs_embeds)
        self._run_layers(T, pos0)
        return self.buf["x"][:T]

    def compute_logits(self, hidden_states=None, sampling_metadata=None, row=None):
        """final RMSNorm + lm_head on ONE row of the residual stream (default: the last) -> [V_local] float32."""
        if hidden_states is not None and hidden_states.data_ptr() != self.buf["x"].data_ptr():
            self.buf["x"][:hidden_states.shape[0]].copy_(hidden_states)
        if row is None:
            row = (hidden_states.shape[0] - 1) if hidden_states is not None else 0
        _lib.check(self.lib.chatts_decoder_logits(self._decoder, int(row), _lib.stream_ptr()))
        return self.buf["logits"]

    # ---------------------------------------------------------------------------------------------
    # engine
    # ---------------------------------------------------------------------------------------------
    def _tp_bulk(self, T):
        """tensor parallel: the attached exchange can sum [T, H] partials itself (chatts_allreduce_bulk) -> one C call per chunk"""
        import os
        if os.environ.get("CHATTS_TP_BULK", "1") == "0":          # A/B and fault isolation: the host-driven sums (RCCL / gloo) instead
            return False
        return self._tp is not None and self._tp.bulk_elems >= T * self.config.hidden_size

    def _run_layers(self, T, pos0, pos_dev=None, n_splits=1, last_only=False):
        lib, st = self.lib, _lib.stream_ptr()
        if pos_dev is None and (self.plan.world == 1 or self._tp_bulk(T)):
            if last_only:         # only the next token + the KV cache are wanted: the final layer runs for the last row only
                _lib.check(lib.chatts_decoder_prefill_last(self._decoder, T, pos0, st))
            else:
                _lib.check(lib.chatts_decoder_prefill(self._decoder, T, pos0, st))
            return
        H = self.config.hidden_size
        delta = self.buf["delta"][:T]
        tp = self.plan.world > 1
        p2p = tp and self._tp is not None and T <= 16 and T * H <= self._tp.max_elems
        pending = 0                      # TP: the all-reduced delta of the previous part is added by the next C call
        for l in range(self.config.num_hidden_layers):
            for part in (0, 1):
                _lib.check(lib.chatts_decoder_layer_part_add(self._decoder, pending, l, part, T, pos0, _lib.ptr(pos_dev),
                                                             n_splits, st))
                if tp and p2p:
                    self._tp.all_reduce(delta, out=self.buf["x"][:T], resid=self.buf["x"][:T])      # x += sum of the partials
                elif tp:
                    self.comm.all_reduce(delta)         # RCCL for prefill-sized messages
                    pending = 1
        if pending:
            _lib.check(lib.chatts_residual_add(_lib.ptr(self.buf["x"]), _lib.ptr(delta), T * H, st))

    # ---- block-paged KV cache: host bookkeeping (chatts_amd/kv_blocks.py) ------------------------------------------------
    def _push_kv_row(self, slot):
        row = self._kv.rows[slot]
        if row:                                  # stream-ordered: kernels enqueued after this see the new row
            self.buf["kv_table"][slot, :len(row)] = torch.tensor(row, dtype=torch.int32)

    def _kv_evicted(self, victim):
        self._slot_idents[victim] = []           # nothing is resident there any more (its stale table row is never read: parked)

    def reserve_kv(self, slot, n_tokens, idents=None, protect=(), write_from=0):
        """Make cache slot `slot` able to hold n_tokens positions (no-op with a contiguous cache) and mark it active.  idents = the
        request's token identities: the slot whose resident prefix will be reused is protected from eviction (like `protect`), and
        every block the request is going to WRITE - everything past the reused prefix; `write_from` positions for direct callers -
        is made private first if another slot shares it.  Raises kv_blocks.KvPoolExhausted (nothing changed) when even evicting
        every finished sequence does not free enough blocks."""
        if self._kv is None:
            return
        if n_tokens > self.max_ctx:
            raise ValueError(f"{n_tokens} positions exceed max_ctx={self.max_ctx}")
        keep = set(protect)
        first = int(write_from) // self._kv.block_size
        if idents is not None and self.enable_prefix_caching:
            n, src = prefix_cache.match_prefix(self._slot_idents, idents, slot)
            n = min(n, len(idents) - 1)
            if src >= 0 and n >= prefix_cache.MIN_REUSE:
                keep.add(src)
                first = n // self._kv.block_size          # own slot: rows below stay; other slot: blocks below get adopted
        order = sorted(range(self.max_batch), key=lambda sl: len(self._slot_idents[sl]))       # least resident first
        changed = self._kv.reserve(slot, n_tokens, protect=keep, evict_order=order, on_evict=self._kv_evicted, private_from=first)
        self._kv_replaced[slot] = self._kv_replaced.get(slot, set()) | self._kv.last_replaced
        if changed:
            self._push_kv_row(slot)

    def kv_fits(self, token_counts):
        """could requests needing these many positions (prompt + new tokens each) be admitted into free slots now?"""
        return self._kv is None or self._kv.fits(token_counts)

    def request_tokens(self, ids, series=None, lengths=None):
        """expanded prompt length of a request (host arithmetic when the series lengths are known)"""
        if series is not None and series.shape[0] > 0 and lengths is None:
            lengths = self.ts_encoder.get_patch_cnt(series.to(self.device, dtype=torch.float32))[0].tolist()
        return len(self.expand_input_ids(list(ids), self._patch_counts(lengths or [])))

    def kv_stats(self):
        if self._kv is None:
            return None
        return {"block_size": self._kv.block_size, "blocks": self._kv.n_blocks, "free": len(self._kv.free),
                "active_slots": len(self._kv.active), "evictions": self._kv.evictions, "dynamic": self._kv_dynamic,
                "shared_blocks": self._kv.shared_blocks()}

    def reset(self):
        self.buf["pos"].zero_()
        self.buf["step"].zero_()
        self._spec_active = self._spec_request = False      # (a sequence set up by hand - prefill(), _first_token() - takes the plain step)

    def prefill(self, inputs_embeds, pos0=0, for_next_token=False):
        """Chunked prefill of [T,H] embeddings starting at cache position pos0; leaves the last chunk in x and returns the
        number of rows whose LAST one yields the next token's logits (chatts_decoder_logits(row = returned - 1)).
        for_next_token: the hidden states are not wanted, only the next token and the cache - the final layer of the last chunk
        then runs attention / o_proj / MLP for the last row only (chatts_decoder_prefill_last) and that row is row 0: returns 1."""
        T = inputs_embeds.shape[0]
        if pos0 + T > self.max_ctx:
            raise ValueError(f"sequence of {pos0 + T} tokens exceeds max_ctx={self.max_ctx}")
        if self._kv is not None and (self._kv.capacity_tokens(self._cur_slot) < pos0 + T or self._kv.shared_blocks()):
            self.reserve_kv(self._cur_slot, pos0 + T, write_from=pos0)      # direct callers; generate_* reserve prompt + new tokens up front
        fast_last = for_next_token and (self.plan.world == 1 or self._tp_bulk(min(T, self.t_max)))
        done, last = 0, 0
        while done < T:
            n = min(self.t_max, T - done)
            self.buf["x"][:n].copy_(inputs_embeds[done:done + n])
            final = done + n >= T
            self._run_layers(n, pos0 + done, last_only=fast_last and final)
            done += n
            last = 1 if (fast_last and final) else n
        return last

    def set_sampling(self, temperature=0.0, top_k=0, top_p=1.0, seed=0, repetition_penalty=None, frequency_penalty=None,
                     presence_penalty=None, min_p=None):
        """Token selection of every following step: greedy (temperature 0 / None, the default) or temperature / top-k /
        top-p sampling on the GPU (chatts_sample_batched).  Same seed + same prompt => same tokens.  The four logit controls: when any
        is given, all four are set for every cache slot (set_slot_controls; one not given = its default); when none is, the slots keep
        theirs."""
        if any(v is not None for v in (repetition_penalty, frequency_penalty, presence_penalty, min_p)):
            self.set_slot_controls(None, repetition_penalty, frequency_penalty, presence_penalty, min_p)
        if "lc_temp" in self.buf:
            self.buf["lc_temp"].fill_(float(temperature or 0.0))
        if not temperature:
            args = None
        else:
            if temperature < 0 or not (0.0 < top_p <= 1.0):
                raise ValueError(f"temperature={temperature} must be >= 0 and top_p={top_p} in (0, 1]")
            args = _lib.SamplingArgs(temperature=float(temperature), top_k=int(top_k or 0), top_p=float(top_p),
                                     seed=int(seed) & 0xFFFFFFFF, n_kept=None, kept_mass=None)
        key = None if args is None else (args.temperature, args.top_k, args.top_p, args.seed)
        if key == getattr(self, "_sampling_key", None):
            return
        _lib.check(self.lib.chatts_decoder_set_sampling(self._decoder, None if args is None else C.byref(args)))
        self._sampling, self._sampling_key = args, key
        self._drop_graphs()              # the captured steps have the old selection kernel baked in

    def _sampling_arrays(self):
        if "samp_temp" not in self.buf:
            dev, n = self.device, max(1, self.max_batch)
            self.buf["samp_temp"] = torch.zeros(n, dtype=torch.float32, device=dev)     # 0 = the slot decodes greedily
            self.buf["samp_topk"] = torch.zeros(n, dtype=torch.int32, device=dev)
            self.buf["samp_topp"] = torch.ones(n, dtype=torch.float32, device=dev)
            self.buf["samp_seed"] = torch.zeros(n, dtype=torch.int32, device=dev)       # (bit pattern of the uint32 seed)
        return self.buf

    def _rows_args(self, slot):
        B = self._sampling_arrays()
        return _lib.SamplingArgs(temperature=1.0, top_k=0, top_p=1.0, seed=0, n_kept=None, kept_mass=None,
                                 temperature_rows=B["samp_temp"][slot:].data_ptr(), top_k_rows=B["samp_topk"][slot:].data_ptr(),
                                 top_p_rows=B["samp_topp"][slot:].data_ptr(), seed_rows=B["samp_seed"][slot:].data_ptr())

    def set_sampling_rows(self):
        """Per-slot sampling (ChattsSamplingArgs.*_rows): every cache slot draws with its own (temperature, top_k, top_p, seed), read on
        the device at run time from four small arrays - requests with different settings share one captured step, and
        set_slot_sampling() changes a slot without re-capturing.  Slots start greedy (temperature 0)."""
        if getattr(self, "_sampling_key", None) == "rows":
            return
        args = self._rows_args(0)
        _lib.check(self.lib.chatts_decoder_set_sampling(self._decoder, C.byref(args)))
        self._sampling, self._sampling_key = args, "rows"
        if "lc_temp" in self.buf:
            self.buf["lc_temp"].copy_(self.buf["samp_temp"])
        self._drop_graphs()

    def set_slot_sampling(self, slot, temperature=0.0, top_k=0, top_p=1.0, seed=0, repetition_penalty=1.0, frequency_penalty=0.0,
                          presence_penalty=0.0, min_p=0.0):
        """Sampling settings of the sequence in cache slot `slot`: used by every step in per-slot mode (set_sampling_rows), inert in
        the other modes.  A plain device write - no re-capture.  The four logit controls: set_slot_controls."""
        temperature = 0.0 if temperature is None else float(temperature)
        if temperature < 0 or not (0.0 < top_p <= 1.0):
            raise ValueError(f"temperature={temperature} must be >= 0 and top_p={top_p} in (0, 1]")
        self.set_slot_controls(slot, repetition_penalty, frequency_penalty, presence_penalty, min_p)
        B = self._sampling_arrays()
        if "lc_temp" in B and getattr(self, "_sampling_key", None) == "rows":
            B["lc_temp"][slot] = temperature
        B["samp_temp"][slot] = temperature
        B["samp_topk"][slot] = max(int(top_k or 0), 0)
        B["samp_topp"][slot] = float(top_p)
        s32 = int(seed) & 0xFFFFFFFF
        B["samp_seed"][slot] = s32 - (1 << 32) if s32 >= (1 << 31) else s32

    # ---- logit controls: repetition / frequency / presence penalties and min_p (csrc/logit_controls.hip) ----------------------------
    @staticmethod
    def check_controls(repetition_penalty=None, frequency_penalty=None, presence_penalty=None, min_p=None):
        """-> the four values as floats (None = the default); ValueError outside vLLM's ranges (engine.validate_controls)"""
        from .sampling import validate_controls
        return validate_controls(repetition_penalty, frequency_penalty, presence_penalty, min_p)

    def _control_buffers(self):
        B = self.buf
        if "lc_state" not in B:
            dev, n, V = self.device, max(1, self.max_batch), self.plan.vocab * self.plan.world
            B["lc_state"] = torch.zeros((n, V), dtype=torch.int32, device=dev)     # bit 30: in the prompt; bits 0..29: times generated
            B["lc_out"] = torch.zeros((n, V), dtype=torch.float32, device=dev)     # the penalised logits the selection reads
            B["lc_rep"] = torch.ones(n, dtype=torch.float32, device=dev)
            B["lc_freq"] = torch.zeros(n, dtype=torch.float32, device=dev)
            B["lc_pres"] = torch.zeros(n, dtype=torch.float32, device=dev)
            B["lc_minp"] = torch.zeros(n, dtype=torch.float32, device=dev)
            B["lc_temp"] = torch.zeros(n, dtype=torch.float32, device=dev)         # the temperature each slot is sampled with (min_p cut)
            key, sa = getattr(self, "_sampling_key", None), getattr(self, "_sampling", None)
            if key == "rows":
                B["lc_temp"].copy_(B["samp_temp"])
            elif sa is not None:
                B["lc_temp"].fill_(float(sa.temperature))
        return B

    def _control_args(self, slot):
        B = self._control_buffers()
        V = B["lc_state"].shape[1]
        return _lib.LogitControlArgs(state=B["lc_state"][slot:].data_ptr(), state_stride=V, out=B["lc_out"][slot:].data_ptr(), out_stride=V,
                                     repetition_rows=B["lc_rep"][slot:].data_ptr(), frequency_rows=B["lc_freq"][slot:].data_ptr(),
                                     presence_rows=B["lc_pres"][slot:].data_ptr(), min_p_rows=B["lc_minp"][slot:].data_ptr(),
                                     temperature_rows=B["lc_temp"][slot:].data_ptr())

    def set_logit_controls(self, on):
        """Logit controls on / off for every following selection.  On: each selection (decode steps, first tokens of every admission
        path) first writes the penalised logits of its rows (repetition / frequency / presence penalties from the per-slot state, the
        min_p cut) to a buffer of their own, selects from those, and counts the chosen tokens into the state; the raw logits - and so the
        logprobs - are untouched.  A switch drops the captured decode graphs; off, the steps are exactly what they are without the
        feature.  set_slot_controls switches it on when a slot needs it; the engine switches it off after greedy_return_steps
        iterations without a request that does."""
        on = bool(on)
        if on == self._controls_on:
            return
        if on and self.plan.world > 1 and self._tp is None:
            raise NotImplementedError("repetition / frequency / presence penalties and min_p under tensor parallelism need the "
                                      "peer-to-peer exchange (use_p2p=True)")
        if on:
            args = self._control_args(0)
            _lib.check(self.lib.chatts_decoder_set_logit_controls(self._decoder, C.byref(args)))
        else:
            _lib.check(self.lib.chatts_decoder_set_logit_controls(self._decoder, None))
        self._controls_on = on
        self._drop_graphs()

    def set_slot_controls(self, slot, repetition_penalty=1.0, frequency_penalty=0.0, presence_penalty=0.0, min_p=0.0):
        """Logit controls of the sequence in cache slot `slot` (None: of every slot), with vLLM's names, defaults and ranges: plain
        device writes, no re-capture.  Values other than the defaults switch the mode on (set_logit_controls); all-default values never
        allocate anything."""
        r, f, p, m = self.check_controls(repetition_penalty, frequency_penalty, presence_penalty, min_p)
        if (r, f, p, m) != (1.0, 0.0, 0.0, 0.0):
            self.set_logit_controls(True)
        elif "lc_rep" not in self.buf:
            return
        B = self.buf
        for key, v in (("lc_rep", r), ("lc_freq", f), ("lc_pres", p), ("lc_minp", m)):
            if slot is None:
                B[key].fill_(v)
            else:
                B[key][slot] = v

    def _request_controls(self, controls, n):
        """controls argument of generate_batch -> one checked dict or None per request"""
        per = list(controls) if isinstance(controls, (list, tuple)) else [controls] * n
        if len(per) != n:
            raise ValueError("controls: one value per request")
        for c in per:
            if c is not None:
                self.check_controls(**c)
        return per

    def _controls_admit(self, slot, ids):
        """(controls on) a request enters cache slot `slot`: clear the slot's state and mark its prompt ids"""
        if not self._controls_on:
            return
        B = self.buf
        prompt = torch.tensor(list(ids), dtype=torch.int64, device=self.device)
        _lib.check(self.lib.chatts_logit_state_reset(B["lc_state"][slot].data_ptr(), B["lc_state"].shape[1], 0,
                                                     _lib.ptr(prompt) if prompt.numel() else None, prompt.numel(), _lib.stream_ptr()))

    # ---- logit masks: allowed_token_ids / logit_bias / min_tokens (csrc/logit_masks.hip) ------------------------------------------------
    def _mask_buffers(self):
        B = self.buf
        if "lm_out" not in B:
            dev, n, V = self.device, max(1, self.max_batch), self.plan.vocab * self.plan.world
            i32 = dict(dtype=torch.int32, device=dev)
            B["lm_out"] = torch.zeros((n, V), dtype=torch.float32, device=dev)      # the masked logits the controls / the selection read
            B["lm_allow"] = torch.zeros((n, (V + 31) // 32), **i32)                 # bit of id i: word i / 32, bit i % 32
            B["lm_allow_on"] = torch.zeros(n, **i32)
            B["lm_bias_ids"] = torch.zeros((n, _lib.LOGIT_BIAS_MAX), **i32)
            B["lm_bias_val"] = torch.zeros((n, _lib.LOGIT_BIAS_MAX), dtype=torch.float32, device=dev)
            B["lm_bias_n"] = torch.zeros(n, **i32)
            B["lm_end_ids"] = torch.zeros((n, _lib.LOGIT_END_IDS_MAX), **i32)
            B["lm_end_n"] = torch.zeros(n, **i32)
            B["lm_min_tokens"] = torch.zeros(n, **i32)
        return B

    def _mask_args(self, slot):
        B = self._mask_buffers()
        return _lib.LogitMaskArgs(out=B["lm_out"][slot:].data_ptr(), out_stride=B["lm_out"].shape[1],
                                  allow_bits=B["lm_allow"][slot:].data_ptr(), allow_stride=B["lm_allow"].shape[1],
                                  allow_on=B["lm_allow_on"][slot:].data_ptr(), bias_ids=B["lm_bias_ids"][slot:].data_ptr(),
                                  bias_val=B["lm_bias_val"][slot:].data_ptr(), bias_n=B["lm_bias_n"][slot:].data_ptr(),
                                  bias_stride=_lib.LOGIT_BIAS_MAX, end_ids=B["lm_end_ids"][slot:].data_ptr(),
                                  end_n=B["lm_end_n"][slot:].data_ptr(), min_tokens=B["lm_min_tokens"][slot:].data_ptr(),
                                  end_stride=_lib.LOGIT_END_IDS_MAX)

    def set_logit_masks(self, on):
        """Logit masks on / off for every following selection.  On: each selection (decode steps, first tokens of every admission
        path) first writes the masked logits of its rows (allowed_token_ids, logit_bias, min_tokens from the per-slot arrays) to a buffer
        of their own; the penalties (when on) read that buffer, and the selection the last one written.  The raw logits - and so the
        logprobs - are untouched.  A switch drops the captured decode graphs; off, the steps are exactly what they are without the
        feature.  set_slot_masks switches it on when a slot needs it; the engine switches it off after greedy_return_steps iterations
        without a request that does."""
        on = bool(on)
        if on == self._masks_on:
            return
        if on and self.plan.world > 1 and self._tp is None:
            raise NotImplementedError("logit_bias / allowed_token_ids / min_tokens under tensor parallelism need the peer-to-peer "
                                      "exchange (use_p2p=True)")
        if on:
            args = self._mask_args(0)
            _lib.check(self.lib.chatts_decoder_set_logit_masks(self._decoder, C.byref(args)))
        else:
            _lib.check(self.lib.chatts_decoder_set_logit_masks(self._decoder, None))
            for k in ("lm_allow_on", "lm_bias_n", "lm_end_n", "lm_min_tokens"):      # no slot's settings survive the mode
                self.buf[k].zero_()
        self._masks_on = on
        self._drop_graphs()

    def check_masks(self, logit_bias=None, allowed_token_ids=None, min_tokens=0, end_ids=(), max_tokens=None):
        """-> (bias {id: float} or None, allowed ids or None, min_tokens, sorted end ids inside the vocabulary); ValueError outside the
        ranges of sampling.validate_masks for THIS model's vocabulary (Engine.check / the server refuse a min_tokens request whose
        stop_token_ids lie outside it; here such ids are dropped, as they were inert before)"""
        from .sampling import validate_masks
        V = self.plan.vocab * self.plan.world
        ends = sorted({int(t) for t in (end_ids or ()) if t is not None and 0 <= int(t) < V})      # (an id outside the vocabulary can never
        bias, allowed, m = validate_masks(logit_bias, allowed_token_ids, min_tokens, max_tokens, V, ends)    # be chosen: nothing to keep away)
        return bias, allowed, m, ends

    def set_slot_masks(self, slot, logit_bias=None, allowed_token_ids=None, min_tokens=0, end_ids=()):
        """logit_bias / allowed_token_ids / min_tokens of the sequence in cache slot `slot`, with vLLM's names and meaning; end_ids: the
        ids that would end it (its stop_token_ids and the EOS ids it obeys), kept away while it has fewer than min_tokens tokens.  Plain
        device copies, no re-capture.  Values other than the defaults switch the mode on (set_logit_masks); all-default values never
        allocate anything, and reset the slot's rows while the mode is on (nothing leaks from the slot's previous tenant)."""
        bias, allowed, m, ends = self.check_masks(logit_bias, allowed_token_ids, min_tokens, end_ids)
        if not ends:
            m = 0                                    # nothing could end the sequence: min_tokens has nothing to keep away
        if bias is not None or allowed is not None or m:
            self.set_logit_masks(True)
        elif not self._masks_on:                     # (switching the mode off cleared every slot's flags and counts)
            return
        B, dev, slot = self._mask_buffers(), self.device, int(slot)
        if allowed is not None:
            bits = np.zeros(B["lm_allow"].shape[1], dtype=np.uint32)
            ids = np.asarray(allowed, dtype=np.int64)
            np.bitwise_or.at(bits, ids >> 5, (np.uint32(1) << (ids & 31).astype(np.uint32)))
            B["lm_allow"][slot].copy_(torch.from_numpy(bits.view(np.int32)).to(dev))
        B["lm_allow_on"][slot] = int(allowed is not None)
        if bias is not None:
            ids = sorted(bias)
            B["lm_bias_ids"][slot, :len(ids)].copy_(torch.tensor(ids, dtype=torch.int32).to(dev))
            B["lm_bias_val"][slot, :len(ids)].copy_(torch.tensor([bias[i] for i in ids], dtype=torch.float32).to(dev))
        B["lm_bias_n"][slot] = len(bias or ())
        if m:
            B["lm_end_ids"][slot, :len(ends)].copy_(torch.tensor(ends, dtype=torch.int32).to(dev))
        B["lm_end_n"][slot] = len(ends) if m else 0
        B["lm_min_tokens"][slot] = m

    def _request_masks(self, masks, n, max_new_tokens):
        """masks argument of generate_batch -> one checked dict or None per request"""
        per = list(masks) if isinstance(masks, (list, tuple)) else [masks] * n
        if len(per) != n:
            raise ValueError("masks: one value per request")
        for c in per:
            if c is not None:
                self.check_masks(**c, max_tokens=max_new_tokens)
        return per

    def set_logprobs(self, on):
        """Token logprobs on / off for every following selection.  On: each selection (decode steps, first tokens of every admission
        path) is followed by chatts_decoder_logprobs into the per-slot rings - log_softmax of the raw logits, the chosen token's rank and
        the max_logprobs best alternatives.  A switch drops the captured decode graphs (like a sampling-mode change); off, the steps are
        exactly what they are without the feature.  generate_one / generate_batch switch it on when asked and leave it on; the engine
        switches it off after greedy_return_steps iterations without a requester."""
        on = bool(on)
        if on == self._logprobs_on:
            return
        if on and self.plan.world > 1 and self._tp is None and self.max_batch > 1:
            raise NotImplementedError("logprobs under tensor parallelism need the peer-to-peer exchange (use_p2p=True) for batched decode")
        if on:
            self._logprob_rings()
        self._logprobs_on = on
        self._drop_graphs()

    def _logprob_rings(self):
        if "lp" not in self.buf:
            B, dev, n = self.buf, self.device, max(1, self.max_batch)
            S, K = B["out_tokens_all"].shape[1], self.max_logprobs
            B["lp"] = torch.full((n, S), float("nan"), dtype=torch.float32, device=dev)
            B["lp_rank"] = torch.zeros((n, S), dtype=torch.int32, device=dev)
            B["lp_top_ids"] = torch.full((n, S, max(K, 1)), -1, dtype=torch.int32, device=dev)
            B["lp_top_lp"] = torch.full((n, S, max(K, 1)), float("nan"), dtype=torch.float32, device=dev)
        B = self.buf
        return {"lp": B["lp"], "rank": B["lp_rank"], "top_ids": B["lp_top_ids"], "top_lp": B["lp_top_lp"], "stride": B["lp"].shape[1]}

    def _logprobs_after(self, logits, batch, slot):
        """(logprobs on) the cells of the tokens the selection just wrote for slots slot .. slot + batch - 1"""
        if not self._logprobs_on:
            return
        B, R = self.buf, self._logprob_rings()
        S, K = R["stride"], self.max_logprobs
        _lib.check(self.lib.chatts_decoder_logprobs(
            self._decoder, _lib.ptr(logits), batch, self.plan.vocab, K, B["token_all"][slot:].data_ptr(), B["step_all"][slot:].data_ptr(),
            S, R["lp"][slot:].data_ptr(), R["rank"][slot:].data_ptr(), R["top_ids"][slot:].data_ptr(), R["top_lp"][slot:].data_ptr(),
            _lib.stream_ptr()))

    def read_logprobs(self, slot, start, stop, k):
        """Host entries of cells [start, stop) of a slot: one (logprob, rank, [(id, logprob)] * k) per generated token."""
        k = int(k)
        if not self._logprobs_on and "lp" not in self.buf:
            raise RuntimeError("logprobs were not turned on (set_logprobs)")
        if stop <= start:
            return []
        if k > self.max_logprobs:
            raise ValueError(f"logprobs={k} exceeds max_logprobs={self.max_logprobs}")
        R = self._logprob_rings()
        lp = R["lp"][slot, start:stop].tolist()
        rank = R["rank"][slot, start:stop].tolist()
        ids = R["top_ids"][slot, start:stop, :k].tolist() if k else [[] for _ in lp]
        tlp = R["top_lp"][slot, start:stop, :k].tolist() if k else [[] for _ in lp]
        return [(a, b, list(zip(i, v))) for a, b, i, v in zip(lp, rank, ids, tlp)]

    def _select_token(self):
        """logits of this rank -> next token in B['token'] (appended to out_tokens, step bumped) on every rank: greedy or the
        configured sampler, agreed across TP ranks by chatts_decoder_select_tokens ((max, idx) pairs / gathered logits)."""
        if self.plan.world == 1 or self._tp is not None:
            self._select_one(0, 0, None)
            return
        if self._controls_on:
            raise NotImplementedError("logit controls are not available on the host-driven tensor-parallel path (use_p2p=False)")
        if self._masks_on:
            raise NotImplementedError("logit_bias / allowed_token_ids / min_tokens are not available on the host-driven tensor-parallel "
                                      "path (use_p2p=False)")
        lib, st, B = self.lib, _lib.stream_ptr(), self.buf
        self._select_token_host_tp()
        if self._logprobs_on:     # every rank: the same kernel on the same gathered logits
            full = self.comm.all_gather_cat(B["logits"])
            R = self._logprob_rings()
            _lib.check(lib.chatts_logprobs_batched(_lib.ptr(full), 1, full.numel(), full.numel(), 0, self.max_logprobs,
                                                   _lib.ptr(B["token"]), _lib.ptr(B["step"]), R["stride"], _lib.ptr(R["lp"]),
                                                   _lib.ptr(R["rank"]), _lib.ptr(R["top_ids"]), _lib.ptr(R["top_lp"]),
                                                   _lib.ptr(B["ws"]), B["ws"].numel(), st))

    def _select_one(self, slot, out_stride, sampling):
        """chatts_decoder_select_tokens on the logits of one row -> the sequence in cache slot `slot` (+ its logprobs).
        sampling: SamplingArgs for this call, None = the decoder's own setting."""
        B = self.buf
        sa = None if sampling is None else C.byref(sampling)
        if self._masks_on:             # this single-row call sees row 0: hand it the slot's settings (and state)
            lm, lc = self._mask_args(slot), self._control_args(slot) if self._controls_on else None
            _lib.check(self.lib.chatts_decoder_select_tokens_masked(
                self._decoder, _lib.ptr(B["logits"]), 1, self.plan.vocab, B["token_all"][slot:].data_ptr(),
                B["token_logit_all"][slot:].data_ptr(), B["out_tokens_all"][slot].data_ptr(), out_stride,
                B["step_all"][slot:].data_ptr(), None, 0, sa, None if lc is None else C.byref(lc), C.byref(lm), _lib.stream_ptr()))
        elif self._controls_on:        # this single-row call sees row 0: hand it the slot's state and settings
            lc = self._control_args(slot)
            _lib.check(self.lib.chatts_decoder_select_tokens_controlled(
                self._decoder, _lib.ptr(B["logits"]), 1, self.plan.vocab, B["token_all"][slot:].data_ptr(),
                B["token_logit_all"][slot:].data_ptr(), B["out_tokens_all"][slot].data_ptr(), out_stride,
                B["step_all"][slot:].data_ptr(), None, 0, sa, C.byref(lc), _lib.stream_ptr()))
        else:
            _lib.check(self.lib.chatts_decoder_select_tokens(
                self._decoder, _lib.ptr(B["logits"]), 1, self.plan.vocab, B["token_all"][slot:].data_ptr(),
                B["token_logit_all"][slot:].data_ptr(), B["out_tokens_all"][slot].data_ptr(), out_stride,
                B["step_all"][slot:].data_ptr(), None, 0, sa, _lib.stream_ptr()))
        self._logprobs_after(B["logits"], 1, slot)

    def _select_token_host_tp(self):
        lib, st, B = self.lib, _lib.stream_ptr(), self.buf
        # TP without the peer-to-peer exchange (use_p2p=False): host-driven RCCL gathers
        sa = getattr(self, "_sampling", None)
        if sa is None:      # greedy: one (logit, index) pair per rank instead of the [V / W] logits
            _lib.check(lib.chatts_argmax(_lib.ptr(B["logits"]), self.plan.vocab, self.plan.v0, _lib.ptr(B["token"]),
                                         _lib.ptr(B["token_logit"]), None, None, None, st))
            B["token"].copy_(self.comm.argmax_pair(B["token_logit"], B["token"]))
            B["out_tokens"].index_copy_(0, B["step"].to(torch.int64), B["token"])
            B["step"] += 1
            return
        full = self.comm.all_gather_cat(B["logits"])     # every rank draws from the full logits with the same seed
        _lib.check(lib.chatts_sample_batched(_lib.ptr(full), 1, full.numel(), full.numel(), 0, C.byref(sa),
                                             _lib.ptr(B["token"]), _lib.ptr(B["token_logit"]), _lib.ptr(B["out_tokens"]), 0,
                                             _lib.ptr(B["step"]), None, 0, st))

    def _first_token(self, last_rows):
        """logits of the last prompt row -> first generated token -> next input embedding in x[0]."""
        _lib.check(self.lib.chatts_decoder_logits(self._decoder, last_rows - 1, _lib.stream_ptr()))
        self._select_token()
        self._load_token_embedding()

    def _load_token_embedding(self):
        B = self.buf
        _lib.check(self.lib.chatts_embed_token(_lib.ptr(B["token"]), _lib.ptr(self._tensors["embed"]), 0,
                                               self.config.vocab_size, self.config.hidden_size, _lib.ptr(B["x"]),
                                               _lib.stream_ptr()))

    def _decode_step_eager(self):
        lib, st, B = self.lib, _lib.stream_ptr(), self.buf
        if self.plan.world == 1 or self._tp is not None:         # one C call enqueues the whole (TP) step
            _lib.check(lib.chatts_decoder_decode_step(self._decoder, _lib.ptr(B["pos"]), _lib.ptr(B["step"]),
                                                      _lib.ptr(B["token"]), _lib.ptr(B["token_logit"]),
                                                      _lib.ptr(B["out_tokens"]), self.n_splits, st))
            self._logprobs_after(B["logits"], 1, 0)
            return
        self._run_layers(1, 0, pos_dev=B["pos"], n_splits=self.n_splits)
        _lib.check(lib.chatts_decoder_logits(self._decoder, 0, st))
        B["pos"] += 1
        self._select_token()
        self._load_token_embedding()

    def decode_step(self):
        """One token.  A hipGraph of the whole step (captured on first use) is replayed - under tensor parallelism too, when the
        peer-to-peer exchange is attached (its collectives are ordinary kernels with device-resident epochs).  A request that was
        admitted for speculative decoding (speculative_config) takes the speculative step instead: 1 .. k + 1 tokens."""
        if self._spec_active:
            if self._spec_allowed():
                return self._spec_decode_step()
            self._spec_active = False            # a sampler / logprobs / controls were switched on under the request: plain steps from here,
            self._load_token_embedding()         # which start from the current token's embedding in x[0]
        if self.graph_capturable():
            if self._graph is None:
                self._capture()
            self._graph.replay()
        else:
            self._decode_step_eager()

    def graph_capturable(self):
        return bool(self.use_graph and (self.plan.world == 1 or self._tp is not None))

    def _capture(self, warm=True):
        """Capture one decode step.  warm: run one eager step first (populates every lazy host-side cache; under tensor
        parallelism all ranks do, so it really exchanges) and restore the state; capturing itself executes nothing."""
        self._graph = self._capture_graph(self._decode_step_eager, ("pos", "step", "token", "token_logit", "x", "out_tokens"), warm)

    def _capture_graph(self, step_fn, keys, warm=True):
        """-> a graph of step_fn(); the buffers `keys` (the decode-loop state step_fn advances) are left as they were."""
        B = self.buf
        if self._controls_on:
            keys = tuple(keys) + ("lc_state",)      # the selection counts its tokens into the state
        saved = {k: B[k].clone() for k in keys}
        torch.cuda.synchronize()
        if warm:
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                step_fn()
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            for k, v in saved.items():
                B[k].copy_(v)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            step_fn()
        torch.cuda.synchronize()
        for k, v in saved.items():          # capture does not execute, but keep the state pristine anyway
            B[k].copy_(v)
        return g

    def _drop_graphs(self):
        """forget the captured decode steps: the next one captures again (after a change of what a step launches)"""
        self._graph = None
        self._graph_batched = None
        self._spec_graphs = {}

    # ---------------------------------------------------------------------------------------------
    # speculative decoding by prompt lookup (csrc/spec_decode.hip, chatts_decoder_spec_step; greedy, one sequence, TP = 1)
    # ---------------------------------------------------------------------------------------------
    def _spec_buffers(self):
        """device state of the speculative step, allocated on first use: token history, drafts, the rows' logits, counters"""
        B = self.buf
        if "spec_hist" not in B:
            dev, R = self.device, _lib.SPEC_MAX_ROWS
            B["spec_hist"] = torch.zeros(self.max_ctx, dtype=torch.int32, device=dev)
            B["spec_draft"] = torch.full((R - 1,), -1, dtype=torch.int32, device=dev)
            B["spec_tokens"] = torch.zeros(R, dtype=torch.int64, device=dev)
            B["spec_argmax"] = torch.zeros(R, dtype=torch.int64, device=dev)
            B["spec_logits"] = torch.zeros((R, self.plan.vocab), dtype=torch.float32, device=dev)
            B["spec_cap"] = torch.zeros(1, dtype=torch.int32, device=dev)
            B["spec_counters"] = torch.zeros(4, dtype=torch.int64, device=dev)
        return B

    def _spec_allowed(self):
        """may the selected sequence take the speculative step now?  Greedy, no logit controls, no logit masks, no logprobs, one
        sequence, TP = 1."""
        return (self.plan.world == 1 and self.max_batch == 1 and getattr(self, "_sampling_key", None) is None
                and not self._controls_on and not self._masks_on and not self._logprobs_on)

    def _spec_config_for(self, T, max_new_tokens):
        """-> the speculative configuration the request of T prompt positions will run with, or None (plain steps)"""
        cfg = self._spec_call or self._spec_cfg
        if cfg is None or not self._spec_allowed():
            return None
        R = cfg["k"] + 1
        if T + max_new_tokens + cfg["k"] > self.max_ctx or R > self.t_max:     # the k + 1 rows of a step must fit behind the last token
            return None
        if self._spec_cfg is None and self.buf["ws"].numel() < self._spec_workspace_bytes():
            # per-call configuration on a model whose workspace was sized without the feature and cannot hold a step's scratch
            import warnings
            warnings.warn("prompt_lookup_num_tokens is ignored: this model's workspace was sized without speculative decoding and is too "
                          "small for it; build the model with speculative_config=... to use it")
            return None
        return cfg

    def spec_reserve(self, T, max_new_tokens):
        """KV positions a request of T prompt positions needs BEYOND T + max_new_tokens: the k rows a speculative step writes past the
        last token when the request would speculate under the model's own configuration, else 0 (the engine's pool gate asks)"""
        if self._spec_cfg is None or not self._spec_allowed():
            return 0
        k = self._spec_cfg["k"]
        return k if T + max_new_tokens + k <= self.max_ctx and k + 1 <= self.t_max else 0

    def _spec_begin(self, cfg, full, T, max_new_tokens):
        """after the prefill and the first token of a request: its history and output capacity go to the device"""
        B = self._spec_buffers()
        B["spec_hist"][:T].copy_(torch.tensor(full, dtype=torch.int32))
        B["spec_hist"][T:T + 1].copy_(B["token"])
        B["spec_cap"].fill_(int(max_new_tokens))
        self._spec_now = cfg
        self._spec_active = self._spec_request = True

    def _spec_args(self, cfg, skip_propose):
        B = self._spec_buffers()
        return _lib.SpecArgs(k=cfg["k"], ngram_min=cfg["ngram_min"], ngram_max=cfg["ngram_max"], n_splits=self.n_splits,
                             skip_propose=int(skip_propose), hist=_lib.ptr(B["spec_hist"]), draft=_lib.ptr(B["spec_draft"]),
                             spec_tokens=_lib.ptr(B["spec_tokens"]), argmax=_lib.ptr(B["spec_argmax"]), logits=_lib.ptr(B["spec_logits"]),
                             pos_dev=_lib.ptr(B["pos"]), step_dev=_lib.ptr(B["step"]), token_dev=_lib.ptr(B["token"]),
                             out_tokens=_lib.ptr(B["out_tokens"]), out_capacity_dev=_lib.ptr(B["spec_cap"]),
                             counters=_lib.ptr(B["spec_counters"]))

    def _spec_propose(self):
        """The proposer on its own (chatts_spec_propose): drafts and the step's input tokens from the sequence's history.  The eager
        step calls it through this method, so a test can put another proposer in its place."""
        B, cfg = self._spec_buffers(), self._spec_now
        _lib.check(self.lib.chatts_spec_propose(_lib.ptr(B["pos"]), _lib.ptr(B["spec_hist"]), self.max_ctx, cfg["k"], cfg["ngram_min"],
                                                cfg["ngram_max"], self.config.vocab_size, _lib.ptr(B["spec_draft"]),
                                                _lib.ptr(B["spec_tokens"]), _lib.stream_ptr()))

    def _spec_step_eager(self, propose_in_step=False):
        """propose_in_step: chatts_decoder_spec_step launches the proposer itself (skip_propose = 0) instead of this object's
        _spec_propose: the same kernel on the same buffers"""
        if not propose_in_step:
            self._spec_propose()
        args = self._spec_args(self._spec_now, not propose_in_step)
        _lib.check(self.lib.chatts_decoder_spec_step(self._decoder, C.byref(args), _lib.stream_ptr()))

    def _spec_decode_step(self):
        """One speculative step of the running request: the captured graph of (propose, R-row pass, argmax, verify), or the same
        launches eagerly (use_graph=False)."""
        if not self.graph_capturable():
            return self._spec_step_eager()
        cfg = self._spec_now
        key = (cfg["k"], cfg["ngram_min"], cfg["ngram_max"])
        g = self._spec_graphs.get(key)
        if g is None:
            keys = ("pos", "step", "token", "out_tokens", "x", "spec_hist", "spec_draft", "spec_tokens", "spec_counters")
            g = self._spec_graphs[key] = self._capture_graph(self._spec_step_eager, keys)
        g.replay()

    def _spec_produced(self, produced, limit):
        """host token count of the running request at a sync point: with speculative steps the count kept by the host (one per
        step) is a lower bound and the device's step counter is the truth; never more than `limit` (max_new_tokens)"""
        if not self._spec_request:
            return produced
        return min(max(produced, int(self.buf["step"][0])), limit)

    @property
    def spec_stats(self):
        """speculative decoding counters since the model was built (or spec_stats_reset): steps, drafted (valid draft tokens),
        accepted (drafts that were emitted), emitted (tokens the speculative steps produced)"""
        if "spec_counters" not in self.buf:
            return {"steps": 0, "drafted": 0, "accepted": 0, "emitted": 0}
        return dict(zip(("steps", "drafted", "accepted", "emitted"), self.buf["spec_counters"].tolist()))

    def spec_stats_reset(self):
        if "spec_counters" in self.buf:
            self.buf["spec_counters"].zero_()

    # ---------------------------------------------------------------------------------------------
    # batched decode / continuous batching (TP = 1)
    # ---------------------------------------------------------------------------------------------
    def select_sequence(self, slot):
        _lib.check(self.lib.chatts_decoder_select_sequence(self._decoder, int(slot)))
        self._cur_slot = int(slot)

    def _n_splits_batched(self):
        """16-key slots per sequence of the batched decode attention: with many sequences in flight the grid is full anyway and
        fewer, longer slots save partials traffic (round 2, B = 16 at ctx 0.8k: 64 -> 8 slots, 7.10 -> 6.91 ms per step; round 3, with
        the next tile prefetched under the current one and ctx 1.2k: 16 slots, profiles/r3_cfg5_nsplits_sweep.txt)."""
        import os
        forced = int(os.environ.get("CHATTS_BATCH_NSPLITS", "0") or 0)          # tuning only
        if forced > 0:
            return max(1, min(self.n_splits, forced))
        if self.max_batch <= 4:
            return self.n_splits
        return max(1, min(self.n_splits, max(16, 256 // self.max_batch)))      # (B = 16 at ctx 1.2k: 8 -> 16 slots, 7.83 -> 7.01 ms per step)

    def _batched_step_eager(self):
        B = self.buf
        _lib.check(self.lib.chatts_decoder_decode_step_batched(
            self._decoder, self.max_batch, _lib.ptr(B["pos_all"]), _lib.ptr(B["step_all"]), _lib.ptr(B["token_all"]),
            _lib.ptr(B["token_logit_all"]), _lib.ptr(B["out_tokens_all"]), B["out_tokens_all"].shape[1],
            _lib.ptr(B["logits_all"]), self._n_splits_batched(), _lib.stream_ptr()))
        self._logprobs_after(B["logits_all"], self.max_batch, 0)

    def batched_step(self):
        """One greedy token for EVERY cache slot (idle slots compute harmlessly; their position saturates)."""
        if self.plan.world != 1 and self._tp is None:
            raise NotImplementedError("batched decode under tensor parallelism needs the peer-to-peer exchange (use_p2p=True)")
        if not self.use_graph:
            return self._batched_step_eager()
        if self._graph_batched is None:
            self._graph_batched = self._capture_graph(
                self._batched_step_eager, ("pos_all", "step_all", "token_all", "token_logit_all", "out_tokens_all"))
        self._graph_batched.replay()

    # ---- prefix reuse (policy: chatts_amd/prefix_cache.py) and request preparation ---------------------------------------
    def _patch_counts(self, lengths):
        """valid series lengths -> TS encoder patches (<ts> placeholders) per series"""
        ps = self.config.ts["patch_size"]
        return [(int(v) + ps - 1) // ps for v in lengths]

    def _request_idents(self, ids, series, lengths):
        """token identities of a request before it is admitted (slot choice): host-side only, no device work"""
        if not self.enable_prefix_caching:
            return None
        if series is not None and series.shape[0] > 0 and lengths is None:
            return None
        counts = self._patch_counts(lengths or [])
        try:
            full = self.expand_input_ids(list(ids), counts)
        except ValueError:
            return None
        return prefix_cache.token_idents(full, series, lengths, counts, self.config.ts_token_start_index)

    def _prepare_request(self, ids, series, lengths, max_new_tokens):
        """TS encoder, prompt expansion, embeddings and token identities of one request - what every admission path does before it
        touches a cache slot.  -> (T, emb [T, H], idents, series on the device, lengths) (series / lengths resolved: None lengths
        are measured on the device)."""
        mm, counts = None, []
        if series is not None and series.shape[0] > 0:
            series = series.to(self.device, dtype=torch.float32)
            if lengths is None:
                lengths = self.ts_encoder.get_patch_cnt(series)[0].tolist()
            counts = self._patch_counts(lengths)
            mm = self.get_multimodal_embeddings(timeseries=series, valid_lengths=lengths)
        full = self.expand_input_ids(list(ids), counts)
        T = len(full)
        if T + max_new_tokens > self.max_ctx:       # a sequence must never outgrow its cache
            raise ValueError(f"prompt ({T}) + max_new_tokens ({max_new_tokens}) exceeds max_ctx={self.max_ctx}")
        emb = self.get_input_embeddings(torch.tensor(full, dtype=torch.int64), mm)
        idents = prefix_cache.token_idents(full, series, lengths, counts, self.config.ts_token_start_index)
        return T, emb, idents, series, lengths

    def _reuse_prefix(self, slot, idents, T, exclude=()):
        """Longest prefix of `idents` already resident in some slot's cache -> copy those K/V rows into `slot` (nothing to copy
        when it is the slot itself) and return how many leading tokens need no prefill (at most T - 1: the last prompt
        position is always recomputed, it yields the logits)."""
        self.prefix_stats["requests"] += 1
        replaced = self._kv_replaced.pop(slot, set())      # (paged) blocks reserve_kv swapped for private, EMPTY ones
        if not self.enable_prefix_caching:
            return 0
        best, src = prefix_cache.match_prefix(self._slot_idents, idents, slot, exclude)
        n = min(best, T - 1)
        if n < prefix_cache.MIN_REUSE:
            return 0
        if self._kv is not None:
            # paged: nothing is copied.  Another slot's prefix is SHARED block by block (reference counted), so the reuse ends at a
            # block boundary; the slot's own prefix ends where reserve_kv had to swap a shared block for a private (empty) one.
            bs = self._kv.block_size
            if src != slot:
                nshare = n // bs
                if nshare == 0 or len(self._kv.rows[slot]) < nshare or len(self._kv.rows[src]) < nshare:
                    return 0                     # less than a block in common (or not reserved by the caller): recompute
                if self._kv.adopt(slot, src, nshare):
                    self._push_kv_row(slot)
                n = nshare * bs
            else:
                lost = [i for i in replaced if i * bs < n]
                if lost:
                    n = min(lost) * bs
                if n < prefix_cache.MIN_REUSE:
                    return 0
        elif src != slot:
            B = self.buf
            B["kv_k"][slot, :, :, :n].copy_(B["kv_k"][src, :, :, :n])
            B["kv_v"][slot, :, :, :n].copy_(B["kv_v"][src, :, :, :n])
        self.prefix_stats["hits"] += 1
        self.prefix_stats["tokens_reused"] += n
        return n

    def note_generated(self, slot, tokens):
        """After a request finished: its generated tokens (all but the last, which was never fed back) also have K/V rows in
        the slot - a follow-up turn that re-sends prompt + answer reuses them."""
        if self.enable_prefix_caching and tokens:
            self._slot_idents[slot] = self._slot_idents[slot] + [int(t) for t in tokens[:-1]]
        if self._kv is not None:
            self._kv.retire(slot)                # blocks stay resident for prefix reuse; evictable from now on

    def pick_slot(self, free_slots, idents=None):
        """Which free cache slot a new request should take: the one whose resident prefix matches best (zero copy), else the
        one whose resident tokens are least worth keeping (fewest)."""
        if not self.enable_prefix_caching or idents is None:
            return free_slots[0]
        return prefix_cache.pick_slot(self._slot_idents, free_slots, idents)

    def admit_begin(self, slot, ids, series, lengths, max_new_tokens=1):
        """First half of an admission into cache slot `slot`: TS encoder, prompt expansion, embeddings, KV reservation and prefix
        reuse - everything but the prefill itself.  -> the state admit_step() consumes."""
        T, emb, idents, _, _ = self._prepare_request(ids, series, lengths, max_new_tokens)
        self._controls_admit(slot, ids)
        self.reserve_kv(slot, T + max_new_tokens, idents)
        n0 = self._reuse_prefix(slot, idents, T)
        self._slot_idents[slot] = []                # not a prefix source for others until all of its rows exist
        self.prefix_stats["tokens_prefilled"] += T - n0
        return {"slot": slot, "emb": emb, "T": T, "done": n0, "idents": idents}

    def admit_step(self, st, max_rows=None):
        """Prefill the next <= max_rows prompt rows of an admission begun with admit_begin (all that is left when None).  Between two
        calls the engine may run decode steps of the OTHER slots (vLLM's chunked prefill: a long prompt does not stall the running
        sequences for its whole prefill); this slot stays parked until its last row is in, then its first token is produced.
        -> True when the admission is complete."""
        slot, T, a = st["slot"], st["T"], st["done"]
        b = T if max_rows is None else min(T, a + max(int(max_rows), 1))
        final = b >= T
        self.select_sequence(slot)
        last = self.prefill(st["emb"][a:b], a, for_next_token=final)
        st["done"] = b
        if final:
            if st.get("fork"):               # parallel sampling: every sibling's first token from this one logits row
                self._first_tokens_forked(slot, last - 1, T, st["fork"])
                for c in st["fork"]:
                    self._slot_idents[c] = list(st["idents"])
            else:
                self._first_token_into_slot(slot, last - 1, T)
            self._slot_idents[slot] = st["idents"]
            st["emb"] = None
        self.select_sequence(0)
        return final

    def _admit(self, slot, ids, series, lengths, max_new_tokens=1):
        """Prefill one request into cache slot `slot` and produce its first token (out_tokens_all[slot, 0])."""
        st = self.admit_begin(slot, ids, series, lengths, max_new_tokens)
        self.admit_step(st)
        return st["T"]

    def _first_token_into_slot(self, slot, row, T):
        """logits of x[row] -> first token of the sequence in cache slot `slot` (out_tokens_all[slot, 0]); position / step set."""
        _lib.check(self.lib.chatts_decoder_logits(self._decoder, row, _lib.stream_ptr()))
        self._select_first(slot, T)

    def _select_first(self, slot, T):
        """the logits buffer -> first token of the sequence in cache slot `slot`, whose prompt of T positions is in its cache"""
        B = self.buf
        B["pos_all"][slot] = T
        B["step_all"][slot] = 0
        sa = getattr(self, "_sampling", None)
        sa1 = None
        if getattr(self, "_sampling_key", None) == "rows":
            sa1 = self._rows_args(slot)          # this single-row call sees row 0: hand it the slot's entries
        elif sa is not None:   # the batched steps draw with (seed, slot, step); this single-row call would see slot 0: fold the slot into the seed
            sa1 = _lib.SamplingArgs(temperature=sa.temperature, top_k=sa.top_k, top_p=sa.top_p,
                                    seed=(sa.seed ^ (0x51ED27 * (slot + 1))) & 0xFFFFFFFF, n_kept=None, kept_mass=None)
        self._select_one(slot, B["out_tokens_all"].shape[1], sa1)

    # ---- fork: n samples of one prompt from ONE prefill (csrc/kv_fork.hip) ------------------------------------------------
    def fork_tokens(self, T, max_new_tokens):
        """KV positions a sibling has to reserve beside the prompt blocks it shares with the slot that is prefilled (kv_fits)"""
        shared = (T // self._kv.block_size) * self._kv.block_size if self._kv is not None else 0
        return T + max_new_tokens - shared

    def admit_fork(self, st, children, max_new_tokens=1):
        """Between admit_begin and admit_step of a request with n > 1: the free cache slots `children` become siblings of st's slot.
        Paged cache: each child gives up its row and reserves private blocks for everything from the trailing, partly filled prompt
        block on (children write position T next); the whole prompt blocks are shared with the parent's row by reference count once
        they are written (fork_slots).  When the pool cannot cover a child nothing stays reserved and KvPoolExhausted is raised.
        The sharing, the copies and the n first tokens follow the prefill (admit_step)."""
        children = [int(c) for c in children]
        slot, T = st["slot"], st["T"]
        if slot in children or len(set(children)) != len(children) or not all(0 <= c < self.max_batch for c in children):
            raise ValueError(f"fork: children {children} must be distinct cache slots other than {slot}")
        for c in children:
            self._slot_idents[c] = []
            self._kv_replaced.pop(c, None)
        if self._kv is not None:
            from .kv_blocks import KvPoolExhausted
            nshare = T // self._kv.block_size
            order = sorted(range(self.max_batch), key=lambda sl: len(self._slot_idents[sl]))
            made = []
            try:
                for c in children:
                    self._kv.release(c)
                    made.append(c)
                    self._kv.reserve(c, T + max_new_tokens - nshare * self._kv.block_size, protect={slot, *children}, evict_order=order,
                                     on_evict=self._kv_evicted)
            except KvPoolExhausted:
                for c in made:
                    self._kv.release(c)
                self._kv.retire(slot)
                n0 = st["done"]                      # the admission did not happen: take back what admit_begin counted for it
                self.prefix_stats["requests"] -= 1
                self.prefix_stats["hits"] -= int(n0 > 0)
                self.prefix_stats["tokens_reused"] -= n0
                self.prefix_stats["tokens_prefilled"] -= T - n0
                raise
        st["fork"] = children
        return st

    def fork_slots(self, src, dst, T):
        """Device side of the fork: K / V rows [0, T) of cache slot `src` reach the slots `dst` (paged: only the rows of the trailing
        prompt block - the whole blocks are shared through the tables), and with logit controls on the state row of `src` reaches their
        rows.  One launch each per CHATTS_FORK_MAX_DST destinations; stream-ordered after the prefill."""
        B, st = self.buf, _lib.stream_ptr()
        dst = [int(c) for c in dst]
        if self._kv is not None:                     # the prompt blocks are written: share the whole ones, table rows to the device
            for c in dst:
                self._kv.fork(c, int(src), T // self._kv.block_size)
                self._push_kv_row(c)
        kc = _lib.KvCache(k=B["kv_k"].data_ptr(), v=B["kv_v"].data_ptr(), max_ctx=self.max_ctx,
                          dtype=_lib.KV_F16 if self.kv_cache_dtype == torch.float16 else _lib.KV_F32,
                          block_table=_lib.ptr(B["kv_table"]), block_size=self.kv_block_size,
                          table_stride=(self.max_ctx // self.kv_block_size) if self.kv_block_size else 0)
        if self.kv_block_size:
            layer_stride, seq_stride, n_blocks = B["kv_k"].stride(0), 0, B["kv_k"].shape[1]
            t0 = T - T % self.kv_block_size
        else:
            layer_stride, seq_stride, n_blocks, t0 = B["kv_k"].stride(1), B["kv_k"].stride(0), 0, 0
        for i in range(0, len(dst), _lib.FORK_MAX_DST):
            part = dst[i:i + _lib.FORK_MAX_DST]
            arr = (C.c_int32 * len(part))(*part)
            _lib.check(self.lib.chatts_kv_fork(C.byref(kc), self.config.num_hidden_layers, self.plan.nkv, self.max_batch, layer_stride,
                                               seq_stride, n_blocks, int(src), arr, len(part), t0, T, st))
            if self._controls_on:
                V = B["lc_state"].shape[1]
                _lib.check(self.lib.chatts_logit_state_fork(B["lc_state"].data_ptr(), V, V, self.max_batch, int(src), arr, len(part), st))
        self.prefix_stats["forks"] = self.prefix_stats.get("forks", 0) + 1
        self.prefix_stats["fork_children"] = self.prefix_stats.get("fork_children", 0) + len(dst)

    def _first_tokens_forked(self, slot, row, T, children):
        """logits of x[row], ONCE -> fork -> the first token of `slot` and of every child, each drawn with its own slot's settings (and
        followed by its own logprobs / counted into its own state where those modes are on).  The decoder is not run again."""
        _lib.check(self.lib.chatts_decoder_logits(self._decoder, row, _lib.stream_ptr()))
        self.fork_slots(slot, children, T)           # (before the first selection counts its token into the source's state row)
        for s in [slot] + list(children):
            self._select_first(s, T)

    def plan_pack(self, candidates, free_slots):
        """Which of the waiting requests should be prefilled TOGETHER (chatts_decoder_prefill_packed).  candidates: list of
        (ids, series, lengths, max_new_tokens) in arrival order.  Greedy: take requests while their not-yet-cached rows fit the
        prefill buffers and slots are free; a request that shares most of its prompt with one already in the pack is left for the
        next round (it will then reuse that request's K/V rows instead of computing them again).  -> indices into candidates."""
        if self.plan.world != 1 or len(free_slots) < 2 or len(candidates) < 2:
            return []
        pack, rows, pack_idents = [], 0, []
        for i, (ids, series, lengths, max_new) in enumerate(candidates):
            if len(pack) >= len(free_slots):
                break
            idents = self._request_idents(ids, series, lengths)
            if idents is None:          # lengths unknown / prefix caching off: size by the expanded prompt alone
                try:
                    T = len(self.expand_input_ids(list(ids), self._patch_counts(lengths or [])))
                except ValueError:
                    continue
                need = T
            else:
                T = len(idents)
                n, _ = prefix_cache.match_prefix(self._slot_idents, idents, -1)
                n = min(n, T - 1)
                need = T - (n if n >= prefix_cache.MIN_REUSE else 0)
                if any(other is not None and prefix_cache.common_prefix_len(idents, other) >= max(prefix_cache.MIN_REUSE, T // 2)
                       for other in pack_idents):
                    continue
            if T + max_new > self.max_ctx or rows + need > self.t_max:
                continue
            pack.append(i)
            pack_idents.append(idents)
            rows += need
        return pack if len(pack) >= 2 else []

    def _admit_packed(self, items):
        """Prefill several requests in ONE packed pass.  items: list of (slot, ids, series, lengths, max_new_tokens) with distinct
        free slots whose uncached rows fit max_prefill_tokens together (plan_pack).  Returns the prompt lengths."""
        B = self.buf
        segs, embs, Ts, row, late = [], [], [], 0, []
        if self._kv_dynamic:        # oversubscribed block pool: reserve for EVERY member before anything changes, or for none
            from .kv_blocks import KvPoolExhausted
            newly, touched = [], []
            try:
                for slot, ids, series, lengths, max_new in items:
                    was_active = slot in self._kv.active
                    touched.append(slot)
                    self.reserve_kv(slot, self.request_tokens(ids, series, lengths) + max_new, self._request_idents(ids, series, lengths))
                    if not was_active:
                        newly.append(slot)
            except KvPoolExhausted:
                # roll back: the members reserved so far may already have had shared prefix blocks swapped for EMPTY private ones, so
                # what their slots advertise as resident is no longer true - forget it (a later request must not adopt those blocks)
                for sl in touched:
                    self._slot_idents[sl] = []
                    self._kv_replaced.pop(sl, None)
                for sl in newly:
                    self._kv.retire(sl)
                raise
        for slot, ids, series, lengths, max_new in items:
            T, emb, idents, series, lengths = self._prepare_request(ids, series, lengths, max_new)
            self._controls_admit(slot, ids)
            # reuse from ANY slot, the member's own and other members' included: every K/V row copy is enqueued here, i.e. before
            # the packed pass overwrites anything; a slot stops being a source once its member has been processed (idents cleared)
            self.reserve_kv(slot, T + max_new, idents)       # (dynamic pool: already covered by the pre-pass above)
            n0 = self._reuse_prefix(slot, idents, T)
            self._slot_idents[slot] = []
            if row + T - n0 > self.t_max:                    # an earlier member's copy took away the prefix this one counted on
                late.append((slot, ids, series, lengths, max_new))
                self.prefix_stats["requests"] -= 1
                self.prefix_stats["hits"] -= int(n0 > 0)
                self.prefix_stats["tokens_reused"] -= n0
                Ts.append(None)
                continue
            self.prefix_stats["tokens_prefilled"] += T - n0
            segs.append((row, T - n0, n0, slot, idents))
            embs.append(emb[n0:])
            Ts.append(T)
            row += T - n0
        if segs:
            B["x"][:row].copy_(torch.cat(embs, dim=0))
            arr = (_lib.PrefillSegment * len(segs))(*[_lib.PrefillSegment(row0=r0, t=t, pos0=p0, slot=sl) for r0, t, p0, sl, _ in segs])
            _lib.check(self.lib.chatts_decoder_prefill_packed(self._decoder, arr, len(segs), _lib.stream_ptr()))
            self.prefix_stats["packed_prefills"] = self.prefix_stats.get("packed_prefills", 0) + 1
            for r0, t, p0, sl, idents in segs:
                self._slot_idents[sl] = idents
                self._first_token_into_slot(sl, r0 + t - 1, p0 + t)
        for it in late:                                      # (rare) did not fit after all: the ordinary path
            Ts[Ts.index(None)] = self._admit(*it)
        return Ts

    @torch.no_grad()
    def generate_batch(self, requests, max_new_tokens=64, eos_token_id=None, sync_every=8, logprobs=None, controls=None, masks=None):
        """Continuous batching over `max_batch` cache slots.  requests: list of (ids, series [n,2Lmax,1] | None,
        lengths | None).  A finished sequence frees its slot for the next waiting request at the next sync point.
        Returns the list of generated token lists, in request order.  logprobs: k for every request, or a list with one k / None per
        request -> (token lists, entry lists) (entries as in generate_one; None for a request that did not ask).
        controls: None = the slots keep their logit controls (set_sampling / set_slot_controls); a dict of repetition_penalty /
        frequency_penalty / presence_penalty / min_p for every request, or a list with one dict / None (= the defaults) per request.
        masks: the same for logit_bias / allowed_token_ids / min_tokens (set_slot_masks; the ids min_tokens keeps away are eos_token_id)."""
        ctl = None if controls is None else self._request_controls(controls, len(requests))
        msk = None if masks is None else self._request_masks(masks, len(requests), max_new_tokens)
        ks = list(logprobs) if isinstance(logprobs, (list, tuple)) else [logprobs] * len(requests)
        if len(ks) != len(requests):
            raise ValueError("logprobs: one value per request")
        for k in ks:
            if k is not None:
                self._check_logprobs(k)
        want = any(k is not None for k in ks)
        if want:
            self.set_logprobs(True)
        if self.max_batch < 2:
            outs = [self.generate_one(i, s, l, max_new_tokens, eos_token_id, logprobs=k, controls=None if ctl is None else (ctl[j] or {}),
                                      masks=None if msk is None else (msk[j] or {}))
                    for j, ((i, s, l), k) in enumerate(zip(requests, ks))]
            if logprobs is None:
                return outs
            return [o[0] if k is not None else o for o, k in zip(outs, ks)], [o[1] if k is not None else None for o, k in zip(outs, ks)]
        eos = _eos_set(eos_token_id)
        B = self.buf
        results = [None] * len(requests)
        entries = [None] * len(requests)
        waiting = list(range(len(requests)))[::-1]
        slots = [None] * self.max_batch              # request index per slot
        produced = [0] * self.max_batch
        B["pos_all"].fill_(-1); B["step_all"].zero_(); B["token_all"].zero_()
        steps_since_sync = 0

        def harvest(final=False):
            toks_all = B["out_tokens_all"].cpu()
            self._check_exchange()
            for s, r in enumerate(slots):
                if r is None:
                    continue
                toks = toks_all[s, :produced[s]].tolist()
                cut = _eos_end(toks, eos)
                if cut is not None or produced[s] >= max_new_tokens or final:
                    results[r] = toks[:cut] if cut is not None else toks[:max_new_tokens]
                    if ks[r] is not None:
                        entries[r] = self.read_logprobs(s, 0, len(results[r]), ks[r])
                    slots[s] = None
                    B["pos_all"][s] = -1         # parked: the batched step neither attends nor writes this slot's cache
                    self.note_generated(s, results[r])

        while waiting or any(r is not None for r in slots):
            while waiting and any(v is None for v in slots):
                free = [i for i, v in enumerate(slots) if v is None]
                cands = waiting[::-1][:len(free)]            # the next requests in arrival order
                pack = self.plan_pack([requests[r] + (max_new_tokens,) for r in cands], free)
                if pack and self._kv_dynamic and not self.kv_fits(
                        [self.request_tokens(*requests[cands[j]]) + max_new_tokens for j in pack]):
                    pack = []                                # the block pool cannot take them all at once: one at a time
                if pack:                                     # several short prompts: one packed prefill pass
                    items, members = [], []
                    for j in pack:
                        r = cands[j]
                        ids, series, lengths = requests[r]
                        s = self.pick_slot(free, self._request_idents(ids, series, lengths))
                        free.remove(s)
                        if ctl is not None:
                            self.set_slot_controls(s, **(ctl[r] or {}))
                        if msk is not None:
                            self.set_slot_masks(s, **(msk[r] or {}), end_ids=_eos_set(eos_token_id))
                        items.append((s, ids, series, lengths, max_new_tokens))
                        members.append((s, r))
                    try:
                        self._admit_packed(items)
                    except RuntimeError as e:                # the pool could not cover the pack after all (a protected prefix
                        if type(e).__name__ != "KvPoolExhausted" or all(v is None for v in slots):     # source): the touched slots forgot their resident prefixes
                            raise
                        break
                    for s, r in members:
                        slots[s], produced[s] = r, 1
                        waiting.remove(r)
                    continue
                ids, series, lengths = requests[waiting[-1]]
                if self._kv_dynamic and not self.kv_fits([self.request_tokens(ids, series, lengths) + max_new_tokens]):
                    if all(v is None for v in slots):        # nothing left to finish and free blocks: it can never fit
                        from .kv_blocks import KvPoolExhausted
                        raise KvPoolExhausted(f"request {waiting[-1]} needs more KV blocks than the pool holds ({self.kv_stats()})")
                    break                                    # wait until a running sequence finishes and its blocks become evictable
                s = self.pick_slot(free, self._request_idents(ids, series, lengths))
                if ctl is not None:
                    self.set_slot_controls(s, **(ctl[waiting[-1]] or {}))
                if msk is not None:
                    self.set_slot_masks(s, **(msk[waiting[-1]] or {}), end_ids=_eos_set(eos_token_id))
                try:
                    self._admit(s, ids, series, lengths, max_new_tokens)
                except RuntimeError as e:                    # (the reservation is _admit's first change: nothing to undo)
                    if type(e).__name__ != "KvPoolExhausted" or all(v is None for v in slots):
                        raise
                    break
                r = waiting.pop()
                slots[s], produced[s] = r, 1
            if all(r is None or produced[s] >= max_new_tokens for s, r in enumerate(slots)):
                harvest()
                continue
            self.batched_step()
            for s, r in enumerate(slots):
                if r is not None and produced[s] < max_new_tokens:
                    produced[s] += 1
            steps_since_sync += 1
            if steps_since_sync >= sync_every or all(r is None or produced[s] >= max_new_tokens for s, r in enumerate(slots)):
                harvest()
                steps_since_sync = 0
        return (results, entries) if logprobs is not None else results

    # ---------------------------------------------------------------------------------------------
    # HF surface
    # ---------------------------------------------------------------------------------------------
    def expand_input_ids(self, ids, patch_counts):
        """Replace each [<ts>, <ts/>] pair by patch_cnt <ts> placeholders (chatts_vllm.py:402-415, 441)."""
        ts0 = self.config.ts_token_start_index
        out, k, i, n = [], 0, 0, len(ids)
        while i < n:
            if ids[i] == ts0 and i + 1 < n and ids[i + 1] == ts0 + 1:
                if k >= len(patch_counts):
                    raise ValueError("more <ts><ts/> pairs than time series")
                out.extend([ts0] * int(patch_counts[k]))
                k += 1
                i += 2
            else:
                out.append(ids[i])
                i += 1
        if k != len(patch_counts):
            raise ValueError(f"{len(patch_counts)} time series but {k} <ts><ts/> pairs in the prompt")
        return out

    @torch.no_grad()
    def generate_one(self, ids, series=None, lengths=None, max_new_tokens=64, eos_token_id=None, sync_every=16,
                     return_logits=False, logprobs=None, controls=None, masks=None):
        """ids: un-expanded prompt ids (host list); series: [n, 2*Lmax, 1] tensor of this prompt's series.
        logprobs=k (0 <= k <= max_logprobs): also return one (logprob, rank, top-k [(id, logprob)]) entry per returned token, last in
        the result tuple (toks[, logits0], entries).  controls: None = slot 0 keeps its logit controls; a dict of repetition_penalty /
        frequency_penalty / presence_penalty / min_p (missing = default) sets them for this request.  masks: the same for logit_bias /
        allowed_token_ids / min_tokens (set_slot_masks; the ids min_tokens keeps away are eos_token_id)."""
        if controls is not None:
            self.set_slot_controls(0, **controls)
        if masks is not None:
            self.check_masks(**masks, max_tokens=max_new_tokens)
            self.set_slot_masks(0, **masks, end_ids=_eos_set(eos_token_id))
        if logprobs is not None:
            self._check_logprobs(logprobs)
            self.set_logprobs(True)
        self._prefill_request(ids, series, lengths, max_new_tokens)
        logits0 = self.buf["logits"].clone() if return_logits else None
        eos = _eos_set(eos_token_id)
        produced = 1
        toks = None
        steps = 1
        most = 1                     # speculative request: upper bound of the tokens on the device (a step emits at most k + 1)
        while produced < max_new_tokens:
            self.decode_step()
            produced += 1
            steps += 1
            if self._spec_request:
                # a speculative step emits 1 .. k + 1 tokens: ask the device at the usual sync points, and whenever the request MAY be
                # complete - a step launched after the last token would be a whole pass over the weights for nothing
                most += self._spec_now["k"] + 1
                if steps % sync_every == 0 or most >= max_new_tokens:
                    produced = most = self._spec_produced(produced, max_new_tokens)
            if eos and (steps % sync_every == 0):
                toks = self.buf["out_tokens"][:produced].tolist()
                if any(t in eos for t in toks):
                    break
        produced = self._spec_produced(produced, max_new_tokens)
        toks = self.buf["out_tokens"][:produced].tolist()
        self._check_exchange()
        toks = toks[:_eos_end(toks, eos)]
        self.note_generated(0, toks)
        out = (toks,) + ((logits0,) if return_logits else ()) + ((self.read_logprobs(0, 0, len(toks), logprobs),) if logprobs is not None else ())
        return out[0] if len(out) == 1 else out

    def _check_exchange(self):
        """TP: the tokens read since the last check are invalid if the peer-to-peer exchange timed out meanwhile"""
        if self._tp is not None and self._tp.status():
            raise RuntimeError("tensor-parallel exchange timed out (a peer rank did not reach the collective): tokens are invalid")

    def _check_logprobs(self, k):
        if isinstance(k, bool) or not isinstance(k, int) or not 0 <= k <= self.max_logprobs:
            raise ValueError(f"logprobs={k!r} must be an integer in 0..max_logprobs={self.max_logprobs}")

    @torch.no_grad()
    def generate_stream(self, ids, series=None, lengths=None, max_new_tokens=64, eos_token_id=None, chunk=1, controls=None, masks=None):
        """Generator over the new tokens of ONE request: yields a list of token ids every `chunk` decode steps (chunk=1: token by
        token, what an SSE stream / HF TextStreamer consumes; each yield costs one device->host read of the tokens so far).
        Stops after an EOS token (which is yielded) or max_new_tokens.  Same kernels and tokens as generate_one (controls too)."""
        if controls is not None:
            self.set_slot_controls(0, **controls)
        if masks is not None:
            self.check_masks(**masks, max_tokens=max_new_tokens)
            self.set_slot_masks(0, **masks, end_ids=_eos_set(eos_token_id))
        eos = _eos_set(eos_token_id)
        self._prefill_request(ids, series, lengths, max_new_tokens)
        produced, sent = 1, 0
        while True:
            if produced - sent >= chunk or produced >= max_new_tokens:
                produced = self._spec_produced(produced, max_new_tokens)
                toks = self.buf["out_tokens"][sent:produced].tolist()
                self._check_exchange()
                end = _eos_end(toks, eos)
                if end is not None:
                    yield toks[:end]
                    return
                yield toks
                sent = produced
            if produced >= max_new_tokens:
                return
            self.decode_step()
            produced += 1

    def _prefill_request(self, ids, series, lengths, max_new_tokens):
        """TS encode + merge + prefill + first token of one request on the single-sequence path -> prompt length T."""
        T, emb, idents, _, lengths = self._prepare_request(ids, series, lengths, max_new_tokens)
        self._spec_active = self._spec_request = False
        spec = self._spec_config_for(T, max_new_tokens) if (self._spec_cfg or self._spec_call) else None
        self._controls_admit(0, ids)
        self.reserve_kv(0, T + max_new_tokens + (spec["k"] if spec else 0), idents)     # (a speculative step writes k rows past the token)
        n0 = self._reuse_prefix(0, idents, T)
        self._slot_idents[0] = idents
        self.prefix_stats["tokens_prefilled"] += T - n0
        self.reset()
        last = self.prefill(emb[n0:], n0, for_next_token=True)
        self.buf["pos"].fill_(T)
        self._first_token(last)
        if spec:
            self._spec_begin(spec, self.expand_input_ids(list(ids), self._patch_counts(lengths or [])), T, max_new_tokens)
        return T

    @torch.no_grad()
    def generate(self, input_ids=None, attention_mask=None, timeseries=None, max_new_tokens=64, max_length=None,
                 streamer=None, eos_token_id=None, do_sample=False, temperature=None, top_k=None, top_p=None,
                 seed=0, synced_gpus=False, valid_lengths=None, repetition_penalty=None, min_p=None, prompt_lookup_num_tokens=None,
                 max_matching_ngram_size=None, min_new_tokens=None, **kw):
        """model.generate(**inputs, max_new_tokens=...) -> LongTensor [B, T_in + new] (README.md:102, demo_hf.ipynb
        cell 5).  Greedy unless do_sample=True, like HF; with do_sample the HF GenerationConfig defaults apply to what is
        not given (temperature 1.0, top_k 50, top_p 1.0; the reference's deepspeed driver passes temperature=0.2,
        inference_tsmllm_deepspeed.py:95-100).  Rows start with the un-expanded input_ids; shorter rows are
        right-padded with pad_token_id.  A flat `timeseries` tensor is consumed across the batch in prompt order.
        repetition_penalty and min_p have HF's meaning: the penalty applies with and without do_sample, min_p only with it.
        prompt_lookup_num_tokens=k (HF's name; max_matching_ngram_size=n, default 2 like HF): prompt-lookup speculative decoding for
        THIS call, when it is greedy, has no repetition penalty and no min_new_tokens; otherwise the two are ignored with a warning.
        min_new_tokens=k has HF's meaning (no EOS token among the first k new tokens): min_tokens of set_slot_masks."""
        self._spec_call = None
        if min_new_tokens is not None and (isinstance(min_new_tokens, bool) or not isinstance(min_new_tokens, int) or min_new_tokens < 0):
            raise ValueError(f"min_new_tokens must be an integer >= 0, got {min_new_tokens!r}")
        if not min_new_tokens:
            self.set_logit_masks(False)              # per call, like the sampling mode: a plain call runs the plain selection
        if prompt_lookup_num_tokens is not None:
            greedy = not do_sample and (repetition_penalty is None or float(repetition_penalty) == 1.0) and not min_new_tokens
            call = parse_speculative_config({"method": "ngram", "num_speculative_tokens": prompt_lookup_num_tokens,
                                             "prompt_lookup_max": 2 if max_matching_ngram_size is None else max_matching_ngram_size,
                                             "prompt_lookup_min": 1}, self.plan.world, self.max_batch)
            if greedy:
                self._spec_call = call
            else:
                import warnings
                warnings.warn("prompt_lookup_num_tokens is ignored: speculative decoding serves greedy requests without a repetition "
                              "penalty and without min_new_tokens only")
        try:
            return self._generate(input_ids, attention_mask, timeseries, max_new_tokens, max_length, streamer, eos_token_id, do_sample,
                                  temperature, top_k, top_p, seed, valid_lengths, repetition_penalty, min_p, min_new_tokens)
        finally:
            self._spec_call = None

    def _generate(self, input_ids, attention_mask, timeseries, max_new_tokens, max_length, streamer, eos_token_id, do_sample,
                  temperature, top_k, top_p, seed, valid_lengths, repetition_penalty, min_p, min_new_tokens=None):
        if do_sample:
            self.set_sampling(1.0 if temperature is None else temperature, 50 if top_k is None else top_k,
                              1.0 if top_p is None else top_p, seed, repetition_penalty=1.0 if repetition_penalty is None else repetition_penalty,
                              min_p=min_p)
        else:
            self.set_sampling(0.0, repetition_penalty=1.0 if repetition_penalty is None else repetition_penalty)
        cfg = self.config
        ids = input_ids if isinstance(input_ids, torch.Tensor) else torch.tensor(input_ids)
        if ids.dim() == 1:
            ids = ids[None]
        ids = ids.cpu()
        mask = attention_mask.cpu() if attention_mask is not None else torch.ones_like(ids)
        if eos_token_id is None:
            eos_token_id = cfg.eos_token_id
        ts0 = cfg.ts_token_start_index
        cursor, rows, reqs = 0, [], []
        for b in range(ids.shape[0]):
            seq = ids[b][mask[b].bool()].tolist()
            n_ts = sum(1 for i in range(len(seq) - 1) if seq[i] == ts0 and seq[i + 1] == ts0 + 1)
            ser = timeseries[cursor:cursor + n_ts] if (timeseries is not None and n_ts) else None
            lens = valid_lengths[cursor:cursor + n_ts] if valid_lengths is not None else None
            cursor += n_ts
            reqs.append((seq, ser, lens))
        budget = max_new_tokens if max_length is None else max(1, max_length - max(len(r[0]) for r in reqs))
        masks = {"min_tokens": min(int(min_new_tokens), budget)} if min_new_tokens else None
        if self.max_batch > 1 and len(reqs) > 1 and streamer is None and (self.plan.world == 1 or self._tp is not None):
            outs = self.generate_batch(reqs, budget, eos_token_id, masks=masks)          # continuous batching over the cache slots
        else:
            outs = []
            if streamer is not None:          # HF generate(): the prompt goes to the streamer first, then every token as it is made
                streamer.put(ids)
            for seq, ser, lens in reqs:
                if streamer is None:
                    toks = self.generate_one(seq, ser, lens, budget, eos_token_id, masks=masks)
                else:
                    toks = []
                    for new in self.generate_stream(seq, ser, lens, budget, eos_token_id, chunk=1, masks=masks):
                        for t in new:
                            streamer.put(torch.tensor([t]))
                        toks += new
                outs.append(toks)
        rows = [ids[b].tolist() + outs[b] for b in range(ids.shape[0])]
        if streamer is not None:
            streamer.end()
        n = max(len(r) for r in rows)
        pad = cfg.pad_token_id
        return torch.tensor([r + [pad] * (n - len(r)) for r in rows], dtype=torch.long)

    def eval(self):
        return self

    def to(self, *a, **k):
        return self
