// decoder.hip - host-side composition: chatts_linear dispatch and the Qwen2/Qwen3 decoder schedule.
// Replaces Qwen2TSForCausalLM.forward / compute_logits (NetManAIOps/ChatTS chatts/vllm/chatts_vllm.py:576-610),
// whose decoder is vLLM's Qwen2Model (NOT IN REFERENCE); layer math per oracle/qwen_decoder.py.
// Nothing here allocates device memory or synchronises: every call only enqueues kernels on the
// caller's stream, so a whole decode step can be captured into one hipGraph and replayed per token.
//
// Map of the schedule (top to bottom):
//   Pass                    the mode of one whole-pass entry point (chained / verify rows / in-launch exchange), scoped: idle on every exit
//   Proj, proj()            one projection (qkv, o, gate_up, down, lm_head) in every weight format; linear_args() + Copies { BF16, W8, W8_W4 }
//                           is the only place a ChattsLinearArgs is filled; fp8_proj() / layer_half_f16q's args() are that for the two modes
//   a_planes, c_planes, norm_into, resid_dest, request_post_norm     the recurring operand bindings and the fused-norm hand-off (d->normed)
//   Rows                    WHAT a layer half works on: SEQ, SLOTS, VERIFY, PACKED, LAST - the entry points differ in this and nothing else
//   layer_half()            precision mode for these rows (layer_half_fp8, layer_half_f16q) or the default kernels: attn_half() with
//                           attention_stage() - the one part that differs by kind of rows - and mlp_half()
//   run_layers()            the layer loop with the tensor-parallel sum after each half (sum_bulk / sum_unless_fused / none)
//   chatts_decoder_prefill, _prefill_last, _prefill_packed, _decode_step, _decode_step_batched, _spec_step     Pass + run_layers + tail
#include <new>
#include <type_traits>
#include <vector>

#include "common.h"
#include "tp_common.h"

namespace chatts {
int launch_gemv(const ChattsLinearArgs* a, hipStream_t s);
int launch_gemm(const ChattsLinearArgs* a, hipStream_t s, const RopeFuse* rope = nullptr, bool* rope_done = nullptr);
int attention_decode_batched_impl(const float* qkv_raw, int batch, int n_q, int n_kv, const float* q_norm_w, const float* k_norm_w,
                                  float norm_eps, const float* cos_tab, const float* sin_tab, int pos, const int32_t* pos_dev,
                                  const ChattsKvCache* cache, size_t seq_stride, float* out, uint16_t* out_hi, uint16_t* out_lo,
                                  int n_splits, void* workspace, size_t workspace_bytes, chatts_stream_t stream);
int attention_impl(const float* qkv, int t, int n_q, int n_kv, int pos0, const int32_t* pos0_dev, const ChattsKvCache* cache, float* out,
                   uint16_t* out_hi, uint16_t* out_lo, int n_splits, void* workspace, size_t workspace_bytes, chatts_stream_t stream);
int launch_split_bf16x2(const float* x, int m, int k, int ldx, uint16_t* hi, uint16_t* lo, int ldp, hipStream_t s);
size_t gemm_workspace(int m, int n, int k);
int attention_verify_impl(const float* qkv_raw, int rows, int n_q, int n_kv, const float* q_norm_w, const float* k_norm_w, float norm_eps,
                          const float* cos_tab, const float* sin_tab, const int32_t* pos_dev, const ChattsKvCache* cache, float* out,
                          uint16_t* out_hi, uint16_t* out_lo, int n_splits, void* workspace, size_t workspace_bytes,
                          chatts_stream_t stream);
}  // namespace chatts

using namespace chatts;

struct ChattsDecoder {
  ChattsDecoderConfig cfg;
  ChattsDecoderWeights w;
  std::vector<ChattsLayerWeights> layers;
  ChattsDecoderBuffers b;
  int cur_seq = 0;          // sequence (KV-cache slot) the single-sequence entry points operate on
  bool sampling = false;    // token selection of the decode steps: greedy argmax, or the sampler with `sa`
  ChattsSamplingArgs sa{};
  bool controls = false;    // logit controls (penalties / min_p) ahead of every selection, with `lc` (chatts_decoder_set_logit_controls)
  ChattsLogitControlArgs lc{};
  bool masks = false;       // logit masks (allowed_token_ids / logit_bias / min_tokens) ahead of the controls, with `lm` (chatts_decoder_set_logit_masks)
  ChattsLogitMaskArgs lm{};
  ChattsTpComm* tp = nullptr;   // tensor-parallel exchange (borrowed); required by the whole-step entry points when tp_world > 1
  bool prefill_f16q = false; // opt-in parity-grade mode (chatts_decoder_set_prefill_f16q): prefill chunks of >= 96 rows on the f16 + e4m3 operand split
  bool prefill_fp8 = false; // SPEED MODE (chatts_decoder_set_prefill_fp8): prefill chunks of >= 16 rows multiply fp8 x fp8 (gemm_fp8.hip)
  // The mode of the running whole-pass entry point: set by Pass, idle (false / 0) outside one - also for layer halves called directly.
  bool chain = false;       // the layers run back to back inside one call: only then may a projection write the NEXT projection's normed operand
  bool fuse_tp = false;     // the M == 1 o_proj / down_proj GEMVs carry the exchange in their own launch (decode step; the last row's MLP)
  int spec_rows = 0;        // > 0: the rows of the batched halves are consecutive positions of the SELECTED sequence (verify attention on its
                            // cache), not one token of each of the cache slots 0 .. batch - 1 (speculative step)
  // Hand-off from one launch to the next: set by the producer, cleared by the consumer (and by Pass on every exit).
  bool normed = false;      // planes 0 already hold RMSNorm(x) for the next projection (the previous one's fused epilogue): norm_into only binds them
  bool normed_q = false;    // ... the same for the f16q planes A (layer_half_f16q only)
  bool x_in_xn = false;     // batched step: o_proj left the residual stream in b.xn (ping-pong, see attn_half); down_proj brings it back
  bool tp_fused = false;    // the last residual projection carried its exchange itself (otherwise the caller launches chatts_allreduce)
};

static int64_t embed_rows(const ChattsDecoder* d) { return d->cfg.embed_rows > 0 ? d->cfg.embed_rows : d->cfg.vocab_local; }
static int64_t embed_offset(const ChattsDecoder* d) { return d->cfg.embed_rows > 0 ? d->cfg.embed_offset : d->cfg.vocab_offset; }

extern "C" size_t chatts_linear_workspace(int m, int n, int k) { return gemm_workspace(m, n, k); }

static int linear_impl(const ChattsLinearArgs* a, chatts_stream_t stream, const RopeFuse* rope, bool* rope_done);
extern "C" int chatts_linear(const ChattsLinearArgs* a, chatts_stream_t stream) { return linear_impl(a, stream, nullptr, nullptr); }

// rope / rope_done: the qkv projection of a prefill chunk may carry rope_kv_kernel's work in its split-K epilogue (*rope_done says
// whether it did; otherwise the caller launches chatts_rope_kv_write as before)
static int linear_impl(const ChattsLinearArgs* a, chatts_stream_t stream, const RopeFuse* rope, bool* rope_done) {
  CHATTS_REQUIRE(a != nullptr, CHATTS_E_BADARG, "linear: null args");
  CHATTS_REQUIRE(a->m >= 0 && a->n > 0 && a->k > 0, CHATTS_E_BADARG, "linear: bad sizes m=%d n=%d k=%d", a->m, a->n, a->k);
  if (a->m == 0) return CHATTS_OK;
  const bool planes = a->a_hi || a->a_lo;
  const bool cplanes = a->c_hi || a->c_lo;
  CHATTS_REQUIRE((a->a || planes) && a->w && (a->c || cplanes), CHATTS_E_BADARG, "linear: null pointer");
  if (cplanes)
    CHATTS_REQUIRE(a->c_hi && a->c_lo && a->m > 1 && a->ld_cplanes >= (a->epilogue == CHATTS_EPI_SWIGLU ? a->n / 2 : a->n),
                   CHATTS_E_SHAPE, "linear: plane output needs both planes, M > 1 and ld_cplanes >= the output width");
  if (planes)
    CHATTS_REQUIRE(a->a_hi && a->a_lo && a->ld_planes >= a->k && a->ld_planes % 8 == 0 && ((uintptr_t)a->a_hi % 16) == 0 &&
                       ((uintptr_t)a->a_lo % 16) == 0 && a->m > 1 && !a->norm_w,
                   CHATTS_E_SHAPE, "linear: pre-split A needs both planes, ld_planes >= K and %% 8, 16-byte alignment, M > 1");
  CHATTS_REQUIRE(a->epilogue >= CHATTS_EPI_NONE && a->epilogue <= CHATTS_EPI_SWIGLU, CHATTS_E_BADARG,
                 "linear: epilogue %d", a->epilogue);
  CHATTS_REQUIRE(a->epilogue != CHATTS_EPI_RESID || a->resid, CHATTS_E_BADARG, "linear: EPI_RESID without resid");
  CHATTS_REQUIRE(a->k % 32 == 0, CHATTS_E_SHAPE, "linear: K=%d must be a multiple of 32 (pad the weight)", a->k);
  CHATTS_REQUIRE(a->n % 16 == 0 && (a->epilogue != CHATTS_EPI_SWIGLU || a->n % 32 == 0), CHATTS_E_SHAPE,
                 "linear: N=%d must be a multiple of 16 (32 for SwiGLU)", a->n);
  CHATTS_REQUIRE((!a->a || (a->lda >= a->k && a->lda % 4 == 0)) && a->ldw >= a->k && a->ldw % 8 == 0, CHATTS_E_SHAPE,
                 "linear: leading dimensions lda=%d ldw=%d", a->lda, a->ldw);
  const int ncols = a->epilogue == CHATTS_EPI_SWIGLU ? a->n / 2 : a->n;
  CHATTS_REQUIRE(a->ldc >= ncols || (cplanes && a->epilogue != CHATTS_EPI_RESID), CHATTS_E_SHAPE, "linear: ldc=%d < %d", a->ldc, ncols);
  CHATTS_REQUIRE(((uintptr_t)a->a % 16) == 0 && ((uintptr_t)a->w % 16) == 0 && ((uintptr_t)a->c % 16) == 0,
                 CHATTS_E_SHAPE, "linear: pointers must be 16-byte aligned");
  if (a->w8)
    CHATTS_REQUIRE(a->w8_scale && a->ldw8 >= a->k && a->ldw8 % 16 == 0 && ((uintptr_t)a->w8 % 16) == 0 && a->k % 16 == 0,
                   CHATTS_E_SHAPE, "linear: fp8 weights need a scale, ldw8 >= K, 16-byte alignment");
  if (a->w4)
    CHATTS_REQUIRE(a->w4_sz && a->w4_group >= 16 && (a->w4_group & (a->w4_group - 1)) == 0 && a->k % a->w4_group == 0 && a->ldw4 >= a->k / 2 &&
                       a->ldw4 % 8 == 0 && ((uintptr_t)a->w4 % 8) == 0 && ((uintptr_t)a->w4_sz % 8) == 0,
                   CHATTS_E_SHAPE, "linear: 4-bit weights need w4_sz, a power-of-two group size >= 16 that divides K, ldw4 >= K/2 and %% 8");
  if (a->post_norm_w)
    CHATTS_REQUIRE(a->m > 1 && a->c && a->post_hi && a->post_lo && a->ld_post >= a->n && a->ld_post % 4 == 0 && a->n % 4 == 0 &&
                       a->ldc % 4 == 0 && (a->epilogue == CHATTS_EPI_NONE || a->epilogue == CHATTS_EPI_RESID) && !cplanes,
                   CHATTS_E_BADARG, "linear: post-norm planes need M > 1, float32 c with ldc %% 4 == 0, EPI_NONE / EPI_RESID, both planes, ld_post >= N");
  if (a->tp_reduce) CHATTS_REQUIRE(a->m == 1, CHATTS_E_BADARG, "linear: tp_reduce is available for M == 1 (the decode GEMV) only");
  if (a->m == 1 && a->epilogue != CHATTS_EPI_GELU) return launch_gemv(a, as_stream(stream));
  CHATTS_REQUIRE(a->norm_w == nullptr, CHATTS_E_BADARG, "linear: fused RMSNorm is only available for M == 1");
  return launch_gemm(a, as_stream(stream), rope, rope_done);
}

extern "C" int chatts_split_bf16x2(const float* x, int m, int k, int ldx, chatts_bf16* hi, chatts_bf16* lo, int ld_planes,
                                   chatts_stream_t stream) {
  CHATTS_REQUIRE(m >= 0 && k >= 0 && k % 8 == 0, CHATTS_E_SHAPE, "split_bf16x2: m=%d k=%d (K must be a multiple of 8)", m, k);
  if (m == 0 || k == 0) return CHATTS_OK;
  CHATTS_REQUIRE(x && hi && lo, CHATTS_E_BADARG, "split_bf16x2: null pointer");
  CHATTS_REQUIRE(ldx >= k && ldx % 4 == 0 && ld_planes >= k && ld_planes % 8 == 0, CHATTS_E_SHAPE,
                 "split_bf16x2: leading dimensions ldx=%d ld_planes=%d", ldx, ld_planes);
  CHATTS_REQUIRE(((uintptr_t)x % 16) == 0 && ((uintptr_t)hi % 16) == 0 && ((uintptr_t)lo % 16) == 0, CHATTS_E_SHAPE,
                 "split_bf16x2: pointers must be 16-byte aligned");
  return launch_split_bf16x2(x, m, k, ldx, hi, lo, ld_planes, as_stream(stream));
}

constexpr int kF16qMinRows = 96;      // f16q mode: chunks below this take the default kernels (also parity grade)

extern "C" size_t chatts_decoder_workspace(const ChattsDecoderConfig* c, int t_max, int n_splits_max) {
  if (!c) return 0;
  size_t ws = 0;
  const int qkv_n = (c->n_q + 2 * c->n_kv) * c->head_dim;
  const int shapes[4][2] = {{qkv_n, c->hidden}, {c->hidden, c->n_q * c->head_dim}, {2 * c->inter, c->hidden},
                            {c->hidden, c->inter}};
  for (int t = 2; t <= t_max; ++t) {   // geometry depends on M; take the max over all M (cheap: <= t_max iterations)
    for (auto& s : shapes) {
      size_t w = gemm_workspace(t, s[0], s[1]);
      if (t >= kF16qMinRows && s[1] % 128 == 0) { const size_t wq = chatts_linear_f16q_workspace(t, s[0], s[1]); if (wq > w) w = wq; }
      if (w > ws) ws = w;
    }
  }
  size_t aw = chatts_attn_workspace(1, c->n_q, n_splits_max);
  const size_t pw = chatts_attn_workspace(t_max, c->n_q, 2);      // prefill attention with the keys split in two
  if (pw > aw) aw = pw;
  return (ws > aw ? ws : aw) + 256;
}

extern "C" ChattsDecoder* chatts_decoder_create(const ChattsDecoderConfig* c, const ChattsDecoderWeights* w,
                                                const ChattsDecoderBuffers* b) {
  if (!c || !w || !b || !w->layers) { set_error("decoder_create: null argument"); return nullptr; }
  if (c->head_dim != kHeadDim) { set_error("decoder_create: head_dim %d != 128", c->head_dim); return nullptr; }
  if (c->n_q % c->n_kv != 0 || c->n_q / c->n_kv > 8) { set_error("decoder_create: unsupported GQA group"); return nullptr; }
  if (c->hidden % 32 || c->inter % 32) { set_error("decoder_create: hidden/inter must be multiples of 32"); return nullptr; }
  if (kv_elem_bytes(b->kv_dtype) == 0) {
    set_error("decoder_create: unknown KV cache dtype %d (CHATTS_KV_F32 = 0, CHATTS_KV_F16 = 1)", b->kv_dtype);
    return nullptr;
  }
  if (b->kv_block_table) {
    const int B = b->kv_block_size;
    if (kv_log_block(B) < 0 || c->max_ctx % B != 0 || b->kv_table_stride < c->max_ctx / B || b->kv_pool_blocks < 1) {
      set_error("decoder_create: paged KV needs a power-of-two block size in 64..32768 dividing max_ctx (%d), a table row of >= "
                "max_ctx / block_size entries and a non-empty pool (block %d, row %d, pool %d)", c->max_ctx, B, b->kv_table_stride,
                b->kv_pool_blocks);
      return nullptr;
    }
  }
  ChattsDecoder* d = new (std::nothrow) ChattsDecoder();
  if (!d) { set_error("decoder_create: out of host memory"); return nullptr; }
  d->cfg = *c;
  d->w = *w;
  d->layers.assign(w->layers, w->layers + c->n_layers);
  d->w.layers = d->layers.data();
  d->b = *b;
  return d;
}

extern "C" void chatts_decoder_destroy(ChattsDecoder* d) { delete d; }

static size_t seq_stride(const ChattsDecoder* d) {      // elements (of b.kv_dtype) between the caches of consecutive sequences
  return (size_t)d->cfg.n_layers * d->cfg.n_kv * d->cfg.max_ctx * kHeadDim;
}

// base + `elems` elements of the cache's type (kv_k / kv_v are typed float* in the ABI, the storage may be _Float16)
static float* kv_at(float* base, size_t elems, int dtype) {
  return reinterpret_cast<float*>(reinterpret_cast<char*>(base) + elems * kv_elem_bytes(dtype));
}

static ChattsKvCache layer_cache(const ChattsDecoder* d, int layer, int seq) {
  ChattsKvCache c{};
  c.max_ctx = d->cfg.max_ctx;
  c.dtype = d->b.kv_dtype;
  if (d->b.kv_block_table) {      // block-paged: the layer's pool + this sequence's row of the block table
    const size_t pool = (size_t)d->b.kv_pool_blocks * d->cfg.n_kv * d->b.kv_block_size * kHeadDim;
    c.k = kv_at(d->b.kv_k, pool * layer, c.dtype);
    c.v = kv_at(d->b.kv_v, pool * layer, c.dtype);
    c.block_table = d->b.kv_block_table + (size_t)seq * d->b.kv_table_stride;
    c.block_size = d->b.kv_block_size;
    c.table_stride = d->b.kv_table_stride;
    return c;
  }
  const size_t per = (size_t)d->cfg.n_kv * d->cfg.max_ctx * kHeadDim;
  c.k = kv_at(d->b.kv_k, seq_stride(d) * seq + per * layer, c.dtype);
  c.v = kv_at(d->b.kv_v, seq_stride(d) * seq + per * layer, c.dtype);
  return c;
}

static int max_batch(const ChattsDecoder* d) { return d->b.max_batch > 0 ? d->b.max_batch : 1; }      // (0 or 1 = single sequence)

// The mode a whole-pass entry point runs in, for exactly as long as it runs: every exit path, error exits included, leaves the decoder
// idle (no chaining, no verify rows, no in-launch exchange, no hand-off pending), so that nothing leaks into the next call.
struct Pass {
  ChattsDecoder* d;
  Pass(ChattsDecoder* d_, bool chain, int spec_rows = 0, bool fuse_tp = false) : d(d_) {
    idle();
    d->chain = chain; d->spec_rows = spec_rows; d->fuse_tp = fuse_tp;
  }
  ~Pass() { idle(); }
  void idle() { d->chain = false; d->spec_rows = 0; d->fuse_tp = false; d->normed = false; d->normed_q = false; d->x_in_xn = false; }
};

// ---- one description of a projection ---------------------------------------------------------------------------------------------
enum Which { QKV, O, GATE_UP, DOWN, LM_HEAD };
struct Proj {      // one [n, k] matrix in every format the decoder holds it in (NULL = that copy does not exist)
  const chatts_bf16* w; const chatts_bf16* w_tiled; const float* bias;
  const uint8_t* w8; const float* w8_scale;                               // 8-bit copy + row scale (cfg.w8_format)
  const uint8_t* w4; const float* w4_sz; int w4_group;                    // 4-bit codes + (scale, scale * zero) per group
  const chatts_f16* w16; const uint8_t* q8; const uint8_t* q8e;           // f16q triple: f16 high part, e4m3 residual, e8m0 row exponent
  int n, k;
};
static Proj proj(const ChattsDecoder* d, int layer, Which which) {
  const ChattsDecoderConfig& c = d->cfg;
  const int H = c.hidden, na = c.n_q * kHeadDim;
  if (which == LM_HEAD)
    return {d->w.lm_head, nullptr, nullptr, d->w.lm_head8, d->w.lm_head8_scale, nullptr, nullptr, 0, nullptr, nullptr, nullptr, (int)c.vocab_local, H};
  const ChattsLayerWeights& lw = d->layers[layer];
  switch (which) {
    case QKV: return {lw.qkv, lw.qkv_t, lw.qkv_bias, lw.qkv8, lw.qkv8_scale, lw.qkv4, lw.qkv4_sz, lw.w4_group, lw.qkv16, lw.qkv_q8, lw.qkv_q8e,
                      (c.n_q + 2 * c.n_kv) * kHeadDim, H};
    case O: return {lw.o, lw.o_t, nullptr, lw.o8, lw.o8_scale, lw.o4, lw.o4_sz, lw.w4_group, lw.o16, lw.o_q8, lw.o_q8e, H, na};
    case GATE_UP: return {lw.gate_up, lw.gate_up_t, nullptr, lw.gate_up8, lw.gate_up8_scale, lw.gate_up4, lw.gate_up4_sz, lw.w4_group, lw.gate_up16,
                          lw.gate_up_q8, lw.gate_up_q8e, 2 * c.inter, H};
    default: return {lw.down, lw.down_t, nullptr, lw.down8, lw.down8_scale, lw.down4, lw.down4_sz, lw.w4_group, lw.down16, lw.down_q8, lw.down_q8e,
                     H, c.inter};
  }
}
static int out_cols(const Proj& p, int epilogue) { return epilogue == CHATTS_EPI_SWIGLU ? p.n / 2 : p.n; }

// Which copies of the matrix a call offers the kernels besides bf16 (row-major + tiled).  The M == 1 GEMV streams the smallest copy it
// is given, the M <= 16 weight-streaming GEMM the 8-bit one; a prefill chunk is MFMA-bound and gets neither.
enum Copies { BF16, W8, W8_W4 };
static void attach_w8(const ChattsDecoder* d, const Proj& p, ChattsLinearArgs* la) {
  la->w8 = p.w8; la->w8_scale = p.w8_scale; la->ldw8 = p.k; la->w8_format = d->cfg.w8_format;
}
static void attach_w4(const Proj& p, ChattsLinearArgs* la) { la->w4 = p.w4; la->w4_sz = p.w4_sz; la->ldw4 = p.k / 2; la->w4_group = p.w4_group; }

// The one place a ChattsLinearArgs is filled from a projection: dense rows in (lda = K) and out (ldc = the output width).  The caller
// binds A (a / planes / norm_in_launch), C and, for o_proj / down_proj, the residual destination.
static ChattsLinearArgs linear_args(const ChattsDecoder* d, const Proj& p, int m, int epilogue, Copies copies) {
  ChattsLinearArgs la{};
  la.w = p.w; la.w_tiled = p.w_tiled; la.bias = p.bias; la.m = m; la.n = p.n; la.k = p.k;
  la.lda = p.k; la.ldw = p.k; la.ldc = out_cols(p, epilogue); la.epilogue = epilogue;
  la.workspace = d->b.workspace; la.workspace_bytes = d->b.workspace_bytes;
  if (copies != BF16) attach_w8(d, p, &la);
  if (copies == W8_W4) attach_w4(p, &la);
  return la;
}

// ---- the recurring bindings ------------------------------------------------------------------------------------------------------
// Projections whose A operand is a pair of bf16 hi / lo planes: prefill chunks of >= 96 rows (LDS-DMA GEMM) and batched
// decode with 2..16 sequences on bf16 weights (weight-streaming kernel).
static bool planes_path(const ChattsDecoder* d, int m, int k, bool fp8 = false) {
  if (!(d->b.planes_hi && d->b.planes_lo && d->b.planes2_hi && d->b.planes2_lo) || k % 64 != 0) return false;
  if (m >= 2 && m <= 16) return !fp8 || k % 128 == 0;      // (the fp8 stream's K-step is one 128-byte line = 128 values)
  return m >= 96 && !fp8;
}

// A is planes pair `pair` (0: projection input, 1: gate_up output).  KEEP_F32 leaves the float32 `a` bound next to the planes: the
// GEMM dispatch then takes the prefill kernel from 96 rows only and the float32 operand below (the split attention output).
enum KeepA { DROP_F32, KEEP_F32 };
static void a_planes(const ChattsDecoder* d, int pair, ChattsLinearArgs* la, KeepA keep = DROP_F32) {
  if (keep == DROP_F32) la->a = nullptr;
  la->a_hi = pair ? d->b.planes2_hi : d->b.planes_hi; la->a_lo = pair ? d->b.planes2_lo : d->b.planes_lo; la->ld_planes = la->k;
}
// C is planes pair 1 (the SwiGLU output goes straight into down_proj's operand format)
static void c_planes(const ChattsDecoder* d, ChattsLinearArgs* la) {
  la->c = nullptr; la->c_hi = d->b.planes2_hi; la->c_lo = d->b.planes2_lo; la->ld_cplanes = la->ldc;
}
// decode (M == 1): RMSNorm fused in the GEMV prologue
static void norm_in_launch(const ChattsDecoder* d, const float* x, const float* norm_w, ChattsLinearArgs* la) {
  la->a = x; la->norm_w = norm_w; la->norm_eps = d->cfg.rms_eps;
}

// x -> RMSNorm -> la's input: planes written by the norm kernel itself (plane path) or float32 xn.
static int norm_into(ChattsDecoder* d, const float* norm_w, ChattsLinearArgs* la, chatts_stream_t stream) {
  if (planes_path(d, la->m, la->k, la->w8 != nullptr)) {
    a_planes(d, 0, la);
    if (d->normed) { d->normed = false; return CHATTS_OK; }
    return chatts_rmsnorm_planes(d->b.x, norm_w, d->b.planes_hi, d->b.planes_lo, la->k, la->m, la->k, d->cfg.rms_eps, stream);
  }
  d->normed = false;
  la->a = d->b.xn;
  return chatts_rmsnorm(d->b.x, norm_w, d->b.xn, la->m, la->k, d->cfg.rms_eps, stream);
}

// Where a residual projection (o_proj / down_proj) puts its result, for all three argument types:
//   tensor parallel, fuse_in_launch   x = resid + sum over the ranks, inside the GEMV launch (ChattsLinearArgs.tp_reduce; d->tp_fused)
//   tensor parallel otherwise         delta = the partial product: the caller all-reduces it into x
//   one rank                          x = resid_in + product (resid_in: where the residual stream is - x, or xn in the batched ping-pong)
template <class Args>
static void resid_dest(ChattsDecoder* d, Args* la, bool fuse_in_launch, const float* resid_in) {
  const bool tp = d->cfg.tp_world > 1;
  d->tp_fused = false;
  if (tp && !fuse_in_launch) { la->c = d->b.delta; la->epilogue = CHATTS_EPI_NONE; return; }
  la->c = d->b.x; la->resid = tp ? d->b.x : resid_in; la->epilogue = CHATTS_EPI_RESID;
  if constexpr (std::is_same<Args, ChattsLinearArgs>::value) {
    if (tp) { la->tp_reduce = d->tp; d->tp_fused = true; }
  }
}

// The residual-updating projection (o_proj / down_proj, tp_world == 1) also produces the NEXT projection's operand:
// RMSNorm(x) with `next_norm_w` as planes 0, when that projection will take the plane path for the same M.
static bool gemm_post_norm_small_m() { return opt_get(OPT_POST_NORM_SMALL_M, 1) != 0; }
static void request_post_norm(ChattsDecoder* d, ChattsLinearArgs* la, const float* next_norm_w, bool next_fp8) {
  if (!d->chain || d->cfg.tp_world > 1 || !next_norm_w || la->epilogue != CHATTS_EPI_RESID) return;
  // the fused epilogue runs one workgroup per row - fine for a prefill chunk; at batched-decode M it needs several workgroups per row,
  // which re-read resid while others write c: only when the caller gave it a c that does not alias resid (the batched ping-pong)
  if (la->m < 64 && !(la->m <= 16 && la->c != la->resid && gemm_post_norm_small_m())) return;
  if (!planes_path(d, la->m, la->n, next_fp8)) return;
  la->post_norm_w = next_norm_w; la->post_norm_eps = d->cfg.rms_eps;
  la->post_hi = d->b.planes_hi; la->post_lo = d->b.planes_lo; la->ld_post = la->n;
  d->normed = true;
}

// row t - 1 of x -> row 0 (what follows a last-row prefill reads row 0)
static int last_row_to_row0(ChattsDecoder* d, int t, chatts_stream_t stream) {
  if (t <= 1) return CHATTS_OK;
  const size_t H = (size_t)d->cfg.hidden;
  const hipError_t e = hipMemcpyAsync(d->b.x, d->b.x + (size_t)(t - 1) * H, H * sizeof(float), hipMemcpyDeviceToDevice, as_stream(stream));
  CHATTS_REQUIRE(e == hipSuccess, CHATTS_E_LAUNCH, "prefill_last: row copy: %s", hipGetErrorString(e));
  return CHATTS_OK;
}

extern "C" int chatts_decoder_set_sampling(ChattsDecoder* d, const ChattsSamplingArgs* sa) {
  CHATTS_REQUIRE(d, CHATTS_E_BADARG, "decoder_set_sampling: null decoder");
  if (sa) CHATTS_REQUIRE(sa->temperature_rows || (sa->temperature > 0.f && sa->top_p > 0.f), CHATTS_E_BADARG,
                         "decoder_set_sampling: temperature %g / top_p %g must be positive (pass NULL for greedy)",
                         (double)sa->temperature, (double)sa->top_p);
  d->sampling = sa != nullptr;
  if (sa) d->sa = *sa;
  return CHATTS_OK;
}

extern "C" int chatts_decoder_set_tp(ChattsDecoder* d, ChattsTpComm* comm) {
  CHATTS_REQUIRE(d, CHATTS_E_BADARG, "decoder_set_tp: null decoder");
  if (comm) {
    CHATTS_REQUIRE(chatts_tp_world(comm) == d->cfg.tp_world, CHATTS_E_BADARG, "decoder_set_tp: comm of %d ranks, decoder built for %d",
                   chatts_tp_world(comm), d->cfg.tp_world);
    const int mb = max_batch(d);
    CHATTS_REQUIRE(chatts_tp_max_elems(comm) >= (int64_t)mb * d->cfg.hidden, CHATTS_E_SHAPE,
                   "decoder_set_tp: exchange buffer holds %lld elements, a step needs %lld", (long long)chatts_tp_max_elems(comm),
                   (long long)mb * d->cfg.hidden);
    CHATTS_REQUIRE(d->b.tp_pair_logit && d->b.tp_pair_token && d->b.delta, CHATTS_E_BADARG,
                   "decoder_set_tp: buffers.delta / tp_pair_logit / tp_pair_token are required");
  }
  d->tp = comm;
  return CHATTS_OK;
}

extern "C" int chatts_decoder_set_logit_controls(ChattsDecoder* d, const ChattsLogitControlArgs* lc) {
  CHATTS_REQUIRE(d, CHATTS_E_BADARG, "decoder_set_logit_controls: null decoder");
  if (lc) CHATTS_REQUIRE(lc->state && lc->out, CHATTS_E_BADARG, "decoder_set_logit_controls: args.state and args.out are required");
  d->controls = lc != nullptr;
  if (lc) d->lc = *lc;
  return CHATTS_OK;
}

extern "C" int chatts_decoder_set_logit_masks(ChattsDecoder* d, const ChattsLogitMaskArgs* lm) {
  CHATTS_REQUIRE(d, CHATTS_E_BADARG, "decoder_set_logit_masks: null decoder");
  if (lm) CHATTS_REQUIRE(lm->out, CHATTS_E_BADARG, "decoder_set_logit_masks: args.out is required");
  d->masks = lm != nullptr;
  if (lm) d->lm = *lm;
  return CHATTS_OK;
}

// ---- token selection and logprobs ------------------------------------------------------------------------------------------------
// What a rank must have before it may gather the full-vocabulary logits into buffers.logits_full.  Call it, and every other check of
// the caller, AHEAD of chatts_allgather: a refusal on one rank must not leave the others waiting in the collective.
static int require_full_logits_tp(const ChattsDecoder* d, int batch, int64_t logits_stride, const char* name, const char* who_needs) {
  CHATTS_REQUIRE(d->tp, CHATTS_E_BADARG, "%s: tp_world = %d but no exchange attached (chatts_decoder_set_tp)", name, d->cfg.tp_world);
  CHATTS_REQUIRE(batch <= max_batch(d), CHATTS_E_SHAPE, "%s: batch %d exceeds max_batch %d", name, batch, max_batch(d));
  CHATTS_REQUIRE(d->b.logits_full, CHATTS_E_BADARG, "%s: %s buffers.logits_full", name, who_needs);
  CHATTS_REQUIRE(logits_stride == d->cfg.vocab_local || batch == 1, CHATTS_E_SHAPE, "%s: logits rows must be contiguous", name);
  return CHATTS_OK;
}

// Selection with the logit masks and / or the logit controls on: masked logits into lm->out, penalised logits (of those) into lc->out,
// the TP = 1 selection on the last buffer written, the chosen tokens into the controls' state.
// Tensor parallel: every rank gathers the full-vocabulary logits and does the same work on the same bytes -> the same token.
static int select_processed(ChattsDecoder* d, const float* logits, int batch, int64_t logits_stride, int64_t* token, float* token_logit,
                            int64_t* out_tokens, int64_t out_stride, int32_t* step_dev, int32_t* pos_dev, int pos_limit,
                            const ChattsSamplingArgs* sa, const ChattsLogitControlArgs* lc, const ChattsLogitMaskArgs* lm,
                            chatts_stream_t stream) {
  const ChattsDecoderConfig& c = d->cfg;
  int64_t vocab = c.vocab_local, offset = c.vocab_offset;
  int rc;
  if (c.tp_world > 1) {
    if ((rc = require_full_logits_tp(d, batch, logits_stride, "decoder_select_tokens",
                                     "logit controls and logit masks under tensor parallelism need")) != 0)
      return rc;
    vocab = c.vocab_local * c.tp_world; offset = 0;
  }
  if (lc) {
    CHATTS_REQUIRE(lc->state && lc->out && lc->state_stride >= vocab && lc->out_stride >= vocab, CHATTS_E_BADARG,
                   "decoder_select_tokens: logit controls need state and out rows of >= %lld cells", (long long)vocab);
    CHATTS_REQUIRE(d->b.workspace && d->b.workspace_bytes >= chatts_logit_controls_workspace(batch), CHATTS_E_WORKSPACE,
                   "decoder_select_tokens: the workspace is too small for the logit controls of %d rows", batch);
  }
  if (lm) {
    CHATTS_REQUIRE(lm->out && lm->out_stride >= vocab && lm->out != logits && lm->out != d->b.logits_full && (!lc || lm->out != lc->out),
                   CHATTS_E_BADARG, "decoder_select_tokens: logit masks need out rows of >= %lld cells in a buffer of their own",
                   (long long)vocab);
    if ((rc = logit_mask_arrays_check(lm, vocab, offset, step_dev, "decoder_select_tokens")) != 0) return rc;
  }
  if (c.tp_world > 1) {
    if ((rc = chatts_allgather(d->tp, logits, d->b.logits_full, batch, c.vocab_local, stream)) != 0) return rc;
    logits = d->b.logits_full; logits_stride = vocab;
  }
  if (lm) {
    if ((rc = chatts_logit_masks_apply(logits, batch, logits_stride, vocab, offset, lm, step_dev, stream)) != 0) return rc;
    logits = lm->out; logits_stride = lm->out_stride;
  }
  if (lc) {
    // (the split-K / attention workspace is idle here: every kernel that used it is ahead of this call on the stream)
    if ((rc = chatts_logit_controls_apply(logits, batch, logits_stride, vocab, offset, lc, d->b.workspace, d->b.workspace_bytes, stream)) != 0)
      return rc;
    logits = lc->out; logits_stride = lc->out_stride;
  }
  if (sa)
    rc = chatts_sample_batched(logits, batch, logits_stride, vocab, offset, sa, token, token_logit, out_tokens, out_stride, step_dev,
                               pos_dev, pos_limit, stream);
  else
    rc = chatts::argmax_batched_scratch(logits, batch, logits_stride, vocab, offset, token, token_logit, out_tokens, out_stride, step_dev,
                                        pos_dev, pos_limit, d->b.workspace, d->b.workspace_bytes, reinterpret_cast<hipStream_t>(stream));
  if (rc || !lc) return rc;
  return chatts_logit_state_update(lc->state, lc->state_stride, batch, vocab, offset, token, stream);
}

extern "C" int chatts_decoder_select_tokens(ChattsDecoder* d, const float* logits, int batch, int64_t logits_stride, int64_t* token,
                                            float* token_logit, int64_t* out_tokens, int64_t out_stride, int32_t* step_dev,
                                            int32_t* pos_dev, int pos_limit, const ChattsSamplingArgs* override_sa,
                                            chatts_stream_t stream) {
  return chatts_decoder_select_tokens_controlled(d, logits, batch, logits_stride, token, token_logit, out_tokens, out_stride, step_dev,
                                                 pos_dev, pos_limit, override_sa, nullptr, stream);
}

extern "C" int chatts_decoder_select_tokens_controlled(ChattsDecoder* d, const float* logits, int batch, int64_t logits_stride,
                                                       int64_t* token, float* token_logit, int64_t* out_tokens, int64_t out_stride,
                                                       int32_t* step_dev, int32_t* pos_dev, int pos_limit,
                                                       const ChattsSamplingArgs* override_sa, const ChattsLogitControlArgs* override_lc,
                                                       chatts_stream_t stream) {
  return chatts_decoder_select_tokens_masked(d, logits, batch, logits_stride, token, token_logit, out_tokens, out_stride, step_dev, pos_dev,
                                             pos_limit, override_sa, override_lc, nullptr, stream);
}

// Greedy / sampled token for `batch` logits rows of this rank, agreed across the TP ranks (see the header).
extern "C" int chatts_decoder_select_tokens_masked(ChattsDecoder* d, const float* logits, int batch, int64_t logits_stride,
                                                   int64_t* token, float* token_logit, int64_t* out_tokens, int64_t out_stride,
                                                   int32_t* step_dev, int32_t* pos_dev, int pos_limit,
                                                   const ChattsSamplingArgs* override_sa, const ChattsLogitControlArgs* override_lc,
                                                   const ChattsLogitMaskArgs* override_lm, chatts_stream_t stream) {
  CHATTS_REQUIRE(d && logits && token && batch >= 1, CHATTS_E_BADARG, "decoder_select_tokens: bad arguments");
  StageRange stage("chatts.select_tokens");
  const ChattsDecoderConfig& c = d->cfg;
  const ChattsSamplingArgs* sa = override_sa ? override_sa : (d->sampling ? &d->sa : nullptr);
  const ChattsLogitControlArgs* lc = override_lc ? override_lc : (d->controls ? &d->lc : nullptr);
  const ChattsLogitMaskArgs* lm = override_lm ? override_lm : (d->masks ? &d->lm : nullptr);
  if (lc || lm)
    return select_processed(d, logits, batch, logits_stride, token, token_logit, out_tokens, out_stride, step_dev, pos_dev, pos_limit, sa,
                            lc, lm, stream);
  if (c.tp_world <= 1) {
    if (sa)
      return chatts_sample_batched(logits, batch, logits_stride, c.vocab_local, c.vocab_offset, sa, token, token_logit, out_tokens,
                                   out_stride, step_dev, pos_dev, pos_limit, stream);
    // (the split-K / attention workspace is idle here: every kernel that used it is ahead of this call on the stream)
    return chatts::argmax_batched_scratch(logits, batch, logits_stride, c.vocab_local, c.vocab_offset, token, token_logit, out_tokens,
                                          out_stride, step_dev, pos_dev, pos_limit, d->b.workspace, d->b.workspace_bytes,
                                          reinterpret_cast<hipStream_t>(stream));
  }
  int rc;
  if (!sa) {      // one (max logit, global id) pair per rank and sequence instead of the [V / W] logits
    CHATTS_REQUIRE(d->tp, CHATTS_E_BADARG, "decoder_select_tokens: tp_world = %d but no exchange attached (chatts_decoder_set_tp)", c.tp_world);
    CHATTS_REQUIRE(batch <= max_batch(d), CHATTS_E_SHAPE, "decoder_select_tokens: batch %d exceeds max_batch %d", batch, max_batch(d));
    if ((rc = chatts_argmax_batched(logits, batch, logits_stride, c.vocab_local, c.vocab_offset, d->b.tp_pair_token, d->b.tp_pair_logit,
                                    nullptr, 0, nullptr, nullptr, 0, stream)) != 0) return rc;
    return chatts_tp_argmax(d->tp, batch, d->b.tp_pair_logit, d->b.tp_pair_token, token, token_logit, out_tokens, out_stride, step_dev,
                            pos_dev, pos_limit, stream);
  }
  // sampling: every rank draws from the gathered full-vocabulary logits with the same counter-hash variate -> the same token
  if ((rc = require_full_logits_tp(d, batch, logits_stride, "decoder_select_tokens", "sampling under tensor parallelism needs")) != 0) return rc;
  if ((rc = chatts_allgather(d->tp, logits, d->b.logits_full, batch, c.vocab_local, stream)) != 0) return rc;
  const int64_t vfull = c.vocab_local * c.tp_world;
  return chatts_sample_batched(d->b.logits_full, batch, vfull, vfull, 0, sa, token, token_logit, out_tokens, out_stride, step_dev,
                               pos_dev, pos_limit, stream);
}

// Logprobs of the tokens chatts_decoder_select_tokens just chose (see the header).  Under tensor parallelism every rank gathers the
// full-vocabulary logits into buffers.logits_full (the sampled selection's chatts_allgather) and runs the same kernel on them: the
// same launches on the same bytes, so every rank writes the same bits.
extern "C" int chatts_decoder_logprobs(ChattsDecoder* d, const float* logits, int batch, int64_t logits_stride, int k,
                                       const int64_t* token, const int32_t* step_dev, int64_t out_stride, float* out_lp,
                                       int32_t* out_rank, int32_t* out_top_ids, float* out_top_lp, chatts_stream_t stream) {
  CHATTS_REQUIRE(d && logits && token && batch >= 1, CHATTS_E_BADARG, "decoder_logprobs: bad arguments");
  const ChattsDecoderConfig& c = d->cfg;
  // (the split-K / attention workspace is idle here, as for the selection ahead of this call)
  if (c.tp_world <= 1)
    return chatts_logprobs_batched(logits, batch, logits_stride, c.vocab_local, c.vocab_offset, k, token, step_dev, out_stride, out_lp,
                                   out_rank, out_top_ids, out_top_lp, d->b.workspace, d->b.workspace_bytes, stream);
  int rc;
  if ((rc = require_full_logits_tp(d, batch, logits_stride, "decoder_logprobs", "logprobs under tensor parallelism need")) != 0) return rc;
  CHATTS_REQUIRE(k >= 0 && k <= CHATTS_LOGPROBS_MAX_K && (k == 0 || (out_top_ids && out_top_lp)) && out_lp && out_rank, CHATTS_E_BADARG,
                 "decoder_logprobs: k = %d / outputs", k);
  if ((rc = chatts_allgather(d->tp, logits, d->b.logits_full, batch, c.vocab_local, stream)) != 0) return rc;
  const int64_t vfull = c.vocab_local * c.tp_world;
  return chatts_logprobs_batched(d->b.logits_full, batch, vfull, vfull, 0, k, token, step_dev, out_stride, out_lp, out_rank, out_top_ids,
                                 out_top_lp, d->b.workspace, d->b.workspace_bytes, stream);
}

extern "C" int chatts_decoder_select_sequence(ChattsDecoder* d, int seq) {
  CHATTS_REQUIRE(d && seq >= 0 && seq < max_batch(d), CHATTS_E_BADARG, "decoder_select_sequence: slot %d out of range", seq);
  d->cur_seq = seq;
  return CHATTS_OK;
}

// ---- SPEED MODE: a prefill chunk's layer half on the fp8 matrix pipe (gemm_fp8.hip) ----------------------------------------------
// Activation rows are quantised per token (RMSNorm fused), the four projections are fp8 x fp8 GEMMs on the e4m3 weight copies;
// RoPE / cache write / attention / residual stream stay float32.  Scratch: the bf16 plane buffers as byte arrays, xn for the row scales.
extern "C" int chatts_decoder_set_prefill_fp8(ChattsDecoder* d, int on) {
  CHATTS_REQUIRE(d, CHATTS_E_BADARG, "decoder_set_prefill_fp8: null decoder");
  if (on) {
    const ChattsDecoderConfig& c = d->cfg;
    CHATTS_REQUIRE(c.w8_format == CHATTS_W8_FP8, CHATTS_E_BADARG, "decoder_set_prefill_fp8: the 8-bit weight copies are not e4m3");
    for (const ChattsLayerWeights& lw : d->layers)
      CHATTS_REQUIRE(lw.qkv8 && lw.o8 && lw.gate_up8 && lw.down8, CHATTS_E_BADARG, "decoder_set_prefill_fp8: a layer has no fp8 weight copies "
                     "(weight_format=\"fp8\")");
    CHATTS_REQUIRE(c.hidden % 128 == 0 && c.inter % 128 == 0, CHATTS_E_SHAPE, "decoder_set_prefill_fp8: hidden / inter must be multiples of 128");
    CHATTS_REQUIRE(d->b.planes_hi && d->b.planes_lo && d->b.planes2_hi && d->b.xn && d->b.t_max >= 1, CHATTS_E_BADARG,
                   "decoder_set_prefill_fp8: the plane buffers and xn are needed as scratch");
  }
  d->prefill_fp8 = on != 0;
  return CHATTS_OK;
}

// ---- OPT-IN, PARITY GRADE: a prefill chunk's layer half on the f16q operand split (gemm_f16q.hip) -------------------------------------
// The four projections multiply f16 high parts on the f16 MFMA and e4m3 residuals x e4m3 weights on the block-scaled fp8 MFMA; every
// activation matrix between them travels as f16q planes written by its producer (RMSNorm, attention output split, SwiGLU epilogue, the
// residual projections' post-norm).  Scratch: the bf16 plane buffers re-typed - pair 0 / pair 1 = (f16 hi | e4m3 lo, then the e8m0 scales).
extern "C" int chatts_decoder_set_prefill_f16q(ChattsDecoder* d, int on) {
  CHATTS_REQUIRE(d, CHATTS_E_BADARG, "decoder_set_prefill_f16q: null decoder");
  if (on) {
    const ChattsDecoderConfig& c = d->cfg;
    for (const ChattsLayerWeights& lw : d->layers)
      CHATTS_REQUIRE(lw.qkv16 && lw.qkv_q8 && lw.qkv_q8e && lw.o16 && lw.o_q8 && lw.o_q8e && lw.gate_up16 && lw.gate_up_q8 && lw.gate_up_q8e &&
                         lw.down16 && lw.down_q8 && lw.down_q8e, CHATTS_E_BADARG, "decoder_set_prefill_f16q: a layer has no (tiled) f16q weight copies");
    CHATTS_REQUIRE(c.hidden % 128 == 0 && c.inter % 128 == 0, CHATTS_E_SHAPE, "decoder_set_prefill_f16q: hidden / inter must be multiples of 128");
    CHATTS_REQUIRE(d->b.planes_hi && d->b.planes_lo && d->b.planes2_hi && d->b.planes2_lo && d->b.t_max >= 1, CHATTS_E_BADARG,
                   "decoder_set_prefill_f16q: the plane buffers are needed as scratch");
    CHATTS_REQUIRE(!d->prefill_fp8, CHATTS_E_BADARG, "decoder_set_prefill_f16q: the fp8 speed mode is on");
  }
  d->prefill_f16q = on != 0;
  d->normed_q = false;
  return CHATTS_OK;
}

// ---- the rows a layer half works on ----------------------------------------------------------------------------------------------
struct Rows {
  enum Kind {
    SEQ,        // m rows of the selected sequence at positions pos0 .. (or *pos_dev ..): a prefill chunk, or the decode row (m == 1)
    SLOTS,      // one row of each of the cache slots 0 .. m - 1, row b at position pos_dev[b]: a batched decode step
    VERIFY,     // m consecutive positions pos_dev[0 .. m) of the selected sequence, attended together: a speculative step
    PACKED,     // the rows of n_segs prompts back to back, each segment with its own cache slot and pos0: packed prefill
    LAST        // m rows of the selected sequence whose K / V go to the cache, while only the last row goes on (layer_last_row)
  } kind;
  int m, pos0;                                          // rows; first position on the host (SEQ, LAST)
  const int32_t* pos_dev; int n_splits;                 // position(s) on the device (SEQ at m == 1, SLOTS, VERIFY) and their attention splits
  const ChattsPrefillSegment* segs; int n_segs;         // PACKED
};

// RoPE + cache write (unless the qkv GEMM's epilogue did both) and causal attention of t rows `q` against the cache of `slot`
static int rope_attend(ChattsDecoder* d, int layer, int slot, float* q, float* out, int t, int pos0, const int32_t* pos0_dev, bool rope_done,
                       int ks, bool out_planes, chatts_stream_t stream) {
  const ChattsDecoderConfig& c = d->cfg;
  const ChattsLayerWeights& lw = d->layers[layer];
  ChattsKvCache kc = layer_cache(d, layer, slot);
  int rc;
  if (!rope_done && (rc = chatts_rope_kv_write(q, t, c.n_q, c.n_kv, lw.q_norm, lw.k_norm, c.rms_eps, d->w.cos_tab, d->w.sin_tab, pos0, pos0_dev,
                                               &kc, stream)) != 0) return rc;
  return attention_impl(q, t, c.n_q, c.n_kv, pos0, pos0_dev, &kc, out, out_planes ? d->b.planes_hi : nullptr, out_planes ? d->b.planes_lo : nullptr,
                        ks, d->b.workspace, d->b.workspace_bytes, stream);
}

// The attention stage between the qkv projection and o_proj - the one part that truly differs by the kind of rows.  tuned: the default
// kernels' choices for a chunk (key split, planes written by the attention kernel); the precision modes and packed rows run it plain:
// ks = 1, float32 output.  *wrote_planes: the attention kernel (or its combine) left its output in planes 0, o_proj's operand format.
static int attention_stage(ChattsDecoder* d, int layer, const Rows& R, bool tuned, bool rope_done, bool* wrote_planes, chatts_stream_t stream) {
  const ChattsDecoderConfig& c = d->cfg;
  const ChattsLayerWeights& lw = d->layers[layer];
  const int m = R.m, na = c.n_q * kHeadDim, qkv_n = (c.n_q + 2 * c.n_kv) * kHeadDim;
  ChattsKvCache kc = layer_cache(d, layer, R.kind == Rows::SLOTS ? 0 : d->cur_seq);      // (packed rows: one cache per segment)
  int rc;
  *wrote_planes = false;
  switch (R.kind) {
    case Rows::SEQ: {
      if (m == 1 && tuned)      // decode: RoPE + cache write fused into the attention kernel
        return chatts_attention_decode_fused(d->b.qkv, c.n_q, c.n_kv, lw.q_norm, lw.k_norm, c.rms_eps, d->w.cos_tab, d->w.sin_tab, R.pos0, R.pos_dev,
                                             &kc, d->b.attn, R.n_splits, d->b.workspace, d->b.workspace_bytes, stream);
      // long chunks: split the keys over 2 workgroups per (query tile, head) - one sequence has too few waves otherwise
      const int env_ks = opt_get(OPT_ATTN_KSPLIT, 0);
      // (the bf16x3 kernel is fast enough per tile that the second key split + its combine launch no longer pay: 73.3 us
      // against 74.0 + 12 at T = 798; the float32-MFMA kernel, CHATTS_ATTN_BF16X3=0, still wants the split)
      const bool f32_attn = opt_get(OPT_ATTN_BF16X3, 1) == 0;
      int ks = env_ks >= 1 && env_ks <= 4 ? env_ks : (m >= 256 && f32_attn ? 2 : 1);
      if (!tuned || chatts_attn_workspace(m, c.n_q, ks) > d->b.workspace_bytes) ks = 1;
      // ... and, on the plane path, let the attention kernel (or its combine) write o_proj's operand format itself
      *wrote_planes = tuned && m >= 16 && planes_path(d, m, na) && opt_get(OPT_ATTN_ROWS, 0) == 0;
      return rope_attend(d, layer, d->cur_seq, d->b.qkv, d->b.attn, m, R.pos0, R.pos_dev, rope_done, ks, *wrote_planes, stream);
    }
    case Rows::SLOTS:
    case Rows::VERIFY: {
      *wrote_planes = planes_path(d, m, na, lw.o8 != nullptr);      // the combine writes o_proj's operand format
      uint16_t* hi = *wrote_planes ? d->b.planes_hi : nullptr;
      uint16_t* lo = *wrote_planes ? d->b.planes_lo : nullptr;
      if (R.kind == Rows::VERIFY)
        return attention_verify_impl(d->b.qkv, m, c.n_q, c.n_kv, lw.q_norm, lw.k_norm, c.rms_eps, d->w.cos_tab, d->w.sin_tab, R.pos_dev, &kc,
                                     d->b.attn, hi, lo, R.n_splits, d->b.workspace, d->b.workspace_bytes, stream);
      return attention_decode_batched_impl(d->b.qkv, m, c.n_q, c.n_kv, lw.q_norm, lw.k_norm, c.rms_eps, d->w.cos_tab, d->w.sin_tab, 0, R.pos_dev, &kc,
                                           seq_stride(d), d->b.attn, hi, lo, R.n_splits, d->b.workspace, d->b.workspace_bytes, stream);
    }
    case Rows::PACKED:      // segment by segment, each against its own cache slot and positions
      for (int i = 0; i < R.n_segs; ++i) {
        const ChattsPrefillSegment& sg = R.segs[i];
        if ((rc = rope_attend(d, layer, sg.slot, d->b.qkv + (size_t)sg.row0 * qkv_n, d->b.attn + (size_t)sg.row0 * na, sg.t, sg.pos0, nullptr, false,
                              1, false, stream)) != 0) return rc;
      }
      return CHATTS_OK;
    case Rows::LAST: {
      if ((rc = chatts_rope_kv_write(d->b.qkv, m, c.n_q, c.n_kv, lw.q_norm, lw.k_norm, c.rms_eps, d->w.cos_tab, d->w.sin_tab, R.pos0, nullptr, &kc,
                                     stream)) != 0) return rc;
      // one query row against pos0 + t keys: spread the 64-key tiles over up to 16 workgroups per kv head (one workgroup walking 800
      // keys alone took 137 us in the round-2 trace)
      int ks = (R.pos0 + m + 63) / 64;
      if (ks > 16) ks = 16;
      if (ks < 1 || chatts_attn_workspace(1, c.n_q, ks) > d->b.workspace_bytes) ks = 1;
      if ((rc = chatts_attention(d->b.qkv + (size_t)(m - 1) * qkv_n, 1, c.n_q, c.n_kv, R.pos0 + m - 1, nullptr, &kc, d->b.attn, ks, d->b.workspace,
                                 d->b.workspace_bytes, stream)) != 0) return rc;
      return last_row_to_row0(d, m, stream);      // ... and from here on the layer is one row: row 0 of x
    }
  }
  return CHATTS_E_BADARG;
}

struct F16qBuf { chatts_f16* hi; uint8_t* lo8; uint8_t* sc; };
static F16qBuf f16q_buf(const ChattsDecoder* d, int pair) {
  const ChattsDecoderConfig& c = d->cfg;
  int maxdim = c.hidden > c.inter ? c.hidden : c.inter;
  if (c.n_q * kHeadDim > maxdim) maxdim = c.n_q * kHeadDim;
  const size_t plane = (size_t)((d->b.t_max + 31) / 32 * 32) * maxdim;      // elements of one bf16 plane (rows rounded up to 32: the tiled planes
                                                                           // hold whole 16-row blocks) = bytes of the e4m3 plane
  F16qBuf b;
  b.hi = reinterpret_cast<chatts_f16*>(pair ? d->b.planes2_hi : d->b.planes_hi);
  b.lo8 = reinterpret_cast<uint8_t*>(pair ? d->b.planes2_lo : d->b.planes_lo);
  b.sc = b.lo8 + plane;
  return b;
}

// f16q mode, one sequence's chunk of >= kF16qMinRows rows (Rows::SEQ): both halves.  Every operand travels as f16q planes: pair 0 is
// the input of qkv / o_proj / gate_up, pair 1 the SwiGLU output that down_proj reads.
static int layer_half_f16q(ChattsDecoder* d, int layer, int part, const Rows& R, chatts_stream_t stream) {
  StageRange stage(part == 0 ? "chatts.layer.attn.f16q" : "chatts.layer.mlp.f16q");
  const ChattsDecoderConfig& c = d->cfg;
  const ChattsLayerWeights& lw = d->layers[layer];
  const int H = c.hidden, na = c.n_q * kHeadDim, t = R.m;
  const F16qBuf A = f16q_buf(d, 0), B = f16q_buf(d, 1);
  d->normed = false;
  int rc;
  bool attn_planes;      // (always false here: the attention stage runs plain)
  auto args = [&](const Proj& p, const F16qBuf& in, int epilogue) {
    ChattsLinearF16qArgs q{};
    q.a_hi = in.hi; q.a_lo8 = in.lo8; q.a_scale = in.sc; q.ld_a = p.k; q.ld_scale = p.k / 128;
    q.w16 = p.w16; q.w8 = p.q8; q.w8_exp = p.q8e; q.ldw = p.k; q.bias = p.bias; q.m = t; q.n = p.n; q.k = p.k;
    q.ldc = out_cols(p, epilogue); q.epilogue = epilogue;
    q.workspace = d->b.workspace; q.workspace_bytes = d->b.workspace_bytes;
    q.planes_tiled = 1; q.w_tiled = 1;      // every plane set and both weight copies in the kernel's own 1 KB / 512 B block order
    return q;
  };
  // pair 0 = RMSNorm(x), unless the projection before this one already wrote it (d->normed_q)
  auto norm_into_A = [&](const float* norm_w) {
    const bool have = d->normed_q;
    d->normed_q = false;
    return have ? CHATTS_OK : chatts_rmsnorm_f16q(d->b.x, norm_w, A.hi, A.lo8, A.sc, H, H / 128, t, H, c.rms_eps, 1, stream);
  };
  // a residual projection: its destination, and RMSNorm(x) for the projection after it - only inside the entry points that run the
  // layers back to back (d->chain) on one rank
  auto resid_into_x = [&](ChattsLinearF16qArgs& q, const float* next_norm_w) {
    resid_dest(d, &q, false, d->b.x);
    if (!d->chain || c.tp_world > 1 || !next_norm_w) return;
    q.post_norm_w = next_norm_w; q.post_norm_eps = c.rms_eps;
    q.post_hi = A.hi; q.post_lo8 = A.lo8; q.post_scale = A.sc; q.ld_post = H; q.ld_pscale = H / 128;
    d->normed_q = true;
  };
  ChattsLinearF16qArgs q;
  if (part == 0) {
    if ((rc = norm_into_A(lw.input_norm)) != 0) return rc;
    q = args(proj(d, layer, QKV), A, CHATTS_EPI_NONE);
    q.c = d->b.qkv;
    if ((rc = chatts_linear_f16q(&q, stream)) != 0) return rc;
    if ((rc = attention_stage(d, layer, R, false, false, &attn_planes, stream)) != 0) return rc;
    if ((rc = chatts_split_f16q(d->b.attn, t, na, na, A.hi, A.lo8, A.sc, na, na / 128, 1, stream)) != 0) return rc;
    q = args(proj(d, layer, O), A, CHATTS_EPI_NONE);
    resid_into_x(q, lw.post_norm);
    return chatts_linear_f16q(&q, stream);
  }
  if ((rc = norm_into_A(lw.post_norm)) != 0) return rc;
  q = args(proj(d, layer, GATE_UP), A, CHATTS_EPI_SWIGLU);
  q.c_hi = B.hi; q.c_lo8 = B.lo8; q.c_scale = B.sc; q.ld_cplanes = c.inter; q.ld_cscale = c.inter / 128;
  if ((rc = chatts_linear_f16q(&q, stream)) != 0) return rc;
  q = args(proj(d, layer, DOWN), B, CHATTS_EPI_NONE);
  resid_into_x(q, layer + 1 < c.n_layers ? d->layers[layer + 1].input_norm : nullptr);
  return chatts_linear_f16q(&q, stream);
}

// Speed mode, one projection: rows of `src` quantised per token (after RMSNorm with norm_w, when given) into scratch set `set`, then the
// fp8 x fp8 GEMM on them into c - or, c == NULL, to the residual destination.  Scratch sets (bytes | row scales): 0 = planes_hi | xn
// (qkv, gate_up), 1 = planes_lo | xn + t_max (o_proj), 2 = planes2_hi | xn + t_max (down_proj).
static int fp8_proj(ChattsDecoder* d, const Proj& p, int t, const float* src, const float* norm_w, int set, int epilogue, float* c,
                    chatts_stream_t stream) {
  uint8_t* a8 = reinterpret_cast<uint8_t*>(set == 0 ? d->b.planes_hi : set == 1 ? d->b.planes_lo : d->b.planes2_hi);
  float* scale = set == 0 ? d->b.xn : d->b.xn + d->b.t_max;
  const int rc = chatts_quantize_rows_fp8(src, t, p.k, p.k, norm_w, norm_w ? d->cfg.rms_eps : 0.f, a8, p.k, scale, stream);
  if (rc) return rc;
  ChattsLinearFp8Args f{};
  f.a8 = a8; f.a_scale = scale; f.w8 = p.w8; f.w_scale = p.w8_scale; f.bias = p.bias; f.c = c;
  f.m = t; f.n = p.n; f.k = p.k; f.lda8 = p.k; f.ldw8 = p.k; f.ldc = out_cols(p, epilogue); f.epilogue = epilogue;
  if (!c) resid_dest(d, &f, false, d->b.x);
  return chatts_linear_fp8(&f, stream);
}

// speed mode, chunks of >= 16 rows of one sequence (Rows::SEQ) or of packed prompts (Rows::PACKED, attention half): both halves
static int layer_half_fp8(ChattsDecoder* d, int layer, int part, const Rows& R, chatts_stream_t stream) {
  const ChattsLayerWeights& lw = d->layers[layer];
  const int t = R.m;
  d->normed = false; d->normed_q = false;
  int rc;
  bool attn_planes;      // (always false here: the attention stage runs plain)
  if (part == 0) {
    if ((rc = fp8_proj(d, proj(d, layer, QKV), t, d->b.x, lw.input_norm, 0, CHATTS_EPI_NONE, d->b.qkv, stream)) != 0) return rc;
    if ((rc = attention_stage(d, layer, R, false, false, &attn_planes, stream)) != 0) return rc;
    return fp8_proj(d, proj(d, layer, O), t, d->b.attn, nullptr, 1, CHATTS_EPI_NONE, nullptr, stream);
  }
  if ((rc = fp8_proj(d, proj(d, layer, GATE_UP), t, d->b.x, lw.post_norm, 0, CHATTS_EPI_SWIGLU, d->b.act, stream)) != 0) return rc;
  return fp8_proj(d, proj(d, layer, DOWN), t, d->b.act, nullptr, 2, CHATTS_EPI_NONE, nullptr, stream);
}

// ---- the default kernels: attention half and MLP half, once each -----------------------------------------------------------------
// RMSNorm -> qkv (+ bias) -> RoPE / cache write / attention -> o_proj (+ residual, or the partial sum for the TP all-reduce)
static int attn_half(ChattsDecoder* d, int layer, const Rows& R, chatts_stream_t stream) {
  const ChattsDecoderConfig& c = d->cfg;
  const ChattsLayerWeights& lw = d->layers[layer];
  const int H = c.hidden, na = c.n_q * kHeadDim, m = R.m;
  const bool tp = c.tp_world > 1;
  // What differs by entry point, besides the attention stage:
  const bool seq = R.kind == Rows::SEQ, last = R.kind == Rows::LAST;
  const bool gemv = seq && m == 1;              // decode_step (layer_part at t == 1): norm fused in the GEMV prologue, 8- and 4-bit copies
  const bool slots = R.kind == Rows::SLOTS || R.kind == Rows::VERIFY;      // decode_step_batched / spec_step: 8-bit copies, ping-pong
  const Copies qkv_copies = gemv ? W8_W4 : slots ? W8 : BF16;               // (prefill, prefill_last, prefill_packed: bf16 only)
  const Copies o_copies = gemv || last ? W8_W4 : slots ? W8 : BF16;         // (the last row's o_proj is a GEMV like the decode step's)
  const bool rope_in_gemm = seq && m > 1 && opt_get(OPT_ROPE_FUSE, 1) != 0;    // prefill / prefill_last: the qkv GEMM's split-K epilogue (when
                                                                            // it has one) also rotates q / k and fills the cache
  const bool split_attn = seq || R.kind == Rows::PACKED;                    // float32 attention output on the plane path: split it for o_proj
  const bool next_fp8 = slots && lw.gate_up8 != nullptr;                    // planes_path flag of the projection after o_proj (prefill: false)
  int rc;
  ChattsLinearArgs la = linear_args(d, proj(d, layer, QKV), m, CHATTS_EPI_NONE, qkv_copies);
  la.c = d->b.qkv;
  if (gemv) norm_in_launch(d, d->b.x, lw.input_norm, &la);
  else if ((rc = norm_into(d, lw.input_norm, &la, stream)) != 0) return rc;
  bool rope_done = false;
  if (rope_in_gemm) {
    ChattsKvCache kc = layer_cache(d, layer, d->cur_seq);
    RopeFuse rf;
    if ((rc = rope_fuse_prepare(m, c.n_q, c.n_kv, lw.q_norm, lw.k_norm, c.rms_eps, d->w.cos_tab, d->w.sin_tab, R.pos0, R.pos_dev, &kc, &rf)) != 0)
      return rc;
    if ((rc = linear_impl(&la, stream, &rf, &rope_done)) != 0) return rc;
  } else if ((rc = chatts_linear(&la, stream)) != 0) {
    return rc;
  }
  bool attn_planes = false;
  if ((rc = attention_stage(d, layer, R, true, rope_done, &attn_planes, stream)) != 0) return rc;

  la = linear_args(d, proj(d, layer, O), last ? 1 : m, CHATTS_EPI_NONE, o_copies);
  la.a = d->b.attn;
  if (attn_planes) {
    a_planes(d, 0, &la);
  } else if (split_attn && planes_path(d, m, na)) {      // the VALU attention kernel writes float32: split it
    if ((rc = chatts_split_bf16x2(d->b.attn, m, na, na, d->b.planes_hi, d->b.planes_lo, na, stream)) != 0) return rc;
    a_planes(d, 0, &la, KEEP_F32);
  }
  // x += sum over the ranks inside the GEMV launch: the decode step when it asked for it (d->fuse_tp), the last row always
  resid_dest(d, &la, ((gemv && d->fuse_tp && d->tp) || last) && !la.w4, d->b.x);
  if (slots) {
    // The residual stream ping-pongs x -> xn (here) -> x (down_proj) inside a chained step, so that the post-norm epilogue may use
    // several workgroups per row (they read resid columns other workgroups update: c must not alias resid).
    d->x_in_xn = !tp && d->chain && d->b.xn && m <= 16 && planes_path(d, m, H, next_fp8);
    if (d->x_in_xn) la.c = d->b.xn;
  }
  if (!last) request_post_norm(d, &la, lw.post_norm, next_fp8);
  if (slots && d->x_in_xn && !la.post_norm_w) { la.c = d->b.x; d->x_in_xn = false; }      // not fused after all: the norm launch reads x
  rc = chatts_linear(&la, stream);
  if (last && rc == CHATTS_OK && tp && !d->tp_fused) rc = chatts_allreduce(d->tp, d->b.delta, d->b.x, d->b.x, H, stream);
  return rc;
}

// RMSNorm -> gate_up + SwiGLU -> down (+ residual / partial).  Rows::SEQ (packed prefill and the last row run it as such) or SLOTS / VERIFY.
static int mlp_half(ChattsDecoder* d, int layer, const Rows& R, chatts_stream_t stream) {
  const ChattsDecoderConfig& c = d->cfg;
  const ChattsLayerWeights& lw = d->layers[layer];
  const int H = c.hidden, m = R.m;
  const bool last_layer = layer + 1 >= c.n_layers;
  // What differs by entry point:
  const bool gemv = R.kind == Rows::SEQ && m == 1;      // decode_step, and row 0 of layer_last_row: fused norm, 8- and 4-bit copies
  const bool slots = R.kind == Rows::SLOTS || R.kind == Rows::VERIFY;      // decode_step_batched / spec_step: 8-bit copies
  const Copies copies = gemv ? W8_W4 : slots ? W8 : BF16;                   // (prefill chunks: bf16 only)
  // SwiGLU output straight into down_proj's operand planes.  Prefill asks for down_proj's K alone; the batched step asks with each
  // projection's own 8-bit flag and wants gate_up on the plane path too.
  const bool act_planes = slots ? planes_path(d, m, c.inter, lw.down8 != nullptr) && planes_path(d, m, H, lw.gate_up8 != nullptr)
                                : m > 1 && planes_path(d, m, c.inter);
  const float* resid_in = slots && d->x_in_xn ? d->b.xn : d->b.x;           // batched ping-pong: o_proj left the residual stream in xn
  // what down_proj pre-norms for: the next layer's qkv; after the last layer final_norm + lm_head in the batched step
  // (chatts_decoder_logits_batched follows) and nothing for one sequence (chatts_decoder_logits norms its one row in the GEMV)
  const float* next_norm_w = !last_layer ? d->layers[layer + 1].input_norm : slots ? d->w.final_norm : nullptr;
  const bool next_fp8 = slots && (!last_layer ? d->layers[layer + 1].qkv8 : d->w.lm_head8) != nullptr;
  int rc;
  ChattsLinearArgs la = linear_args(d, proj(d, layer, GATE_UP), m, CHATTS_EPI_SWIGLU, copies);
  la.c = d->b.act;
  if (gemv) norm_in_launch(d, d->b.x, lw.post_norm, &la);
  else if ((rc = norm_into(d, lw.post_norm, &la, stream)) != 0) return rc;
  if (act_planes) c_planes(d, &la);
  if ((rc = chatts_linear(&la, stream)) != 0) return rc;

  la = linear_args(d, proj(d, layer, DOWN), m, CHATTS_EPI_NONE, copies);
  la.a = d->b.act;
  if (act_planes) a_planes(d, 1, &la);
  resid_dest(d, &la, gemv && d->fuse_tp && d->tp && !la.w4, resid_in);
  if (slots) d->x_in_xn = false;
  request_post_norm(d, &la, next_norm_w, next_fp8);
  return chatts_linear(&la, stream);
}

constexpr int kFp8MinRows = 16;       // speed mode: chunks below this take the default kernels

// One layer half on rows R: the precision mode that applies to these rows, or the default kernels.
static int layer_half(ChattsDecoder* d, int layer, int part, const Rows& R, chatts_stream_t stream) {
  const bool chunk = R.kind == Rows::SEQ || R.kind == Rows::PACKED;      // the opt-in modes are for prefill chunks only
  if (chunk && d->prefill_fp8 && R.m >= kFp8MinRows) return layer_half_fp8(d, layer, part, R, stream);
  if (R.kind == Rows::SEQ && d->prefill_f16q && R.m >= kF16qMinRows) return layer_half_f16q(d, layer, part, R, stream);
  d->normed_q = false;        // (a following f16q half recomputes its norm: planes 0 are about to hold bf16 data)
  if (part == 0 && (R.kind == Rows::PACKED || R.kind == Rows::LAST)) return attn_half(d, layer, R, stream);      // (no stage range of their own)
  StageRange stage(part == 0 ? "chatts.layer.attn" : "chatts.layer.mlp");
  return part == 0 ? attn_half(d, layer, R, stream) : mlp_half(d, layer, R, stream);
}

extern "C" int chatts_decoder_layer_part(ChattsDecoder* d, int layer, int part, int t, int pos0,
                                         const int32_t* pos0_dev, int n_splits, chatts_stream_t stream) {
  CHATTS_REQUIRE(d && layer >= 0 && layer < d->cfg.n_layers && (part == 0 || part == 1), CHATTS_E_BADARG,
                 "decoder_layer_part: bad arguments");
  CHATTS_REQUIRE(t >= 1 && t <= d->b.t_max, CHATTS_E_SHAPE, "decoder_layer_part: t=%d exceeds buffers (%d)", t, d->b.t_max);
  return layer_half(d, layer, part, Rows{Rows::SEQ, t, pos0, pos0_dev, n_splits, nullptr, 0}, stream);
}

extern "C" int chatts_decoder_layer_part_add(ChattsDecoder* d, int add_delta, int layer, int part, int t, int pos0,
                                             const int32_t* pos0_dev, int n_splits, chatts_stream_t stream) {
  CHATTS_REQUIRE(d && t >= 1 && t <= d->b.t_max, CHATTS_E_BADARG, "decoder_layer_part_add: bad arguments");
  if (add_delta) {
    CHATTS_REQUIRE(d->b.delta, CHATTS_E_BADARG, "decoder_layer_part_add: no delta buffer");
    const int rc = chatts_residual_add(d->b.x, d->b.delta, (int64_t)t * d->cfg.hidden, stream);
    if (rc) return rc;
  }
  return chatts_decoder_layer_part(d, layer, part, t, pos0, pos0_dev, n_splits, stream);
}

// rows of a batched call: cache slots 0 .. batch - 1 (bounded by max_batch), or inside a speculative step its R verify rows
static int max_rows_batched(const ChattsDecoder* d) { return d->spec_rows > 0 ? d->spec_rows : max_batch(d); }

// Batched decode: `batch` sequences advance one token each.  Row b of x / qkv / attn /
// act belongs to sequence b (cache slot b, position pos_dev[b]).  The projections run as M = batch GEMMs (bf16x2
// MFMA, weights streamed once for the whole batch); attention runs per sequence on its own cache.
extern "C" int chatts_decoder_layer_part_batched(ChattsDecoder* d, int layer, int part, int batch,
                                                 const int32_t* pos_dev, int n_splits, chatts_stream_t stream) {
  CHATTS_REQUIRE(d && layer >= 0 && layer < d->cfg.n_layers && (part == 0 || part == 1) && pos_dev, CHATTS_E_BADARG,
                 "decoder_layer_part_batched: bad arguments");
  const int maxb = max_rows_batched(d);      // (max_batch guards cache slots)
  CHATTS_REQUIRE(batch >= 1 && batch <= maxb && batch <= d->b.t_max, CHATTS_E_SHAPE,
                 "decoder_layer_part_batched: batch %d exceeds max_batch %d", batch, maxb);
  return layer_half(d, layer, part, Rows{d->spec_rows > 0 ? Rows::VERIFY : Rows::SLOTS, batch, 0, pos_dev, n_splits, nullptr, 0}, stream);
}

// final norm + lm_head for rows 0 .. batch-1 of x (cache slots 0 .. batch-1) -> logits_all [batch, vocab_local]: the tail of a
// batched step (compute_logits for a batch, chatts_vllm.py:603-610).  M = batch weight-streaming GEMM on this rank's vocabulary slice.
extern "C" int chatts_decoder_logits_batched(ChattsDecoder* d, int batch, float* logits_all, chatts_stream_t stream) {
  CHATTS_REQUIRE(d && logits_all, CHATTS_E_BADARG, "decoder_logits_batched: null argument");
  const int maxb = max_rows_batched(d);
  CHATTS_REQUIRE(batch >= 1 && batch <= maxb && batch <= d->b.t_max, CHATTS_E_SHAPE, "decoder_logits_batched: batch %d exceeds max_batch %d",
                 batch, maxb);
  ChattsLinearArgs la = linear_args(d, proj(d, 0, LM_HEAD), batch, CHATTS_EPI_NONE, W8);
  la.c = logits_all;
  const int rc = norm_into(d, d->w.final_norm, &la, stream);      // binds planes a fused epilogue already wrote (d->normed), or launches the norm
  if (rc) return rc;
  return chatts_linear(&la, stream);
}

extern "C" int chatts_decoder_logits(ChattsDecoder* d, int row, chatts_stream_t stream) {
  CHATTS_REQUIRE(d && row >= 0 && row < d->b.t_max, CHATTS_E_BADARG, "decoder_logits: bad row");
  StageRange stage("chatts.logits");
  ChattsLinearArgs la = linear_args(d, proj(d, 0, LM_HEAD), 1, CHATTS_EPI_NONE, W8);
  la.c = d->b.logits;
  norm_in_launch(d, d->b.x + (size_t)row * d->cfg.hidden, d->w.final_norm, &la);
  return chatts_linear(&la, stream);
}

// ---- the layer loop --------------------------------------------------------------------------------------------------------------
// Layers [first, last): half(layer, part) for part 0 and 1, each followed by sum() - the tensor-parallel sum of the half's partial
// result into x (sum_bulk, sum_unless_fused), or nothing.  Stops at the first error and returns it.
template <class Half, class Sum>
static int run_layers(int first, int last, Half half, Sum sum) {
  int rc = CHATTS_OK;
  for (int l = first; l < last && rc == CHATTS_OK; ++l)
    for (int part = 0; part < 2 && rc == CHATTS_OK; ++part)
      if ((rc = half(l, part)) == CHATTS_OK) rc = sum();
  return rc;
}
static int no_sum() { return CHATTS_OK; }

// tensor parallel: can the [t, H] sums between the layer halves run as chatts_allreduce_bulk launches of the same call?
static bool tp_bulk_ready(const ChattsDecoder* d, int t) {
  return d->tp && chatts_tp_bulk_elems(d->tp) >= (int64_t)t * d->cfg.hidden;
}
#define CHATTS_REQUIRE_TP_BULK(d, t, name)                                                                                         \
  CHATTS_REQUIRE((d)->cfg.tp_world == 1 || tp_bulk_ready((d), (t)), CHATTS_E_BADARG,                                                \
                 name ": tp_world = %d needs an attached exchange whose bulk region holds t * hidden = %lld float32 (chatts_tp_buffer_bytes_bulk); " \
                 "otherwise drive chatts_decoder_layer_part_add and all-reduce buffers.delta yourself", (d)->cfg.tp_world,          \
                 (long long)(t) * (d)->cfg.hidden)
// prefill chunks: x[0:t] += sum over the ranks of delta[0:t]
static int sum_bulk(ChattsDecoder* d, int t, chatts_stream_t stream) {
  if (d->cfg.tp_world <= 1) return CHATTS_OK;
  return chatts_allreduce_bulk(d->tp, d->b.delta, d->b.x, (int64_t)t * d->cfg.hidden, stream);
}
// decode rows: x[0:rows] += sum over the ranks of delta[0:rows], unless the projection's own launch carried the exchange (d->tp_fused)
static int sum_unless_fused(ChattsDecoder* d, int rows, chatts_stream_t stream) {
  if (d->cfg.tp_world <= 1 || d->tp_fused) return CHATTS_OK;
  return chatts_allreduce(d->tp, d->b.delta, d->b.x, d->b.x, (int64_t)rows * d->cfg.hidden, stream);
}
// layers [first, last) of one sequence's chunk of t rows at pos0
static int run_chunk_layers(ChattsDecoder* d, int first, int last, int t, int pos0, chatts_stream_t stream) {
  return run_layers(first, last, [&](int l, int part) { return chatts_decoder_layer_part(d, l, part, t, pos0, nullptr, 1, stream); },
                    [&] { return sum_bulk(d, t, stream); });
}

// ---- the whole-pass entry points -------------------------------------------------------------------------------------------------
// One greedy step for `batch` sequences (TP = 1): all layers, final norm + lm_head for every row, per-sequence
// argmax (token / step / pos / out_tokens rows advance independently; pos saturates at max_ctx - 1).
// logits_all: [batch, vocab_local] float32 scratch owned by the caller.
extern "C" int chatts_decoder_decode_step_batched(ChattsDecoder* d, int batch, int32_t* pos_dev, int32_t* step_dev,
                                                  int64_t* token_dev, float* token_logit_dev, int64_t* out_tokens,
                                                  int64_t out_stride, float* logits_all, int n_splits,
                                                  chatts_stream_t stream) {
  CHATTS_REQUIRE(d && pos_dev && step_dev && token_dev && logits_all, CHATTS_E_BADARG, "decode_step_batched: null argument");
  StageRange stage("chatts.decode_step_batched");
  const bool tp = d->cfg.tp_world > 1;
  CHATTS_REQUIRE(!tp || d->tp, CHATTS_E_BADARG, "decode_step_batched: tp_world = %d but no exchange attached (chatts_decoder_set_tp)",
                 d->cfg.tp_world);
  CHATTS_REQUIRE(!tp || chatts_tp_pending(d->tp) == 0, CHATTS_E_BADARG, "decode_step_batched: the exchange has %d collectives whose epochs were "
                 "never settled (chatts_tp_flush_epochs)", tp ? chatts_tp_pending(d->tp) : 0);
  int rc;
  const ChattsDecoderConfig& c = d->cfg;
  // the step STARTS by loading the input embeddings from the current tokens (so a prefill of another request may
  // use x between two steps) and ENDS with the per-sequence argmax
  if ((rc = chatts_embed_token_batched(token_dev, batch, d->w.embed, embed_offset(d), embed_rows(d), c.hidden, d->b.x,
                                       stream)) != 0) return rc;
  Pass pass(d, /*chain=*/true);      // layers run back to back: a projection may write the next one's normed operand
  rc = run_layers(0, c.n_layers, [&](int l, int part) { return chatts_decoder_layer_part_batched(d, l, part, batch, pos_dev, n_splits, stream); },
                  [&] { return sum_unless_fused(d, batch, stream); });
  if (rc) return rc;
  if ((rc = chatts_decoder_logits_batched(d, batch, logits_all, stream)) != 0) return rc;
  return chatts_decoder_select_tokens(d, logits_all, batch, c.vocab_local, token_dev, token_logit_dev, out_tokens, out_stride, step_dev,
                                      pos_dev, c.max_ctx - 1, nullptr, stream);
}

extern "C" int chatts_decoder_prefill(ChattsDecoder* d, int t, int pos0, chatts_stream_t stream) {
  CHATTS_REQUIRE(d, CHATTS_E_BADARG, "decoder_prefill: null decoder");
  CHATTS_REQUIRE(t >= 1 && t <= d->b.t_max, CHATTS_E_SHAPE, "decoder_prefill: t=%d exceeds buffers (%d)", t, d->b.t_max);
  CHATTS_REQUIRE_TP_BULK(d, t, "decoder_prefill");
  StageRange stage("chatts.prefill");
  Pass pass(d, /*chain=*/true);
  return run_chunk_layers(d, 0, d->cfg.n_layers, t, pos0, stream);
}

// The LAST layer of a prefill whose only consumers are the next token and the KV cache: K / V of every row are needed
// (cache), everything else only for the last row.  So: RMSNorm + qkv GEMM + RoPE / cache write for all t rows as usual, then
// the last row alone is attended (t = 1 against the cache), moved to row 0 of the residual stream and taken through o_proj
// and the MLP as weight-streaming GEMVs.  Saves one layer's attention + o / gate_up / down GEMMs (~0.9 of 44 ms at the
// benchmark prompt).  The result lives in row 0 of x (rows 1.. are stale).  (f16q mode: this layer runs the default kernels.)
static int layer_last_row(ChattsDecoder* d, int layer, int t, int pos0, chatts_stream_t stream) {
  int rc = layer_half(d, layer, 0, Rows{Rows::LAST, t, pos0, nullptr, 1, nullptr, 0}, stream);
  if (rc) return rc;
  d->fuse_tp = d->cfg.tp_world > 1;      // for this half only: the exchange rides in the down_proj GEMV, as in a decode step
  rc = chatts_decoder_layer_part(d, layer, 1, 1, 0, nullptr, 1, stream);      // MLP on row 0: the decode path's GEMVs
  d->fuse_tp = false;
  return rc == CHATTS_OK ? sum_unless_fused(d, 1, stream) : rc;
}

extern "C" int chatts_decoder_prefill_last(ChattsDecoder* d, int t, int pos0, chatts_stream_t stream) {
  CHATTS_REQUIRE(d, CHATTS_E_BADARG, "decoder_prefill_last: null decoder");
  CHATTS_REQUIRE(t >= 1 && t <= d->b.t_max, CHATTS_E_SHAPE, "decoder_prefill_last: t=%d exceeds buffers (%d)", t, d->b.t_max);
  CHATTS_REQUIRE_TP_BULK(d, t, "decoder_prefill_last");
  StageRange stage("chatts.prefill_last");
  const int L = d->cfg.n_layers;
  Pass pass(d, /*chain=*/true);
  int rc = run_chunk_layers(d, 0, L - 1, t, pos0, stream);
  if (rc == CHATTS_OK && d->prefill_fp8 && t >= kFp8MinRows) {      // speed mode: the final layer at full width too, then the last row moves to row 0
    rc = run_chunk_layers(d, L - 1, L, t, pos0, stream);
    if (rc == CHATTS_OK) rc = last_row_to_row0(d, t, stream);
  } else if (rc == CHATTS_OK) {
    rc = layer_last_row(d, L - 1, t, pos0, stream);
  }
  // the last row's o_proj / down_proj carried their exchange without advancing the device-side call counter (host-counted epochs):
  // settle it here, always, so that whatever runs next on this communicator - a replayed decode graph above all - starts from a flushed count
  if (d->cfg.tp_world > 1 && d->tp) { const int frc = chatts_tp_flush_epochs(d->tp, stream); if (rc == CHATTS_OK) rc = frc; }
  return rc;
}

// Packed multi-prompt prefill: the rows of several prompts (or of their not-yet-cached tails) sit
// back to back in x; everything row-wise - norms, the four projections, SwiGLU, residuals - runs ONCE over all rows (one big-M
// GEMM instead of one ragged small-M GEMM per prompt), only RoPE / cache write / attention run per segment, each against
// its own cache slot and positions (Rows::PACKED: ks = 1 and no attention-written planes).  Speed mode: qkv and o_proj as fp8 x fp8
// GEMMs like any chunk; f16q mode: the attention half runs the default kernels, the MLP half is a chunk's.
extern "C" int chatts_decoder_prefill_packed(ChattsDecoder* d, const ChattsPrefillSegment* segs, int n_segs, chatts_stream_t stream) {
  CHATTS_REQUIRE(d && segs && n_segs >= 1, CHATTS_E_BADARG, "decoder_prefill_packed: bad arguments");
  CHATTS_REQUIRE(d->cfg.tp_world == 1, CHATTS_E_BADARG, "decoder_prefill_packed: tensor_parallel_size 1 only");
  const int maxb = max_batch(d);
  int t = 0;
  for (int i = 0; i < n_segs; ++i) {
    const ChattsPrefillSegment& sg = segs[i];
    CHATTS_REQUIRE(sg.t >= 1 && sg.row0 == t && sg.pos0 >= 0 && sg.pos0 + sg.t <= d->cfg.max_ctx && sg.slot >= 0 && sg.slot < maxb,
                   CHATTS_E_SHAPE, "decoder_prefill_packed: segment %d (row0 %d, t %d, pos0 %d, slot %d) is not contiguous / out of range",
                   i, sg.row0, sg.t, sg.pos0, sg.slot);
    for (int j = 0; j < i; ++j)
      CHATTS_REQUIRE(segs[j].slot != sg.slot, CHATTS_E_BADARG, "decoder_prefill_packed: cache slot %d appears twice", sg.slot);
    t += sg.t;
  }
  CHATTS_REQUIRE(t <= d->b.t_max, CHATTS_E_SHAPE, "decoder_prefill_packed: %d rows exceed buffers (%d)", t, d->b.t_max);
  StageRange stage("chatts.prefill_packed");
  Pass pass(d, /*chain=*/true);
  const Rows packed{Rows::PACKED, t, 0, nullptr, 1, segs, n_segs};
  return run_layers(0, d->cfg.n_layers, [&](int l, int part) {
    return part == 0 ? layer_half(d, l, 0, packed, stream) : chatts_decoder_layer_part(d, l, 1, t, 0, nullptr, 1, stream);
  }, no_sum);
}

extern "C" int chatts_decoder_decode_step(ChattsDecoder* d, int32_t* pos_dev, int32_t* step_dev, int64_t* token_dev,
                                          float* token_logit_dev, int64_t* out_tokens, int n_splits,
                                          chatts_stream_t stream) {
  CHATTS_REQUIRE(d && pos_dev && step_dev && token_dev, CHATTS_E_BADARG, "decode_step: null argument");
  StageRange stage("chatts.decode_step");
  const bool tp = d->cfg.tp_world > 1;
  CHATTS_REQUIRE(!tp || d->tp, CHATTS_E_BADARG, "decode_step: tp_world = %d but no exchange attached (chatts_decoder_set_tp)", d->cfg.tp_world);
  CHATTS_REQUIRE(!tp || chatts_tp_pending(d->tp) == 0, CHATTS_E_BADARG, "decode_step: the exchange has %d collectives whose epochs were never settled "
                 "(chatts_tp_flush_epochs): a step enqueued or captured now would reuse their epochs", tp ? chatts_tp_pending(d->tp) : 0);
  int rc;
  {
    // Tensor parallel: the two exchanges of a layer ride in the o_proj / down_proj GEMV launches (6 launches per layer instead of 8;
    // CHATTS_TP_FUSE=0 keeps the stand-alone chatts_allreduce kernels: same bits - tests/test_gpu_tp_p2p.py)
    Pass pass(d, /*chain=*/false, /*spec_rows=*/0, /*fuse_tp=*/tp && opt_get(OPT_TP_FUSE, 1) != 0);
    rc = run_layers(0, d->cfg.n_layers, [&](int l, int part) { return chatts_decoder_layer_part(d, l, part, 1, 0, pos_dev, n_splits, stream); },
                    [&] { return sum_unless_fused(d, 1, stream); });
  }
  if (rc) {      // a refused launch part-way: settle the epochs of the exchange-carrying GEMVs that WERE issued (every rank fails alike)
    if (tp) (void)chatts_tp_flush_epochs(d->tp, stream);
    return rc;
  }
  if ((rc = chatts_decoder_logits(d, 0, stream)) != 0) return rc;
  if ((rc = chatts_decoder_select_tokens(d, d->b.logits, 1, d->cfg.vocab_local, token_dev, token_logit_dev, out_tokens, 0, step_dev,
                                         pos_dev, 0, nullptr, stream)) != 0) return rc;
  return chatts_embed_token(token_dev, d->w.embed, embed_offset(d), embed_rows(d), d->cfg.hidden, d->b.x, stream);
}

// One speculative step (spec_decode.hip; include/chatts_amd.h): R = k + 1 rows of the selected sequence - its last chosen token and k
// drafts from its own history - through the batched-row projections in ONE pass over the weights, the verify attention in place of
// the per-slot attention, then per-row argmax and the accept / rollback kernel.  Device-driven like the plain step: capture once, replay.
extern "C" int chatts_decoder_spec_step(ChattsDecoder* d, const ChattsSpecArgs* a, chatts_stream_t stream) {
  CHATTS_REQUIRE(d && a, CHATTS_E_BADARG, "decoder_spec_step: null argument");
  CHATTS_REQUIRE(a->hist && a->draft && a->spec_tokens && a->argmax && a->logits && a->pos_dev && a->step_dev && a->token_dev &&
                     a->out_tokens && a->out_capacity_dev && a->counters, CHATTS_E_BADARG, "decoder_spec_step: null pointer in the arguments");
  CHATTS_REQUIRE(a->k >= 1 && a->k <= CHATTS_SPEC_MAX_DRAFT, CHATTS_E_BADARG, "decoder_spec_step: k = %d must be in 1..%d", a->k,
                 CHATTS_SPEC_MAX_DRAFT);
  CHATTS_REQUIRE(a->ngram_min >= 1 && a->ngram_max >= a->ngram_min && a->ngram_max <= CHATTS_SPEC_MAX_NGRAM, CHATTS_E_BADARG,
                 "decoder_spec_step: n-gram sizes %d..%d must satisfy 1 <= min <= max <= %d", a->ngram_min, a->ngram_max, CHATTS_SPEC_MAX_NGRAM);
  CHATTS_REQUIRE(d->cfg.tp_world <= 1, CHATTS_E_BADARG, "decoder_spec_step: tensor_parallel_size 1 only (tp_world = %d)", d->cfg.tp_world);
  CHATTS_REQUIRE(!d->sampling && !d->controls && !d->masks, CHATTS_E_BADARG,
                 "decoder_spec_step: greedy decoding only (a sampler, logit controls or logit masks are set on the decoder)");
  const ChattsDecoderConfig& c = d->cfg;
  const int R = a->k + 1;
  CHATTS_REQUIRE(R <= d->b.t_max && R < c.max_ctx, CHATTS_E_SHAPE, "decoder_spec_step: %d rows exceed the buffers (%d) or the context", R,
                 d->b.t_max);
  int ns = a->n_splits < 1 ? 1 : (a->n_splits > 64 ? 64 : a->n_splits);      // clamped before anything is enqueued
  while (ns > 1 && chatts_attn_workspace(R, c.n_q, ns) > d->b.workspace_bytes) ns /= 2;      // fewer, longer tile slots: the partials must fit
  CHATTS_REQUIRE(d->b.workspace && chatts_attn_workspace(R, c.n_q, ns) <= d->b.workspace_bytes, CHATTS_E_WORKSPACE,
                 "decoder_spec_step: the workspace does not hold the attention partials of %d rows", R);
  StageRange stage("chatts.spec_step");
  int rc;
  const int64_t vocab = embed_offset(d) + embed_rows(d);
  if (!a->skip_propose &&
      (rc = chatts_spec_propose(a->pos_dev, a->hist, c.max_ctx, a->k, a->ngram_min, a->ngram_max, vocab, a->draft, a->spec_tokens, stream)) != 0)
    return rc;
  if ((rc = chatts_embed_token_batched(a->spec_tokens, R, d->w.embed, embed_offset(d), embed_rows(d), c.hidden, d->b.x, stream)) != 0) return rc;
  Pass pass(d, /*chain=*/true, /*spec_rows=*/R);      // the batched halves and the logits take R verify rows of the selected sequence
  rc = run_layers(0, c.n_layers, [&](int l, int part) { return chatts_decoder_layer_part_batched(d, l, part, R, a->pos_dev, ns, stream); }, no_sum);
  if (rc == CHATTS_OK) rc = chatts_decoder_logits_batched(d, R, a->logits, stream);
  if (rc) return rc;
  // per-row argmax without side effects (the split-K / attention workspace is idle here)
  if ((rc = chatts::argmax_batched_scratch(a->logits, R, c.vocab_local, c.vocab_local, c.vocab_offset, a->argmax, nullptr, nullptr, 0, nullptr,
                                           nullptr, 0, d->b.workspace, d->b.workspace_bytes, reinterpret_cast<hipStream_t>(stream))) != 0)
    return rc;
  return chatts_spec_verify(a->argmax, a->draft, a->k, vocab, a->pos_dev, a->step_dev, a->token_dev, a->out_tokens, a->out_capacity_dev,
                            a->hist, c.max_ctx, a->counters, stream);
}
