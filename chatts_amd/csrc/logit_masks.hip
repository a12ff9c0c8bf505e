// logit_masks.hip - allowed_token_ids, logit_bias and min_tokens: the controls that constrain WHICH token may be chosen, applied to the
// logits of a step ahead of the penalties (vLLM V1's order: raw logits -> allowed_token_ids -> logit_bias -> min_tokens -> repetition ->
// frequency and presence -> [greedy rows: argmax] -> temperature -> min_p -> top-k -> top-p -> draw).
//
// State per row (plain device arrays, written at admission): an allow bitset (bit of global id i = word i / 32, bit i % 32) with an on
// flag; up to bias_stride (id, bias) pairs with their count; up to end_stride ids that would end the sequence, their count and min_tokens.
//   lm_apply_kernel    the grid and slice arithmetic of lc_apply_kernel (G = min(64, ceil(V / 1024)) workgroups of 256 threads per row):
//                      out[i] = (allow_on && !bit(i)) ? -inf : logits[i], 16-byte accesses when the rows are 16-byte aligned (one bitset
//                      word covers an aligned quad).  The logits travel as integers: a row with nothing set is copied bit for bit, NaN
//                      payloads included.
//   lm_sparse_kernel   one workgroup per row, after the dense pass on the stream: out[id] += bias for the row's pairs (distinct ids: nothing
//                      races; -inf + b stays -inf), a workgroup barrier, then -inf over the row's end ids while step[row] < min_tokens[row].
// The raw logits are only read.  Per-row settings come from device arrays at run time, so one captured decode step serves requests with
// different settings.  No atomics and no reductions: the same logits and settings give the same bits in every run, replay and cache slot.
#include "common.h"

namespace chatts {

constexpr int kLmThreads = 256;
constexpr int kLmMaxParts = 64;
constexpr uint32_t kLmNegInf = 0xff800000u;

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

struct LmParams {
  const float* logits;
  int64_t stride;
  int vocab, parts, chunk;          // chunk is a multiple of 4
  int64_t offset;                   // global id of logits[0]
  float* out;
  int64_t out_stride;
  const uint32_t* allow;            // NULL: no row has an allow list
  int64_t allow_stride;
  const int32_t* allow_on;
  const int32_t* bias_ids;          // NULL: no row has a bias
  const float* bias_val;
  const int32_t* bias_n;
  int64_t bias_stride;
  const int32_t* end_ids;           // NULL: no row has min_tokens
  const int32_t* end_n;
  const int32_t* min_tokens;
  int64_t end_stride;
  const int32_t* step;
  int vec;                          // every row of logits / out starts 16-byte aligned and offset is a multiple of 4
};

__global__ __launch_bounds__(kLmThreads) void lm_apply_kernel(LmParams q) {
  const int row = blockIdx.y, g = blockIdx.x, t = threadIdx.x;
  const uint32_t* L = reinterpret_cast<const uint32_t*>(q.logits + (size_t)row * q.stride);
  uint32_t* O = reinterpret_cast<uint32_t*>(q.out + (size_t)row * q.out_stride);
  const bool on = q.allow && q.allow_on[row] != 0;
  const uint32_t* A = on ? q.allow + (size_t)row * q.allow_stride : nullptr;
  const int lo = g * q.chunk, hi = lo + q.chunk < q.vocab ? lo + q.chunk : q.vocab;
  int tail = lo;                                  // first index the scalar loop handles
  if (q.vec && hi > lo) {
    const int nq = (hi - lo) >> 2;                // whole quads of the slice (lo and offset are multiples of 4)
    for (int j = t; j < nq; j += kLmThreads) {
      const int i = lo + 4 * j;
      u32x4 o = *reinterpret_cast<const u32x4*>(L + i);
      if (on) {
        const int64_t id = q.offset + i;
        const uint32_t b = A[id >> 5] >> (id & 31);     // the quad's four bits: id % 32 is a multiple of 4
        o.x = (b & 1u) ? o.x : kLmNegInf;
        o.y = (b & 2u) ? o.y : kLmNegInf;
        o.z = (b & 4u) ? o.z : kLmNegInf;
        o.w = (b & 8u) ? o.w : kLmNegInf;
      }
      *reinterpret_cast<u32x4*>(O + i) = o;
    }
    tail = lo + 4 * nq;
  }
  for (int i = tail + t; i < hi; i += kLmThreads) {
    uint32_t o = L[i];
    if (on) {
      const int64_t id = q.offset + i;
      if (!((A[id >> 5] >> (id & 31)) & 1u)) o = kLmNegInf;
    }
    O[i] = o;
  }
}

__global__ __launch_bounds__(kLmThreads) void lm_sparse_kernel(LmParams q) {
  const int row = blockIdx.x, t = threadIdx.x;
  float* O = q.out + (size_t)row * q.out_stride;
  if (q.bias_ids) {
    int n = q.bias_n[row];
    n = n < 0 ? 0 : (n > q.bias_stride ? (int)q.bias_stride : n);
    const int32_t* ids = q.bias_ids + (size_t)row * q.bias_stride;
    const float* val = q.bias_val + (size_t)row * q.bias_stride;
    for (int j = t; j < n; j += kLmThreads) {
      const int64_t i = (int64_t)ids[j] - q.offset;
      if (i >= 0 && i < q.vocab) O[i] = O[i] + val[j];
    }
  }
  __syncthreads();                                // an end id may carry a bias: the -inf is stored after the add
  if (q.end_ids && q.step[row] < q.min_tokens[row]) {
    int n = q.end_n[row];
    n = n < 0 ? 0 : (n > q.end_stride ? (int)q.end_stride : n);
    const int32_t* ids = q.end_ids + (size_t)row * q.end_stride;
    for (int j = t; j < n; j += kLmThreads) {
      const int64_t i = (int64_t)ids[j] - q.offset;
      if (i >= 0 && i < q.vocab) O[i] = -INFINITY;
    }
  }
}

}  // namespace chatts

using namespace chatts;

extern "C" int chatts_logit_masks_apply(const float* logits, int batch, int64_t logits_stride, int64_t vocab, int64_t vocab_offset,
                                        const ChattsLogitMaskArgs* a, const int32_t* step_dev, chatts_stream_t stream) {
  CHATTS_REQUIRE(logits && a && a->out, CHATTS_E_BADARG, "logit_masks: logits, args and args.out are required");
  CHATTS_REQUIRE(batch >= 1 && vocab > 0 && logits_stride >= vocab && a->out_stride >= vocab, CHATTS_E_BADARG,
                 "logit_masks: bad sizes batch=%d vocab=%lld strides %lld / %lld", batch, (long long)vocab, (long long)logits_stride,
                 (long long)a->out_stride);
  CHATTS_REQUIRE(vocab_offset >= 0 && vocab_offset + vocab <= 0x7fffffffLL, CHATTS_E_BADARG, "logit_masks: ids must fit int32");
  CHATTS_REQUIRE(a->out != logits, CHATTS_E_BADARG, "logit_masks: the raw logits are not written: args.out must be another buffer");
  const bool allow = a->allow_bits && a->allow_on;
  const bool bias = a->bias_ids && a->bias_val && a->bias_n;
  const bool ends = a->end_ids && a->end_n && a->min_tokens;
  if (const int rc = logit_mask_arrays_check(a, vocab, vocab_offset, step_dev, "logit_masks")) return rc;
  LmParams q;
  q.logits = logits; q.stride = logits_stride; q.vocab = (int)vocab; q.offset = vocab_offset;
  q.out = a->out; q.out_stride = a->out_stride;
  q.allow = allow ? a->allow_bits : nullptr; q.allow_stride = a->allow_stride; q.allow_on = a->allow_on;
  q.bias_ids = bias ? a->bias_ids : nullptr; q.bias_val = a->bias_val; q.bias_n = a->bias_n; q.bias_stride = a->bias_stride;
  q.end_ids = ends ? a->end_ids : nullptr; q.end_n = a->end_n; q.min_tokens = a->min_tokens; q.end_stride = a->end_stride;
  q.step = step_dev;
  const int64_t g = (vocab + 1023) / 1024;
  q.parts = g < kLmMaxParts ? (int)g : kLmMaxParts;
  q.chunk = (int)(((vocab + q.parts - 1) / q.parts + 3) & ~(int64_t)3);
  const auto rows16 = [batch](const void* p, int64_t stride) {
    return (reinterpret_cast<uintptr_t>(p) & 15) == 0 && (batch == 1 || stride % 4 == 0);
  };
  q.vec = rows16(logits, logits_stride) && rows16(a->out, a->out_stride) && vocab_offset % 4 == 0;
  hipStream_t s = as_stream(stream);
  hipLaunchKernelGGL(lm_apply_kernel, dim3(q.parts, batch), dim3(kLmThreads), 0, s, q);
  CHATTS_CHECK_LAUNCH("lm_apply");
  if (bias || ends) {
    hipLaunchKernelGGL(lm_sparse_kernel, dim3(batch), dim3(kLmThreads), 0, s, q);
    CHATTS_CHECK_LAUNCH("lm_sparse");
  }
  return CHATTS_OK;
}
