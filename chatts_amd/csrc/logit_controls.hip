// logit_controls.hip - repetition / frequency / presence penalties and the min_p cut, applied to the logits of a step before the
// selection sees them (vLLM V1's sampler order: raw logits -> repetition -> frequency and presence -> [greedy rows: argmax] ->
// temperature -> min_p -> top-k -> top-p -> draw).
//
// State: one int32 per (sequence, vocabulary id): bit 30 = "the id occurs in the prompt", bits 0..29 = how often the id has been
// generated so far (saturating).  A cell of 0 means the id is neither in the prompt nor in the history: its logit is copied bit for bit.
//   lc_zero_kernel / lc_mark_kernel   admission: clear the sequence's row, then mark the prompt ids (integer atomic OR: the result does
//                                     not depend on the order)
//   lc_update_kernel                  after a selection: the chosen token's count += 1 (one thread per row)
//   lc_apply_kernel                   G = min(64, ceil(V / 1024)) workgroups of 256 threads per row: out = penalised logits of the
//                                     workgroup's slice (16-byte accesses when rows are 16-byte aligned), and the slice's maximum
//   lc_minp_kernel                    same grid: merges the row's G maxima (a fixed wave butterfly), cut = m + T * log(min_p), and stores
//                                     -inf over every out[i] < cut.  Rows with min_p == 0 or T == 0 (greedy) leave at once.
// The raw logits are only read.  Per-row parameters come from device arrays at run time, so one captured decode step serves requests
// with different settings.  No float atomics: same logits and state give the same bits in every run, graph replay and cache slot.
#include "common.h"

namespace chatts {

constexpr int kLcThreads = 256;
constexpr int kLcMaxParts = 64;
constexpr int kLcPromptBit = 1 << 30;
constexpr int kLcCountMask = kLcPromptBit - 1;

struct LcParams {
  const float* logits;
  int64_t stride;
  int vocab, parts, chunk;          // chunk is a multiple of 4
  const int32_t* state;
  int64_t state_stride;
  float* out;
  int64_t out_stride;
  const float* rep;
  const float* freq;
  const float* pres;
  const float* minp;
  const float* temp;
  float* part_m;                    // [batch, kLcMaxParts]
  int vec;                          // every row of logits / state / out starts 16-byte aligned
};

// l / r or l * r for an id of the prompt or the history, then - f * c - p for an id generated c > 0 times
__device__ __forceinline__ float lc_penalise(float l, int cell, float r, float f, float p) {
  if (cell == 0) return l;
  l = l > 0.f ? l / r : l * r;
  const int c = cell & kLcCountMask;
  if (c > 0) l = l - f * (float)c - p;
  return l;
}

__global__ __launch_bounds__(kLcThreads) void lc_apply_kernel(LcParams q) {
  __shared__ float s_m[kLcThreads / 64];
  const int row = blockIdx.y, g = blockIdx.x, t = threadIdx.x;
  const float* L = q.logits + (size_t)row * q.stride;
  const int32_t* S = q.state + (size_t)row * q.state_stride;
  float* O = q.out + (size_t)row * q.out_stride;
  const int lo = g * q.chunk, hi = lo + q.chunk < q.vocab ? lo + q.chunk : q.vocab;
  const float r = q.rep ? q.rep[row] : 1.f, f = q.freq ? q.freq[row] : 0.f, p = q.pres ? q.pres[row] : 0.f;
  float m = -INFINITY;
  int tail = lo;                                  // first index the scalar loop handles
  if (q.vec && hi > lo) {
    const int nq = (hi - lo) >> 2;                // whole quads of the slice (lo is a multiple of 4)
    for (int j = t; j < nq; j += kLcThreads) {
      const int i = lo + 4 * j;
      const f32x4 l = *reinterpret_cast<const f32x4*>(L + i);
      const int4 c = *reinterpret_cast<const int4*>(S + i);
      f32x4 o;
      o.x = lc_penalise(l.x, c.x, r, f, p);
      o.y = lc_penalise(l.y, c.y, r, f, p);
      o.z = lc_penalise(l.z, c.z, r, f, p);
      o.w = lc_penalise(l.w, c.w, r, f, p);
      *reinterpret_cast<f32x4*>(O + i) = o;
      m = fmaxf(fmaxf(m, o.x), fmaxf(fmaxf(o.y, o.z), o.w));
    }
    tail = lo + 4 * nq;
  }
  for (int i = tail + t; i < hi; i += kLcThreads) {
    const float o = lc_penalise(L[i], S[i], r, f, p);
    O[i] = o;
    m = fmaxf(m, o);
  }
  m = wave_max(m);
  if ((t & 63) == 0) s_m[t >> 6] = m;
  __syncthreads();
  if (t == 0) q.part_m[(size_t)row * kLcMaxParts + g] = fmaxf(fmaxf(s_m[0], s_m[1]), fmaxf(s_m[2], s_m[3]));
}

__global__ __launch_bounds__(kLcThreads) void lc_minp_kernel(LcParams q) {
  const int row = blockIdx.y, g = blockIdx.x, t = threadIdx.x, lane = t & 63;
  const float mp = q.minp[row], T = q.temp[row];
  if (!(mp > 0.f) || !(T > 0.f)) return;          // off, or a greedy row: inert
  const float m = wave_max(lane < q.parts ? q.part_m[(size_t)row * kLcMaxParts + lane] : -INFINITY);
  const float cut = m + T * logf(mp);             // p_i >= min_p * p_max  <=>  l_i >= m + T * log(min_p); ties at the cut are kept
  float* O = q.out + (size_t)row * q.out_stride;
  const int lo = g * q.chunk, hi = lo + q.chunk < q.vocab ? lo + q.chunk : q.vocab;
  int tail = lo;
  if (q.vec && hi > lo) {
    const int nq = (hi - lo) >> 2;
    for (int j = t; j < nq; j += kLcThreads) {
      const int i = lo + 4 * j;
      f32x4 o = *reinterpret_cast<const f32x4*>(O + i);
      const bool any = o.x < cut || o.y < cut || o.z < cut || o.w < cut;
      if (o.x < cut) o.x = -INFINITY;
      if (o.y < cut) o.y = -INFINITY;
      if (o.z < cut) o.z = -INFINITY;
      if (o.w < cut) o.w = -INFINITY;
      if (any) *reinterpret_cast<f32x4*>(O + i) = o;
    }
    tail = lo + 4 * nq;
  }
  for (int i = tail + t; i < hi; i += kLcThreads)
    if (O[i] < cut) O[i] = -INFINITY;
}

__global__ __launch_bounds__(kLcThreads) void lc_zero_kernel(int32_t* row, int64_t n) {
  const int64_t i0 = (int64_t)blockIdx.x * kLcThreads + threadIdx.x, step = (int64_t)gridDim.x * kLcThreads;
  if ((reinterpret_cast<uintptr_t>(row) & 15) == 0) {
    const int64_t nq = n >> 2;
    for (int64_t j = i0; j < nq; j += step) reinterpret_cast<int4*>(row)[j] = make_int4(0, 0, 0, 0);
    for (int64_t i = 4 * nq + i0; i < n; i += step) row[i] = 0;
  } else {
    for (int64_t i = i0; i < n; i += step) row[i] = 0;
  }
}

__global__ __launch_bounds__(kLcThreads) void lc_mark_kernel(int32_t* row, int64_t vocab, int64_t vocab_offset, const int64_t* ids,
                                                             int64_t n) {
  const int64_t j = (int64_t)blockIdx.x * kLcThreads + threadIdx.x;
  if (j >= n) return;
  const int64_t i = ids[j] - vocab_offset;
  if (i >= 0 && i < vocab) atomicOr(row + i, kLcPromptBit);
}

__global__ __launch_bounds__(64) void lc_update_kernel(int32_t* state, int64_t state_stride, int batch, int64_t vocab,
                                                       int64_t vocab_offset, const int64_t* token) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= batch) return;
  const int64_t i = token[b] - vocab_offset;
  if (i < 0 || i >= vocab) return;
  int32_t* cell = state + (size_t)b * state_stride + i;
  const int32_t v = *cell;
  if ((v & kLcCountMask) != kLcCountMask) *cell = v + 1;
}

}  // namespace chatts

using namespace chatts;

extern "C" size_t chatts_logit_controls_workspace(int batch) {
  return batch < 1 ? 0 : (size_t)batch * kLcMaxParts * sizeof(float) + 16;
}

extern "C" int chatts_logit_controls_apply(const float* logits, int batch, int64_t logits_stride, int64_t vocab, int64_t vocab_offset,
                                           const ChattsLogitControlArgs* a, void* workspace, size_t workspace_bytes,
                                           chatts_stream_t stream) {
  CHATTS_REQUIRE(logits && a && a->state && a->out, CHATTS_E_BADARG, "logit_controls: logits, args, args.state and args.out are required");
  CHATTS_REQUIRE(batch >= 1 && vocab > 0 && logits_stride >= vocab && a->state_stride >= vocab && a->out_stride >= vocab, CHATTS_E_BADARG,
                 "logit_controls: bad sizes batch=%d vocab=%lld strides %lld / %lld / %lld", batch, (long long)vocab,
                 (long long)logits_stride, (long long)a->state_stride, (long long)a->out_stride);
  CHATTS_REQUIRE(vocab_offset >= 0 && vocab_offset + vocab <= 0x7fffffffLL, CHATTS_E_BADARG, "logit_controls: ids must fit int32");
  CHATTS_REQUIRE(a->out != logits, CHATTS_E_BADARG, "logit_controls: the raw logits are not written: args.out must be another buffer");
  const size_t need = chatts_logit_controls_workspace(batch);
  CHATTS_REQUIRE(workspace && workspace_bytes >= need, CHATTS_E_WORKSPACE, "logit_controls: needs %zu workspace bytes, got %zu", need,
                 workspace_bytes);
  LcParams q;
  q.logits = logits; q.stride = logits_stride; q.vocab = (int)vocab;
  q.state = a->state; q.state_stride = a->state_stride; q.out = a->out; q.out_stride = a->out_stride;
  q.rep = a->repetition_rows; q.freq = a->frequency_rows; q.pres = a->presence_rows; q.minp = a->min_p_rows; q.temp = a->temperature_rows;
  const int64_t g = (vocab + 1023) / 1024;
  q.parts = g < kLcMaxParts ? (int)g : kLcMaxParts;
  q.chunk = (int)(((vocab + q.parts - 1) / q.parts + 3) & ~(int64_t)3);
  const auto rows16 = [batch](const void* p, int64_t stride) {
    return (reinterpret_cast<uintptr_t>(p) & 15) == 0 && (batch == 1 || stride % 4 == 0);
  };
  q.vec = rows16(logits, logits_stride) && rows16(a->state, a->state_stride) && rows16(a->out, a->out_stride);
  q.part_m = reinterpret_cast<float*>((reinterpret_cast<uintptr_t>(workspace) + 15) & ~(uintptr_t)15);
  hipStream_t s = as_stream(stream);
  hipLaunchKernelGGL(lc_apply_kernel, dim3(q.parts, batch), dim3(kLcThreads), 0, s, q);
  CHATTS_CHECK_LAUNCH("lc_apply");
  if (q.minp && q.temp) {
    hipLaunchKernelGGL(lc_minp_kernel, dim3(q.parts, batch), dim3(kLcThreads), 0, s, q);
    CHATTS_CHECK_LAUNCH("lc_minp");
  }
  return CHATTS_OK;
}

extern "C" int chatts_logit_state_reset(int32_t* state_row, int64_t vocab, int64_t vocab_offset, const int64_t* prompt_ids,
                                        int64_t n_prompt, chatts_stream_t stream) {
  CHATTS_REQUIRE(state_row && vocab > 0 && vocab_offset >= 0 && n_prompt >= 0 && (prompt_ids || n_prompt == 0), CHATTS_E_BADARG,
                 "logit_state_reset: bad arguments");
  hipStream_t s = as_stream(stream);
  const int64_t blocks = (vocab / 4 + kLcThreads - 1) / kLcThreads + 1;
  hipLaunchKernelGGL(lc_zero_kernel, dim3((unsigned)(blocks < 256 ? blocks : 256)), dim3(kLcThreads), 0, s, state_row, vocab);
  CHATTS_CHECK_LAUNCH("lc_zero");
  if (n_prompt > 0) {
    hipLaunchKernelGGL(lc_mark_kernel, dim3((unsigned)((n_prompt + kLcThreads - 1) / kLcThreads)), dim3(kLcThreads), 0, s, state_row, vocab,
                       vocab_offset, prompt_ids, n_prompt);
    CHATTS_CHECK_LAUNCH("lc_mark");
  }
  return CHATTS_OK;
}

extern "C" int chatts_logit_state_update(int32_t* state, int64_t state_stride, int batch, int64_t vocab, int64_t vocab_offset,
                                         const int64_t* token, chatts_stream_t stream) {
  CHATTS_REQUIRE(state && token && batch >= 1 && vocab > 0 && state_stride >= vocab && vocab_offset >= 0, CHATTS_E_BADARG,
                 "logit_state_update: bad arguments");
  hipLaunchKernelGGL(lc_update_kernel, dim3((batch + 63) / 64), dim3(64), 0, as_stream(stream), state, state_stride, batch, vocab,
                     vocab_offset, token);
  CHATTS_CHECK_LAUNCH("lc_update");
  return CHATTS_OK;
}
