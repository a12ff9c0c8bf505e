// logprobs.hip - log-probabilities of the chosen tokens and the top-K alternatives, from the raw logits of the step that chose them.
// For every row: lse = m + log(sum_j exp(l_j - m)) over the full vocabulary slice, the chosen token's l_tok - lse and its 1-based
// rank in the order (logit descending, id ascending), and the K best (id, logprob) pairs in that order.  vLLM V1's default
// (raw_logprobs): before temperature / top-k / top-p.
//
// Two launches, the shape of the two-stage argmax (elementwise.hip):
//   logprobs_part_kernel   G = min(64, ceil(V / 256)) workgroups of 256 threads per row; workgroup g holds its slice of <= 4096
//                          logits in registers (16 per thread) and writes its max, sum exp(l - max), its count toward the chosen
//                          token's rank, and its K best candidates (each wave extracts its own sorted top-K by K wave-wide
//                          (value, id) reductions, wave 0 merges the four sorted lists).
//   logprobs_final_kernel  one wave per row: rescales and sums the G partials (float64, a fixed butterfly), merges the G sorted
//                          candidate lists by K head-of-list reductions, writes the [row, step - 1] cell.
// Every reduction has a fixed shape that depends on V only, so the same logits give the same bits in every run, graph replay and
// rank.  NaN logits are never selected or counted.
#include "common.h"

namespace chatts {

constexpr int kLpThreads = 256;
constexpr int kLpPer = 16;                              // logits per thread in a workgroup's slice
constexpr int kLpMaxParts = 64;
constexpr int kLpSlice = kLpThreads * kLpPer;           // 4096: V <= 64 * 4096
constexpr int kLpNone = 0x7fffffff;                     // id of the "no candidate" sentinel: orders after every real id

struct LpParams {
  const float* logits;
  int64_t stride;
  int vocab, parts, chunk, k;
  int64_t vocab_offset;
  const int64_t* token;
  const int32_t* step;
  int64_t out_stride;
  float* out_lp;
  int32_t* out_rank;
  int32_t* out_top_ids;
  float* out_top_lp;
  float* part_m;       // [batch, parts]
  float* part_s;
  int32_t* part_cnt;
  float* cand_v;       // [batch, parts, k]
  int32_t* cand_i;
};

// (v, i) before (bv, bi) in the order (value descending, id ascending)
__device__ __forceinline__ bool lp_before(float v, int i, float bv, int bi) { return v > bv || (v == bv && i < bi); }

__device__ __forceinline__ void lp_wave_best(float& v, int& i) {   // every lane ends with the wave's first pair
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(v, o, 64);
    const int oi = __shfl_xor(i, o, 64);
    if (lp_before(ov, oi, v, i)) { v = ov; i = oi; }
  }
}

__global__ __launch_bounds__(kLpThreads) void logprobs_part_kernel(LpParams p) {
  __shared__ float s_m[4], s_s[4];
  __shared__ int s_c[4];
  __shared__ float s_cv[4][CHATTS_LOGPROBS_MAX_K];
  __shared__ int s_ci[4][CHATTS_LOGPROBS_MAX_K];
  const int row = blockIdx.y, g = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const float* L = p.logits + (size_t)row * p.stride;
  const int lo = g * p.chunk, hi = lo + p.chunk < p.vocab ? lo + p.chunk : p.vocab;
  const int64_t tok64 = p.token[row] - p.vocab_offset;
  const int tok = tok64 >= 0 && tok64 < p.vocab ? (int)tok64 : -1;
  const float lt = tok >= 0 ? L[tok] : NAN;             // NaN: no token in this slice, nothing counts toward its rank

  float v[kLpPer];
  float m = -INFINITY;
  int cnt = 0;
#pragma unroll
  for (int r = 0; r < kLpPer; ++r) {
    const int i = lo + t + kLpThreads * r;
    v[r] = i < hi ? L[i] : NAN;
    m = fmaxf(m, v[r]);
    cnt += (v[r] > lt) || (v[r] == lt && i < tok);
  }
  m = wave_max(m);
  cnt = wave_sum_i(cnt);
  if (lane == 0) { s_m[wave] = m; s_c[wave] = cnt; }
  __syncthreads();
  m = fmaxf(fmaxf(s_m[0], s_m[1]), fmaxf(s_m[2], s_m[3]));
  float s = 0.f;
  if (m != -INFINITY) {                                  // (an all -inf slice has no mass; exp(-inf - -inf) would be NaN)
#pragma unroll
    for (int r = 0; r < kLpPer; ++r)
      if (v[r] == v[r]) s += expf(v[r] - m);
  }
  s = wave_sum(s);
  if (lane == 0) s_s[wave] = s;

  // this wave's K best, sorted: round j takes the first pair strictly after round j - 1's
  float pv = INFINITY;
  int pi = -1;
  for (int j = 0; j < p.k; ++j) {
    float bv = -INFINITY;
    int bi = kLpNone;
#pragma unroll
    for (int r = 0; r < kLpPer; ++r) {
      const int i = lo + t + kLpThreads * r;
      const bool after = v[r] < pv || (v[r] == pv && i > pi);
      if (after && lp_before(v[r], i, bv, bi)) { bv = v[r]; bi = i; }
    }
    lp_wave_best(bv, bi);
    if (lane == 0) { s_cv[wave][j] = bv; s_ci[wave][j] = bi; }
    pv = bv; pi = bi;
  }
  __syncthreads();
  if (wave != 0) return;

  const size_t part = (size_t)row * p.parts + g;
  if (lane == 0) {
    p.part_m[part] = m;
    p.part_s[part] = (s_s[0] + s_s[1]) + (s_s[2] + s_s[3]);
    p.part_cnt[part] = (s_c[0] + s_c[1]) + (s_c[2] + s_c[3]);
  }
  // merge the four sorted lists: lane w < 4 owns list w; the lane whose head won advances
  int ptr = 0;
  for (int j = 0; j < p.k; ++j) {
    float hv = -INFINITY;
    int hid = kLpNone;
    if (lane < 4 && ptr < p.k) { hv = s_cv[lane][ptr]; hid = s_ci[lane][ptr]; }
    float bv = hv;
    int bi = hid;
    lp_wave_best(bv, bi);
    if (lane < 4 && ptr < p.k && hid == bi) ++ptr;       // ids are unique, except the sentinel (then every list is spent)
    if (lane == 0) { p.cand_v[part * p.k + j] = bv; p.cand_i[part * p.k + j] = bi; }
  }
}

__global__ __launch_bounds__(64) void logprobs_final_kernel(LpParams p) {
  const int row = blockIdx.x, lane = threadIdx.x;
  const int32_t cell = p.step ? p.step[row] - 1 : 0;     // the selection has written out_tokens[row][cell] and bumped the counter
  if (cell < 0 || (p.out_stride > 0 && cell >= p.out_stride)) return;
  const size_t part0 = (size_t)row * p.parts;
  const bool mine = lane < p.parts;
  const float mg = mine ? p.part_m[part0 + lane] : -INFINITY;
  const float sg = mine ? p.part_s[part0 + lane] : 0.f;
  const int cg = mine ? p.part_cnt[part0 + lane] : 0;
  const float M = wave_max(mg);
  double S = sg > 0.f ? (double)sg * exp((double)mg - (double)M) : 0.0;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) S += __shfl_xor(S, o, 64);
  const int above = wave_sum_i(cg);
  const double logS = log(S);                           // lse = M + log(S); logprob(l) = (l - M) - log(S), rounded once to float32
  const size_t c = (size_t)row * p.out_stride + cell;
  if (lane == 0) {
    const int64_t tok64 = p.token[row] - p.vocab_offset;
    const bool have = tok64 >= 0 && tok64 < p.vocab;
    const float lt = have ? p.logits[(size_t)row * p.stride + tok64] : NAN;
    p.out_lp[c] = have ? (float)(((double)lt - (double)M) - logS) : NAN;
    p.out_rank[c] = have ? 1 + above : 0;
  }
  // merge the parts' sorted lists: lane g owns list g
  int ptr = 0;
  const float* cv = p.cand_v + (part0 + lane) * p.k;
  const int32_t* ci = p.cand_i + (part0 + lane) * p.k;
  for (int j = 0; j < p.k; ++j) {
    float hv = -INFINITY;
    int hid = kLpNone;
    if (mine && ptr < p.k) { hv = cv[ptr]; hid = ci[ptr]; }
    float bv = hv;
    int bi = hid;
    lp_wave_best(bv, bi);
    if (mine && ptr < p.k && hid == bi) ++ptr;
    if (lane == 0) {
      const bool real = bi != kLpNone;
      p.out_top_ids[c * p.k + j] = real ? (int32_t)(bi + p.vocab_offset) : -1;
      p.out_top_lp[c * p.k + j] = real ? (float)(((double)bv - (double)M) - logS) : -INFINITY;
    }
  }
}

inline int lp_parts(int64_t vocab) {
  const int64_t g = (vocab + kLpThreads - 1) / kLpThreads;
  return g < kLpMaxParts ? (int)g : kLpMaxParts;
}

}  // namespace chatts

using namespace chatts;

extern "C" size_t chatts_logprobs_workspace(int batch, int k) {
  if (batch < 1 || k < 0) return 0;
  const size_t kk = k > 0 ? (size_t)k : 1;
  return (size_t)batch * kLpMaxParts * (3 * sizeof(float) + kk * (sizeof(float) + sizeof(int32_t))) + 64;
}

extern "C" int chatts_logprobs_batched(const float* logits, int batch, int64_t logits_stride, int64_t vocab, int64_t vocab_offset,
                                       int k, const int64_t* token, const int32_t* step_dev, int64_t out_stride, float* out_lp,
                                       int32_t* out_rank, int32_t* out_top_ids, float* out_top_lp, void* workspace,
                                       size_t workspace_bytes, chatts_stream_t stream) {
  CHATTS_REQUIRE(logits && token && out_lp && out_rank, CHATTS_E_BADARG, "logprobs: logits, token, out_lp and out_rank are required");
  CHATTS_REQUIRE(batch >= 1 && vocab > 0 && logits_stride >= vocab, CHATTS_E_BADARG,
                 "logprobs: bad sizes batch=%d vocab=%lld stride=%lld", batch, (long long)vocab, (long long)logits_stride);
  CHATTS_REQUIRE(vocab <= (int64_t)kLpMaxParts * kLpSlice, CHATTS_E_SHAPE, "logprobs: vocab %lld exceeds %d", (long long)vocab,
                 kLpMaxParts * kLpSlice);
  CHATTS_REQUIRE(k >= 0 && k <= CHATTS_LOGPROBS_MAX_K, CHATTS_E_BADARG, "logprobs: k = %d outside 0..%d", k, CHATTS_LOGPROBS_MAX_K);
  CHATTS_REQUIRE(k == 0 || (out_top_ids && out_top_lp), CHATTS_E_BADARG, "logprobs: k = %d needs out_top_ids and out_top_lp", k);
  CHATTS_REQUIRE(out_stride >= 0 && (batch == 1 || out_stride > 0), CHATTS_E_BADARG, "logprobs: out_stride %lld (batch %d)",
                 (long long)out_stride, batch);
  CHATTS_REQUIRE(vocab_offset >= 0 && vocab_offset + vocab <= 0x7fffffffLL, CHATTS_E_BADARG, "logprobs: ids must fit int32");
  const size_t need = chatts_logprobs_workspace(batch, k);
  CHATTS_REQUIRE(workspace && workspace_bytes >= need, CHATTS_E_WORKSPACE, "logprobs: needs %zu workspace bytes, got %zu", need,
                 workspace_bytes);
  LpParams p;
  p.logits = logits; p.stride = logits_stride; p.vocab = (int)vocab; p.vocab_offset = vocab_offset; p.k = k;
  p.parts = lp_parts(vocab);
  p.chunk = (int)((vocab + p.parts - 1) / p.parts);
  p.token = token; p.step = step_dev; p.out_stride = out_stride;
  p.out_lp = out_lp; p.out_rank = out_rank; p.out_top_ids = out_top_ids; p.out_top_lp = out_top_lp;
  const size_t np = (size_t)batch * kLpMaxParts;
  char* ws = reinterpret_cast<char*>((reinterpret_cast<uintptr_t>(workspace) + 15) & ~(uintptr_t)15);
  p.part_m = reinterpret_cast<float*>(ws);
  p.part_s = p.part_m + np;
  p.part_cnt = reinterpret_cast<int32_t*>(p.part_s + np);
  p.cand_v = reinterpret_cast<float*>(p.part_cnt + np);
  p.cand_i = reinterpret_cast<int32_t*>(p.cand_v + np * (k > 0 ? k : 1));
  hipStream_t s = as_stream(stream);
  hipLaunchKernelGGL(logprobs_part_kernel, dim3(p.parts, batch), dim3(kLpThreads), 0, s, p);
  CHATTS_CHECK_LAUNCH("logprobs_part");
  hipLaunchKernelGGL(logprobs_final_kernel, dim3(batch), dim3(64), 0, s, p);
  CHATTS_CHECK_LAUNCH("logprobs_final");
  return CHATTS_OK;
}
