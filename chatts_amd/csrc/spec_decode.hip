// spec_decode.hip - speculative decoding by prompt lookup (vLLM speculative_config {"method": "ngram"}, HF prompt_lookup_num_tokens;
// NOT IN REFERENCE): the n-gram proposer, the multi-row verify attention and the accept / rollback kernel.  The step that strings
// them together is chatts_decoder_spec_step (decoder.hip).  Greedy, one sequence, tensor_parallel_size 1.
#include <limits.h>

#include "attn_decode.h"

namespace chatts {

constexpr int kSpecMaxRows = CHATTS_SPEC_MAX_ROWS;
constexpr int kSpecMaxNgram = CHATTS_SPEC_MAX_NGRAM;

// ---------------------------------------------------------------------------------------------------
// proposer: one workgroup.  Every thread scans candidate ends e = tid, tid + 256, ... < pos and keeps its best (match length, end);
// (longer match, then smaller end) is a total order, so the reduction shape does not matter: deterministic.
// ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool spec_better(const int m, const int e, const int bm, const int be) { return m > bm || (m == bm && e < be); }

__global__ __launch_bounds__(256) void spec_propose_kernel(const int32_t* __restrict__ pos_dev, const int32_t* __restrict__ hist,
                                                          const int max_ctx, const int k, const int nmin, const int nmax,
                                                          const int64_t vocab, int32_t* __restrict__ draft,
                                                          int64_t* __restrict__ spec_tokens) {
  __shared__ int sm[4], se[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int pos = *pos_dev;
  const bool live = pos >= 0 && pos < max_ctx;
  int tail[kSpecMaxNgram];
#pragma unroll
  for (int j = 0; j < kSpecMaxNgram; ++j) tail[j] = (live && j < nmax && pos - j >= 0) ? hist[pos - j] : INT_MIN;
  int bm = 0, be = INT_MAX;
  if (live) {
    for (int e = tid; e < pos; e += 256) {
      int m = 0;
#pragma unroll
      for (int j = 0; j < kSpecMaxNgram; ++j) {
        if (m == j && j < nmax && e - j >= 0 && hist[e - j] == tail[j]) m = j + 1;
      }
      if (m >= nmin && spec_better(m, e, bm, be)) { bm = m; be = e; }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int om = __shfl_xor(bm, o, 64), oe = __shfl_xor(be, o, 64);
    if (spec_better(om, oe, bm, be)) { bm = om; be = oe; }
  }
  if (lane == 0) { sm[wave] = bm; se[wave] = be; }
  __syncthreads();
#pragma unroll
  for (int w = 0; w < 4; ++w)
    if (spec_better(sm[w], se[w], bm, be)) { bm = sm[w]; be = se[w]; }
  if (tid < k) {
    int dft = -1;
    if (bm >= nmin && be < pos && be + 1 + tid <= pos) dft = hist[be + 1 + tid];
    draft[tid] = dft;
    spec_tokens[1 + tid] = (dft >= 0 && dft < vocab) ? dft : 0;
  }
  if (tid == 0) {
    const int last = live ? hist[pos] : 0;
    spec_tokens[0] = (last >= 0 && last < vocab) ? last : 0;
  }
}

// ---------------------------------------------------------------------------------------------------
// accept / rollback: one wave, the work is a serial walk over <= 8 drafts
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void spec_verify_kernel(const int64_t* __restrict__ argmax, const int32_t* __restrict__ draft, const int k,
                                                        const int64_t vocab, int32_t* __restrict__ pos_dev, int32_t* __restrict__ step_dev,
                                                        int64_t* __restrict__ token_dev, int64_t* __restrict__ out_tokens,
                                                        const int32_t* __restrict__ cap_dev, int32_t* __restrict__ hist, const int max_ctx,
                                                        int64_t* __restrict__ counters) {
  if (threadIdx.x != 0) return;
  const int pos = *pos_dev, step = *step_dev;
  if (pos < 0 || step < 0) return;
  int a = 0, valid = 0;
  bool run = true;
  for (int i = 0; i < k; ++i) {
    const int dft = draft[i];
    const bool ok = dft >= 0 && dft < vocab;
    valid += ok ? 1 : 0;
    run = run && ok && (int64_t)dft == argmax[i];
    a += run ? 1 : 0;
  }
  int e = a + 1;
  const int room_out = *cap_dev - step;               // cells left in out_tokens
  const int room_ctx = max_ctx - (k + 1) - pos;       // the next step writes K / V rows pos' .. pos' + k: keep them inside the cache
  if (e > room_out) e = room_out;
  if (e > room_ctx) e = room_ctx;
  if (e <= 0) return;
  for (int i = 0; i < e; ++i) {
    out_tokens[step + i] = argmax[i];
    hist[pos + 1 + i] = (int32_t)argmax[i];
  }
  *step_dev = step + e;
  *pos_dev = pos + e;
  *token_dev = argmax[e - 1];
  counters[0] += 1;
  counters[1] += valid;
  counters[2] += e - 1;
  counters[3] += e;
}

// ---------------------------------------------------------------------------------------------------
// verify attention: grid (n_kv, n_slots), one wave per row (rows x 64 threads).  Slot s walks the 16-key tiles s, s + n_slots, ...;
// wave r is query row r (position pos + r) with all heads of the kv head's group, on the register layout and the arithmetic of the
// decode kernel (attn_decode.h).  The workgroup first rotates its rows' q and K into LDS (and V beside them); the workgroup of slot 0
// also stores the K / V rows into the cache.  A key j >= pos is one of the rows in flight: its K / V come from LDS, the cache rows
// [pos, pos + rows) are never read in this launch.  All waves of the workgroup read the same cache tile, one after the other: it
// comes from HBM once and is served to the others by the CU's caches (plain loads, unlike the decode kernel's streaming ones).
// ---------------------------------------------------------------------------------------------------
template <typename KV>
__device__ __forceinline__ void verify_load_tile(const KvLayout& kvl, const KV* kcache, const KV* vcache, const int hk, const int tile,
                                                 const int pos, const int lane, f32x4 (&kw)[8], f32x4 (&vw)[8]) {
  const int j0 = tile * kDTile;
  const int kg = lane >> 3, c = lane & 7, h = lane >> 5, vc = lane & 31;
  if (j0 >= pos) {      // every key of the tile is in flight (or masked): nothing is read
#pragma unroll
    for (int i = 0; i < 8; ++i) { kw[i] = (f32x4){0.f, 0.f, 0.f, 0.f}; vw[i] = (f32x4){0.f, 0.f, 0.f, 0.f}; }
    return;
  }
  const int last = pos - 1;      // last cached row: lies in this tile or after it, so clamped addresses stay inside the tile
  const size_t toff = kv_tile_off(kvl, hk, j0);
  const int ja = j0 + kg <= last ? j0 + kg : last, jb = j0 + 8 + kg <= last ? j0 + 8 + kg : last;
  if constexpr (sizeof(KV) == 2) {
    const KV* ka = kcache + toff + (size_t)(ja - j0) * kHeadDim + c * 8;
    const KV* kb = kcache + toff + (size_t)(jb - j0) * kHeadDim + c * 8;
    const f16x8 a0 = *reinterpret_cast<const f16x8*>(ka), a1 = *reinterpret_cast<const f16x8*>(ka + 64);
    const f16x8 b0 = *reinterpret_cast<const f16x8*>(kb), b1 = *reinterpret_cast<const f16x8*>(kb + 64);
    // kw[i] / kw[4 + i]: dims attn_kdim<KV>(i, c) = (i >> 1) * 64 + c * 8 + (i & 1) * 4 of keys kg / 8 + kg
    kw[0] = kv_widen4(__builtin_shufflevector(a0, a0, 0, 1, 2, 3)); kw[1] = kv_widen4(__builtin_shufflevector(a0, a0, 4, 5, 6, 7));
    kw[2] = kv_widen4(__builtin_shufflevector(a1, a1, 0, 1, 2, 3)); kw[3] = kv_widen4(__builtin_shufflevector(a1, a1, 4, 5, 6, 7));
    kw[4] = kv_widen4(__builtin_shufflevector(b0, b0, 0, 1, 2, 3)); kw[5] = kv_widen4(__builtin_shufflevector(b0, b0, 4, 5, 6, 7));
    kw[6] = kv_widen4(__builtin_shufflevector(b1, b1, 0, 1, 2, 3)); kw[7] = kv_widen4(__builtin_shufflevector(b1, b1, 4, 5, 6, 7));
  } else {
    const KV* ka = kcache + toff + (size_t)(ja - j0) * kHeadDim + c * 4;
    const KV* kb = kcache + toff + (size_t)(jb - j0) * kHeadDim + c * 4;
#pragma unroll
    for (int i = 0; i < 4; ++i) { kw[i] = *reinterpret_cast<const f32x4*>(ka + i * 32); kw[4 + i] = *reinterpret_cast<const f32x4*>(kb + i * 32); }
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) {      // vw[i]: dims vc * 4 .. of key 2 i + h
    const int ju = j0 + 2 * i + h <= last ? j0 + 2 * i + h : last;
    vw[i] = kv_widen4(kv_load4<KV>(vcache + toff + (size_t)(ju - j0) * kHeadDim + vc * 4));
  }
}

template <int GMAX, typename KV>
__global__ __launch_bounds__(kSpecMaxRows * 64) void attn_verify_kernel(const AttnParams p) {
  __shared__ __attribute__((aligned(16))) float q_s[kSpecMaxRows * GMAX * kHeadDim];
  __shared__ __attribute__((aligned(16))) float knew_s[kSpecMaxRows * kHeadDim];
  __shared__ __attribute__((aligned(16))) float vnew_s[kSpecMaxRows * kHeadDim];
  const int hk = blockIdx.x, slot = blockIdx.y, lane = threadIdx.x & 63, r = threadIdx.x >> 6;
  const int R = p.t, NS = p.n_splits, G = p.n_q / p.n_kv;
  const int pos = *p.pos0_dev;
  if (pos < 0 || pos + R > p.max_ctx) return;      // (uniform over the launch: no cache write, the combine writes zeros)
  const int pr = pos + r;                          // this wave's position
  const int qkv_n = (p.n_q + 2 * p.n_kv) * kHeadDim;
  const float* qkv = p.qkv + (size_t)r * qkv_n;
  KV* kcache = kv_ptr<KV>(p.kc);
  KV* vcache = kv_ptr<KV>(p.vc);
  const KvLayout kvl{p.table, p.n_kv, p.max_ctx, p.log_block};
  float* q_r = q_s + (size_t)r * GMAX * kHeadDim;
  {
    const float c = p.cos_tab[(size_t)pr * 64 + lane], s = p.sin_tab[(size_t)pr * 64 + lane];
#pragma unroll
    for (int g = 0; g < GMAX; ++g) {
      if (g < G) {
        const int src = (hk * G + g) * kHeadDim;
        float a = qkv[src + lane], b = qkv[src + lane + 64];
        norm_rope(a, b, p.q_norm_w, p.eps, c, s, lane);
        q_r[g * kHeadDim + lane] = a;
        q_r[g * kHeadDim + lane + 64] = b;
      }
    }
    const int ks = (p.n_q + hk) * kHeadDim, vs = (p.n_q + p.n_kv + hk) * kHeadDim;
    float a = qkv[ks + lane], b = qkv[ks + lane + 64];
    norm_rope(a, b, p.k_norm_w, p.eps, c, s, lane);
    a = kv_cached_value<KV>(a, p.kv_round); b = kv_cached_value<KV>(b, p.kv_round);
    const float va = kv_cached_value<KV>(qkv[vs + lane], p.kv_round), vb = kv_cached_value<KV>(qkv[vs + lane + 64], p.kv_round);
    knew_s[r * kHeadDim + lane] = a; knew_s[r * kHeadDim + lane + 64] = b;
    vnew_s[r * kHeadDim + lane] = va; vnew_s[r * kHeadDim + lane + 64] = vb;
    if (slot == 0) {      // pr < max_ctx (checked above): the row exists in the cache
      const size_t noff = kv_tile_off(kvl, hk, pr);
      kcache[noff + lane] = (KV)a; kcache[noff + lane + 64] = (KV)b;
      vcache[noff + lane] = (KV)va; vcache[noff + lane + 64] = (KV)vb;
    }
  }
  __syncthreads();

  const float scale = 0.08838834764831845f * 1.4426950408889634f;    // 128^-1/2 * log2(e): the softmax runs on exp2
  const int kg = lane >> 3, kc = lane & 7, vh = lane >> 5, vc = lane & 31;
  float m_run[GMAX], l_run[GMAX];
  f32x4 acc[GMAX];
#pragma unroll
  for (int g = 0; g < GMAX; ++g) { m_run[g] = -INFINITY; l_run[g] = 0.f; acc[g] = (f32x4){0.f, 0.f, 0.f, 0.f}; }
  const int ntiles = pr / kDTile + 1;
  const int hi = pos + R;                          // keys [pos, hi) are in flight
  for (int tile = slot; tile < ntiles; tile += NS) {
    f32x4 kvb[8], vvb[8];
    verify_load_tile<KV>(kvl, kcache, vcache, hk, tile, pos, lane, kvb, vvb);
    const int j0 = tile * kDTile;
    const int ja = j0 + kg, jb = j0 + 8 + kg;
    if (j0 + kDTile > pos) {                        // the tile holds rows in flight: theirs come from LDS
      if (ja >= pos && ja < hi) {
#pragma unroll
        for (int i = 0; i < 4; ++i) kvb[i] = *reinterpret_cast<const f32x4*>(knew_s + (ja - pos) * kHeadDim + attn_kdim<KV>(i, kc));
      }
      if (jb >= pos && jb < hi) {
#pragma unroll
        for (int i = 0; i < 4; ++i) kvb[4 + i] = *reinterpret_cast<const f32x4*>(knew_s + (jb - pos) * kHeadDim + attn_kdim<KV>(i, kc));
      }
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int j = j0 + 2 * i + vh;
        if (j >= pos && j < hi) vvb[i] = *reinterpret_cast<const f32x4*>(vnew_s + (j - pos) * kHeadDim + vc * 4);
      }
    }
    float da[GMAX], db[GMAX];
#pragma unroll
    for (int g = 0; g < GMAX; ++g) { da[g] = 0.f; db[g] = 0.f; }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
      for (int g = 0; g < GMAX; ++g) {
        if (g < G) {
          const f32x4 qv = *reinterpret_cast<const f32x4*>(q_r + g * kHeadDim + attn_kdim<KV>(i, kc));
          da[g] = fmaf(kvb[i].x, qv.x, da[g]); da[g] = fmaf(kvb[i].y, qv.y, da[g]);
          da[g] = fmaf(kvb[i].z, qv.z, da[g]); da[g] = fmaf(kvb[i].w, qv.w, da[g]);
          db[g] = fmaf(kvb[4 + i].x, qv.x, db[g]); db[g] = fmaf(kvb[4 + i].y, qv.y, db[g]);
          db[g] = fmaf(kvb[4 + i].z, qv.z, db[g]); db[g] = fmaf(kvb[4 + i].w, qv.w, db[g]);
        }
      }
    }
    float pa[GMAX], pb[GMAX];
#pragma unroll
    for (int g = 0; g < GMAX; ++g) {
      pa[g] = 0.f; pb[g] = 0.f;
      if (g < G) {
        float sa = da[g], sb = db[g];
        sa += lane_xor1(sa); sb += lane_xor1(sb);
        sa += lane_xor2(sa); sb += lane_xor2(sb);
        sa += half_mirror(sa); sb += half_mirror(sb);
        sa = ja <= pr ? sa * scale : -INFINITY;      // causal: row r sees keys 0 .. pos + r
        sb = jb <= pr ? sb * scale : -INFINITY;
        const float m2 = fmaxf(sa, sb);
        const float mt = rows4_max(fmaxf(m2, row_ror8(m2)));
        const float m_new = fmaxf(m_run[g], mt);     // finite: key j0 <= pr is always valid
        const float ea = __builtin_amdgcn_exp2f(sa - m_new), eb = __builtin_amdgcn_exp2f(sb - m_new);
        const float e2 = ea + eb;
        const float es = rows4_sum(e2 + row_ror8(e2));
        const float alpha = __builtin_amdgcn_exp2f(m_run[g] - m_new);
        l_run[g] = l_run[g] * alpha + es;
        m_run[g] = m_new;
        acc[g].x *= alpha; acc[g].y *= alpha; acc[g].z *= alpha; acc[g].w *= alpha;
        pa[g] = ea; pb[g] = eb;
      }
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
#pragma unroll
      for (int g = 0; g < GMAX; ++g) {
        if (g < G) {
          const float pe = i < 4 ? readlane_f(pa[g], 16 * i) : readlane_f(pb[g], 16 * (i - 4));
          const float po = i < 4 ? readlane_f(pa[g], 16 * i + 8) : readlane_f(pb[g], 16 * (i - 4) + 8);
          const float pu = vh ? po : pe;
          acc[g].x = fmaf(pu, vvb[i].x, acc[g].x); acc[g].y = fmaf(pu, vvb[i].y, acc[g].y);
          acc[g].z = fmaf(pu, vvb[i].z, acc[g].z); acc[g].w = fmaf(pu, vvb[i].w, acc[g].w);
        }
      }
    }
  }
  if (slot >= ntiles) return;                      // this row has no keys in this slot (the combine reads slots < min(ntiles, NS))
#pragma unroll
  for (int g = 0; g < GMAX; ++g) {
    if (g < G) {
      f32x4 o = acc[g];
      o.x += __shfl_xor(o.x, 32, 64); o.y += __shfl_xor(o.y, 32, 64); o.z += __shfl_xor(o.z, 32, 64); o.w += __shfl_xor(o.w, 32, 64);
      const size_t pi = ((size_t)r * p.n_q + hk * G + g) * NS + slot;
      if (lane < 32) *reinterpret_cast<f32x4*>(p.part_o + pi * kHeadDim + vc * 4) = o;
      if (lane == 0) { p.part_ml[pi * 2] = m_run[g] * 0.6931471805599453f; p.part_ml[pi * 2 + 1] = l_run[g]; }
    }
  }
}

// grid (n_q, rows), 2 waves per head: the decode combine with the row's own position pos + row
__global__ __launch_bounds__(128) void attn_verify_combine_kernel(const AttnParams p) {
  const int row = blockIdx.y;
  const int pos = *p.pos0_dev;
  const int pr = (pos < 0 || pos + p.t > p.max_ctx) ? -1 : pos + row;
  attn_combine_wave_at(p, blockIdx.x, row, threadIdx.x, threadIdx.x & 63, p.part_o, p.part_ml,
                       ((size_t)row * p.n_q + blockIdx.x) * p.n_splits, pr);
}

template <typename KV>
static void launch_verify(const int group, const dim3 grid, const dim3 block, hipStream_t s, const AttnParams& p) {
  if (group <= 4) hipLaunchKernelGGL((attn_verify_kernel<4, KV>), grid, block, 0, s, p);
  else if (group == 5) hipLaunchKernelGGL((attn_verify_kernel<5, KV>), grid, block, 0, s, p);
  else if (group == 6) hipLaunchKernelGGL((attn_verify_kernel<6, KV>), grid, block, 0, s, p);
  else hipLaunchKernelGGL((attn_verify_kernel<kMaxGroup, KV>), grid, block, 0, s, p);
}

// chatts_attention_verify with an optional plane output (the decoder's step feeds o_proj's weight-streaming kernel from the combine)
int attention_verify_impl(const float* qkv_raw, int rows, int n_q, int n_kv, const float* q_norm_w, const float* k_norm_w, float norm_eps,
                          const float* cos_tab, const float* sin_tab, const int32_t* pos_dev, const ChattsKvCache* cache, float* out,
                          uint16_t* out_hi, uint16_t* out_lo, int n_splits, void* workspace, size_t workspace_bytes,
                          chatts_stream_t stream) {
  CHATTS_REQUIRE(rows >= 1 && rows <= kSpecMaxRows && n_q > 0 && n_kv > 0 && n_splits >= 1 && n_splits <= kMaxSlots, CHATTS_E_BADARG,
                 "attention_verify: bad sizes (1 <= rows <= %d, 1 <= n_splits <= %d)", kSpecMaxRows, kMaxSlots);
  CHATTS_REQUIRE(qkv_raw && (out || (out_hi && out_lo)) && cos_tab && sin_tab && pos_dev && cache && cache->k && cache->v, CHATTS_E_BADARG,
                 "attention_verify: null pointer");
  CHATTS_REQUIRE((q_norm_w == nullptr) == (k_norm_w == nullptr), CHATTS_E_BADARG,
                 "attention_verify: q_norm and k_norm must both be set or both be null");
  CHATTS_REQUIRE(n_q % n_kv == 0 && n_q / n_kv <= kMaxGroup, CHATTS_E_SHAPE, "attention_verify: GQA group %d/%d unsupported (max %d)", n_q,
                 n_kv, kMaxGroup);
  CHATTS_REQUIRE(kv_elem_bytes(cache->dtype) != 0, CHATTS_E_BADARG,
                 "attention_verify: unknown KV cache dtype %d (CHATTS_KV_F32 = 0, CHATTS_KV_F16 = 1)", cache->dtype);
  AttnParams p{};
  p.qkv = qkv_raw; p.out = out; p.out_hi = out_hi; p.out_lo = out_lo; p.pos0_dev = pos_dev;
  p.t = rows; p.n_q = n_q; p.n_kv = n_kv; p.n_splits = n_splits;
  p.kc = cache->k; p.vc = cache->v; p.max_ctx = cache->max_ctx; p.kv_f16 = cache->dtype == CHATTS_KV_F16;
  p.table = cache->block_table; p.table_stride = cache->table_stride;
  if (cache->block_table) {
    p.log_block = kv_log_block(cache->block_size);
    CHATTS_REQUIRE(p.log_block > 0 && cache->max_ctx % cache->block_size == 0, CHATTS_E_BADARG,
                   "attention_verify: paged cache needs a power-of-two block size in 64..32768 dividing max_ctx");
  }
  p.q_norm_w = q_norm_w; p.k_norm_w = k_norm_w; p.cos_tab = cos_tab; p.sin_tab = sin_tab; p.eps = norm_eps;
  p.kv_round = p.kv_f16 ? 0 : kv_round_mode();
  const size_t need = chatts_attn_workspace(rows, n_q, n_splits);
  CHATTS_REQUIRE(workspace && workspace_bytes >= need, CHATTS_E_WORKSPACE, "attention_verify: needs %zu workspace bytes, got %zu", need,
                 workspace_bytes);
  p.part_o = reinterpret_cast<float*>(workspace);
  p.part_ml = p.part_o + (size_t)rows * n_q * n_splits * kHeadDim;
  const dim3 grid(n_kv, n_splits), block(rows * 64);
  if (p.kv_f16) launch_verify<_Float16>(n_q / n_kv, grid, block, as_stream(stream), p);
  else launch_verify<float>(n_q / n_kv, grid, block, as_stream(stream), p);
  CHATTS_CHECK_LAUNCH("attn_verify");
  hipLaunchKernelGGL(attn_verify_combine_kernel, dim3(n_q, rows), dim3(128), 0, as_stream(stream), p);
  CHATTS_CHECK_LAUNCH("attn_verify_combine");
  return CHATTS_OK;
}

}  // namespace chatts

using namespace chatts;

extern "C" int chatts_attention_verify(const float* qkv_raw, int rows, int n_q, int n_kv, const float* q_norm_w, const float* k_norm_w,
                                       float norm_eps, const float* cos_tab, const float* sin_tab, const int32_t* pos_dev,
                                       const ChattsKvCache* cache, float* out, int n_splits, void* workspace, size_t workspace_bytes,
                                       chatts_stream_t stream) {
  return attention_verify_impl(qkv_raw, rows, n_q, n_kv, q_norm_w, k_norm_w, norm_eps, cos_tab, sin_tab, pos_dev, cache, out, nullptr,
                               nullptr, n_splits, workspace, workspace_bytes, stream);
}

extern "C" int chatts_spec_propose(const int32_t* pos_dev, const int32_t* hist, int max_ctx, int k, int ngram_min, int ngram_max,
                                   int64_t vocab, int32_t* draft, int64_t* spec_tokens, chatts_stream_t stream) {
  CHATTS_REQUIRE(pos_dev && hist && draft && spec_tokens, CHATTS_E_BADARG, "spec_propose: null pointer");
  CHATTS_REQUIRE(k >= 1 && k <= CHATTS_SPEC_MAX_DRAFT, CHATTS_E_BADARG, "spec_propose: k = %d must be in 1..%d", k, CHATTS_SPEC_MAX_DRAFT);
  CHATTS_REQUIRE(ngram_min >= 1 && ngram_max >= ngram_min && ngram_max <= kSpecMaxNgram, CHATTS_E_BADARG,
                 "spec_propose: n-gram sizes %d..%d must satisfy 1 <= min <= max <= %d", ngram_min, ngram_max, kSpecMaxNgram);
  CHATTS_REQUIRE(max_ctx >= 1 && vocab >= 1, CHATTS_E_BADARG, "spec_propose: max_ctx / vocab must be positive");
  hipLaunchKernelGGL(spec_propose_kernel, dim3(1), dim3(256), 0, as_stream(stream), pos_dev, hist, max_ctx, k, ngram_min, ngram_max, vocab,
                     draft, spec_tokens);
  CHATTS_CHECK_LAUNCH("spec_propose");
  return CHATTS_OK;
}

extern "C" int chatts_spec_verify(const int64_t* argmax, const int32_t* draft, int k, int64_t vocab, int32_t* pos_dev, int32_t* step_dev,
                                  int64_t* token_dev, int64_t* out_tokens, const int32_t* out_capacity_dev, int32_t* hist, int max_ctx,
                                  int64_t* counters, chatts_stream_t stream) {
  CHATTS_REQUIRE(argmax && draft && pos_dev && step_dev && token_dev && out_tokens && out_capacity_dev && hist && counters, CHATTS_E_BADARG,
                 "spec_verify: null pointer");
  CHATTS_REQUIRE(k >= 1 && k <= CHATTS_SPEC_MAX_DRAFT && max_ctx >= 1 && vocab >= 1, CHATTS_E_BADARG,
                 "spec_verify: k = %d must be in 1..%d, max_ctx / vocab positive", k, CHATTS_SPEC_MAX_DRAFT);
  hipLaunchKernelGGL(spec_verify_kernel, dim3(1), dim3(64), 0, as_stream(stream), argmax, draft, k, vocab, pos_dev, step_dev, token_dev,
                     out_tokens, out_capacity_dev, hist, max_ctx, counters);
  CHATTS_CHECK_LAUNCH("spec_verify");
  return CHATTS_OK;
}
