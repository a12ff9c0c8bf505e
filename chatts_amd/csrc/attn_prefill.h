// attn_prefill.h - what the prefill attention kernels of attention.hip share: the (query tile, query head) coordinates of a flash
// workgroup, the bf16 hi / lo value split, the three-pass bf16 product, the online softmax of the C layout and the output / partial
// stores.  Everything is __forceinline__: each kernel's instruction stream is what it was with the pieces written out in place
// (profiles/attention_unify_isa.txt).
#pragma once
#include "attn_decode.h"

namespace chatts {

typedef __bf16 abf16x8_t __attribute__((ext_vector_type(8)));
typedef __bf16 abf16x4_t __attribute__((ext_vector_type(4)));
typedef __bf16 abf16x2_t __attribute__((ext_vector_type(2)));
template <int N> struct Bf16Vec;
template <> struct Bf16Vec<2> { typedef abf16x2_t T; };
template <> struct Bf16Vec<4> { typedef abf16x4_t T; };
template <> struct Bf16Vec<8> { typedef abf16x8_t T; };

constexpr float kScale2 = 0.08838834764831845f * 1.4426950408889634f;   // d^-1/2 * log2(e): the flash softmax runs on exp2
constexpr float kLn2 = 0.6931471805599453f;

__device__ __forceinline__ int attn_pos0(const AttnParams& p) { return p.pos0_dev ? *p.pos0_dev : p.pos0; }

// ---------------------------------------------------------------------------------------------------
// x = hi + lo in bf16: hi = rne(x), lo = rne(x - hi).  The VALUE split ((__bf16) conversions), not common.h's integer
// split_bf16x2; where x is a product the caller computes it under `fp contract(off)` so that lo is the split of the ROUNDED value.
// HI / LO: any two things indexable to a __bf16 lvalue (a bf16 vector, an array).
// ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ void split_hi_lo(const float x, __bf16& hi, __bf16& lo) {
#pragma clang fp contract(off)
  hi = (__bf16)x;
  lo = (__bf16)(x - (float)hi);
}
template <int N, typename V>
__device__ __forceinline__ void split_hi_lo(const float (&x)[N], V& hi, V& lo) {
#pragma unroll
  for (int j = 0; j < N; ++j) {
#pragma clang fp contract(off)
    const __bf16 h = (__bf16)x[j];
    hi[j] = h;
    lo[j] = (__bf16)(x[j] - (float)h);
  }
}
__device__ __forceinline__ void split_hi_lo(const f32x4 v, abf16x4_t& hi, abf16x4_t& lo) {
  const float x[4] = {v.x, v.y, v.z, v.w};
  split_hi_lo(x, hi, lo);
}
__device__ __forceinline__ void split_hi_lo(const f32x4 a, const f32x4 b, abf16x8_t& hi, abf16x8_t& lo) {
  const float x[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
  split_hi_lo(x, hi, lo);
}

// acc += x.y on the bf16 matrix pipe with both operands split: x_lo.y_hi, x_hi.y_lo, x_hi.y_hi in that order (the dropped lo.lo
// term is 2^-16 of the product).  x is q or P, y is K or V; x sits in the A slot, or in the B slot when TRANSPOSED.
template <bool TRANSPOSED>
__device__ __forceinline__ void mfma3(const abf16x8_t x_hi, const abf16x8_t x_lo, const abf16x8_t y_hi, const abf16x8_t y_lo, f32x4& acc) {
  if constexpr (TRANSPOSED) {
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(y_hi, x_lo, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(y_lo, x_hi, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(y_hi, x_hi, acc, 0, 0, 0);
  } else {
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(x_lo, y_hi, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(x_hi, y_lo, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(x_hi, y_hi, acc, 0, 0, 0);
  }
}

// row `key` of the tile that starts at key k0, clamped to the last valid key: a finite row to load, masked by its key index later
__device__ __forceinline__ int tile_row(const int k0, const int key, const int last) { return k0 + key <= last ? key : last - k0; }

// ---------------------------------------------------------------------------------------------------
// What a flash workgroup (256 threads, 64 query rows of ONE query head, wave w rows q0 + 16 w .. + 15, KT-key tiles) knows.
// ---------------------------------------------------------------------------------------------------
template <int KT>
struct FlashTile {
  int tid, lane, wave;
  int fi, fg;              // lane & 15: the lane's row of an A / B fragment and its column of the C layout; lane >> 4: its group of
                           // K values in a fragment, 4 fg .. 4 fg + 3 its C rows
  int hq, hk, heads;
  int T, pos0, q0, wrow0;  // wrow0: first query row of this wave
  int kmax, nkt;           // last key any row of this workgroup may see; tiles up to it

  __device__ __forceinline__ FlashTile(const AttnParams& p, const int qt, const int hq_, const int pos0_) {
    tid = threadIdx.x; lane = tid & 63; wave = tid >> 6;
    fi = lane & 15; fg = lane >> 4;
    hq = hq_; hk = hq / (p.n_q / p.n_kv); heads = p.n_q + 2 * p.n_kv;
    T = p.t; pos0 = pos0_; q0 = qt * 64; wrow0 = q0 + wave * 16;
    const int last_q = q0 + 63 < T - 1 ? q0 + 63 : T - 1;
    kmax = pos0 + last_q;
    nkt = kmax / KT + 1;
  }
  // row i of this wave, clamped: padded rows compute garbage that is never stored
  __device__ __forceinline__ int qrow(const int i) const { const int r = wrow0 + i; return r > T - 1 ? T - 1 : r; }
  __device__ __forceinline__ int qpos(const int i) const { return pos0 + q0 + wave * 16 + i; }
  // wave-uniform: only such a tile holds keys some row of this wave cannot see (without it no key exceeds any qpos)
  __device__ __forceinline__ bool diag(const int k0) const { return k0 + KT - 1 > pos0 + q0 + wave * 16; }
  // wave-uniform: the workgroup walks the keys its LAST row sees; a wave whose 16 rows all lie before the tile has nothing to add
  __device__ __forceinline__ bool wave_sees(const int k0) const { return !(k0 > pos0 + q0 + wave * 16 + 15); }
  __device__ __forceinline__ int tile_row(const int kt, const int key) const { return chatts::tile_row(kt * KT, key, kmax); }
};

// Q rows as split bf16 fragments: row qrow of head hq, dims ks*32 + g*8 .. +7 for the four K-steps ks
__device__ __forceinline__ void load_q_split(const AttnParams& p, const int qrow, const int heads, const int hq, const int g,
                                             abf16x8_t (&q_hi)[4], abf16x8_t (&q_lo)[4]) {
  const float* qp = p.qkv + ((size_t)qrow * heads + hq) * kHeadDim + g * 8;
#pragma unroll
  for (int ks = 0; ks < 4; ++ks)
    split_hi_lo(*reinterpret_cast<const f32x4*>(qp + ks * 32), *reinterpret_cast<const f32x4*>(qp + ks * 32 + 4), q_hi[ks], q_lo[ks]);
}

// One step of the online softmax in the log2 domain, for one row: the new running maximum, alpha = 2^(m_old - m_ref) for what was
// accumulated so far; returns m_ref, the exponent reference of this tile's scores.  A key split other than 0 may start on a tile the
// row cannot see at all: m stays -inf, m_ref = 0 and every 2^(-inf - 0) contributes nothing.
__device__ __forceinline__ float softmax_shift(float& m_run, const float mx, float& alpha) {
  const float m_new = fmaxf(m_run, mx);
  const float m_ref = m_new == -INFINITY ? 0.f : m_new;
  alpha = __builtin_amdgcn_exp2f(m_run - m_ref);
  m_run = m_new;
  return m_ref;
}

// Online softmax of S in the C layout (column ccol = key k0 + nb*16 + ccol, 4 rows per lane): s_acc becomes P, m_run is updated,
// alpha (for the caller's rescale of O) and the row sums ps of P (for its l = l * alpha + ps) come back.  Scores are pre-scaled by
// d^-1/2 * log2 e, so every exponential is one v_exp_f32.  Written stage by stage over the four rows a lane holds: the DPP
// reductions are dependent chains with wait states, and four independent chains in flight are what hides them (measured with
// s_memtime: this block was 3.5k cycles per tile as a per-row loop with expf, against 2k cycles for the 64 MFMAs of Q.K^T).
// DIAG = false: the causal mask is applied to every tile.  DIAG = true: only when the caller's wave-uniform `diag` says the tile can
// hold a key some row cannot see - a short-circuit that changes no bit (the float32 kernel has it; in the bf16x3 kernel a run-time
// flag, even a constant one, cost the tile loop hazard nops, and l updated in here cost it two VGPRs:
// profiles/attention_unify_isa.txt).
template <int NB, bool DIAG>
__device__ __forceinline__ void flash_softmax_rows(f32x4 (&s_acc)[NB], const int k0, const int ccol, const int (&qpos)[4],
                                                   float (&m_run)[4], float (&ps)[4], float (&alpha)[4], const bool diag = false) {
  float mx[4], m_ref[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    mx[r] = -INFINITY;
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
      float sc = s_acc[nb][r] * kScale2;
      if ((!DIAG || diag) && k0 + nb * 16 + ccol > qpos[r]) sc = -INFINITY;  // causal mask
      s_acc[nb][r] = sc;
      mx[r] = fmaxf(mx[r], sc);
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) mx[r] = fmaxf(mx[r], lane_xor1(mx[r]));
#pragma unroll
  for (int r = 0; r < 4; ++r) mx[r] = fmaxf(mx[r], lane_xor2(mx[r]));
#pragma unroll
  for (int r = 0; r < 4; ++r) mx[r] = fmaxf(mx[r], row_ror4(mx[r]));
#pragma unroll
  for (int r = 0; r < 4; ++r) mx[r] = fmaxf(mx[r], row_ror8(mx[r]));
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    m_ref[r] = softmax_shift(m_run[r], mx[r], alpha[r]);
    ps[r] = 0.f;
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
      const float e = __builtin_amdgcn_exp2f(s_acc[nb][r] - m_ref[r]);
      s_acc[nb][r] = e;
      ps[r] += e;
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) ps[r] += lane_xor1(ps[r]);
#pragma unroll
  for (int r = 0; r < 4; ++r) ps[r] += lane_xor2(ps[r]);
#pragma unroll
  for (int r = 0; r < 4; ++r) ps[r] += row_ror4(ps[r]);
#pragma unroll
  for (int r = 0; r < 4; ++r) ps[r] += row_ror8(ps[r]);
}

// ---------------------------------------------------------------------------------------------------
// Results.  attn_store: N consecutive dims of the final output at element oi, as float32 `out` or - the o_proj operand format,
// written where the value is made - as the out_hi / out_lo planes, split from the ROUNDED value: the caller computes v (o * 1/l, or
// num / den) under `fp contract(off)`, as chatts_split_bf16x2 of the float32 output would see it.
// ---------------------------------------------------------------------------------------------------
template <int N>
__device__ __forceinline__ void attn_store(const AttnParams& p, const size_t oi, const float (&v)[N]) {
  if (p.out_hi) {
    if constexpr (N == 1) {
      __bf16 h, l;
      split_hi_lo(v[0], h, l);
      p.out_hi[oi] = __builtin_bit_cast(uint16_t, h);
      p.out_lo[oi] = __builtin_bit_cast(uint16_t, l);
    } else {
      typename Bf16Vec<N>::T h, l;
      split_hi_lo(v, h, l);
      *reinterpret_cast<typename Bf16Vec<N>::T*>(p.out_hi + oi) = h;
      *reinterpret_cast<typename Bf16Vec<N>::T*>(p.out_lo + oi) = l;
    }
  } else if constexpr (N == 1) {
    p.out[oi] = v[0];
  } else {
#pragma unroll
    for (int j = 0; j < N; j += 4) *reinterpret_cast<f32x4*>(p.out + oi + j) = (f32x4){v[j], v[j + 1], v[j + 2], v[j + 3]};
  }
}

// The unnormalised partial of one key split, slot pi = (row * n_q + head) * n_splits + split: o[j] is head dim d0 + j * STRIDE
// (STRIDE 1: two 16-byte stores); the lane with `lead` adds (m, l) with m, kept in the log2 domain by the flash kernels, back in nats.
template <int STRIDE>
__device__ __forceinline__ void attn_store_partial(const AttnParams& p, const size_t pi, const int d0, const float (&o)[8], const bool lead,
                                                   const float m_log2, const float l) {
  float* dst = p.part_o + pi * kHeadDim + d0;
  if constexpr (STRIDE == 1) {
    *reinterpret_cast<f32x4*>(dst) = (f32x4){o[0], o[1], o[2], o[3]};
    *reinterpret_cast<f32x4*>(dst + 4) = (f32x4){o[4], o[5], o[6], o[7]};
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) dst[j * STRIDE] = o[j];
  }
  if (lead) { p.part_ml[pi * 2] = m_log2 * kLn2; p.part_ml[pi * 2 + 1] = l; }
}

// One query row of a C-layout flash kernel, 8 accumulators per lane for head dims d0 + j * STRIDE: the partial of key split `split`
// when the keys are split, else the normalised output.
template <int STRIDE>
__device__ __forceinline__ void flash_store_row(const AttnParams& p, const int qrow, const int hq, const int split, const int d0,
                                                const float (&acc)[8], const bool lead, const float m_log2, const float l) {
#pragma clang fp contract(off)   // lo = split of the ROUNDED product, as chatts_split_bf16x2 of the float32 output would give
  const size_t row = (size_t)qrow * p.n_q + hq;
  if (p.n_splits > 1) {
    attn_store_partial<STRIDE>(p, row * p.n_splits + split, d0, acc, lead, m_log2, l);
    return;
  }
  const float inv = 1.0f / l;
  if constexpr (STRIDE == 1) {
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = acc[j] * inv;
    attn_store<8>(p, row * kHeadDim + d0, v);
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float v[1] = {acc[j] * inv};
      attn_store<1>(p, row * kHeadDim + d0 + j * STRIDE, v);
    }
  }
}

}  // namespace chatts
