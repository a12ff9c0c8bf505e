// splitk_epilogue.h - the pieces the split-K epilogues share (gemm.hip, gemm_f16q.hip): the argument block, the slab prefetch and its in-order
// sum, the finishing arithmetic, the register-form row body and the host-side choice of its instantiation.  The RMSNorm arithmetic
// (sumsq4, rms_rstd, norm4) and the guarded load (load4_if) are common.h's and the bf16 plane writer (store_planes4) gemm_common.h's.  One definition each: the forms are
// bit-identical to one another because they call the same code, and tests/linear_ref.py holds each of them against float64 on its own.
#pragma once
#include <type_traits>

#include "gemm_common.h"

namespace chatts {

// what every row-wise / element-wise split-K epilogue is launched with (by value: 96 bytes of kernel arguments)
struct SplitkEpi {
  const float* ws;       // partials [sk][M][N]
  int sk, m, n;
  const float* bias;
  const float* resid;
  float* c;
  int ldc, epilogue;
  const float* scale;    // per-column scale of an 8-bit weight copy, or null
  const float* norm_w;   // the consumer's RMSNorm weight (post-norm forms)
  float eps;
  uint16_t* hi;          // bf16 planes [M, ldp]: the post-norm planes of the row-wise forms, the output planes of the element-wise pair
  uint16_t* lo;
  int ldp;
};

// S slabs of 4 columns requested at once; the clamp re-reads the last slab for s >= sk and slab_sum drops the value.  The lane's share of
// the address, `at`, is added last: the row-wise kernels pass ws + row * N and their column - a scalar base and a 32-bit offset per load.
template <int S>
__device__ __forceinline__ void slab_load(const float* ws, int sk, size_t plane, size_t at, f32x4 (&t)[S], bool live = true) {
#pragma unroll
  for (int s = 0; s < S; ++s) t[s] = load4_if(live, ws + (s < sk ? s : sk - 1) * plane + at);
}
template <int S>
__device__ __forceinline__ f32x4 slab_sum(const f32x4 (&t)[S], int sk) {      // in split order, from zero
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int s = 0; s < S; ++s)
    if (s < sk) { v.x += t[s].x; v.y += t[s].y; v.z += t[s].z; v.w += t[s].w; }
  return v;
}

// scale, bias, (GELU,) residual - in this order, the residual as r + v
template <bool GELU>
__device__ __forceinline__ f32x4 epi_finish4(f32x4 v, const f32x4 sc, const f32x4 b, const f32x4 r, bool has_scale, bool has_bias, int epilogue) {
  if (has_scale) { v.x *= sc.x; v.y *= sc.y; v.z *= sc.z; v.w *= sc.w; }
  if (has_bias) { v.x += b.x; v.y += b.y; v.z += b.z; v.w += b.w; }
  if (GELU && epilogue == CHATTS_EPI_GELU) { v.x = gelu_erf_f(v.x); v.y = gelu_erf_f(v.y); v.z = gelu_erf_f(v.z); v.w = gelu_erf_f(v.w); }
  if (epilogue == CHATTS_EPI_RESID) { v.x = r.x + v.x; v.y = r.y + v.y; v.z = r.z + v.z; v.w = r.w + v.w; }
  return v;
}

// One row of the register form (splitk_epilogue_norm_reg_kernel, splitk_epilogue_f16q_kernel): sk <= 4 slabs, rows of <= 1024 kIt columns.
// A thread requests all slabs, the residual, bias and norm weights of all its kIt column groups up front, keeps the row values in
// registers, and writes c and the planes from them: every memory round trip of a thread is taken ONCE.  Sums in split order per element,
// the row's sum of squares in column-group order per thread.  put(col, o, live) writes 4 normed values as planes.  F16Q, the f16q side:
// no scale operand; norm_w == null ends the row before the reduction (no planes); every lane calls put, `live` or not (f16q_put4).
template <int kIt, bool F16Q, typename Put>
__device__ __forceinline__ void splitk_epilogue_reg_row(const SplitkEpi& e, int row, float* red, Put put) {
  const size_t plane = (size_t)e.m * e.n;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  const bool has_scale = !F16Q && e.scale;
  f32x4 t[kIt][4], rs[kIt], gw[kIt], sc4[kIt], b4[kIt];
#pragma unroll
  for (int it = 0; it < kIt; ++it) {
    const int col = threadIdx.x * 4 + it * 1024;
    const bool live = col < e.n;
    slab_load<4>(e.ws + (size_t)row * e.n, e.sk, plane, col, t[it], live);
    rs[it] = load4_if(live && e.epilogue == CHATTS_EPI_RESID, e.resid + (size_t)row * e.ldc + col);
    gw[it] = load4_if(live && (!F16Q || e.norm_w), e.norm_w + col);
    sc4[it] = load4_if(live && has_scale, e.scale + col);
    b4[it] = load4_if(live && e.bias, e.bias + col);
  }
  f32x4 keep[kIt];
  float ss = 0.f;
#pragma unroll
  for (int it = 0; it < kIt; ++it) {
    const int col = threadIdx.x * 4 + it * 1024;
    f32x4 v = zero;
    if (col < e.n) {
      v = epi_finish4<false>(slab_sum<4>(t[it], e.sk), sc4[it], b4[it], rs[it], has_scale, e.bias, e.epilogue);
      *reinterpret_cast<f32x4*>(e.c + (size_t)row * e.ldc + col) = v;
      ss = sumsq4(ss, v);
    }
    keep[it] = v;
  }
  if (F16Q && !e.norm_w) return;
  const float rstd = rms_rstd(ss, red, e.n, e.eps);
#pragma unroll
  for (int it = 0; it < kIt; ++it) {
    const int col = threadIdx.x * 4 + it * 1024;
    if (!F16Q && col >= e.n) continue;
    float o[4];
    norm4(keep[it], gw[it], rstd, o);
    put(col, o, col < e.n);
  }
}

// host: the register form's instantiation for `its` column groups of 1024 - 1 .. 6 as they are, 7 and 8 take <8>
template <typename F>
static inline void splitk_epilogue_its(int its, F&& launch) {
  switch (its) {
    case 1: launch(std::integral_constant<int, 1>{}); break;
    case 2: launch(std::integral_constant<int, 2>{}); break;
    case 3: launch(std::integral_constant<int, 3>{}); break;
    case 4: launch(std::integral_constant<int, 4>{}); break;
    case 5: launch(std::integral_constant<int, 5>{}); break;
    case 6: launch(std::integral_constant<int, 6>{}); break;
    default: launch(std::integral_constant<int, 8>{}); break;
  }
}

}  // namespace chatts
