// gemv_common.h - the arithmetic of the batch-1 weight-streaming GEMV (gemv.hip) that fixes the bits of a result: the FMA order of a
// bf16 load, SiLU, and the row map of a task (the RMSNorm sum of squares, sumsq4, is common.h's: every kernel shares it).
#pragma once
#include "common.h"

namespace chatts {

__device__ __forceinline__ float dot8(const u32x4 wv, const f32x4 xa, const f32x4 xb, float acc) {
  acc = fmaf(bf16_lo(wv.x), xa.x, acc);
  acc = fmaf(bf16_hi(wv.x), xa.y, acc);
  acc = fmaf(bf16_lo(wv.y), xa.z, acc);
  acc = fmaf(bf16_hi(wv.y), xa.w, acc);
  acc = fmaf(bf16_lo(wv.z), xb.x, acc);
  acc = fmaf(bf16_hi(wv.z), xb.y, acc);
  acc = fmaf(bf16_lo(wv.w), xb.z, acc);
  acc = fmaf(bf16_hi(wv.w), xb.w, acc);
  return acc;
}

__device__ __forceinline__ float silu_f(float x) { return x / (1.0f + expf(-x)); }

template <int ROWS, int EPI>
__device__ __forceinline__ int task_row(int task, int r) {
  if (EPI == CHATTS_EPI_SWIGLU) {   // gate/up interleaved in blocks of 16 rows: unit u -> rows g(u), g(u)+16
    const int unit = task * (ROWS / 2) + (r >> 1);
    return (unit >> 4) * 32 + (unit & 15) + (r & 1) * 16;
  }
  return task * ROWS + r;
}

}  // namespace chatts
