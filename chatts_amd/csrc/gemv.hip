// gemv.hip - batch-1 decode projections: y[N] = epilogue(W[N,K] . x[K]),  W streamed from HBM as bf16, 8-bit (fp8 / int8) or 4-bit codes.
//
// This file sets generated tokens/s: every decode step streams all decoder weights once (27.98 GB for ChatTS-14B in bf16), so it is
// HBM-bound by construction.  It follows the guide's "GEMV / M<=16 decode weights" rule: weights go straight to VGPRs as non-temporal
// loads, many loads in flight per lane, no LDS round trip for the streamed operand.
//
// One prologue (gemv_stage_x), one stream loop (gemv_stream) and one task loop (gemv_whole_k) serve three weight formats (FmtBf16,
// FmtW8, FmtInt4: what differs between them is written down once, in those structs); the __global__ kernels are entry points that name
// a format.  Geometry: one wave per group of ROWS rows over the whole K; the small, re-used operand x (20-55 KB f32) is staged once per
// workgroup in LDS (4-16 waves share it), permuted so that each lane's 16-byte reads of a chunk are lane-linear (conflict-free
// ds_read_b128); ROWS x UNR independent weight loads in flight per lane, 16-32 waves per CU.  A row is summed by ONE wave in a fixed
// lane and chunk order whatever the geometry, with or without the exchange of tp_reduce.  gemv_ksplit_kernel (bf16, shard-sized
// projections) shares a row between several waves and is the one exception.  A variant that kept x in registers and issued 12-14
// loads per lane was measured and lost on every shape (tools/gemv_sweep.py).
// Arithmetic: every weight widens exactly to f32 and x is f32, so every product is exact in the f32 FMA; only the summation order
// differs from the CPU oracle (parity budget: 1e-3 relative on logits).  (The 4-bit form meets x as a bf16 hi + lo pair: FmtInt4.)
// Fusions: RMSNorm of x in the prologue (Qwen2RMSNorm.forward), bias, residual add, SwiGLU.
#include "common.h"
#include "gemv_common.h"
#include "tp_common.h"

namespace chatts {

// EPI_RESID of a row-parallel projection under tensor parallelism (ChattsLinearArgs.tp_reduce): the sum over the ranks is formed
// inside the launch.  Internal template value, not part of the C-ABI's epilogue enum.
constexpr int kEpiResidTp = 4;

struct GemvParams {
  const uint16_t* w;
  const float* x;
  const float* bias;
  const float* resid;
  float* out;
  const float* norm_w;
  float eps;
  int n;       // weight rows
  int k;
  int ldw;
  int tasks;   // number of row-group tasks
  const uint8_t* w8;      // fp8 (OCP e4m3fn) weights [N, ldw8] or NULL
  const float* w8_scale;  // per-row power-of-two scale: w = scale[row] * float(w8)
  int ldw8;
  int w8_format;          // CHATTS_W8_FP8 / CHATTS_W8_INT8
  // optional 4-bit copy of W (GPTQ codes, row-major: byte j of a row = codes 2j | 2j+1 << 4) with one (scale, scale * zero) pair
  // per `w4_group` weights of a row: w = bf16_rne(q * scale - scale_zero) - exactly the bf16 matrix the other kernels stream
  const uint8_t* w4;
  const float* w4_sz;     // [N, K / w4_group, 2]
  int ldw4, w4_group;
  TpParams tp;            // kEpiResidTp only
  int ks;                 // gemv_ksplit_kernel: waves per row group
};

// ---- the exchange inside the launch (kEpiResidTp) ---------------------------------------------------------------------------
// A wave that has finished the ROWS rows of a task PUSHES them at once - lane l holds (row l % ROWS, destination l / ROWS): ROWS x W
// independent 8-byte granule stores, one per xGMI link and row - and goes on streaming its next task.  After its last task it
// POLLS the rows of each of its tasks from the local exchange buffer - lane l = (row l % ROWS, source rank l / ROWS), all W x ROWS
// polls of a task in flight at once - adds them in RANK ORDER (v_readlane: every rank forms the same sum, bit for bit, so the
// replicated residual stream cannot diverge) and writes out = resid + sum: the arithmetic of tp_allreduce_kernel.  Between a
// wave's push and its poll lie the peers' pushes of the same rows, i.e. one link latency when the ranks run in step; the other waves
// of the CU keep the weight stream going meanwhile.  Every rank launches the same geometry, so the workgroup that waits for a row
// and the peer workgroup that produces it have the same index: no circular wait even if a grid were not fully resident.
template <int ROWS>
__device__ __forceinline__ void tp_push_task(const GemvParams& p, uint32_t epoch, int task, int lane, const float (&acc)[ROWS]) {
  static_assert(ROWS * kMaxWorld <= 64, "one lane per (row, rank)");
  const int r = lane % ROWS, k = lane / ROWS;
  const int row = task * ROWS + r;
  float v = acc[0];
#pragma unroll
  for (int i = 1; i < ROWS; ++i)
    if (r == i) v = acc[i];
  if (k < p.tp.world && row < p.n) {
    const int q = (p.tp.rank + k) % p.tp.world;           // start with myself, then ring order: spreads the links
    put(push_ptr(p.tp, q, epoch) + row, epoch, push_bits(p.tp, q, __float_as_uint(v)));
  }
}
template <int ROWS>
__device__ __forceinline__ void tp_take_task(const GemvParams& p, uint32_t epoch, int task, int lane) {
  const int r = lane % ROWS, src = lane / ROWS;
  const int row = task * ROWS + r;
  uint32_t bits = 0;
  if (src < p.tp.world && row < p.n) (void)take(slot_ptr(p.tp, p.tp.rank, epoch, src) + row, epoch, bits, &p.tp.ctr[2]);
  float sum[ROWS];
#pragma unroll
  for (int i = 0; i < ROWS; ++i) sum[i] = 0.f;
#pragma unroll
  for (int s = 0; s < kMaxWorld; ++s) {
    if (s < p.tp.world) {                                  // (wave-uniform)
#pragma unroll
      for (int i = 0; i < ROWS; ++i) {
        const float v = __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)bits, s * ROWS + i));
        sum[i] = s == 0 ? v : sum[i] + v;
      }
    }
  }
#pragma unroll
  for (int i = 0; i < ROWS; ++i) {
    const int rw = task * ROWS + i;
    if (lane == i && rw < p.n) p.out[rw] = p.resid[rw] + sum[i];
  }
}

// lane r (< ROWS, or < ROWS/2 for SwiGLU) of the finishing wave writes row r
template <int ROWS, int EPI>
__device__ __forceinline__ void gemv_epilogue(const GemvParams& p, int task, int lane, const float (&acc)[ROWS], uint32_t epoch = 0) {
  if (EPI == kEpiResidTp) {
    tp_push_task<ROWS>(p, epoch, task, lane, acc);
  } else if (EPI == CHATTS_EPI_SWIGLU) {
#pragma unroll
    for (int u = 0; u < ROWS / 2; ++u) {
      const int rg = task_row<ROWS, EPI>(task, 2 * u);
      if (lane == u && rg + 16 < p.n) {
        float g = acc[2 * u], v = acc[2 * u + 1];
        if (p.bias) { g += p.bias[rg]; v += p.bias[rg + 16]; }
        p.out[task * (ROWS / 2) + u] = silu_f(g) * v;
      }
    }
  } else {
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
      const int row = task * ROWS + r;
      if (lane == r && row < p.n) {
        float v = acc[r];
        if (p.bias) v += p.bias[row];
        if (EPI == CHATTS_EPI_RESID) v = p.resid[row] + v;
        p.out[row] = v;
      }
    }
  }
}

// ---- the three weight formats ----------------------------------------------------------------------------------------------------
// A format supplies what differs between the kernels: the chunk (1 << kShift elements of K: what 64 lanes cover with one load each),
// the LDS store of one staged float4 of x, a row's state, the zero-filled load, a lane's x fragment of a chunk, the dot of one load, the
// scalar handed to wave_sum and what is applied to the sum.  The FMA order inside each dot function is part of the result's bits.

// bf16: 16-byte loads of 8 weights, 512-element chunks, x staged as [chunk][half][lane] float4.
struct FmtBf16 {
  static constexpr int kShift = 9;
  struct Row { const uint16_t* w; };
  typedef u32x4 Load;
  struct X { f32x4 a, b; };
  typedef float Acc;
  __device__ __forceinline__ explicit FmtBf16(const GemvParams&) {}
  static __device__ __forceinline__ void stage(char* smem, int k4, const f32x4 v) {
    const int chunk = k4 >> 9, within = k4 & 511;
    reinterpret_cast<f32x4*>(smem)[chunk * 128 + ((within >> 2) & 1) * 64 + (within >> 3)] = v;
  }
  __device__ __forceinline__ Row row(const GemvParams& p, int row, int lane) const { return {p.w + (size_t)row * p.ldw + lane * 8}; }
  __device__ __forceinline__ Load load(const Row& r, int c, int, bool ok) const {
    Load wv = {0u, 0u, 0u, 0u};
    if (ok) wv = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(r.w + (c << 9)));
    return wv;
  }
  static __device__ __forceinline__ X x(const char* smem, int c, int lane) {
    const f32x4* xs4 = reinterpret_cast<const f32x4*>(smem);
    return {xs4[c * 128 + lane], xs4[c * 128 + 64 + lane]};
  }
  static __device__ __forceinline__ void dot(const Load wv, const X& x, Acc& acc) { acc = dot8(wv, x.a, x.b, acc); }
  static __device__ __forceinline__ float sum(const Acc& acc) { return acc; }
  static __device__ __forceinline__ float post(float s, const Row&) { return s; }
};

// 8-bit weights, fp8 (OCP e4m3fn, CDNA4 v_cvt_pk_f32_fp8) or int8: 16 weights per 16-byte load, so a chunk is 1024 elements and x is
// staged as [chunk][quarter][lane] float4.  Each row carries a power-of-two scale, w = scale[row] * float(q): the dequantised weight is
// exactly representable in bf16, i.e. the 8-bit copy is a lossless encoding of the bf16 matrix the prefill GEMM streams.  Halves the
// decode weight traffic.
typedef float f32x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ float dot16_fp8(const u32x4 wv, const f32x4 x0, const f32x4 x1, const f32x4 x2, const f32x4 x3,
                                            float acc) {
  f32x2 a;
  a = __builtin_amdgcn_cvt_pk_f32_fp8(wv.x, false); acc = fmaf(a.x, x0.x, acc); acc = fmaf(a.y, x0.y, acc);
  a = __builtin_amdgcn_cvt_pk_f32_fp8(wv.x, true);  acc = fmaf(a.x, x0.z, acc); acc = fmaf(a.y, x0.w, acc);
  a = __builtin_amdgcn_cvt_pk_f32_fp8(wv.y, false); acc = fmaf(a.x, x1.x, acc); acc = fmaf(a.y, x1.y, acc);
  a = __builtin_amdgcn_cvt_pk_f32_fp8(wv.y, true);  acc = fmaf(a.x, x1.z, acc); acc = fmaf(a.y, x1.w, acc);
  a = __builtin_amdgcn_cvt_pk_f32_fp8(wv.z, false); acc = fmaf(a.x, x2.x, acc); acc = fmaf(a.y, x2.y, acc);
  a = __builtin_amdgcn_cvt_pk_f32_fp8(wv.z, true);  acc = fmaf(a.x, x2.z, acc); acc = fmaf(a.y, x2.w, acc);
  a = __builtin_amdgcn_cvt_pk_f32_fp8(wv.w, false); acc = fmaf(a.x, x3.x, acc); acc = fmaf(a.y, x3.y, acc);
  a = __builtin_amdgcn_cvt_pk_f32_fp8(wv.w, true);  acc = fmaf(a.x, x3.z, acc); acc = fmaf(a.y, x3.w, acc);
  return acc;
}

// int8 form of the same 16 weights: four sign-extended bytes per dword (v_cvt_f32_i32 with an SDWA byte select, or a bit-field extract
// before it - the compiler's choice), the same float32 FMAs.  |q| <= 127: the products are exact as in the fp8 form.
__device__ __forceinline__ float dot16_i8(const u32x4 wv, const f32x4 x0, const f32x4 x1, const f32x4 x2, const f32x4 x3, float acc) {
  auto four = [&](uint32_t d, const f32x4 x) {
    acc = fmaf((float)(int)(int8_t)(d & 0xffu), x.x, acc);
    acc = fmaf((float)(int)(int8_t)((d >> 8) & 0xffu), x.y, acc);
    acc = fmaf((float)(int)(int8_t)((d >> 16) & 0xffu), x.z, acc);
    acc = fmaf((float)((int)d >> 24), x.w, acc);
  };
  four(wv.x, x0); four(wv.y, x1); four(wv.z, x2); four(wv.w, x3);
  return acc;
}

template <bool I8>
struct FmtW8 {
  static constexpr int kShift = 10;
  struct Row { const uint8_t* w; float scale; };
  typedef u32x4 Load;
  struct X { f32x4 x0, x1, x2, x3; };
  typedef float Acc;
  __device__ __forceinline__ explicit FmtW8(const GemvParams&) {}
  static __device__ __forceinline__ void stage(char* smem, int k4, const f32x4 v) {
    const int chunk = k4 >> 10, within = k4 & 1023;
    reinterpret_cast<f32x4*>(smem)[chunk * 256 + ((within >> 2) & 3) * 64 + (within >> 4)] = v;
  }
  // (the scale is loaded here, before the stream loop: its latency hides under the weight loads)
  __device__ __forceinline__ Row row(const GemvParams& p, int row, int lane) const {
    return {p.w8 + (size_t)row * p.ldw8 + lane * 16, p.w8_scale[row]};
  }
  __device__ __forceinline__ Load load(const Row& r, int c, int, bool ok) const {
    Load wv = {0u, 0u, 0u, 0u};
    if (ok) wv = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(r.w + (c << 10)));
    return wv;
  }
  static __device__ __forceinline__ X x(const char* smem, int c, int lane) {
    const f32x4* xb = reinterpret_cast<const f32x4*>(smem) + c * 256 + lane;
    return {xb[0], xb[64], xb[128], xb[192]};
  }
  static __device__ __forceinline__ void dot(const Load wv, const X& x, Acc& acc) {
    acc = I8 ? dot16_i8(wv, x.x0, x.x1, x.x2, x.x3, acc) : dot16_fp8(wv, x.x0, x.x1, x.x2, x.x3, acc);
  }
  static __device__ __forceinline__ float sum(const Acc& acc) { return acc; }
  static __device__ __forceinline__ float post(float s, const Row& r) { return s * r.scale; }      // power-of-two scale: exact
};

// 4-bit weights (GPTQ-Int4 checkpoints: ChatTS-14B-GPTQ-Int4, NetManAIOps/ChatTS README.md:52,262-263).  A lane's load is 8 bytes = 16
// codes, a chunk is 1024 elements, with a (scale, scale * zero) pair per group of `w4_group` (a multiple of 16) weights.  The engine's
// weights are DEFINED as bf16_rne(scale * (q - zero)) (chatts_amd/gptq.py: the prefill GEMM streams that bf16 matrix), so the kernel
// rebuilds exactly that value: q * scale - scale * zero is exact in float32 (fp16 scale x 5-bit integer), one v_cvt_pk_bf16_f32 per
// pair rounds it, and the widened result meets x in an exact-product float32 accumulate.  ~5 VALU ops per weight at 0.5 B per weight:
// the VALU and HBM are about equally loaded.
typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));

// 16 codes (two dwords) of one row against 16 x values held as packed bf16 pairs (hi and lo planes of the float32 x):
//   per byte b of a dword: codes 2b (low nibble) and 2b+1 (high nibble) -> v_cvt_f32_ubyte{b} of the masked dwords (no shifts),
//   one packed FMA builds both float32 weights, one v_cvt_pk_bf16_f32 rounds them to THE bf16 weights as a pair, and two
//   v_dot2c_f32_bf16 multiply the pair with x_hi and x_lo (exact products, float32 accumulate: the bf16x2 scheme of the
//   MFMA GEMMs).  ~3.4 VALU instructions per weight (the first version, unpacking to float32 FMAs, needed 7.7 and ran at
//   the speed of the bf16 kernel - profiles/r2_pmc_gemv4.txt).
#define CHATTS_CVT_UBYTE(dst, src, n) asm("v_cvt_f32_ubyte" #n " %0, %1" : "=v"(dst) : "v"(src))
__device__ __forceinline__ void dot16_int4(const u32x2 wv, const float sc, const float nsz, const u32x4 xh0, const u32x4 xh1,
                                           const u32x4 xl0, const u32x4 xl1, float& acc_h, float& acc_l) {
  auto eight = [&](uint32_t d, const u32x4 xh, const u32x4 xl) {
    const uint32_t lo = d & 0x0f0f0f0fu, hi = (d >> 4) & 0x0f0f0f0fu;      // bytes = codes of the even / odd elements
    float qe[4], qo[4];
    CHATTS_CVT_UBYTE(qe[0], lo, 0); CHATTS_CVT_UBYTE(qo[0], hi, 0);
    CHATTS_CVT_UBYTE(qe[1], lo, 1); CHATTS_CVT_UBYTE(qo[1], hi, 1);
    CHATTS_CVT_UBYTE(qe[2], lo, 2); CHATTS_CVT_UBYTE(qo[2], hi, 2);
    CHATTS_CVT_UBYTE(qe[3], lo, 3); CHATTS_CVT_UBYTE(qo[3], hi, 3);
    const uint32_t xhs[4] = {xh.x, xh.y, xh.z, xh.w}, xls[4] = {xl.x, xl.y, xl.z, xl.w};
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      f32x2 v = {fmaf(qe[b], sc, nsz), fmaf(qo[b], sc, nsz)};               // exact: fp16 scale x 5-bit integer
      const bf16x2_t w = __builtin_convertvector(v, bf16x2_t);             // round to nearest even: the bf16 weights (k, k+1)
      acc_h = __builtin_amdgcn_fdot2_f32_bf16(w, __builtin_bit_cast(bf16x2_t, xhs[b]), acc_h, false);
      acc_l = __builtin_amdgcn_fdot2_f32_bf16(w, __builtin_bit_cast(bf16x2_t, xls[b]), acc_l, false);
    }
  };
  eight(wv.x, xh0, xl0);
  eight(wv.y, xh1, xl1);
}

struct FmtInt4 {
  static constexpr int kShift = 10;
  struct Row { const uint8_t* w; const float2* sz; };
  struct Load { u32x2 w; float2 sz; };
  struct X { u32x4 h0, h1, l0, l1; };
  struct Acc { float h, l; };
  int ngroups, gshift;                                     // group sizes are powers of two (checked by the launcher)
  __device__ __forceinline__ explicit FmtInt4(const GemvParams& p) : ngroups(p.k / p.w4_group), gshift(31 - __builtin_clz(p.w4_group)) {}
  // x as packed bf16 pairs: [chunk][part][lane] 16-byte entries; part 0 / 1 = hi pairs 0-3 / 4-7 of the lane's 16 elements,
  // part 2 / 3 = the lo pairs (x = hi + lo to 2^-17: the bf16x2 split)
  static __device__ __forceinline__ void stage(char* smem, int k4, const f32x4 v) {
    uint32_t* xs1 = reinterpret_cast<uint32_t*>(smem);
    uint16_t h[4], l[4];
    split_bf16x2(v.x, h[0], l[0]); split_bf16x2(v.y, h[1], l[1]); split_bf16x2(v.z, h[2], l[2]); split_bf16x2(v.w, h[3], l[3]);
    const int chunk = k4 >> 10, within = k4 & 1023, ln = within >> 4, pair = (within & 15) >> 1;      // pair in {0, 2, 4, 6}
    const int base = ((chunk * 4 + (pair >> 2)) * 64 + ln) * 4 + (pair & 3);                            // dword index of the hi pair
    xs1[base] = (uint32_t)h[0] | ((uint32_t)h[1] << 16);
    xs1[base + 1] = (uint32_t)h[2] | ((uint32_t)h[3] << 16);
    xs1[base + 2 * 64 * 4] = (uint32_t)l[0] | ((uint32_t)l[1] << 16);
    xs1[base + 2 * 64 * 4 + 1] = (uint32_t)l[2] | ((uint32_t)l[3] << 16);
  }
  __device__ __forceinline__ Row row(const GemvParams& p, int row, int lane) const {
    return {p.w4 + (size_t)row * p.ldw4 + lane * 8, reinterpret_cast<const float2*>(p.w4_sz) + (size_t)row * ngroups};
  }
  __device__ __forceinline__ Load load(const Row& r, int c, int k0, bool ok) const {
    Load wv = {(u32x2){0u, 0u}, make_float2(0.f, 0.f)};
    if (ok) {
      wv.w = __builtin_nontemporal_load(reinterpret_cast<const u32x2*>(r.w + (c << 9)));
      wv.sz = r.sz[k0 >> gshift];
    }
    return wv;
  }
  static __device__ __forceinline__ X x(const char* smem, int c, int lane) {
    const u32x4* xb = reinterpret_cast<const u32x4*>(smem) + c * 256 + lane;
    return {xb[0], xb[64], xb[128], xb[192]};
  }
  static __device__ __forceinline__ void dot(const Load& wv, const X& x, Acc& acc) {
    dot16_int4(wv.w, wv.sz.x, -wv.sz.y, x.h0, x.h1, x.l0, x.l1, acc.h, acc.l);
  }
  static __device__ __forceinline__ float sum(const Acc& acc) { return acc.h + acc.l; }
  static __device__ __forceinline__ float post(float s, const Row&) { return s; }
};

// ---- the prologue: rstd of the fused RMSNorm and x, zero-padded to whole chunks, into LDS ------------------------------------------------
// -> red (behind the staged x: nw floats; the K-split kernel keeps its partial sums at red + 16).  The order of the sum of squares -
// per thread at stride blockDim.x * 4, wave_sum, the waves in wave order - is part of the result's bits: rstd depends on the wave count.
template <class F, bool NORM>
__device__ __forceinline__ float* gemv_stage_x(const GemvParams& p, char* smem, int nchunks, int tid, int nthreads) {
  float* red = reinterpret_cast<float*>(smem) + ((size_t)nchunks << F::kShift);
  const int lane = tid & 63, wave = tid >> 6, nw = nthreads >> 6;
  const int K = p.k;
  float rstd = 1.f;
  if (NORM) {
    float ss = 0.f;
    for (int k4 = tid * 4; k4 < K; k4 += nthreads * 4) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(p.x + k4);
      ss = sumsq4(ss, v);
    }
    ss = wave_sum(ss);
    if (lane == 0) red[wave] = ss;
    __syncthreads();
    float t = 0.f;
    for (int i = 0; i < nw; ++i) t += red[i];
    rstd = rsqrtf(t / (float)K + p.eps);
  }
  for (int k4 = tid * 4; k4 < (nchunks << F::kShift); k4 += nthreads * 4) {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (k4 < K) {
      v = *reinterpret_cast<const f32x4*>(p.x + k4);
      if (NORM) {
        const f32x4 g = *reinterpret_cast<const f32x4*>(p.norm_w + k4);
        v.x = g.x * (v.x * rstd); v.y = g.y * (v.y * rstd); v.z = g.z * (v.z * rstd); v.w = g.w * (v.w * rstd);
      }
    }
    F::stage(smem, k4, v);
  }
  __syncthreads();
  return red;
}

// ---- the stream loop: the ROWS rows of a task against the chunks c0, c0 + cstep, ... (UNR of them per step) -> per-row wave sums ------------
// ROWS x UNR loads are issued before the first of them is used.  Out-of-range loads leave zero registers, out-of-range rows read row 0
// (their sums are never stored); a row's chunks are added in ascending order whatever ROWS and UNR are.
template <class F, int ROWS, int UNR, int EPI>
__device__ __forceinline__ void gemv_stream(const F& f, const GemvParams& p, const char* smem, int task, int lane, int nchunks, int c0,
                                            int cstep, float (&acc)[ROWS]) {
  const int K = p.k;
  typename F::Row rw[ROWS];
#pragma unroll
  for (int r = 0; r < ROWS; ++r) {
    int row = task_row<ROWS, EPI>(task, r);
    if (row >= p.n) row = 0;
    rw[r] = f.row(p, row, lane);
  }
  typename F::Acc part[ROWS] = {};
  for (int c = c0; c < nchunks; c += cstep) {
    typename F::Load wv[UNR][ROWS];
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      const int k0 = ((c + u) << F::kShift) + lane * ((1 << F::kShift) / 64);
      const bool ok = c + u < nchunks && k0 < K;
#pragma unroll
      for (int r = 0; r < ROWS; ++r) wv[u][r] = f.load(rw[r], c + u, k0, ok);
    }
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      if (c + u < nchunks) {
        const typename F::X x = F::x(smem, c + u, lane);
#pragma unroll
        for (int r = 0; r < ROWS; ++r) F::dot(wv[u][r], x, part[r]);
      }
    }
  }
#pragma unroll
  for (int r = 0; r < ROWS; ++r) acc[r] = F::post(wave_sum(F::sum(part[r])), rw[r]);
}

// ---- the whole-K task loop: blockDim = 64 * NW (any 1..16 waves share one staged copy of x), one wave per task, then the exchange tail ---------
template <class F, int ROWS, int UNR, int EPI, bool NORM>
__device__ __forceinline__ void gemv_whole_k(const GemvParams& p, const int nthreads) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nw = nthreads >> 6;
  const int nchunks = (p.k + (1 << F::kShift) - 1) >> F::kShift;
  uint32_t epoch = 0;
  if (EPI == kEpiResidTp) epoch = tp_epoch(p.tp);
  gemv_stage_x<F, NORM>(p, smem, nchunks, tid, nthreads);
  const F f(p);
  for (int task = blockIdx.x * nw + wave; task < p.tasks; task += gridDim.x * nw) {
    float acc[ROWS];
    gemv_stream<F, ROWS, UNR, EPI>(f, p, smem, task, lane, nchunks, 0, UNR, acc);
    gemv_epilogue<ROWS, EPI>(p, task, lane, acc, epoch);
  }
  if (EPI == kEpiResidTp) {
    // (no counter bump: the launch's epoch is counted by the host, TpParams::idx - a later collective of the step bumps the counter)
    for (int task = blockIdx.x * nw + wave; task < p.tasks; task += gridDim.x * nw) tp_take_task<ROWS>(p, epoch, task, lane);
  }
}

// The entry points: the names that kernel traces, bench.py's roofline label and DESIGN.md use.  (blockDim.x is read here, once: only in
// a __global__ function does the compiler know the workgroups to be uniform and fold the read to one scalar load.)
template <int ROWS, int UNR, int EPI, bool NORM>
__global__ __launch_bounds__(1024) void gemv_ldsx_kernel(GemvParams p) { gemv_whole_k<FmtBf16, ROWS, UNR, EPI, NORM>(p, blockDim.x); }

template <int ROWS, int UNR, int EPI, bool NORM, bool I8 = false>
__global__ __launch_bounds__(1024) void gemv8_ldsx_kernel(GemvParams p) { gemv_whole_k<FmtW8<I8>, ROWS, UNR, EPI, NORM>(p, blockDim.x); }

template <int ROWS, int UNR, int EPI, bool NORM>
__global__ __launch_bounds__(1024) void gemv4_ldsx_kernel(GemvParams p) { gemv_whole_k<FmtInt4, ROWS, UNR, EPI, NORM>(p, blockDim.x); }

// ------------------------------------------------------------------------------------------------
// K-split form for SHARD-sized projections (a rank of TP = 4 / 8: qkv is 896 x 5120 at TP = 8 - 448 row groups for 256 CUs).  A wave
// that walks the whole K alone is a chain of K / 1024 dependent HBM round trips, and with one or two such waves per CU nothing
// hides them: the launch sits at 9.6 us for 9 MB (profiles/r4_tp8_shard_kernel_trace.txt) where 3.3 us + bytes / 6.7 TB/s says 4.7.
// Here p.ks waves share a row group: wave j of the group takes the chunk pairs j, j + ks, ... (all of its loads in flight at once when
// ks = chunks / 2), the partial sums meet in LDS and wave 0 of the group adds them in wave order (fixed -> reproducible; NOT the
// bits of the whole-K kernel, which stays the one every TP = 1 shape runs) and applies the epilogue.  Same prologue, same stream loop.
// ------------------------------------------------------------------------------------------------
template <int EPI, bool NORM>
__global__ __launch_bounds__(1024) void gemv_ksplit_kernel(GemvParams p) {
  constexpr int ROWS = 2, UNR = 2;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nthreads = blockDim.x, nw = nthreads >> 6;
  const int nchunks = (p.k + 511) >> 9;
  float* part = gemv_stage_x<FmtBf16, NORM>(p, smem, nchunks, tid, nthreads) + 16;      // [nw][ROWS] partial sums of the K-slices
  const FmtBf16 f(p);

  const int ks = p.ks, ngroups = nw / ks, grp = wave / ks, j = wave - grp * ks;
  for (int t0 = blockIdx.x * ngroups; t0 < p.tasks; t0 += gridDim.x * ngroups) {      // (uniform trip count: barriers inside)
    const int task = t0 + grp;
    const bool valid = grp < ngroups && task < p.tasks;
    float acc[ROWS] = {0.f, 0.f};
    if (valid) {
      gemv_stream<FmtBf16, ROWS, UNR, EPI>(f, p, smem, task, lane, nchunks, j * UNR, ks * UNR, acc);
      if (lane == 0) { part[wave * ROWS] = acc[0]; part[wave * ROWS + 1] = acc[1]; }
    }
    __syncthreads();
    if (valid && j == 0) {
      float tot[ROWS];
#pragma unroll
      for (int r = 0; r < ROWS; ++r) {
        tot[r] = part[wave * ROWS + r];
        for (int i = 1; i < ks; ++i) tot[r] += part[(wave + i) * ROWS + r];          // wave order: fixed
      }
      gemv_epilogue<ROWS, EPI>(p, task, lane, tot);
    }
    __syncthreads();
  }
}

// ---- launch geometry -------------------------------------------------------------------------------------------------------------
enum GemvFormat { kBf16 = 0, kW8 = 1, kInt4 = 2 };

// row-group tasks of a projection: `rows` rows each, or rows / 2 gate / up pairs
static int gemv_tasks(int n, int epilogue, int rows) {
  const int swiglu = epilogue == CHATTS_EPI_SWIGLU;
  const int units = swiglu ? n / 2 : n, upt = swiglu ? rows / 2 : rows;
  return (units + upt - 1) / upt;
}

// Waves per workgroup (and workgroups per CU, 0 = whatever fits) of the GEMV for a shape: the sweep results of tools/gemv_sweep.py.
static void gemv_default_geometry(int n, int k, int epilogue, int cus, int* nw_out, int* occ_out) {
  const int units = epilogue == CHATTS_EPI_SWIGLU ? n / 2 : n;
  int nw_auto, occ_auto = 0;
  if (k > 8192) nw_auto = 16;                       // down_proj: 55 KB of x per workgroup -> amortise over 16 waves
  else if (units >= 65536) { nw_auto = 4; occ_auto = 2; }   // lm_head
  else if (n >= 16384) { nw_auto = 8; occ_auto = 2; }    // gate_up
  else if (n > 6000) nw_auto = 16;                  // qkv
  else nw_auto = 4;                                    // o_proj
  // Balanced layout (profiles/r2_gemv_sweep_balanced.txt): when the CUs divide the row-group tasks, one workgroup per CU whose
  // wave count divides the tasks per CU gives every wave the same number of tasks (no ragged last round): o_proj 11.5 ->
  // 11.2 us, gate_up 44.5 -> 44.1, down_proj 24.9 -> 24.5; lm_head (297 tasks per CU) keeps the 2-workgroup layout.
  const int tasks_r2 = gemv_tasks(n, epilogue, 2);
  int balanced_nw = 0;
  if (units < 65536 && tasks_r2 % cus == 0) {
    const int per_cu = tasks_r2 / cus;
    for (int w = 16; w >= 5 && !balanced_nw; --w)
      if (per_cu % w == 0) balanced_nw = w;
  }
  if (balanced_nw) { nw_auto = balanced_nw; occ_auto = 1; }
  *nw_out = nw_auto;
  *occ_out = occ_auto;
}

// Waves per row group of the bf16 GEMV (1 = the whole-K kernel): a pure function of the shape, so that a host-side test can pin which
// shapes take which kernel (tests/test_host_logic.py: every TP = 1 projection of the supported models resolves to 1 - the K-split form
// sums a row in another order - and the TP = 8 shard shapes to > 1).
//   tasks = row groups (2 rows, or one gate / up pair), nchunks = K / 512, w_bytes = N K 2.
static int gemv_pick_ksplit(int tasks, int nchunks, bool norm, double w_bytes, int cus) {
  if (nchunks < 4) return 1;
  int ks = 1;
  const double per_cu = (double)tasks / cus;
  const int rounds = (nchunks + 1) / 2;                   // chunk pairs of a row: a wave should keep at least one
  if (per_cu < 6.0) {
    // the row groups alone leave the chip nearly empty - fewer than ~6 waves per CU
    ks = (int)(12.0 / (per_cu > 0.25 ? per_cu : 0.25) + 0.999);
    if (ks > rounds) ks = rounds;
    if (ks > 8) ks = 8;
  } else if (norm && per_cu < 16.0 && w_bytes < 48e6) {
    // a SHARD-sized matrix whose row groups alone half-fill the chip (gate_up of a TP = 8 rank: 35 MB, 13.5 waves per CU): every wave
    // still walks K / 1024 dependent round trips; one chunk pair per wave measured 1.2 us per launch better (profiles/r4_tp_shard_step*).
    // The 48 MB bound keeps every TP = 1 shape (o_proj: 52 MB, 10 waves per CU; the 8B qkv: 50.3 MB) on the whole-K kernel; `norm`
    // restricts the rule to the column-parallel projections (qkv, gate_up: RMSNorm in the prologue) - the row-parallel ones (o_proj,
    // down_proj) must sum a row in the same order whether or not they carry the exchange (tp_reduce), which the K-split form does not do.
    ks = rounds > 8 ? 8 : rounds;
  }
  return ks;
}

struct GemvGeometry {
  int rows, unr;        // rows per wave, chunks in flight per row
  int nw, occ;          // waves per workgroup, workgroups per CU
  int tasks, blocks, threads;
  size_t lds;           // dynamic LDS of the launch
};

// The geometry of the whole-K launch of a call.  Defaults from the sweep in tools/gemv_sweep.py (profiles/gemv_sweep_r1.log): what varies
// with the shape is how many waves share one staged copy of x and how many workgroups a CU should hold.  Where the formats differ, the
// line says why.
static GemvGeometry gemv_geometry(const ChattsLinearArgs* a, GemvFormat fmt, int cus) {
  const int swiglu = a->epilogue == CHATTS_EPI_SWIGLU;
  const int units = swiglu ? a->n / 2 : a->n;
  GemvGeometry g;
  if (fmt == kInt4) {                  // the one form the 4-bit sweep kept: 2 rows x 4 chunks (8-byte loads) in flight
    g.rows = 2; g.unr = 4;
  } else if (fmt == kW8) {
    // per shape (kernel trace of the fp8 bench under each geometry, profiles/r6_gemv8_geometry.txt): the vocabulary projection wants 4 rows x 2
    // chunks in flight (778 MB: 144.8 -> 125.0 us), gate_up 4 rows x 1 (27.8 -> 26.9 us); the shorter launches keep 2 x 2 (4 rows halve
    // their task count: o / down 11.8 -> 14.5 us, qkv 10.3 -> 13.1)
    const int rows_auto = (units >= 65536 || (swiglu && a->n >= 16384)) ? 4 : 2, unr_auto = swiglu && a->n >= 16384 ? 1 : 2;
    g.rows = opt_get(OPT_GEMV8_ROWS, rows_auto); g.unr = opt_get(OPT_GEMV8_UNR, unr_auto);
    if (g.rows != 4 || a->tp_reduce) g.rows = 2;          // (the exchange-carrying form pushes 2 rows per task: tp_push_task's lane map)
    if (g.rows == 4) g.unr = g.unr == 2 ? 2 : 1;          // instantiated: <2,2> <2,4> <4,2> <4,1>
    else if (g.unr != 4) g.unr = 2;
  } else {                             // 2 x 2 wins on every decode shape; instantiated: <2,2> <2,4> <4,2> <4,4>
    g.rows = opt_get(OPT_GEMV_ROWS, 2) == 4 ? 4 : 2;
    g.unr = opt_get(OPT_GEMV_UNR, 2) == 4 ? 4 : 2;
  }
  int nw_auto, occ_auto;
  gemv_default_geometry(a->n, a->k, a->epilogue, cus, &nw_auto, &occ_auto);
  g.nw = opt_get(OPT_GEMV_NW, nw_auto);
  if (g.nw < 1 || g.nw > 16) g.nw = 4;
  if (fmt == kW8) {                    // GEMV8_NW: the 8-bit sweeps vary the wave count without moving the bf16 launches
    const int nw8 = opt_get(OPT_GEMV8_NW, g.nw);
    if (nw8 >= 1 && nw8 <= 16) g.nw = nw8;
  }
  const int chunk = fmt == kBf16 ? 512 : 1024;
  g.lds = (size_t)((a->k + chunk - 1) / chunk) * chunk * 4 + 64 * 4;
  if (fmt == kInt4) {
    // ~5 VALU ops per weight make this kernel ALU-latency bound: it wants every wave slot the registers allow (89 VGPRs -> 5 per
    // SIMD = 20 per CU), i.e. two workgroups per CU, not the one of the bf16 layouts
    g.occ = 20 / g.nw >= 1 ? 20 / g.nw : 1;
  } else {
    g.occ = (int)((150 * 1024) / g.lds);          // workgroups per CU that fit in LDS
    if (g.occ > 32 / g.nw) g.occ = 32 / g.nw;     // 32 waves per CU
    if (occ_auto && g.occ > occ_auto) g.occ = occ_auto;
    if (g.occ < 1) g.occ = 1;
  }
  g.occ = opt_get(OPT_GEMV_OCC, g.occ);
  if (fmt == kW8) g.occ = opt_get(OPT_GEMV8_OCC, g.occ);
  g.tasks = gemv_tasks(a->n, a->epilogue, g.rows);
  g.blocks = (g.tasks + g.nw - 1) / g.nw;
  if (g.blocks > cus * g.occ) g.blocks = cus * g.occ;
  if (fmt == kBf16) g.blocks = opt_get(OPT_GEMV_BLOCKS, g.blocks);      // (a test and sweep knob of the bf16 kernel: the tools that set it run bf16)
  // several emulated ranks on ONE device (tests, tools/jobs): their exchange-carrying launches wait for each other, so all of them
  // must be resident at once - cap the grid (results do not depend on it: a row is always summed by one wave in the same order)
  if (a->tp_reduce) { const int cap = opt_get(OPT_TP_FUSE_BLOCKS, 0); if (cap > 0 && g.blocks > cap) g.blocks = cap; }
  if (g.blocks < 1) g.blocks = 1;
  g.threads = g.nw * 64;
  // CHATTS_GEMV_LDSPAD = p (bf16 sweeps only, like GEMV_BLOCKS): declare 1/p of a CU's LDS, so that exactly p workgroups fit per CU and a
  // grid of cus * p workgroups is necessarily spread evenly (every CU streams the same number of bytes)
  const int pad = fmt == kBf16 ? opt_get(OPT_GEMV_LDSPAD, 0) : 0;
  if (pad >= 1 && (size_t)(160 * 1024 / pad) / 16 * 16 > g.lds) {
    const size_t need = g.lds;
    g.lds = (size_t)(160 * 1024 / pad) / 16 * 16;
    if (g.lds > 64 * 1024 && need <= 64 * 1024) g.lds = 64 * 1024;      // default dynamic-LDS cap of a launch (still 2 per CU)
  }
  return g;
}

// ---- dispatch: runtime (epilogue, norm) -> the instantiation of a kernel family ------------------------------------------------------
// A family names its kernel for <EPI, NORM>; kTp says whether it has the exchange-carrying instantiation (kEpiResidTp, never with NORM).
typedef void (*GemvKernel)(GemvParams);
template <int ROWS, int UNR> struct KBf16 {
  static constexpr bool kTp = true;
  template <int EPI, bool NORM> static GemvKernel get() { return gemv_ldsx_kernel<ROWS, UNR, EPI, NORM>; }
};
template <int ROWS, int UNR, bool I8> struct KW8 {
  static constexpr bool kTp = ROWS == 2;  // (tp_reduce launches 2 rows per task: gemv_geometry)
  template <int EPI, bool NORM> static GemvKernel get() { return gemv8_ldsx_kernel<ROWS, UNR, EPI, NORM, I8>; }
};
struct KInt4 {
  static constexpr bool kTp = false;      // (the launcher refuses tp_reduce with 4-bit codes)
  template <int EPI, bool NORM> static GemvKernel get() { return gemv4_ldsx_kernel<2, 4, EPI, NORM>; }
};
struct KSplit {
  static constexpr bool kTp = false;      // (the launcher keeps tp_reduce on the whole-K kernel)
  template <int EPI, bool NORM> static GemvKernel get() { return gemv_ksplit_kernel<EPI, NORM>; }
};

template <class KF>
static void gemv_dispatch(const GemvParams& p, int epi, bool norm, int blocks, int threads, size_t lds, hipStream_t s) {
  GemvKernel k = norm ? KF::template get<CHATTS_EPI_NONE, true>() : KF::template get<CHATTS_EPI_NONE, false>();
  if (epi == CHATTS_EPI_RESID) k = norm ? KF::template get<CHATTS_EPI_RESID, true>() : KF::template get<CHATTS_EPI_RESID, false>();
  if (epi == CHATTS_EPI_SWIGLU) k = norm ? KF::template get<CHATTS_EPI_SWIGLU, true>() : KF::template get<CHATTS_EPI_SWIGLU, false>();
  if constexpr (KF::kTp) {
    if (epi == kEpiResidTp) k = KF::template get<kEpiResidTp, false>();
  }
  hipLaunchKernelGGL(k, dim3(blocks), dim3(threads), lds, s, p);
}

template <bool I8>
static void gemv_dispatch_w8(const GemvParams& p, const GemvGeometry& g, int epi, bool norm, hipStream_t s) {
  if (g.rows == 4 && g.unr == 2) gemv_dispatch<KW8<4, 2, I8>>(p, epi, norm, g.blocks, g.threads, g.lds, s);
  else if (g.rows == 4) gemv_dispatch<KW8<4, 1, I8>>(p, epi, norm, g.blocks, g.threads, g.lds, s);
  else if (g.unr == 4) gemv_dispatch<KW8<2, 4, I8>>(p, epi, norm, g.blocks, g.threads, g.lds, s);
  else gemv_dispatch<KW8<2, 2, I8>>(p, epi, norm, g.blocks, g.threads, g.lds, s);
}

int launch_gemv(const ChattsLinearArgs* a, hipStream_t s) {
  GemvParams p;
  p.tp = TpParams{};
  p.w = a->w; p.x = a->a; p.bias = a->bias; p.resid = a->resid; p.out = a->c;
  p.norm_w = a->norm_w; p.eps = a->norm_eps; p.n = a->n; p.k = a->k; p.ldw = a->ldw;
  p.w8 = a->w8; p.w8_scale = a->w8_scale; p.ldw8 = a->ldw8; p.w8_format = a->w8_format;
  p.w4 = a->w4; p.w4_sz = a->w4_sz; p.ldw4 = a->ldw4; p.w4_group = a->w4_group;
  p.ks = 1;
  const bool norm = a->norm_w != nullptr;
  const int cus = device_cus();
  int epilogue = a->epilogue;
  if (a->tp_reduce) {       // row-parallel projection: the sum over the ranks is formed inside this launch (kEpiResidTp)
    CHATTS_REQUIRE(a->epilogue == CHATTS_EPI_RESID && !a->bias && !a->norm_w && !a->w4, CHATTS_E_BADARG,
                   "gemv: tp_reduce needs EPI_RESID without bias / fused norm / 4-bit codes");
    CHATTS_REQUIRE(a->n <= tp_capacity(a->tp_reduce), CHATTS_E_SHAPE, "gemv: tp_reduce of %d rows exceeds the exchange buffer (%lld)", a->n,
                   (long long)tp_capacity(a->tp_reduce));
    epilogue = kEpiResidTp;
  }
  const int nchunks = (a->k + 511) / 512;
  // (the bound is on the bf16 staging of x for every format, as it has always been; no supported K comes near it)
  CHATTS_REQUIRE((size_t)nchunks * 512 * 4 + 64 * 4 <= 160 * 1024, CHATTS_E_SHAPE, "gemv: K=%d too large for the LDS-resident x", a->k);
  const GemvFormat fmt = a->w4 != nullptr ? kInt4 : a->w8 != nullptr ? kW8 : kBf16;       // 4-bit codes win over an 8-bit copy
  const GemvGeometry g = gemv_geometry(a, fmt, cus);
  p.tasks = g.tasks;
  // K-split form (see gemv_ksplit_kernel): when the row groups alone leave the chip nearly empty - fewer than ~6 waves per CU - and a
  // row is long enough to split.  Every TP = 1 shape of the supported models has >= 10 waves per CU and keeps the whole-K kernel.
  if (fmt == kBf16 && !a->tp_reduce && g.rows == 2 && g.unr == 2 && nchunks >= 4) {
    int ks = gemv_pick_ksplit(g.tasks, nchunks, norm, (double)a->n * a->k * 2.0, cus);
    ks = opt_get(OPT_GEMV_KS, ks);
    if (ks > 16) ks = 16;
    if (ks > 1) {
      const int groups = 16 / ks, nwk = groups * ks;            // as many row groups as fit in 16 waves
      const size_t lds = (size_t)nchunks * 512 * 4 + 64 * 4;    // (never padded: GEMV_LDSPAD shapes the whole-K grid)
      int occk = (int)((150 * 1024) / lds) < 32 / nwk ? (int)((150 * 1024) / lds) : 32 / nwk;
      if (occk < 1) occk = 1;
      int blocksk = (g.tasks + groups - 1) / groups;
      if (blocksk > cus * occk) blocksk = cus * occk;
      p.ks = ks;
      gemv_dispatch<KSplit>(p, epilogue, norm, blocksk, nwk * 64, lds, s);
      CHATTS_CHECK_LAUNCH("gemv_ksplit");
      return CHATTS_OK;
    }
  }
  if (a->tp_reduce) p.tp = tp_issue(a->tp_reduce, false);      // (after the last check that can refuse the call: one issue per launch)
  if (fmt == kInt4) {
    gemv_dispatch<KInt4>(p, epilogue, norm, g.blocks, g.threads, g.lds, s);
    CHATTS_CHECK_LAUNCH("gemv4_ldsx");
  } else if (fmt == kW8) {
    if (p.w8_format == CHATTS_W8_INT8) gemv_dispatch_w8<true>(p, g, epilogue, norm, s);
    else gemv_dispatch_w8<false>(p, g, epilogue, norm, s);
    CHATTS_CHECK_LAUNCH("gemv8_ldsx");
  } else {
    if (g.rows == 4 && g.unr == 2) gemv_dispatch<KBf16<4, 2>>(p, epilogue, norm, g.blocks, g.threads, g.lds, s);
    else if (g.rows == 4) gemv_dispatch<KBf16<4, 4>>(p, epilogue, norm, g.blocks, g.threads, g.lds, s);
    else if (g.unr == 2) gemv_dispatch<KBf16<2, 2>>(p, epilogue, norm, g.blocks, g.threads, g.lds, s);
    else gemv_dispatch<KBf16<2, 4>>(p, epilogue, norm, g.blocks, g.threads, g.lds, s);
    CHATTS_CHECK_LAUNCH("gemv_ldsx");
  }
  return CHATTS_OK;
}

}  // namespace chatts

// host-only query (no device touched): the K-split factor the bf16 decode GEMV picks for a shape on this device - see gemv_pick_ksplit
extern "C" int chatts_gemv_ksplit(int n, int k, int epilogue, int has_norm) {
  if (n <= 0 || k <= 0) return -1;
  const int cus = chatts::device_cus() > 0 ? chatts::device_cus() : 256;
  return chatts::gemv_pick_ksplit(chatts::gemv_tasks(n, epilogue, 2), (k + 511) / 512, has_norm != 0, (double)n * k * 2.0, cus);
}
