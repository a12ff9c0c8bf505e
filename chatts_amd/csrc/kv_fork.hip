// kv_fork.hip - parallel sampling (n samples of one prompt from ONE prefill): what the siblings need from the prompt reaches their cache
// slots without running the decoder again.
//
//   kv_fork_kernel      rows [t0, t1) of every (K | V, layer, kv head) of a source slot -> m destination slots (grid y = the head, x
//                       strides over its rows).  A row is 128 elements =
//                       512 bytes (float32 cache) or 256 bytes (fp16 cache); a thread moves 16 bytes, so a wave access covers two (four)
//                       whole rows of consecutive memory.  Every source unit is loaded ONCE and stored m times; a thread keeps four units in
//                       flight (four loads, then 4 x m stores).  Contiguous cache: the slot is the outermost stride.  Paged cache: the row's
//                       block comes from the slot's table row, for the source and for every destination - the host shares the whole prompt
//                       blocks by reference count and hands this kernel only the trailing, partly filled block's rows.
//   state_fork_kernel   the source row of a per-(slot, id) int32 state (the logit controls' prompt marks and counts) -> m destination rows,
//                       the same way.
// Neither allocates, synchronises or reads anything back: both are graph-capturable.  The destination list is a host array of at most
// CHATTS_FORK_MAX_DST entries that travels in the kernel arguments.  Block numbers read from the table on the device are range-checked
// against the pool before they are used (a stale table can then not write outside the pool).
#include "common.h"

namespace chatts {

constexpr int kForkThreads = 256;
constexpr int kForkUnroll = 4;
constexpr int kForkMaxBlocks = 2048;

struct ForkDst {
  int32_t slot[CHATTS_FORK_MAX_DST];
};

struct KvForkParams {
  uint4* plane[2];                 // K and V: slot 0 / layer 0 (contiguous) or layer 0's pool (paged)
  int64_t layer_stride, seq_stride;        // in 16-byte units
  int n_layers, n_kv, max_ctx, upr_shift;  // upr = 16-byte units per row = 1 << upr_shift (5: float32, 4: fp16)
  const int32_t* table;
  int bs_shift, table_stride, n_blocks;    // block_size = 1 << bs_shift
  int src, m, t0, nrows;
};

// A chunk = the rows of one (slot, layer, head) that lie consecutively: the whole head (contiguous cache, chunk 0) or one block (paged).
// -> unit offset of the chunk's first row inside a plane; -1 when the table names a block outside the pool
__device__ __forceinline__ int64_t kv_fork_chunk(const KvForkParams& q, int slot, int layer, int head, int chunk) {
  if (q.table) {
    const int blk = q.table[(int64_t)slot * q.table_stride + chunk];
    if (blk < 0 || blk >= q.n_blocks) return -1;
    return (int64_t)layer * q.layer_stride + (((int64_t)blk * q.n_kv + head) << (q.bs_shift + q.upr_shift));
  }
  return (int64_t)slot * q.seq_stride + (int64_t)layer * q.layer_stride + (((int64_t)head * q.max_ctx) << q.upr_shift);
}

// grid: y = (plane, layer, head), x strides over that head's units of rows [t0, t1).  The table is read once per chunk a thread's four
// units touch (paged callers pass the rows of ONE block: one lookup for the source and one per destination and iteration).
__global__ __launch_bounds__(kForkThreads) void kv_fork_kernel(KvForkParams q, ForkDst d) {
  const int head = blockIdx.y % q.n_kv, pl = blockIdx.y / q.n_kv;
  const int layer = pl % q.n_layers, plane = pl / q.n_layers;
  uint4* base_ptr = q.plane[plane];
  const int per_head = q.nrows << q.upr_shift;
  const int stride = gridDim.x * kForkThreads * kForkUnroll;
  const int row_mask = q.table ? (1 << q.bs_shift) - 1 : 0x7fffffff;        // position -> row inside its chunk
  for (int base = blockIdx.x * kForkThreads * kForkUnroll; base < per_head; base += stride) {
    uint4 val[kForkUnroll];
    int chunk[kForkUnroll], in_chunk[kForkUnroll];  // chunk < 0: nothing to do; in_chunk = unit offset inside the chunk
    int cur = -1;
    int64_t cb = -1;
#pragma unroll
    for (int j = 0; j < kForkUnroll; ++j) {
      const int r = base + j * kForkThreads + threadIdx.x;
      chunk[j] = -1;
      if (r >= per_head) continue;
      const int p = q.t0 + (r >> q.upr_shift);
      const int c = q.table ? p >> q.bs_shift : 0;
      if (c != cur) { cb = kv_fork_chunk(q, q.src, layer, head, c); cur = c; }
      if (cb < 0) continue;
      chunk[j] = c;
      in_chunk[j] = ((p & row_mask) << q.upr_shift) + (r & ((1 << q.upr_shift) - 1));
      val[j] = base_ptr[cb + in_chunk[j]];
    }
    for (int i = 0; i < q.m; ++i) {
      cur = -1;
#pragma unroll
      for (int j = 0; j < kForkUnroll; ++j) {
        if (chunk[j] < 0) continue;
        if (chunk[j] != cur) { cb = kv_fork_chunk(q, d.slot[i], layer, head, chunk[j]); cur = chunk[j]; }
        if (cb >= 0) base_ptr[cb + in_chunk[j]] = val[j];
      }
    }
  }
}

struct StateForkParams {
  int32_t* state;
  int64_t stride, vocab;
  int src, m, vec;
};

__global__ __launch_bounds__(kForkThreads) void state_fork_kernel(StateForkParams q, ForkDst d) {
  const int32_t* S = q.state + (int64_t)q.src * q.stride;
  const int64_t i0 = (int64_t)blockIdx.x * kForkThreads + threadIdx.x, step = (int64_t)gridDim.x * kForkThreads;
  int64_t done = 0;
  if (q.vec) {                     // every row starts 16-byte aligned
    const int64_t nq = q.vocab / 4;
    const uint4* S4 = reinterpret_cast<const uint4*>(S);
    for (int64_t i = i0; i < nq; i += step) {
      const uint4 v = S4[i];
      for (int k = 0; k < q.m; ++k) reinterpret_cast<uint4*>(q.state + (int64_t)d.slot[k] * q.stride)[i] = v;
    }
    done = nq * 4;
  }
  for (int64_t i = done + i0; i < q.vocab; i += step) {
    const int32_t v = S[i];
    for (int k = 0; k < q.m; ++k) q.state[(int64_t)d.slot[k] * q.stride + i] = v;
  }
}

static int fork_dst(ForkDst* d, const int32_t* dst, int m, int src, int n_slots, const char* what) {
  CHATTS_REQUIRE(dst && m >= 1 && m <= CHATTS_FORK_MAX_DST, CHATTS_E_BADARG, "%s: 1..%d destinations, got %d", what, CHATTS_FORK_MAX_DST, m);
  CHATTS_REQUIRE(n_slots >= 1 && src >= 0 && src < n_slots, CHATTS_E_BADARG, "%s: source %d outside 0..%d", what, src, n_slots - 1);
  for (int i = 0; i < m; ++i) {
    CHATTS_REQUIRE(dst[i] >= 0 && dst[i] < n_slots && dst[i] != src, CHATTS_E_BADARG,
                   "%s: destination %d (entry %d) must lie in 0..%d and differ from the source %d", what, dst[i], i, n_slots - 1, src);
    for (int j = 0; j < i; ++j)
      CHATTS_REQUIRE(dst[j] != dst[i], CHATTS_E_BADARG, "%s: destination %d is listed twice", what, dst[i]);
    d->slot[i] = dst[i];
  }
  for (int i = m; i < CHATTS_FORK_MAX_DST; ++i) d->slot[i] = dst[0];
  return CHATTS_OK;
}

}  // namespace chatts

using namespace chatts;

extern "C" int chatts_kv_fork(const ChattsKvCache* cache, int n_layers, int n_kv, int n_slots, int64_t layer_stride, int64_t seq_stride,
                              int n_blocks, int src_slot, const int32_t* dst_slots, int m, int t0, int t1, chatts_stream_t stream) {
  CHATTS_REQUIRE(cache && cache->k && cache->v, CHATTS_E_BADARG, "kv_fork: cache, cache.k and cache.v are required");
  CHATTS_REQUIRE(cache->dtype == CHATTS_KV_F32 || cache->dtype == CHATTS_KV_F16, CHATTS_E_BADARG, "kv_fork: unknown cache dtype %d",
                 cache->dtype);
  CHATTS_REQUIRE(n_layers >= 1 && n_kv >= 1 && cache->max_ctx >= 1, CHATTS_E_BADARG, "kv_fork: bad sizes layers=%d kv heads=%d max_ctx=%d",
                 n_layers, n_kv, cache->max_ctx);
  CHATTS_REQUIRE(t0 >= 0 && t0 <= t1 && t1 <= cache->max_ctx, CHATTS_E_BADARG, "kv_fork: rows [%d, %d) outside 0..max_ctx=%d", t0, t1,
                 cache->max_ctx);
  ForkDst d;
  const int rc = fork_dst(&d, dst_slots, m, src_slot, n_slots, "kv_fork");
  if (rc != CHATTS_OK) return rc;
  const int shift = cache->dtype == CHATTS_KV_F16 ? 4 : 5;          // 16-byte units per 128-element row: 16 or 32
  const int64_t row_elems = 128;
  KvForkParams q;
  if (cache->block_table) {
    const int bs = cache->block_size;
    CHATTS_REQUIRE(bs >= 64 && bs <= 32768 && (bs & (bs - 1)) == 0 && cache->max_ctx % bs == 0, CHATTS_E_BADARG,
                   "kv_fork: block_size %d must be a power of two in 64..32768 that divides max_ctx=%d", bs, cache->max_ctx);
    CHATTS_REQUIRE(cache->table_stride >= cache->max_ctx / bs, CHATTS_E_BADARG, "kv_fork: table_stride %d < max_ctx / block_size",
                   cache->table_stride);
    CHATTS_REQUIRE(n_blocks >= 1 && layer_stride >= (int64_t)n_blocks * n_kv * bs * row_elems, CHATTS_E_BADARG,
                   "kv_fork: layer_stride %lld does not cover a pool of %d blocks", (long long)layer_stride, n_blocks);
  } else {
    CHATTS_REQUIRE(layer_stride >= (int64_t)n_kv * cache->max_ctx * row_elems && seq_stride >= (int64_t)n_layers * layer_stride,
                   CHATTS_E_BADARG, "kv_fork: strides %lld / %lld do not cover [layers, kv heads, max_ctx, 128]", (long long)layer_stride,
                   (long long)seq_stride);
  }
  CHATTS_REQUIRE(((reinterpret_cast<uintptr_t>(cache->k) | reinterpret_cast<uintptr_t>(cache->v)) & 15) == 0, CHATTS_E_BADARG,
                 "kv_fork: the cache must be 16-byte aligned");
  const int epu = cache->dtype == CHATTS_KV_F16 ? 8 : 4;           // elements per 16-byte unit (row strides are multiples of 128 elements)
  q.plane[0] = reinterpret_cast<uint4*>(cache->k);
  q.plane[1] = reinterpret_cast<uint4*>(cache->v);
  CHATTS_REQUIRE(layer_stride % epu == 0 && seq_stride % epu == 0, CHATTS_E_BADARG, "kv_fork: strides must be multiples of 16 bytes");
  q.layer_stride = layer_stride / epu;
  q.seq_stride = seq_stride / epu;
  q.n_layers = n_layers; q.n_kv = n_kv; q.max_ctx = cache->max_ctx; q.upr_shift = shift;
  q.table = cache->block_table; q.table_stride = cache->table_stride; q.n_blocks = n_blocks;
  q.bs_shift = 0;
  while (cache->block_table && (1 << q.bs_shift) < cache->block_size) ++q.bs_shift;
  q.src = src_slot; q.m = m; q.t0 = t0; q.nrows = t1 - t0;
  const int64_t ny = 2 * (int64_t)n_layers * n_kv;
  CHATTS_REQUIRE(ny <= 65535, CHATTS_E_BADARG, "kv_fork: layers x kv heads = %lld exceeds the grid", (long long)(ny / 2));
  if (t1 == t0) return CHATTS_OK;                                  // nothing to copy (paged: the prompt ends on a block boundary)
  const int per_block = kForkThreads * kForkUnroll;
  const int64_t want = (((int64_t)q.nrows << shift) + per_block - 1) / per_block;
  const int64_t cap = kForkMaxBlocks / ny > 0 ? kForkMaxBlocks / ny : 1;
  hipLaunchKernelGGL(kv_fork_kernel, dim3((unsigned)(want < cap ? want : cap), (unsigned)ny), dim3(kForkThreads), 0, as_stream(stream), q, d);
  CHATTS_CHECK_LAUNCH("kv_fork");
  return CHATTS_OK;
}

extern "C" int chatts_logit_state_fork(int32_t* state, int64_t state_stride, int64_t vocab, int n_rows, int src_row, const int32_t* dst_rows,
                                       int m, chatts_stream_t stream) {
  CHATTS_REQUIRE(state && vocab > 0 && state_stride >= vocab, CHATTS_E_BADARG, "logit_state_fork: state, vocab > 0 and stride >= vocab are required");
  ForkDst d;
  const int rc = fork_dst(&d, dst_rows, m, src_row, n_rows, "logit_state_fork");
  if (rc != CHATTS_OK) return rc;
  StateForkParams q;
  q.state = state; q.stride = state_stride; q.vocab = vocab; q.src = src_row; q.m = m;
  q.vec = (reinterpret_cast<uintptr_t>(state) & 15) == 0 && state_stride % 4 == 0;
  const int64_t blocks = (vocab / 4 + kForkThreads - 1) / kForkThreads + 1;
  hipLaunchKernelGGL(state_fork_kernel, dim3((unsigned)(blocks < 256 ? blocks : 256)), dim3(kForkThreads), 0, as_stream(stream), q, d);
  CHATTS_CHECK_LAUNCH("logit_state_fork");
  return CHATTS_OK;
}
