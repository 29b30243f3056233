// The row walk and the fixed-order fp64 sums of the multi-tensor kernels (optim.hip, sam.hip, summary.hip,
// metrics.hip): one block (or one wave) per row of a host-built table, each row a run of up to CHUNK elements that
// starts at any element offset (tensors are views into flat buffers).
//
// A row is walked as a scalar head up to the first 16-byte boundary, 16-byte accesses over the body and a scalar
// tail - or with coalesced scalar accesses throughout where the arrays a kernel touches do not reach a boundary
// together.  Every kernel visits, per thread, the head element, then its body groups in increasing index with the
// group's elements in order, then the tail element: the per-thread order the fp64 sums are formed in, and the same
// element-wise function on either path, so the two paths give the same bits.
//
// The index arithmetic and the walker need nothing of HIP (csrc/kernels/tests/chunk_walk_test.cpp compiles them with
// the host compiler); the reductions below them are device code.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#include "common.h"
#define DTM_HD __host__ __device__ __forceinline__
#else
#define DTM_HD inline
#endif

namespace dtm {

struct ChunkRow { int t, pad; long start; };  // a chunk-table row: elements [start, start + CHUNK) of tensor t
struct ChunkSpan { int chunk0, nchunks; };    // per tensor: its rows of the chunk table (contiguous, in order)

// elements of the row that starts at `start` in a tensor of n elements
DTM_HD int chunk_len(long n, long start, int chunk) {
  const long rem = n - start;
  return (int)(rem < (long)chunk ? (rem > 0 ? rem : 0) : (long)chunk);
}

// the pointers share their offset from a 16-byte boundary
template <typename... P>
DTM_HD bool same16(const void* a, const P*... b) {
  return ((((uintptr_t)a ^ (uintptr_t)b) | ... | (uintptr_t)0) & 15u) == 0;
}

// elements (of elem_bytes each, 2 or 4) in front of the first 16-byte boundary at or after addr
DTM_HD int head_elems(uintptr_t addr, int elem_bytes) {
  return (int)(((16u - (unsigned)(addr & 15u)) & 15u) / (unsigned)elem_bytes);
}

// the optional bf16 copy of the fp32 array at addr takes 8-byte stores over the body: it is absent, or on an 8-byte
// boundary where the fp32 array is on its 16-byte one (a part of a caller's vec_ok below)
DTM_HD bool copy8_ok(const void* copy, uintptr_t addr) {
  return !copy || (((uintptr_t)copy + 2u * (unsigned)head_elems(addr, 4)) & 7u) == 0;
}

// Scalar indices [0, head) and [tail0, len), 16-byte groups g = 0 .. nvec-1 over [head + g*VEC, head + (g+1)*VEC)
// with VEC = 16 / elem_bytes.  {0, 0, 0}: scalar throughout.
struct WalkPlan {
  int head, nvec, tail0, len;
};

// addr: the leading array's first element of the row; vec_ok: every array the kernel touches may be accessed in
// 16-byte groups once the leading one is (same16, and whatever else the caller needs)
DTM_HD WalkPlan walk_plan(int elem_bytes, uintptr_t addr, int len, bool vec_ok) {
  WalkPlan w = {0, 0, 0, len};
  if (!vec_ok) return w;
  const int h = head_elems(addr, elem_bytes);
  w.head = h < len ? h : len;
  const unsigned vec = 16u / (unsigned)elem_bytes, body = (unsigned)(len - w.head);
  w.nvec = (int)(body / vec);
  w.tail0 = len - (int)(body % vec);  // (= head + nvec * vec)
  return w;
}

// Thread tid of STRIDE: scalar(i) for its head element, vec(g, head + g*VEC) for its groups, scalar(i) for its tail
// element (a tail is shorter than VEC <= STRIDE, so that loop runs more than once only when the plan is scalar
// throughout, where it is the whole walk).
template <int STRIDE, int VEC, typename S, typename V>
DTM_HD void walk(const WalkPlan& w, int tid, S scalar, V vec) {
  static_assert(VEC <= STRIDE, "a tail must fit one pass of the threads");
  if (tid < w.head) scalar(tid);
  for (int g = tid; g < w.nvec; g += STRIDE) vec(g, w.head + g * VEC);
  for (int r = tid; r < w.len - w.tail0; r += STRIDE) scalar(w.tail0 + r);
}

#ifdef __HIPCC__
constexpr int ROW_THREADS = 256;  // the block of a chunk-row kernel

__device__ __forceinline__ float elem_f32(float v) { return v; }
__device__ __forceinline__ float elem_f32(bf16_t v) { return bf2f(v); }
// f(i, v) for every element i of a read-only row x[0, len) of fp32 or bf16, v its value as fp32: thread tid of
// STRIDE takes its share in walk()'s order, with 16-byte loads over the body
template <int STRIDE, typename T, typename F>
__device__ __forceinline__ void visit_row(const T* x, int len, int tid, F f) {
  constexpr int VEC = 16 / (int)sizeof(T);
  typedef T vec_t __attribute__((ext_vector_type(VEC)));
  const WalkPlan w = walk_plan(sizeof(T), (uintptr_t)x, len, true);
  const vec_t* xv = (const vec_t*)(x + w.head);
  walk<STRIDE, VEC>(w, tid, [&](int i) { f(i, elem_f32(x[i])); },
                    [&](int g, int i0) {
                      const vec_t v = xv[g];
#pragma unroll
                      for (int e = 0; e < VEC; ++e) f(i0 + e, elem_f32((T)v[e]));
                    });
}
// group g of a bf16 copy's body (copy8_ok), from the fp32 group
__device__ __forceinline__ void store_bf16x4(bf16_t* body, int g, const f32x4& w) {
  ((uint2*)body)[g] = make_uint2(pack2bf(w[0], w[1]), pack2bf(w[2], w[3]));
}

// ---- fixed-order fp64 sums: a xor butterfly over each wave, then the waves in LDS -------------------------------
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// N sums over a 256-thread block; the result is thread 0's: (w0 + w1) + (w2 + w3)
template <int N>
__device__ __forceinline__ void block_sum_f64(double (&v)[N], int tid) {
  __shared__ double red[ROW_THREADS / 64][N];
#pragma unroll
  for (int k = 0; k < N; ++k) v[k] = wave_sum_f64(v[k]);
  if ((tid & 63) == 0) {
#pragma unroll
    for (int k = 0; k < N; ++k) red[tid >> 6][k] = v[k];
  }
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int k = 0; k < N; ++k) v[k] = (red[0][k] + red[1][k]) + (red[2][k] + red[3][k]);
  }
}

// One wave sums a tensor's records: lane l takes records l, l+64, ... in chunk order, then the butterfly.  Rec is a
// record of fp64 sums and nothing else (double, NormRec); s receives one total per sum, in every lane.
template <typename Rec>
__device__ __forceinline__ void record_sum(const Rec* recs, ChunkSpan m, int lane,
                                           double (&s)[sizeof(Rec) / sizeof(double)]) {
  constexpr int N = sizeof(Rec) / sizeof(double);
  static_assert(sizeof(Rec) == N * sizeof(double), "a record of fp64 sums");
#pragma unroll
  for (int k = 0; k < N; ++k) s[k] = 0.0;
  for (int j = lane; j < m.nchunks; j += 64) {
    const Rec r = recs[m.chunk0 + j];
    double d[N];
    __builtin_memcpy(d, &r, sizeof(Rec));
#pragma unroll
    for (int k = 0; k < N; ++k) s[k] += d[k];
  }
#pragma unroll
  for (int k = 0; k < N; ++k) s[k] = wave_sum_f64(s[k]);
}

// ---- the EMA shadow of the optimizer kernels ----------------------------------------------------------------------
__device__ __forceinline__ float ema_elem(float e, float p, float omd) {  // e -= (1-d)(e - p)
  return __fmaf_rn(-omd, __fsub_rn(e, p), e);
}
// EMA-only row (BN moving statistics): shadow -= (1-d)(shadow - value)
__device__ __forceinline__ void ema_only_row(float* shadow, const float* value, int len, float ema_decay, int tid) {
  for (int i = tid; i < len; i += ROW_THREADS) shadow[i] -= (1.f - ema_decay) * (shadow[i] - value[i]);
}
#endif  // __HIPCC__

}  // namespace dtm
