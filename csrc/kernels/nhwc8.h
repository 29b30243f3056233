// The 8-channel vector of the NHWC kernels and the column-lane work split built on it.
// A lane owns one 16-byte column of channels (8 bf16, or 8 fp32 as two float4) and one pixel (row) lane; the partial
// sums of a column's pixel lanes meet in LDS.  Loads, shifts and pack2bf only: the code is the same under any
// floating-point contraction or packed-fp32 setting of the including file.
#pragma once
#include "common.h"

// eight bf16 of a 16-byte vector as floats, in memory order, and back
__device__ __forceinline__ void unpack8(uint4 u, float* f) {
  f[0] = lo_bf(u.x); f[1] = hi_bf(u.x); f[2] = lo_bf(u.y); f[3] = hi_bf(u.y);
  f[4] = lo_bf(u.z); f[5] = hi_bf(u.z); f[6] = lo_bf(u.w); f[7] = hi_bf(u.w);
}
__device__ __forceinline__ uint4 pack8(const float* f) {
  return make_uint4(pack2bf(f[0], f[1]), pack2bf(f[2], f[3]), pack2bf(f[4], f[5]), pack2bf(f[6], f[7]));
}

// elements i .. i + 7 of a bf16 (BF16) or fp32 tensor
template <bool BF16>
__device__ __forceinline__ void ld8(const void* p, size_t i, float* v) {
  if (BF16) {
    unpack8(*(const uint4*)((const bf16_t*)p + i), v);
  } else {
    const float4 a = *(const float4*)((const float*)p + i), b = *(const float4*)((const float*)p + i + 4);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
  }
}
template <bool BF16>
__device__ __forceinline__ void st8(void* p, size_t i, const float* v) {
  if (BF16) {
    *(uint4*)((bf16_t*)p + i) = pack8(v);
  } else {
    *(float4*)((float*)p + i) = make_float4(v[0], v[1], v[2], v[3]);
    *(float4*)((float*)p + i + 4) = make_float4(v[4], v[5], v[6], v[7]);
  }
}

// 16-byte access, non-temporal where NT (streams that are not read again soon)
typedef unsigned int v4u_t __attribute__((ext_vector_type(4)));
template <bool NT>
__device__ __forceinline__ uint4 ld16(const bf16_t* p) {
  if (NT) {
    v4u_t v = __builtin_nontemporal_load((const v4u_t*)p);
    return make_uint4(v.x, v.y, v.z, v.w);
  }
  return *(const uint4*)p;
}
template <bool NT>
__device__ __forceinline__ void st16(bf16_t* p, uint4 u) {
  if (NT) {
    v4u_t v = {u.x, u.y, u.z, u.w};
    __builtin_nontemporal_store(v, (v4u_t*)p);
  } else {
    *(uint4*)p = u;
  }
}

// The columns [c0, c0 + cc) of a tensor of C8 columns on a block of T lanes: lane t owns column c0 + col and the
// pixel lane pl of PL; c is the column's first channel (c0 and col serve groupnorm.hip's fold of columns to groups).
struct Chunk {
  int c0, cc, PL, col, pl, c;
  bool live;
};
template <int T>
__device__ __forceinline__ Chunk make_chunk(int c0, int C8) {
  Chunk k;
  k.c0 = c0;
  k.cc = min(T, C8 - c0);
  k.PL = T / k.cc;
  k.col = threadIdx.x % k.cc;
  k.pl = threadIdx.x / k.cc;
  k.live = k.pl < k.PL;  // T need not be a multiple of cc
  k.c = (c0 + k.col) * 8;
  return k;
}

// Column-fixed lane mapping: lane t owns channel block (t % cols) * 8 and row-lane t / cols; with RP = NT / cols
// row-lanes, lanes >= RP * cols idle (cols need not divide NT).  col_tree8 sums the per-lane [8] partials s (A == 1)
// or s and q (A == 2) of the RP row-lanes of each column in LDS by a fixed tree: the row-lanes beyond the largest
// power of two fold first, then the rest halves.  It returns false when RP == 1 (a lane's partials are its totals;
// LDS is not touched), else true with the totals of column t in red[0][t] (and red[1][t]), t < cols.  Called by the
// whole block.
template <int A, int NT>
__device__ __forceinline__ bool col_tree8(float (*red)[NT][8], const float* s, const float* q, int cols) {
  static_assert(A == 1 || A == 2, "one or two accumulator sets");
  const int t = threadIdx.x, RP = NT / cols;
  if (RP == 1) return false;
  __syncthreads();  // red may still be read by a previous call
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    red[0][t][e] = s[e];
    if (A == 2) red[1][t][e] = q[e];
  }
  __syncthreads();
  int P = 1;
  while (P * 2 <= RP) P *= 2;
  if (P < RP) {  // fold the row-lanes beyond the largest power of two
    if (t < (RP - P) * cols) {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        red[0][t][e] += red[0][t + P * cols][e];
        if (A == 2) red[1][t][e] += red[1][t + P * cols][e];
      }
    }
    __syncthreads();
  }
  for (int h = P / 2; h >= 1; h >>= 1) {
    if (t < h * cols) {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        red[0][t][e] += red[0][t + h * cols][e];
        if (A == 2) red[1][t][e] += red[1][t + h * cols][e];
      }
    }
    __syncthreads();
  }
  return true;
}

// Two sets (s, q): the per-block partial row out0[c0 .. c0 + 7], out1[...] (plain stores; reduced later by
// reduce_rows).  atomic: add into the final [C] sums instead (small grids: one launch fewer, <= a few hundred adders
// per address).
template <int NT = 256>
__device__ __forceinline__ void col_reduce8(float (*red)[NT][8], const float* s, const float* q, float* out0,
                                            float* out1, int cols, int c0, bool atomic = false) {
  const int t = threadIdx.x;
  if (!col_tree8<2, NT>(red, s, q, cols)) {
    if (t < cols) {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        if (atomic) { atomicAdd(out0 + c0 + e, s[e]); atomicAdd(out1 + c0 + e, q[e]); }
        else { out0[c0 + e] = s[e]; out1[c0 + e] = q[e]; }
      }
    }
    return;
  }
  if (t < cols) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      if (atomic) { atomicAdd(out0 + c0 + e, red[0][t][e]); atomicAdd(out1 + c0 + e, red[1][t][e]); }
      else { out0[c0 + e] = red[0][t][e]; out1[c0 + e] = red[1][t][e]; }
    }
  }
}
