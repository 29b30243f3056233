// Top-k gradient sparsification with error feedback over one bucket of the flat gradient buffer (ops/compress.py,
// parallel/bsp.py).  ``g`` is the bucket's range of this rank's summed gradient, ``res`` the same range of the
// rank-local residual, n their length, k the packet size (a host integer).
//
// Compress:
//   u[i]   = res[i] + g[i]                               (__fadd_rn)
//   key(i) = bits(u[i]) & 0x7fffffff as an unsigned      (prune.hip's key: -0 == +0, denormals order, Inf / NaN top)
//   S      = the first k elements by (key descending, index ascending): exactly k, whatever the ties
//   packet = int32[2k]: idx[j] the indices of S in ascending order, val[j] = bits(u[idx[j]])
//   res[i] = +0 where i is in S or u[i] is not finite, else u[i]
// Decompress (W packets [W][2k], in rank order): g = +0, then for w = 0 .. W-1: g[idx_w[j]] += val_w[j] (__fadd_rn),
// one launch per source rank in stream order: indices are unique within a packet, so there are no float atomics and
// every rank ends with the same bits.
//
// Compress is 10 launches, stream order their only synchronisation:
//   init     clears the histogram, rank = n - k + 1 (the k-th largest key is the rank-th smallest)
//   hist x3  a radix select on the 31-bit key, most significant digit first, 11 + 10 + 10 bits, as prune.hip's: one
//   scan x3  block per chunk row counts the digit in LDS and adds its non-empty bins to the global histogram (uint32
//            adds: order-free), one block finds the bin the rank falls in.  The first hist launch forms u and stores it
//            into res (8 B read, 4 B written per element); later launches read res only.  After the last digit the
//            prefix is tau, the k-th largest key.
//   count    per chunk row: the number of keys > tau and the number == tau
//   rowscan  one block: exclusive sums of both over the rows, in row order; need = k - (number of keys > tau), the
//            ties to take
//   pack     per row, per pass of the block over it: every lane counts its elements above and at tau, an inclusive
//            scan over the wave (shuffles) and the four wave totals in LDS give each element the number of such
//            elements in front of it; element i is taken when key > tau, or key == tau with fewer than need ties in
//            front, and goes to slot (keys > tau in front) + min(ties in front, need).  res is rewritten where it
//            changes.
// About 32 bytes per element in all; nothing is allocated or read back.
//
// A bucket may start at any element: where res and g reach a 16-byte boundary together, row 0 takes the up-to-3
// element head with 4-byte accesses, every row then moves 16 bytes per lane (a lane owns 4 consecutive elements of
// a pass) and the last one ends with a 4-byte tail; otherwise every access is a coalesced 4-byte one.  Either way a
// block visits its row in passes, and within a pass element order is (lane, element of the lane): the index order.
#include "common.h"

namespace dtm {

constexpr int GC_CHUNK = 8192;  // elements per chunk row (a multiple of 4)
constexpr int GC_BINS = 2048;   // the widest digit
constexpr int GC_THREADS = 256;
// scratch (uint32 words): [0, GC_BINS) histogram | GC_ST + {0 prefix, 1 rank, 2 tau, 3 need} | GC_ROWS + 2 * row:
// {keys > tau, keys == tau} of the row, after rowscan their exclusive sums
constexpr int GC_ST = GC_BINS, GC_ROWS = GC_BINS + 8;

struct GcPlan {
  long n;
  int head;  // elements in front of the first 16-byte boundary (vec only)
  int vec;   // 16-byte path
  int rows;
};

static GcPlan gc_plan(const void* res, const void* g, long n) {
  GcPlan P;
  P.n = n;
  P.vec = (((uintptr_t)res ^ (uintptr_t)g) & 15) == 0 ? 1 : 0;
  P.head = 0;
  if (P.vec) {
    P.head = (int)(((16 - ((uintptr_t)res & 15)) & 15) >> 2);
    if (P.head > n) P.head = (int)n;
  }
  const long body = n - P.head;
  P.rows = body <= 0 ? 1 : (int)((body + GC_CHUNK - 1) / GC_CHUNK);
  return P;
}

// f(i0, cnt, vec): this lane's elements [i0, i0 + cnt) of one pass over row j (cnt 0, 1 or 4; 4 with vec set: one
// 16-byte group).  Every thread of the block calls f the same number of times, so f may hold a barrier.
template <class F>
__device__ __forceinline__ void gc_for_row(const GcPlan& P, int j, F f) {
  const int tid = threadIdx.x;
  const long vlo = P.head + (long)j * GC_CHUNK;
  long hi = vlo + GC_CHUNK;
  if (hi > P.n) hi = P.n;
  if (!P.vec) {
    for (long b = vlo; b < hi; b += GC_THREADS) f(b + tid, b + tid < hi ? 1 : 0, false);
    return;
  }
  if (j == 0 && P.head > 0) f((long)tid, tid < P.head ? 1 : 0, false);
  if (vlo >= hi) return;
  const long nvec = (hi - vlo) >> 2;
  for (long vb = 0; vb < nvec; vb += GC_THREADS) f(vlo + ((vb + tid) << 2), vb + tid < nvec ? 4 : 0, true);
  const long t0 = vlo + (nvec << 2);
  if (t0 < hi) f(t0 + tid, t0 + tid < hi ? 1 : 0, false);
}

// the lane's elements of a pass, as bits
__device__ __forceinline__ void gc_load(const uint32_t* __restrict__ p, long i0, int cnt, bool vec, uint32_t (&x)[4]) {
  x[0] = x[1] = x[2] = x[3] = 0u;
  if (vec) {
    if (cnt == 4) {
      const uint4 v = *reinterpret_cast<const uint4*>(p + i0);
      x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
    }
  } else if (cnt == 1) {
    x[0] = p[i0];
  }
}

__device__ __forceinline__ void gc_store(uint32_t* __restrict__ p, long i0, int cnt, bool vec, const uint32_t (&x)[4]) {
  if (vec) {
    if (cnt == 4) *reinterpret_cast<uint4*>(p + i0) = make_uint4(x[0], x[1], x[2], x[3]);
  } else if (cnt == 1) {
    p[i0] = x[0];
  }
}

__global__ __launch_bounds__(GC_THREADS) void gc_init_kernel(uint32_t* __restrict__ scratch, uint32_t rank) {
  for (int b = threadIdx.x; b < GC_BINS; b += GC_THREADS) scratch[b] = 0u;
  if (threadIdx.x < 4) scratch[GC_ST + threadIdx.x] = threadIdx.x == 1 ? rank : 0u;
}

// digit = (key >> shift) & (2^bits - 1), counted where key >> (shift + bits) == the prefix so far.  FORM: the first
// digit's launch, which forms u = res + g and stores it into res.
template <bool FORM>
__global__ __launch_bounds__(GC_THREADS) void gc_hist_kernel(GcPlan P, uint32_t* __restrict__ res,
                                                             const uint32_t* __restrict__ g,
                                                             uint32_t* __restrict__ scratch, int shift, int bits) {
  __shared__ uint32_t h[GC_BINS];
  const int nb = 1 << bits;
  const uint32_t prefix = scratch[GC_ST], dmask = (uint32_t)nb - 1u;
  const int hs = shift + bits;  // <= 31, and key < 2^31: digit 0 compares 0 with the prefix 0
  for (int b = threadIdx.x; b < nb; b += GC_THREADS) h[b] = 0u;
  __syncthreads();
  gc_for_row(P, blockIdx.x, [&](long i0, int cnt, bool vec) {
    uint32_t x[4];
    gc_load(res, i0, cnt, vec, x);
    if constexpr (FORM) {
      uint32_t y[4];
      gc_load(g, i0, cnt, vec, y);
#pragma unroll
      for (int e = 0; e < 4; ++e) x[e] = __float_as_uint(__fadd_rn(__uint_as_float(x[e]), __uint_as_float(y[e])));
      gc_store(res, i0, cnt, vec, x);
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const uint32_t key = x[e] & 0x7fffffffu;
      if (e < cnt && (key >> hs) == prefix) atomicAdd(&h[(key >> shift) & dmask], 1u);
    }
  });
  __syncthreads();
  for (int b = threadIdx.x; b < nb; b += GC_THREADS) {
    const uint32_t c = h[b];
    if (c != 0u) atomicAdd(&scratch[b], c);
  }
}

// one block: the bin with  count before it < rank <= count through it  (rank is 1-based, from the smallest key)
__global__ __launch_bounds__(GC_THREADS) void gc_scan_kernel(uint32_t* __restrict__ scratch, int bits, int last) {
  const int tid = threadIdx.x;
  const uint32_t px = scratch[GC_ST], rank = scratch[GC_ST + 1];
  const int per = (1 << bits) / GC_THREADS;  // 8 or 4 consecutive bins per lane
  uint32_t c[GC_BINS / GC_THREADS];
  uint32_t sum = 0u;
  uint32_t* row = scratch + tid * per;
#pragma unroll
  for (int k = 0; k < GC_BINS / GC_THREADS; ++k) {
    c[k] = 0u;
    if (k < per) { c[k] = row[k]; row[k] = 0u; }
    sum += c[k];
  }
  __shared__ uint32_t s[GC_THREADS];
  s[tid] = sum;
  __syncthreads();  // (also: every lane has read the state before the one store below)
  for (int off = 1; off < GC_THREADS; off <<= 1) {
    const uint32_t v = tid >= off ? s[tid - off] : 0u;
    __syncthreads();
    s[tid] += v;
    __syncthreads();
  }
  uint32_t run = s[tid] - sum;
#pragma unroll
  for (int k = 0; k < GC_BINS / GC_THREADS; ++k) {
    if (k < per && run < rank && rank <= run + c[k]) {
      const uint32_t p = (px << bits) | (uint32_t)(tid * per + k);
      scratch[GC_ST] = p;
      scratch[GC_ST + 1] = rank - run;
      if (last) scratch[GC_ST + 2] = p;
    }
    run += c[k];
  }
}

// (above tau) | (at tau) << 16 of a pass's lane elements
__device__ __forceinline__ uint32_t gc_classify(const uint32_t (&x)[4], int cnt, uint32_t tau) {
  uint32_t v = 0u;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const uint32_t key = x[e] & 0x7fffffffu;
    if (e < cnt) v += key > tau ? 1u : (key == tau ? 0x10000u : 0u);
  }
  return v;
}

__global__ __launch_bounds__(GC_THREADS) void gc_count_kernel(GcPlan P, const uint32_t* __restrict__ res,
                                                              uint32_t* __restrict__ scratch) {
  const uint32_t tau = scratch[GC_ST + 2];
  int gt = 0, eq = 0;
  gc_for_row(P, blockIdx.x, [&](long i0, int cnt, bool vec) {
    uint32_t x[4];
    gc_load(res, i0, cnt, vec, x);
    const uint32_t v = gc_classify(x, cnt, tau);
    gt += (int)(v & 0xffffu);
    eq += (int)(v >> 16);
  });
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    gt += __shfl_xor(gt, o, 64);
    eq += __shfl_xor(eq, o, 64);
  }
  __shared__ int wg[GC_THREADS / 64], we[GC_THREADS / 64];
  if ((threadIdx.x & 63) == 0) { wg[threadIdx.x >> 6] = gt; we[threadIdx.x >> 6] = eq; }
  __syncthreads();
  if (threadIdx.x == 0) {
    scratch[GC_ROWS + 2 * blockIdx.x] = (uint32_t)(wg[0] + wg[1] + wg[2] + wg[3]);
    scratch[GC_ROWS + 2 * blockIdx.x + 1] = (uint32_t)(we[0] + we[1] + we[2] + we[3]);
  }
}

// one block: the row counts become their exclusive sums in row order; need = k - (keys > tau)
__global__ __launch_bounds__(GC_THREADS) void gc_rowscan_kernel(uint32_t* __restrict__ scratch, int rows, uint32_t k) {
  const int tid = threadIdx.x;
  const int per = (rows + GC_THREADS - 1) / GC_THREADS;
  const int r0 = tid * per, r1 = min(rows, r0 + per);
  uint2* rc = reinterpret_cast<uint2*>(scratch + GC_ROWS);
  uint32_t sg = 0u, se = 0u;
  for (int r = r0; r < r1; ++r) { const uint2 c = rc[r]; sg += c.x; se += c.y; }
  __shared__ uint32_t ag[GC_THREADS], ae[GC_THREADS];
  ag[tid] = sg;
  ae[tid] = se;
  __syncthreads();
  for (int off = 1; off < GC_THREADS; off <<= 1) {
    const uint32_t vg = tid >= off ? ag[tid - off] : 0u, ve = tid >= off ? ae[tid - off] : 0u;
    __syncthreads();
    ag[tid] += vg;
    ae[tid] += ve;
    __syncthreads();
  }
  uint32_t rg = ag[tid] - sg, re = ae[tid] - se;
  for (int r = r0; r < r1; ++r) {
    const uint2 c = rc[r];
    rc[r] = make_uint2(rg, re);
    rg += c.x;
    re += c.y;
  }
  if (tid == GC_THREADS - 1) scratch[GC_ST + 3] = k - ag[tid];
}

__device__ __forceinline__ bool gc_nonfinite(uint32_t b) { return (b & 0x7f800000u) == 0x7f800000u; }

__global__ __launch_bounds__(GC_THREADS) void gc_pack_kernel(GcPlan P, uint32_t* __restrict__ res,
                                                             const uint32_t* __restrict__ scratch,
                                                             uint32_t* __restrict__ packet, uint32_t k) {
  const uint32_t tau = scratch[GC_ST + 2], need = scratch[GC_ST + 3];
  uint32_t run_gt = scratch[GC_ROWS + 2 * blockIdx.x], run_eq = scratch[GC_ROWS + 2 * blockIdx.x + 1];
  __shared__ uint32_t wsum[2][GC_THREADS / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int par = 0;
  gc_for_row(P, blockIdx.x, [&](long i0, int cnt, bool vec) {
    uint32_t x[4];
    gc_load(res, i0, cnt, vec, x);
    const uint32_t v = gc_classify(x, cnt, tau);  // a pass holds at most 1024 elements: both halves stay below 2^16
    uint32_t inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t t = __shfl_up(inc, o, 64);
      if (lane >= o) inc += t;
    }
    if (lane == 63) wsum[par][wave] = inc;
    __syncthreads();  // (the other parity's totals are rewritten only behind the next pass's barrier)
    uint32_t base = 0u, total = 0u;
#pragma unroll
    for (int w = 0; w < GC_THREADS / 64; ++w) {
      const uint32_t t = wsum[par][w];
      if (w < wave) base += t;
      total += t;
    }
    par ^= 1;
    const uint32_t ex = base + inc - v;
    uint32_t my_gt = run_gt + (ex & 0xffffu), my_eq = run_eq + (ex >> 16);
    bool changed = false;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (e < cnt) {
        const uint32_t key = x[e] & 0x7fffffffu;
        const bool gt = key > tau, eq = key == tau;
        const bool sel = gt || (eq && my_eq < need);
        if (sel) {
          const uint32_t pos = my_gt + (my_eq < need ? my_eq : need);
          if (pos < k) {  // (always, with the counts the launches before this one left)
            packet[pos] = (uint32_t)(i0 + e);
            packet[k + pos] = x[e];
          }
        }
        if ((sel || gc_nonfinite(x[e])) && x[e] != 0u) { x[e] = 0u; changed = true; }
        my_gt += gt ? 1u : 0u;
        my_eq += eq ? 1u : 0u;
      }
    }
    if (changed) gc_store(res, i0, cnt, vec, x);
    run_gt += total & 0xffffu;
    run_eq += total >> 16;
  });
}

__global__ __launch_bounds__(GC_THREADS) void gc_scatter_add_kernel(float* __restrict__ g, uint32_t n,
                                                                    const uint32_t* __restrict__ packet, uint32_t k) {
  const uint32_t j = blockIdx.x * (uint32_t)GC_THREADS + threadIdx.x;
  if (j >= k) return;
  const uint32_t i = packet[j];
  if (i < n) g[i] = __fadd_rn(g[i], __uint_as_float(packet[k + j]));
}

}  // namespace dtm
using namespace dtm;

DTM_API int dtm_gc_chunk_size() { return GC_CHUNK; }

// uint32 words of scratch that a bucket of n elements needs; -2: n outside [1, 2^31)
DTM_API long dtm_gc_scratch_words(long n) {
  if (n < 1 || n >= (1L << 31)) return -2;
  return GC_ROWS + 2 * (n / GC_CHUNK + 2);
}

static int gc_check(long n, long k) {
  if (n < 1 || n >= (1L << 31)) return -2;
  if (k < 1 || k > n) return -3;
  return 0;
}

static const int GC_SHIFT[3] = {20, 10, 0}, GC_DBITS[3] = {11, 10, 10};

// res, g: n fp32 elements each, not overlapping; packet: int32[2k]; scratch: dtm_gc_scratch_words(n) words.
// Returns -1 for a null or misaligned pointer, -2 for n outside [1, 2^31), -3 for k outside [1, n]; then nothing is
// launched.  ``stages``: the launches to issue, a bit each (1 init + select, 2 count + rowscan, 4 pack): 7 is the
// function, the others are for tools/compress_bench.py to time the parts.
DTM_API int dtm_grad_compress_stages(void* res, void* g, long n, long k, void* packet, void* scratch, int stages,
                                     void* stream) {
  const int rc = gc_check(n, k);
  if (rc != 0) return rc;
  if (!res || !g || !packet || !scratch || ((uintptr_t)res & 3) || ((uintptr_t)g & 3) || ((uintptr_t)packet & 3) ||
      ((uintptr_t)scratch & 7))
    return -1;
  const GcPlan P = gc_plan(res, g, n);
  hipStream_t st = (hipStream_t)stream;
  uint32_t* r32 = (uint32_t*)res;
  const uint32_t* g32 = (const uint32_t*)g;
  uint32_t* sc = (uint32_t*)scratch;
  const dim3 grid((unsigned)P.rows), one(1), block(GC_THREADS);
  if (stages & 1) {
    hipLaunchKernelGGL(gc_init_kernel, one, block, 0, st, sc, (uint32_t)(n - k + 1));
    for (int d = 0; d < 3; ++d) {
      const int sh = GC_SHIFT[d], nb = GC_DBITS[d];
      if (d == 0) hipLaunchKernelGGL(gc_hist_kernel<true>, grid, block, 0, st, P, r32, g32, sc, sh, nb);
      else hipLaunchKernelGGL(gc_hist_kernel<false>, grid, block, 0, st, P, r32, g32, sc, sh, nb);
      hipLaunchKernelGGL(gc_scan_kernel, one, block, 0, st, sc, GC_DBITS[d], d == 2 ? 1 : 0);
    }
  }
  if (stages & 2) {
    hipLaunchKernelGGL(gc_count_kernel, grid, block, 0, st, P, (const uint32_t*)r32, sc);
    hipLaunchKernelGGL(gc_rowscan_kernel, one, block, 0, st, sc, P.rows, (uint32_t)k);
  }
  if (stages & 4)
    hipLaunchKernelGGL(gc_pack_kernel, grid, block, 0, st, P, r32, (const uint32_t*)sc, (uint32_t*)packet, (uint32_t)k);
  return 0;
}

DTM_API int dtm_grad_compress(void* res, void* g, long n, long k, void* packet, void* scratch, void* stream) {
  return dtm_grad_compress_stages(res, g, n, k, packet, scratch, 7, stream);
}

// g: n fp32 elements; packets: int32[W][2k], source ranks in order.  Same return codes as dtm_grad_compress, and -1
// for W < 1.  An index outside [0, n) is skipped.
DTM_API int dtm_grad_decompress(void* g, long n, const void* packets, int W, long k, void* stream) {
  const int rc = gc_check(n, k);
  if (rc != 0) return rc;
  if (!g || !packets || W < 1 || ((uintptr_t)g & 3) || ((uintptr_t)packets & 3)) return -1;
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(g, 0, (size_t)n * 4, st) != hipSuccess) return -4;
  const dim3 grid((unsigned)((k + GC_THREADS - 1) / GC_THREADS)), block(GC_THREADS);
  for (int w = 0; w < W; ++w)
    hipLaunchKernelGGL(gc_scatter_add_kernel, grid, block, 0, st, (float*)g, (uint32_t)n,
                       (const uint32_t*)packets + (size_t)w * 2 * (size_t)k, (uint32_t)k);
  return 0;
}
