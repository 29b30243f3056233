// Gradient accumulation over a range of the flat fp32 gradient buffer (parallel/bsp.py): ``g`` is the range the
// backward of one micro-batch wrote, ``acc`` the same range of the accumulator.
//   mode 0 STORE  acc = g;        g = 0     after the backward of micro-batch 0 (a bit copy: a NaN keeps its payload)
//   mode 1 ADD    acc = acc + g;  g = 0     after the backward of micro-batches 1 .. N-2
//   mode 2 FOLD   g = acc + g               micro-batch N-1, before the range's all-reduce
// The clear of modes 0 and 1 is the next micro-batch's zero-grad: no memset runs between micro-batches.
// ``flag`` (may be null): set to 1 when an element of the incoming g is Inf or NaN (exponent bits all ones), with
// one atomicOr per wave that saw one, as check_finite_kernel does; never cleared here.
//
// Memory-bound: 12, 16 and 12 bytes move per element. A range may start at any element: where acc and g reach a
// 16-byte boundary together (the same offset into two equally laid out buffers) the body moves 16 bytes per lane
// and block 0 does the up-to-3-element head and tail; otherwise every access is a coalesced 4-byte one.
#include "common.h"

namespace dtm {

enum { GA_STORE = 0, GA_ADD = 1, GA_FOLD = 2 };

__device__ __forceinline__ bool ga_nonfinite(uint32_t b) { return (b & 0x7f800000u) == 0x7f800000u; }

// one element; returns the new acc (STORE, ADD) or the new g (FOLD)
template <int MODE>
__device__ __forceinline__ uint32_t ga_combine(uint32_t a, uint32_t g) {
  if constexpr (MODE == GA_STORE) return g;
  else return __float_as_uint(__fadd_rn(__uint_as_float(a), __uint_as_float(g)));
}

template <int MODE>
__device__ __forceinline__ bool ga_scalar(uint32_t* __restrict__ acc, uint32_t* __restrict__ g, long i) {
  const uint32_t gv = g[i];
  const uint32_t r = ga_combine<MODE>(MODE == GA_STORE ? 0u : acc[i], gv);
  if constexpr (MODE == GA_FOLD) g[i] = r;
  else { acc[i] = r; g[i] = 0u; }
  return ga_nonfinite(gv);
}

// four elements from the loaded a (acc) and x (g): stores the result, returns "x held an Inf or a NaN"
template <int MODE>
__device__ __forceinline__ bool ga_vec(uint4* __restrict__ av, uint4* __restrict__ gv, long i, uint4 a, uint4 x) {
  uint4 r;
  r.x = ga_combine<MODE>(a.x, x.x);
  r.y = ga_combine<MODE>(a.y, x.y);
  r.z = ga_combine<MODE>(a.z, x.z);
  r.w = ga_combine<MODE>(a.w, x.w);
  if constexpr (MODE == GA_FOLD) gv[i] = r;
  else { av[i] = r; gv[i] = make_uint4(0u, 0u, 0u, 0u); }
  return ga_nonfinite(x.x) | ga_nonfinite(x.y) | ga_nonfinite(x.z) | ga_nonfinite(x.w);
}

// head: elements in front of the first 16-byte boundary (vector path), or -1: 4-byte accesses throughout
template <int MODE>
__global__ __launch_bounds__(256) void grad_accum_kernel(uint32_t* __restrict__ acc, uint32_t* __restrict__ g, long n,
                                                         int head, int* __restrict__ flag) {
  const long tid = blockIdx.x * 256L + threadIdx.x, nthr = gridDim.x * 256L;
  bool bad = false;
  if (head < 0) {
    for (long i = tid; i < n; i += nthr) bad |= ga_scalar<MODE>(acc, g, i);
  } else {
    const long nvec = (n - head) >> 2;
    uint4* __restrict__ av = reinterpret_cast<uint4*>(acc + head);
    uint4* __restrict__ gv = reinterpret_cast<uint4*>(g + head);
    // (several vectors per lane and trip, or more blocks per CU, measured within 3 % of this loop)
    for (long i = tid; i < nvec; i += nthr) {
      uint4 a = make_uint4(0u, 0u, 0u, 0u);
      if constexpr (MODE != GA_STORE) a = av[i];
      bad |= ga_vec<MODE>(av, gv, i, a, gv[i]);
    }
    if (blockIdx.x == 0) {
      const long tail0 = head + (nvec << 2);
      if ((int)threadIdx.x < head) bad |= ga_scalar<MODE>(acc, g, threadIdx.x);
      if (tail0 + threadIdx.x < n) bad |= ga_scalar<MODE>(acc, g, tail0 + threadIdx.x);
    }
  }
  if (flag != nullptr && __any(bad) && (threadIdx.x & 63) == 0) atomicOr(flag, 1);
}

}  // namespace dtm
using namespace dtm;

// acc, g: n fp32 elements each, not overlapping; flag: device int32 or null.  Nothing is allocated or read back, so
// the launch can be captured into a hipGraph.  Returns -1 for a bad argument.
DTM_API int dtm_grad_accum(void* acc, void* g, long n, int mode, int* flag, void* stream) {
  if (n < 0 || mode < GA_STORE || mode > GA_FOLD) return -1;
  if (n == 0) return 0;
  const uintptr_t pa = (uintptr_t)acc, pg = (uintptr_t)g;
  if (!acc || !g || (pa & 3) || (pg & 3)) return -1;
  int head = -1;
  long work = n;
  if ((pa & 15) == (pg & 15)) {
    head = (int)(((16 - (pg & 15)) & 15) >> 2);
    if (head > n) head = (int)n;
    work = (n - head) >> 2;
  }
  long b = (work + 255) / 256;
  const long cap = 8L * dtm_compute_cus();
  if (b > cap) b = cap;
  if (b < 1) b = 1;
  const dim3 grid((unsigned)b), block(256);
  uint32_t* a32 = (uint32_t*)acc;
  uint32_t* g32 = (uint32_t*)g;
  hipStream_t st = (hipStream_t)stream;
  if (mode == GA_STORE) hipLaunchKernelGGL(grad_accum_kernel<GA_STORE>, grid, block, 0, st, a32, g32, n, head, flag);
  else if (mode == GA_ADD) hipLaunchKernelGGL(grad_accum_kernel<GA_ADD>, grid, block, 0, st, a32, g32, n, head, flag);
  else hipLaunchKernelGGL(grad_accum_kernel<GA_FOLD>, grid, block, 0, st, a32, g32, n, head, flag);
  return 0;
}
