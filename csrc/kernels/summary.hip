// Multi-tensor summary statistics: TensorBoard histograms (TensorFlow's histogram::Histogram with its default
// bucket limits), min / max / sum / sum of squares, the zero count (tf.nn.zero_fraction) and the non-finite
// count of MANY tensors in two launches (reference cnn/cifar10.py:104-121,375-381: one tf.summary.histogram per
// variable, gradient and end point).
//
// Semantics (per element x of a row with scale s): v = float(x) * s, one fp32 multiply.  A non-finite v is only
// counted; a finite v enters num, min, max, sum, sum_squares (fp64) and the bucket whose index is the first
// limit strictly greater than v (upper_bound on the 1551-entry fp64 table; +-0 -> bucket 776).
//
// tensor_stats_kernel: one 256-thread block per (tensor, chunk) row of a host-built chunk table.  The block keeps
//   the fp64 limits and a uint32 histogram in LDS (LDS integer atomics), reduces its per-thread fp64 partial sums
//   through LDS in a fixed order, adds its non-zero bins to the tensor's global bins with INTEGER atomics (their
//   sum does not depend on the arrival order) and writes one partial record with plain stores.
// tensor_stats_finalize_kernel: one block per tensor sums that tensor's partial records in chunk order.
// No float atomics, no flags, no waiting between blocks: the kernel boundary is the only synchronisation, so every
// output is bit-identical from run to run (independent of dtm_set_deterministic).
#include <float.h>

#include "chunk_walk.h"

namespace dtm {

constexpr int STATS_BUCKETS = 1551;  // 774 negated limits + DBL_MAX twice, and 0.0
constexpr int STATS_POS = 775;       // positive limits incl. DBL_MAX
constexpr int STATS_CHUNK = 32768;   // elements per block

struct StatsTensor {
  const void* x;
  unsigned long long n;  // < 2^32
  float scale;
  int bf16;              // 0: fp32 row, 1: bf16 row
  unsigned chunk0;       // this tensor's first row in the chunk table / the partial records
  unsigned nchunks;
};
struct StatsPartial {  // one per chunk
  double sum, sumsq;
  float mn, mx;
  unsigned zeros, nonfinite;
};
struct StatsResult {  // one per tensor
  double sum, sumsq;
  float mn, mx;
  unsigned long long num, zeros, nonfinite;
};

struct StatsAcc {
  double sum, sumsq;
  float mn, mx;
  unsigned zeros, nonfinite;
};

// first index b with lim[b] > v (v finite).  The first guess comes from log2|v| (the limits are 1e-12 * 1.1^j);
// the two loops correct it against the fp64 table, so the result is the exact upper_bound whatever the guess.
__device__ __forceinline__ int stats_bucket(const double* lim, float v) {
  const float a = fabsf(v);
  int b = 776;
  if (a > 0.f) {
    // j ~ log(a / 1e-12) / log(1.1): log2(1e-12) = -39.8631371, 1 / log2(1.1) = 7.27254090
    float g = floorf((__log2f(a) + 39.8631371f) * 7.27254090f) + 1.f;
    g = fminf(fmaxf(g, 0.f), (float)(STATS_POS - 1));  // (fmaxf first: -inf / NaN guesses become 0)
    b = v > 0.f ? 776 + (int)g : 775 - (int)g;
  }
  const double d = (double)v;
  while (b > 0 && lim[b - 1] > d) --b;
  while (b < STATS_BUCKETS - 1 && lim[b] <= d) ++b;
  return b;
}

__device__ __forceinline__ void stats_add(StatsAcc& a, unsigned* hist, const double* lim, float x, float scale) {
  const float v = x * scale;
  if (!(fabsf(v) <= FLT_MAX)) {  // NaN, +-Inf: counted only
    ++a.nonfinite;
    return;
  }
  const double d = (double)v;
  a.sum += d;
  a.sumsq += d * d;
  a.mn = fminf(a.mn, v);
  a.mx = fmaxf(a.mx, v);
  a.zeros += v == 0.f;
  atomicAdd(&hist[stats_bucket(lim, v)], 1u);
}

__global__ __launch_bounds__(256) void tensor_stats_kernel(const StatsTensor* __restrict__ tens,
                                                           const ChunkRow* __restrict__ chunks,
                                                           const double* __restrict__ limits,
                                                           unsigned* __restrict__ bins,
                                                           StatsPartial* __restrict__ partials) {
  __shared__ double lim[STATS_BUCKETS];
  __shared__ unsigned hist[STATS_BUCKETS];
  __shared__ double rs[256], rq[256];
  __shared__ float rmn[256], rmx[256];
  __shared__ unsigned rz[256], rnf[256];
  const int tid = threadIdx.x;
  const ChunkRow c = chunks[blockIdx.x];
  const StatsTensor t = tens[c.t];
  for (int i = tid; i < STATS_BUCKETS; i += 256) {
    lim[i] = limits[i];
    hist[i] = 0u;
  }
  __syncthreads();

  const int len = chunk_len((long)t.n, c.start, STATS_CHUNK);  // >= 1 (host-built table)
  StatsAcc a = {0.0, 0.0, INFINITY, -INFINITY, 0u, 0u};
  // 16-byte loads over the aligned body; a scalar head up to the first 16-byte boundary and a scalar tail
  // (tensors are slices of flat buffers: a chunk can start at any element)
  auto add = [&](int, float x) { stats_add(a, hist, lim, x, t.scale); };
  if (t.bf16) visit_row<256>((const bf16_t*)t.x + c.start, len, tid, add);
  else visit_row<256>((const float*)t.x + c.start, len, tid, add);

  // fixed-order tree over the 256 per-thread partials
  rs[tid] = a.sum; rq[tid] = a.sumsq; rmn[tid] = a.mn; rmx[tid] = a.mx; rz[tid] = a.zeros; rnf[tid] = a.nonfinite;
  __syncthreads();
  for (int h = 128; h >= 1; h >>= 1) {
    if (tid < h) {
      rs[tid] += rs[tid + h];
      rq[tid] += rq[tid + h];
      rmn[tid] = fminf(rmn[tid], rmn[tid + h]);
      rmx[tid] = fmaxf(rmx[tid], rmx[tid + h]);
      rz[tid] += rz[tid + h];
      rnf[tid] += rnf[tid + h];
    }
    __syncthreads();
  }
  if (tid == 0) {
    StatsPartial p;
    p.sum = rs[0]; p.sumsq = rq[0]; p.mn = rmn[0]; p.mx = rmx[0]; p.zeros = rz[0]; p.nonfinite = rnf[0];
    partials[blockIdx.x] = p;
  }
  unsigned* gb = bins + (size_t)c.t * STATS_BUCKETS;
  for (int i = tid; i < STATS_BUCKETS; i += 256) {
    const unsigned h = hist[i];
    if (h) atomicAdd(&gb[i], h);
  }
}

__global__ __launch_bounds__(256) void tensor_stats_finalize_kernel(const StatsTensor* __restrict__ tens,
                                                                    const StatsPartial* __restrict__ partials,
                                                                    StatsResult* __restrict__ results) {
  __shared__ StatsPartial stage[256];
  const StatsTensor t = tens[blockIdx.x];
  const StatsPartial* p = partials + t.chunk0;
  double sum = 0.0, sumsq = 0.0;
  float mn = INFINITY, mx = -INFINITY;
  unsigned long long zeros = 0, nonfinite = 0;
  for (unsigned base = 0; base < t.nchunks; base += 256) {
    const unsigned cnt = t.nchunks - base < 256u ? t.nchunks - base : 256u;
    __syncthreads();
    if (threadIdx.x < cnt) stage[threadIdx.x] = p[base + threadIdx.x];
    __syncthreads();
    if (threadIdx.x == 0) {  // chunk order
      for (unsigned j = 0; j < cnt; ++j) {
        sum += stage[j].sum;
        sumsq += stage[j].sumsq;
        mn = fminf(mn, stage[j].mn);
        mx = fmaxf(mx, stage[j].mx);
        zeros += stage[j].zeros;
        nonfinite += stage[j].nonfinite;
      }
    }
  }
  if (threadIdx.x == 0) {
    StatsResult r;
    r.sum = sum; r.sumsq = sumsq; r.mn = mn; r.mx = mx;
    r.num = t.n - nonfinite; r.zeros = zeros; r.nonfinite = nonfinite;
    results[blockIdx.x] = r;
  }
}

// TensorFlow's default histogram limits (tensorflow/core/lib/histogram/histogram.cc InitDefaultBucketsInner):
// repeated multiplication, NOT pow - the two differ in the last bits.
static const double* stats_host_limits() {
  static double tab[STATS_BUCKETS];
  static bool init = false;
  if (!init) {
    double pos[STATS_POS];
    int n = 0;
    for (double v = 1e-12; v < 1e20; v *= 1.1) pos[n++] = v;  // 774 values
    pos[n++] = DBL_MAX;
    for (int i = 0; i < STATS_POS; ++i) {
      tab[i] = -pos[STATS_POS - 1 - i];
      tab[STATS_POS + 1 + i] = pos[i];
    }
    tab[STATS_POS] = 0.0;
    init = true;
  }
  return tab;
}

}  // namespace dtm

using namespace dtm;

DTM_API int dtm_stats_tensor_bytes() { return (int)sizeof(StatsTensor); }
DTM_API int dtm_stats_chunk_bytes() { return (int)sizeof(ChunkRow); }
DTM_API int dtm_stats_partial_bytes() { return (int)sizeof(StatsPartial); }
DTM_API int dtm_stats_result_bytes() { return (int)sizeof(StatsResult); }
DTM_API int dtm_stats_chunk_size() { return STATS_CHUNK; }
DTM_API int dtm_stats_num_buckets() { return STATS_BUCKETS; }
DTM_API void dtm_stats_limits(double* out) {
  const double* t = stats_host_limits();
  for (int i = 0; i < STATS_BUCKETS; ++i) out[i] = t[i];
}

// bins [ntens][1551] uint32 (zeroed here), partials [nchunks] StatsPartial, results [ntens] StatsResult.
// Not capturable (the limit table is uploaded on the first call): -10 on a capturing stream.
// The device copy of the limits is one per process: like the rest of the library this entry point serves the first
// device used only (dtm_device_ok, -9 from any other), and it is called from one host thread at a time.  The upload
// needs no host synchronisation: it is enqueued on the first caller's stream from a static host table, and every
// call makes its stream wait for the upload's event (a no-op once it has completed).
DTM_API int dtm_tensor_stats(const void* tens, const void* chunks, int nchunks, int ntens, void* bins, void* partials,
                             void* results, void* stream) {
  if (!dtm_device_ok()) return -9;
  hipStream_t st = (hipStream_t)stream;
  if (nchunks <= 0 || ntens <= 0) return -1;
  if (dtm_stream_capturing(st)) return -10;
  static double* d_limits = nullptr;  // 12 KB, kept for the life of the process
  static hipEvent_t uploaded = nullptr;
  if (!d_limits) {
    double* d = nullptr;
    hipEvent_t ev = nullptr;
    if (hipMalloc(&d, sizeof(double) * STATS_BUCKETS) != hipSuccess) return -4;
    if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess ||
        hipMemcpyAsync(d, stats_host_limits(), sizeof(double) * STATS_BUCKETS, hipMemcpyHostToDevice, st) !=
            hipSuccess ||
        hipEventRecord(ev, st) != hipSuccess) {
      if (ev) (void)hipEventDestroy(ev);
      (void)hipFree(d);
      return -4;
    }
    d_limits = d;
    uploaded = ev;
  }
  if (hipStreamWaitEvent(st, uploaded, 0) != hipSuccess) return -2;
  if (hipMemsetAsync(bins, 0, sizeof(unsigned) * (size_t)STATS_BUCKETS * ntens, st) != hipSuccess) return -2;
  hipLaunchKernelGGL(tensor_stats_kernel, dim3(nchunks), dim3(256), 0, st, (const StatsTensor*)tens,
                     (const ChunkRow*)chunks, d_limits, (unsigned*)bins, (StatsPartial*)partials);
  hipLaunchKernelGGL(tensor_stats_finalize_kernel, dim3(ntens), dim3(256), 0, st, (const StatsTensor*)tens,
                     (const StatsPartial*)partials, (StatsResult*)results);
  return (int)hipGetLastError();
}
