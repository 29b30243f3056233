// Channel LayerNorm and layer scale + residual on rows of C contiguous channels, bf16 or fp32 storage, fp32 math.
// The rows are the M = numel / C runs of C channels of a contiguous tensor [..., C]: NHWC pixels and [N, L, C] tokens
// are the same thing here.  Eligible: C % 8 == 0, 8 <= C <= 2048, 1 <= M < 2^31.
//   cln_fwd             y = (x - mean_r) * rstd_r * gamma + beta,  rstd = 1 / sqrt(var + eps), biased variance
//   cln_bwd             g = dy * gamma, xh = (x - mean) * rstd:  dx = rstd * (g - mean_c(g) - xh * mean_c(g * xh)),
//                       dbeta_c = sum_r dy, dgamma_c = sum_r dy * xh
//   scale_residual_fwd  y = x + (s[n] * gamma[c]) * r  (ConvNeXt's layer scale; s: stochastic depth's sample factor)
//   scale_residual_bwd  dr = (s * gamma) * dy,  dgamma_c = sum_r s * dy * r   (dx = dy needs no kernel)
//
// Work split (all four kernels): a row belongs to a group of G lanes of one wave, G the smallest power of two for
// which a lane holds at most V = ceil(C/8 / G) <= 4 vectors of 16 bytes (C = 96: G = 4, V = 3; C = 2048: G = 64,
// V = 4).  Lane j of the group owns the vectors j, j + G, j + 2G, ... of the row, so a group's loads are consecutive
// 16-byte pieces; a wave works on 64 / G rows at a time and a block of 256 lanes on RT = 256 / G consecutive rows per
// trip, walking a contiguous slab of slab_rows rows.  A lane's columns are the same for every row it meets: gamma and
// beta are read once, and the backward kernels keep their per-column sums in registers.
//
// Row statistics: x is read once and stays in registers; the mean is a xor-shuffle butterfly over the group's lanes
// (offsets 1, 2, ..., G/2), the variance the sum of squared centred values from the registers, in a second butterfly
// that also carries the centred values' own sum: the rounding that the first mean leaves (a row at 100 +- 1) corrects
// the mean, the centred values and the squares.  Never E[x^2] - mean^2 of the raw values.  No LDS in the forward.
// Column sums: every lane adds its own columns in row order; at the end of the slab the 256 / G lanes of the block
// that own the same columns meet in LDS by col_tree8's fixed tree and the block writes one fp32 record [sets][C];
// col_records_sum adds the records of each column in record order (16 runs of consecutive records, then the run sums
// in run order).  No atomics, no flags, no waiting between blocks: run to run the bits are the same.
#include "nhwc8.h"

// Products and sums are fused only where fmaf says so: the bits do not depend on the compiler's contraction choices.
#pragma clang fp contract(off)

namespace dtm {
namespace {

constexpr int CLN_T = 256;  // lanes per block

struct ClnGeom {
  int M, C, C8;
  int G, lg;  // lanes per row and log2
  int V;      // vectors per lane
  int RT;     // rows per trip of a block
  int SL;     // rows per slab (block)
  int blocks;
};

__device__ __forceinline__ float group_sum(float v, int G) {
  for (int o = 1; o < G; o <<= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ void group_sum2(float& a, float& b, int G) {
  for (int o = 1; o < G; o <<= 1) {
    a += __shfl_xor(a, o, 64);
    b += __shfl_xor(b, o, 64);
  }
}

// The lane's place: vector j + k * G of the row (k < V; live[k]: inside the row), row lane rl of the trip.
template <int V>
struct ClnLane {
  int j, rl;
  bool live[V];
  int c[V];  // first channel of vector k
};
template <int V>
__device__ __forceinline__ ClnLane<V> make_lane(const ClnGeom& g) {
  ClnLane<V> l;
  l.j = threadIdx.x & (g.G - 1);
  l.rl = threadIdx.x >> g.lg;
#pragma unroll
  for (int k = 0; k < V; ++k) {
    const int vec = l.j + k * g.G;
    l.live[k] = vec < g.C8;
    l.c[k] = vec * 8;
  }
  return l;
}

template <int V>
__device__ __forceinline__ void load_param(const float* p, const ClnLane<V>& l, float fill, float (&out)[V][8]) {
#pragma unroll
  for (int k = 0; k < V; ++k)
#pragma unroll
    for (int e = 0; e < 8; ++e) out[k][e] = (p && l.live[k]) ? p[l.c[k] + e] : fill;
}

template <bool BF16, int V>
__device__ __forceinline__ void load_row(const void* p, size_t base, bool rlive, const ClnLane<V>& l,
                                         float (&v)[V][8]) {
#pragma unroll
  for (int k = 0; k < V; ++k) {
    if (rlive && l.live[k]) {
      ld8<BF16>(p, base + l.c[k], v[k]);
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) v[k][e] = 0.f;
    }
  }
}

template <bool BF16, int V>
__device__ __forceinline__ void store_row(void* p, size_t base, bool rlive, const ClnLane<V>& l,
                                          const float (&v)[V][8]) {
#pragma unroll
  for (int k = 0; k < V; ++k)
    if (rlive && l.live[k]) st8<BF16>(p, base + l.c[k], v[k]);
}

// the lanes that own the same columns meet in LDS; lane j of the first group writes the block's record
template <int A, int V>
__device__ __forceinline__ void write_record(float (*red)[CLN_T][8], const float (&s)[V][8], const float (&q)[V][8],
                                             const ClnLane<V>& l, const ClnGeom& g, float* rec0, float* rec1) {
#pragma unroll
  for (int k = 0; k < V; ++k) {
    col_tree8<A, CLN_T>(red, s[k], q[k], g.G);  // 256 / G >= 4 row lanes: the totals are in red
    if (threadIdx.x < g.G && l.live[k]) {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        rec0[l.c[k] + e] = red[0][threadIdx.x][e];
        if (A == 2) rec1[l.c[k] + e] = red[1][threadIdx.x][e];
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------------------
template <bool BF16, int V>
__global__ __launch_bounds__(CLN_T) void cln_fwd_kernel(const void* __restrict__ x, const float* __restrict__ gamma,
                                                        const float* __restrict__ beta, void* __restrict__ y,
                                                        float* __restrict__ stats, ClnGeom g, float eps) {
  const ClnLane<V> l = make_lane<V>(g);
  float ga[V][8], be[V][8];
  load_param<V>(gamma, l, 1.f, ga);
  load_param<V>(beta, l, 0.f, be);
  const long r0 = (long)blockIdx.x * g.SL;
  const long r1 = r0 + g.SL < (long)g.M ? r0 + g.SL : (long)g.M;
  const float inv = 1.f / (float)g.C;
  for (long rb = r0; rb < r1; rb += g.RT) {  // the same trips for every lane of the block
    const long row = rb + l.rl;
    const bool rlive = row < r1;
    const size_t base = (size_t)row * g.C;
    float v[V][8];
    load_row<BF16, V>(x, base, rlive, l, v);
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < V; ++k)
#pragma unroll
      for (int e = 0; e < 8; ++e) s += v[k][e];
    const float mean0 = group_sum(s, g.G) * inv;
    // the centred values and their squares share one butterfly: what the rounded mean0 leaves of the sum corrects the
    // mean, the centred values and the sum of squares (the corrected two-pass form of Chan, Golub & LeVeque 1983)
    float t = 0.f, q = 0.f;
#pragma unroll
    for (int k = 0; k < V; ++k)
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        v[k][e] -= mean0;
        if (l.live[k]) {  // an idle vector slot is not part of the row
          t += v[k][e];
          q = fmaf(v[k][e], v[k][e], q);
        }
      }
    group_sum2(t, q, g.G);
    const float dm = t * inv;
    const float mean = mean0 + dm;
    const float rstd = rsqrtf(fmaxf(q * inv - dm * dm, 0.f) + eps);
#pragma unroll
    for (int k = 0; k < V; ++k)
#pragma unroll
      for (int e = 0; e < 8; ++e) v[k][e] = fmaf((v[k][e] - dm) * rstd, ga[k][e], be[k][e]);
    store_row<BF16, V>(y, base, rlive, l, v);
    if (rlive && l.j == 0) {
      stats[2 * row] = mean;
      stats[2 * row + 1] = rstd;
    }
  }
}

// rec: [blocks][2][C] (sum dy, sum dy * xh); want: dgamma or dbeta is asked for
template <bool BF16, int V>
__global__ __launch_bounds__(CLN_T) void cln_bwd_kernel(const void* __restrict__ x, const void* __restrict__ dy,
                                                        const float* __restrict__ gamma,
                                                        const float* __restrict__ stats, void* __restrict__ dx,
                                                        float* __restrict__ rec, ClnGeom g, int want) {
  __shared__ float red[2][CLN_T][8];
  const ClnLane<V> l = make_lane<V>(g);
  float ga[V][8];
  load_param<V>(gamma, l, 1.f, ga);
  float pb[V][8], pg[V][8];
#pragma unroll
  for (int k = 0; k < V; ++k)
#pragma unroll
    for (int e = 0; e < 8; ++e) pb[k][e] = pg[k][e] = 0.f;
  const long r0 = (long)blockIdx.x * g.SL;
  const long r1 = r0 + g.SL < (long)g.M ? r0 + g.SL : (long)g.M;
  const float inv = 1.f / (float)g.C;
  for (long rb = r0; rb < r1; rb += g.RT) {
    const long row = rb + l.rl;
    const bool rlive = row < r1;
    const size_t base = (size_t)row * g.C;
    float v[V][8], d[V][8];
    load_row<BF16, V>(x, base, rlive, l, v);
    load_row<BF16, V>(dy, base, rlive, l, d);
    const float mean = rlive ? stats[2 * row] : 0.f, rstd = rlive ? stats[2 * row + 1] : 0.f;
    // a row past the slab and an idle vector slot hold dy = 0: they add nothing to the row or the column sums
    float a = 0.f, b = 0.f;
#pragma unroll
    for (int k = 0; k < V; ++k)
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float xh = (v[k][e] - mean) * rstd;
        v[k][e] = xh;
        pb[k][e] += d[k][e];
        pg[k][e] = fmaf(d[k][e], xh, pg[k][e]);
        d[k][e] *= ga[k][e];
        a += d[k][e];
        b = fmaf(d[k][e], xh, b);
      }
    group_sum2(a, b, g.G);
    a *= inv;
    b *= inv;
#pragma unroll
    for (int k = 0; k < V; ++k)
#pragma unroll
      for (int e = 0; e < 8; ++e) v[k][e] = rstd * (d[k][e] - a - v[k][e] * b);
    store_row<BF16, V>(dx, base, rlive, l, v);
  }
  if (want) {
    float* r = rec + (size_t)blockIdx.x * 2 * g.C;
    write_record<2, V>(red, pb, pg, l, g, r, r + g.C);
  }
}

// out_s[c] = sum over the records of rec[b][s][c], in record order: a block owns CRS_COLS (set, column) pairs, the
// records are cut into CRS_RUNS runs of consecutive records, a lane adds one run of one column in record order, and
// the run sums of a column are added in run order (one thread walking a column's records alone is a chain of a
// thousand dependent loads)
constexpr int CRS_COLS = 16, CRS_RUNS = CLN_T / CRS_COLS;
__global__ __launch_bounds__(CLN_T) void col_records_sum_kernel(const float* __restrict__ rec, int nrec, int C,
                                                                int sets, float* __restrict__ out0,
                                                                float* __restrict__ out1) {
  __shared__ float part[CRS_RUNS][CRS_COLS];
  const int col = threadIdx.x % CRS_COLS, run = threadIdx.x / CRS_COLS;
  const int t = blockIdx.x * CRS_COLS + col;
  const bool live = t < sets * C;
  const size_t ld = (size_t)sets * C;
  const int len = (nrec + CRS_RUNS - 1) / CRS_RUNS;
  const int b1 = min(nrec, (run + 1) * len);
  float s = 0.f;
  if (live) {
    int b = run * len;
    for (; b + 8 <= b1; b += 8) {
      float w[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) w[u] = rec[(size_t)(b + u) * ld + t];
#pragma unroll
      for (int u = 0; u < 8; ++u) s += w[u];
    }
    for (; b < b1; ++b) s += rec[(size_t)b * ld + t];
  }
  part[run][col] = s;
  __syncthreads();
  if (run == 0 && live) {
    s = part[0][col];
    for (int q = 1; q < CRS_RUNS; ++q) s += part[q][col];
    float* out = t < C ? out0 : out1;
    if (out) out[t < C ? t : t - C] = s;
  }
}

// ------------------------------------------------------------------------------------------------------------
// s: [ns] per-sample factor or null; sample of a row = row / rps
template <bool BF16, int V>
__global__ __launch_bounds__(CLN_T) void scale_residual_fwd_kernel(const void* __restrict__ x,
                                                                   const void* __restrict__ r,
                                                                   const float* __restrict__ gamma,
                                                                   const float* __restrict__ s, void* __restrict__ y,
                                                                   ClnGeom g, int rps) {
  const ClnLane<V> l = make_lane<V>(g);
  float ga[V][8];
  load_param<V>(gamma, l, 1.f, ga);
  const long r0 = (long)blockIdx.x * g.SL;
  const long r1 = r0 + g.SL < (long)g.M ? r0 + g.SL : (long)g.M;
  for (long rb = r0; rb < r1; rb += g.RT) {
    const long row = rb + l.rl;
    const bool rlive = row < r1;
    const size_t base = (size_t)row * g.C;
    float v[V][8], w[V][8];
    load_row<BF16, V>(x, base, rlive, l, v);
    load_row<BF16, V>(r, base, rlive, l, w);
    const float sc = (s && rlive) ? s[row / rps] : 1.f;
#pragma unroll
    for (int k = 0; k < V; ++k)
#pragma unroll
      for (int e = 0; e < 8; ++e) v[k][e] = fmaf(sc * ga[k][e], w[k][e], v[k][e]);
    store_row<BF16, V>(y, base, rlive, l, v);
  }
}

// rec: [blocks][C] sum s * dy * r
template <bool BF16, int V>
__global__ __launch_bounds__(CLN_T) void scale_residual_bwd_kernel(const void* __restrict__ dy,
                                                                   const void* __restrict__ r,
                                                                   const float* __restrict__ gamma,
                                                                   const float* __restrict__ s, void* __restrict__ dr,
                                                                   float* __restrict__ rec, ClnGeom g, int rps,
                                                                   int want) {
  __shared__ float red[1][CLN_T][8];
  const ClnLane<V> l = make_lane<V>(g);
  float ga[V][8];
  load_param<V>(gamma, l, 1.f, ga);
  float pg[V][8];
#pragma unroll
  for (int k = 0; k < V; ++k)
#pragma unroll
    for (int e = 0; e < 8; ++e) pg[k][e] = 0.f;
  const long r0 = (long)blockIdx.x * g.SL;
  const long r1 = r0 + g.SL < (long)g.M ? r0 + g.SL : (long)g.M;
  for (long rb = r0; rb < r1; rb += g.RT) {
    const long row = rb + l.rl;
    const bool rlive = row < r1;
    const size_t base = (size_t)row * g.C;
    float d[V][8], w[V][8];
    load_row<BF16, V>(dy, base, rlive, l, d);
    load_row<BF16, V>(r, base, rlive, l, w);
    const float sc = (s && rlive) ? s[row / rps] : 1.f;
#pragma unroll
    for (int k = 0; k < V; ++k)
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        pg[k][e] = fmaf(sc * d[k][e], w[k][e], pg[k][e]);  // a row past the slab holds dy = 0
        d[k][e] = (sc * ga[k][e]) * d[k][e];
      }
    store_row<BF16, V>(dr, base, rlive, l, d);
  }
  if (want) write_record<1, V>(red, pg, pg, l, g, rec + (size_t)blockIdx.x * g.C, nullptr);
}

int make_geom(long M, int C, int slab_rows, ClnGeom* g) {
  if (C < 8 || C > 2048 || C % 8) return -1;
  if (M < 1 || M > 0x7fffffffL || slab_rows < 1) return -2;
  g->M = (int)M; g->C = C; g->C8 = C / 8;
  g->G = 1; g->lg = 0;
  while ((g->C8 + g->G - 1) / g->G > 4) { g->G *= 2; ++g->lg; }
  g->V = (g->C8 + g->G - 1) / g->G;
  g->RT = CLN_T / g->G;
  g->SL = slab_rows;
  g->blocks = (int)((M + slab_rows - 1) / slab_rows);
  return 0;
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace
}  // namespace dtm

using namespace dtm;

// K<BF16, V> for the geometry's V and the storage type
#define CLN_LAUNCH(K, g, bf16, st, ...)                                                                           \
  do {                                                                                                            \
    const dim3 grid_((g).blocks), blk_(CLN_T);                                                                    \
    switch ((g).V * 2 + ((bf16) ? 1 : 0)) {                                                                       \
      case 2: hipLaunchKernelGGL((K<false, 1>), grid_, blk_, 0, st, __VA_ARGS__); break;                          \
      case 3: hipLaunchKernelGGL((K<true, 1>), grid_, blk_, 0, st, __VA_ARGS__); break;                           \
      case 4: hipLaunchKernelGGL((K<false, 2>), grid_, blk_, 0, st, __VA_ARGS__); break;                          \
      case 5: hipLaunchKernelGGL((K<true, 2>), grid_, blk_, 0, st, __VA_ARGS__); break;                           \
      case 6: hipLaunchKernelGGL((K<false, 3>), grid_, blk_, 0, st, __VA_ARGS__); break;                          \
      case 7: hipLaunchKernelGGL((K<true, 3>), grid_, blk_, 0, st, __VA_ARGS__); break;                           \
      case 8: hipLaunchKernelGGL((K<false, 4>), grid_, blk_, 0, st, __VA_ARGS__); break;                          \
      default: hipLaunchKernelGGL((K<true, 4>), grid_, blk_, 0, st, __VA_ARGS__); break;                          \
    }                                                                                                             \
  } while (0)

static void records_sum(const float* rec, const ClnGeom& g, int sets, float* out0, float* out1, hipStream_t st) {
  const dim3 grid((sets * g.C + CRS_COLS - 1) / CRS_COLS);
  hipLaunchKernelGGL(col_records_sum_kernel, grid, dim3(CLN_T), 0, st, rec, g.blocks, g.C, sets, out0, out1);
}

// floats of workspace of a backward with `sets` column sums (dtm_cln_bwd: 2, dtm_scale_residual_bwd: 1): one record
// [sets][C] per slab of slab_rows rows; negative for a shape the kernels refuse
DTM_API long dtm_cln_ws_floats(long M, int C, int slab_rows, int sets) {
  ClnGeom g;
  const int rc = make_geom(M, C, slab_rows, &g);
  if (rc) return rc;
  return (long)g.blocks * sets * C;
}

// stats: [M][2] (mean, rstd) for the backward; gamma / beta: fp32 [C] or null.  -1 ineligible C or null / misaligned
// tensor, -2 M or slab_rows out of range, -3 workspace too small; nothing is launched after a negative code.
DTM_API int dtm_cln_fwd(const void* x, const float* gamma, const float* beta, void* y, float* stats, long M, int C,
                        int slab_rows, float eps, int bf16, void* stream) {
  ClnGeom g;
  const int rc = make_geom(M, C, slab_rows, &g);
  if (rc) return rc;
  if (!x || !y || !stats || !aligned16(x) || !aligned16(y)) return -1;
  CLN_LAUNCH(cln_fwd_kernel, g, bf16, (hipStream_t)stream, x, gamma, beta, y, stats, g, eps);
  return 0;
}

// dgamma / dbeta: fp32 [C] or null; ws: dtm_cln_ws_floats(M, C, slab_rows, 2) floats.  Codes as the forward's.
DTM_API int dtm_cln_bwd(const void* x, const void* dy, const float* gamma, const float* stats, void* dx, float* dgamma,
                        float* dbeta, float* ws, long ws_floats, long M, int C, int slab_rows, int bf16,
                        void* stream) {
  ClnGeom g;
  const int rc = make_geom(M, C, slab_rows, &g);
  if (rc) return rc;
  if (!x || !dy || !stats || !dx || !aligned16(x) || !aligned16(dy) || !aligned16(dx)) return -1;
  const int want = dgamma || dbeta;
  if (want && (!ws || ws_floats < (long)g.blocks * 2 * C)) return -3;
  hipStream_t st = (hipStream_t)stream;
  CLN_LAUNCH(cln_bwd_kernel, g, bf16, st, x, dy, gamma, stats, dx, ws, g, want);
  if (want) records_sum(ws, g, 2, dbeta, dgamma, st);
  return 0;
}

// y = x + (s[row / rows_per_sample] * gamma[c]) * r; s: fp32 [ns] or null (then ns and rows_per_sample are unused),
// else ns * rows_per_sample == M.  Codes as above.
DTM_API int dtm_scale_residual_fwd(const void* x, const void* r, const float* gamma, const float* s, void* y, long M,
                                   int C, int ns, int rows_per_sample, int slab_rows, int bf16, void* stream) {
  ClnGeom g;
  const int rc = make_geom(M, C, slab_rows, &g);
  if (rc) return rc;
  if (!x || !r || !gamma || !y || !aligned16(x) || !aligned16(r) || !aligned16(y)) return -1;
  if (s && (ns < 1 || rows_per_sample < 1 || (long)ns * rows_per_sample != M)) return -2;
  const int rps = s ? rows_per_sample : 1;
  CLN_LAUNCH(scale_residual_fwd_kernel, g, bf16, (hipStream_t)stream, x, r, gamma, s, y, g, rps);
  return 0;
}

// dr = (s * gamma) * dy, dgamma[c] = sum_rows s * dy * r (fp32 [C] or null); ws: dtm_cln_ws_floats(M, C, slab_rows, 1)
DTM_API int dtm_scale_residual_bwd(const void* dy, const void* r, const float* gamma, const float* s, void* dr,
                                   float* dgamma, float* ws, long ws_floats, long M, int C, int ns,
                                   int rows_per_sample, int slab_rows, int bf16, void* stream) {
  ClnGeom g;
  const int rc = make_geom(M, C, slab_rows, &g);
  if (rc) return rc;
  if (!dy || !r || !gamma || !dr || !aligned16(dy) || !aligned16(r) || !aligned16(dr)) return -1;
  if (s && (ns < 1 || rows_per_sample < 1 || (long)ns * rows_per_sample != M)) return -2;
  const int want = dgamma != nullptr;
  if (want && (!ws || ws_floats < (long)g.blocks * C)) return -3;
  const int rps = s ? rows_per_sample : 1;
  hipStream_t st = (hipStream_t)stream;
  CLN_LAUNCH(scale_residual_bwd_kernel, g, bf16, st, dy, r, gamma, s, dr, ws, g, rps, want);
  if (want) records_sum(ws, g, 1, dgamma, nullptr, st);
  return 0;
}
