// Group normalisation (Wu & He 2018) on NHWC, bf16 or fp32 storage, fp32 math.  G == C is instance norm, G == 1
// layer norm.  For sample n and group g (Cg = C / G channels, m = H*W*Cg values):
//   y = act(fma(x, a_c, b_c)),  a_c = rstd * gamma_c,  b_c = beta_c - mean * a_c,  rstd = 1 / sqrt(var + eps)
// Eligible: C % 8 == 0 and Cg in {1, 2, 4} or Cg % 8 == 0, so that a 16-byte channel vector holds whole groups or
// lies inside one.
//
// Work split: the H*W pixels of a sample are cut into slabs of slab_pixels consecutive pixels (the last one may be
// ragged); the grid is (slabs, N).  Lane t of a block owns the 16-byte column t % cols and the pixel lane t / cols
// (cols = C/8, in chunks of 256 columns when C/8 > 256), so in every trip the block reads 256 / cols consecutive
// pixels: one contiguous run of memory.  Pixel lanes are summed through LDS by col_reduce8's fixed tree; channels are
// folded to groups in channel order (inside the vector for Cg < 8, across the group's columns through LDS for
// Cg >= 8, with a carry where a group continues into the next chunk).  Slabs are merged in slab order by every block
// of the sample, which therefore all form the same bits.  No atomics, no flags, no waiting between blocks.
//
// Forward:  gn_stats_kernel  x -> (mean, M2) per (n, slab, g): per-channel sums shifted by the slab's first pixel,
//                            merged as (count, mean, M2) with Chan's formula;
//           gn_apply_kernel  merges the slab records, slab 0 writes stats[n][g] = (mean, rstd), all write y.
// Backward: gn_bwd_sums_kernel   x, dy -> (sum dy, sum dy*xhat) per (n, slab, c) and their gamma-weighted group folds
//                                (A, B) per (n, slab, g); the ReLU mask is the forward's own fma(x, a_c, b_c) > 0;
//           gn_bwd_apply_kernel  merges the group records, slab 0 stores sums[n][c], all write
//                                dx = rstd * (gamma_c * dy - A_g/m - xhat * B_g/m);
//           gn_bwd_param_kernel  dbeta_c = sum_n sums[n][c][0], dgamma_c = sum_n sums[n][c][1], in n order.
#include "nhwc8.h"

// Products and sums are fused only where fmaf says so: the backward's ReLU mask repeats the forward's roundings, and
// gamma * dy minus its own group mean is exactly 0 for a group of one value.
#pragma clang fp contract(off)

namespace dtm {
namespace {

constexpr int GN_T = 256;     // lanes per block = columns per chunk
constexpr int GN_GMAX = 2048;  // groups one chunk can touch (Cg == 1: 8 per column)

struct GnGeom {
  int HW, C, G, Cg, C8, SP, slabs;
  int lg;  // log2(Cg) for Cg < 8
};

// (u, v) of na values absorbs (ub, vb) of nb values.  CHAN: (mean, M2) by Chan's formula; else plain sums.
template <bool CHAN>
__device__ __forceinline__ void merge2(float& u, float& v, float na, float ub, float vb, float nb) {
  if (CHAN) {
    const float d = ub - u, n = na + nb;
    u += d * (nb / n);
    v += vb + d * d * (na * nb / n);
  } else {
    u += ub;
    v += vb;
  }
}

// a_c, b_c of the forward; the backward recomputes the ReLU mask from the same roundings
__device__ __forceinline__ void affine_ab(float mean, float rstd, float gm, float bt, float& a, float& b) {
  a = __fmul_rn(rstd, gm);
  b = __fmaf_rn(-mean, a, bt);
}

// groups that the columns [c0, c0 + cc) touch: first group and their number (<= GN_GMAX)
__device__ __forceinline__ void chunk_groups(const GnGeom& g, const Chunk& k, int& gb, int& ng) {
  if (g.Cg < 8) {
    gb = (k.c0 * 8) >> g.lg;
    ng = (k.cc * 8) >> g.lg;
  } else {
    gb = (k.c0 * 8) / g.Cg;
    ng = ((k.c0 + k.cc) * 8 - 1) / g.Cg - gb + 1;
  }
}

// Per-channel pairs (pref[e] + pu[e], pv[e]: the 8 channels of column c0 + t, held by the lanes t < cc, each of `unit`
// values) fold to groups in channel order; rec[g] = (u, v).  Called by the whole block.  Cg >= 8: a column folds in
// registers, then one lane per group walks the group's columns in colU / colV; a group that runs past the chunk
// leaves its partial in carry[] for the next chunk's first group.  Every fold runs Chan's formula on means taken
// relative to a reference next to them (the pref of a group's first channel, a fold's first mean) and adds it back
// once, so a mean far from 0 is rounded once per fold and not once per merge, and a group of one channel keeps its
// shifted mean pref + pu as it is.
template <bool CHAN>
__device__ __forceinline__ void fold_to_groups(const float (&pu)[8], const float (&pv)[8], const float (&pref)[8],
                                               float unit, const GnGeom& g, const Chunk& k, float* colU, float* colV,
                                               float* carry, float* rec) {
  const int t = threadIdx.x;
  if (t < k.cc) {
    const int mask = min(g.Cg, 8) - 1;
    float u = 0.f, v = 0.f, na = 0.f, ref = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      if ((e & mask) == 0) {
        ref = pref[e]; u = pu[e]; v = pv[e]; na = unit;
      } else {
        merge2<CHAN>(u, v, na, pu[e] + (pref[e] - ref), pv[e], unit);
        na += unit;
      }
      if (((e + 1) & mask) == 0) {
        if (g.Cg < 8) {
          const int gi = ((k.c0 + t) * 8 + e) >> g.lg;
          rec[gi * 2] = ref + u;
          rec[gi * 2 + 1] = v;
        } else {
          colU[t] = ref + u;
          colV[t] = v;
        }
      }
    }
  }
  if (g.Cg < 8) return;
  __syncthreads();
  const int gcols = g.Cg >> 3;
  const float cunit = 8.f * unit;
  const int gfirst = k.c0 / gcols, glast = (k.c0 + k.cc - 1) / gcols;
  if (t <= glast - gfirst) {
    const int gi = gfirst + t;
    const int lo = max(gi * gcols, k.c0), hi = min((gi + 1) * gcols, k.c0 + k.cc);
    float u, v, na;
    int j = lo - k.c0;
    if (gi * gcols < k.c0) {  // continues the group the previous chunk left open
      u = carry[0]; v = carry[1]; na = cunit * (float)(k.c0 - gi * gcols);
    } else {
      u = colU[j]; v = colV[j]; na = cunit; ++j;
    }
    const float ref = CHAN ? u : 0.f;  // (plain sums have no reference)
    u -= ref;
    for (; j < hi - k.c0; ++j) {
      merge2<CHAN>(u, v, na, colU[j] - ref, colV[j], cunit);
      na += cunit;
    }
    if ((gi + 1) * gcols > k.c0 + k.cc) {
      carry[0] = ref + u; carry[1] = v;
    } else {
      rec[gi * 2] = ref + u;
      rec[gi * 2 + 1] = v;
    }
  }
  __syncthreads();  // colU / colV / carry are rewritten by the next chunk
}

// gU / gV[j] = the records of group gb + j merged over the sample's slabs in slab order (lane j, j + GN_T, ...);
// rec0: the sample's first record row, stride floats between slabs
template <bool CHAN>
__device__ __forceinline__ void fold_slabs(const float* rec0, size_t stride, const GnGeom& g, int gb, int ng,
                                           float* gU, float* gV) {
  for (int j = threadIdx.x; j < ng; j += GN_T) {
    const float* r = rec0 + (size_t)(gb + j) * 2;
    const float ref = CHAN ? r[0] : 0.f;  // means relative to the first slab's, as in fold_to_groups
    float u = r[0] - ref, v = r[1], na = (float)min(g.SP, g.HW) * (float)g.Cg;
    for (int s = 1; s < g.slabs; ++s) {
      r += stride;
      const float nb = (float)(min(g.HW, (s + 1) * g.SP) - s * g.SP) * (float)g.Cg;
      merge2<CHAN>(u, v, na, r[0] - ref, r[1], nb);
      na += nb;
    }
    gU[j] = ref + u;
    gV[j] = v;
  }
}

__device__ __forceinline__ int group_of(const GnGeom& g, int ch) { return g.Cg < 8 ? ch >> g.lg : ch / g.Cg; }

// ------------------------------------------------------------------------------------------------------------
// ws[n][slab][g] = (mean, M2) of the slab's pixels x the group's channels
template <bool BF16>
__global__ __launch_bounds__(GN_T) void gn_stats_kernel(const void* __restrict__ x, float* __restrict__ ws, GnGeom g) {
  __shared__ float red[2][GN_T][8];
  __shared__ float colU[GN_T], colV[GN_T], carry[2];
  const int n = blockIdx.y, slab = blockIdx.x;
  const int p0 = slab * g.SP, p1 = min(g.HW, p0 + g.SP);
  const float np = (float)(p1 - p0);
  const size_t base = (size_t)n * g.HW * g.C;
  float* rec = ws + ((size_t)n * g.slabs + slab) * g.G * 2;
  for (int c0 = 0; c0 < g.C8; c0 += GN_T) {
    const Chunk k = make_chunk<GN_T>(c0, g.C8);
    float K[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};  // the shift: this column at the slab's first pixel
    float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, q[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (k.live) {
      ld8<BF16>(x, base + (size_t)p0 * g.C + k.c, K);
      for (int p = p0 + k.pl; p < p1; p += k.PL) {
        float v[8];
        ld8<BF16>(x, base + (size_t)p * g.C + k.c, v);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float d = v[e] - K[e];
          s[e] += d;
          q[e] = fmaf(d, d, q[e]);
        }
      }
    }
    // the totals of column t stay in lane t's own rows red[.][t]: col_reduce8's final store lands where it reads
    col_reduce8(red, s, q, &red[0][0][0], &red[1][0][0], k.cc, k.col * 8);
    float mu[8], m2[8];
    if (threadIdx.x < k.cc) {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float ts = red[0][k.col][e], tq = red[1][k.col][e];
        const float dm = ts / np;
        mu[e] = dm;  // relative to the channel's own shift
        m2[e] = fmaxf(tq - ts * dm, 0.f);  // sum (d - dm)^2 of the shifted values d = x - K
      }
    }
    fold_to_groups<true>(mu, m2, K, np, g, k, colU, colV, carry, rec);
  }
}

template <bool BF16>
__global__ __launch_bounds__(GN_T) void gn_apply_kernel(const void* __restrict__ x, const float* __restrict__ gamma,
                                                        const float* __restrict__ beta, void* __restrict__ y,
                                                        float* __restrict__ stats, const float* __restrict__ ws,
                                                        GnGeom g, float eps, int relu) {
  __shared__ float gM[GN_GMAX], gR[GN_GMAX];
  const int n = blockIdx.y, slab = blockIdx.x;
  const int p0 = slab * g.SP, p1 = min(g.HW, p0 + g.SP);
  const size_t base = (size_t)n * g.HW * g.C;
  const float m = (float)g.HW * (float)g.Cg;
  for (int c0 = 0; c0 < g.C8; c0 += GN_T) {
    const Chunk k = make_chunk<GN_T>(c0, g.C8);
    int gb, ng;
    chunk_groups(g, k, gb, ng);
    fold_slabs<true>(ws + (size_t)n * g.slabs * g.G * 2, (size_t)g.G * 2, g, gb, ng, gM, gR);
    for (int j = threadIdx.x; j < ng; j += GN_T) {
      const float rstd = rsqrtf(gR[j] / m + eps);
      gR[j] = rstd;
      if (slab == 0) {
        stats[((size_t)n * g.G + gb + j) * 2] = gM[j];
        stats[((size_t)n * g.G + gb + j) * 2 + 1] = rstd;
      }
    }
    __syncthreads();
    if (k.live) {
      float a[8], b[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int gi = group_of(g, k.c + e) - gb;
        affine_ab(gM[gi], gR[gi], gamma ? gamma[k.c + e] : 1.f, beta ? beta[k.c + e] : 0.f, a[e], b[e]);
      }
      for (int p = p0 + k.pl; p < p1; p += k.PL) {
        float v[8];
        const size_t off = base + (size_t)p * g.C + k.c;
        ld8<BF16>(x, off, v);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          v[e] = __fmaf_rn(v[e], a[e], b[e]);
          if (relu) v[e] = fmaxf(v[e], 0.f);
        }
        st8<BF16>(y, off, v);
      }
    }
    __syncthreads();  // gM / gR are rewritten by the next chunk
  }
}

// backward workspace of one (n, slab): [2][C] channel sums (sum dy, sum dy*xhat), then [G][2] group folds (A, B)
__device__ __forceinline__ size_t bwd_row(const GnGeom& g) { return 2 * (size_t)g.C + 2 * (size_t)g.G; }

template <bool BF16>
__global__ __launch_bounds__(GN_T) void gn_bwd_sums_kernel(const void* __restrict__ x, const void* __restrict__ dy,
                                                           const float* __restrict__ gamma,
                                                           const float* __restrict__ beta,
                                                           const float* __restrict__ stats, float* __restrict__ ws,
                                                           GnGeom g, int relu) {
  __shared__ float red[2][GN_T][8];
  __shared__ float colU[GN_T], colV[GN_T], carry[2];
  const int n = blockIdx.y, slab = blockIdx.x;
  const int p0 = slab * g.SP, p1 = min(g.HW, p0 + g.SP);
  const size_t base = (size_t)n * g.HW * g.C;
  float* row = ws + ((size_t)n * g.slabs + slab) * bwd_row(g);
  for (int c0 = 0; c0 < g.C8; c0 += GN_T) {
    const Chunk k = make_chunk<GN_T>(c0, g.C8);
    float sg[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, sx[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    float gm[8];
    if (k.live) {
      float mean[8], rstd[8], a[8], b[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const size_t si = ((size_t)n * g.G + group_of(g, k.c + e)) * 2;
        mean[e] = stats[si];
        rstd[e] = stats[si + 1];
        gm[e] = gamma ? gamma[k.c + e] : 1.f;
        affine_ab(mean[e], rstd[e], gm[e], beta ? beta[k.c + e] : 0.f, a[e], b[e]);
      }
      for (int p = p0 + k.pl; p < p1; p += k.PL) {
        float v[8], d[8];
        const size_t off = base + (size_t)p * g.C + k.c;
        ld8<BF16>(x, off, v);
        ld8<BF16>(dy, off, d);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          if (relu && !(__fmaf_rn(v[e], a[e], b[e]) > 0.f)) d[e] = 0.f;
          sg[e] += d[e];
          sx[e] = fmaf(d[e], (v[e] - mean[e]) * rstd[e], sx[e]);
        }
      }
    }
    col_reduce8(red, sg, sx, row, row + g.C, k.cc, k.c);  // lanes t < cc: the channel sums, straight to the workspace
    float pu[8], pv[8];
    if (threadIdx.x < k.cc) {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        pu[e] = __fmul_rn(gm[e], row[k.c + e]);  // this lane's own stores
        pv[e] = __fmul_rn(gm[e], row[g.C + k.c + e]);
      }
    }
    const float none[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    fold_to_groups<false>(pu, pv, none, 0.f, g, k, colU, colV, carry, row + 2 * (size_t)g.C);
  }
}

template <bool BF16>
__global__ __launch_bounds__(GN_T) void gn_bwd_apply_kernel(const void* __restrict__ x, const void* __restrict__ dy,
                                                            const float* __restrict__ gamma,
                                                            const float* __restrict__ beta,
                                                            const float* __restrict__ stats,
                                                            const float* __restrict__ ws, void* __restrict__ dx,
                                                            float* __restrict__ sums, GnGeom g, int relu) {
  __shared__ float gA[GN_GMAX], gB[GN_GMAX];
  const int n = blockIdx.y, slab = blockIdx.x;
  const int p0 = slab * g.SP, p1 = min(g.HW, p0 + g.SP);
  const size_t base = (size_t)n * g.HW * g.C;
  const float inv_m = 1.f / ((float)g.HW * (float)g.Cg);
  const float* rows = ws + (size_t)n * g.slabs * bwd_row(g);
  for (int c0 = 0; c0 < g.C8; c0 += GN_T) {
    const Chunk k = make_chunk<GN_T>(c0, g.C8);
    int gb, ng;
    chunk_groups(g, k, gb, ng);
    fold_slabs<false>(rows + 2 * (size_t)g.C, bwd_row(g), g, gb, ng, gA, gB);
    for (int j = threadIdx.x; j < ng; j += GN_T) { gA[j] *= inv_m; gB[j] *= inv_m; }
    if (slab == 0) {  // sums[n][c] for the parameter gradients: the slab rows in slab order
      for (int ch = c0 * 8 + threadIdx.x; ch < (c0 + k.cc) * 8; ch += GN_T) {
        float s1 = 0.f, s2 = 0.f;
        for (int s = 0; s < g.slabs; ++s) {
          s1 += rows[s * bwd_row(g) + ch];
          s2 += rows[s * bwd_row(g) + g.C + ch];
        }
        sums[((size_t)n * g.C + ch) * 2] = s1;
        sums[((size_t)n * g.C + ch) * 2 + 1] = s2;
      }
    }
    __syncthreads();
    if (k.live) {
      float mean[8], rstd[8], a[8], b[8], gm[8], mA[8], mB[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int gi = group_of(g, k.c + e);
        mean[e] = stats[((size_t)n * g.G + gi) * 2];
        rstd[e] = stats[((size_t)n * g.G + gi) * 2 + 1];
        gm[e] = gamma ? gamma[k.c + e] : 1.f;
        affine_ab(mean[e], rstd[e], gm[e], beta ? beta[k.c + e] : 0.f, a[e], b[e]);
        mA[e] = gA[gi - gb];
        mB[e] = gB[gi - gb];
      }
      for (int p = p0 + k.pl; p < p1; p += k.PL) {
        float v[8], d[8];
        const size_t off = base + (size_t)p * g.C + k.c;
        ld8<BF16>(x, off, v);
        ld8<BF16>(dy, off, d);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          if (relu && !(__fmaf_rn(v[e], a[e], b[e]) > 0.f)) d[e] = 0.f;
          const float xh = (v[e] - mean[e]) * rstd[e];
          // (the product is rounded as the group fold's was: a group of one value gives exactly 0)
          d[e] = rstd[e] * (__fmul_rn(gm[e], d[e]) - mA[e] - xh * mB[e]);
        }
        st8<BF16>(dx, off, d);
      }
    }
    __syncthreads();  // gA / gB are rewritten by the next chunk
  }
}

// sums[n][c] = (sum dy, sum dy*xhat) -> dbeta, dgamma (either may be null), summed in n order
__global__ __launch_bounds__(GN_T) void gn_bwd_param_kernel(const float* __restrict__ sums, float* __restrict__ dgamma,
                                                            float* __restrict__ dbeta, int N, int C) {
  const int c = blockIdx.x * GN_T + threadIdx.x;
  if (c >= C) return;
  float s1 = 0.f, s2 = 0.f;
  for (int n = 0; n < N; ++n) {
    const float2 r = *(const float2*)(sums + ((size_t)n * C + c) * 2);
    s1 += r.x;
    s2 += r.y;
  }
  if (dbeta) dbeta[c] = s1;
  if (dgamma) dgamma[c] = s2;
}

// 0, or the entry points' negative code
int make_geom(int N, int HW, int C, int G, int slab_pixels, GnGeom* g) {
  if (C < 8 || C % 8 != 0 || G < 1 || C % G != 0) return -1;
  const int Cg = C / G;
  if (!(Cg == 1 || Cg == 2 || Cg == 4 || Cg % 8 == 0)) return -1;
  if (N < 1 || N > 65535 || HW < 1 || slab_pixels < 1) return -2;
  g->HW = HW; g->C = C; g->G = G; g->Cg = Cg; g->C8 = C / 8;
  g->SP = slab_pixels < HW ? slab_pixels : HW;
  g->slabs = (HW + g->SP - 1) / g->SP;
  g->lg = Cg == 2 ? 1 : Cg == 4 ? 2 : 0;
  return 0;
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace
}  // namespace dtm

using namespace dtm;

// floats of workspace that dtm_groupnorm_fwd (bwd == 0) or dtm_groupnorm_bwd needs; negative for a shape they refuse
DTM_API long dtm_groupnorm_ws_floats(int N, int HW, int C, int G, int slab_pixels, int bwd) {
  GnGeom g;
  const int rc = make_geom(N, HW, C, G, slab_pixels, &g);
  if (rc) return rc;
  return (long)N * g.slabs * (bwd ? 2 * ((long)C + G) : 2 * (long)G);
}

// slab_pixels: every block merges all slab records of its sample (and slab 0 of the backward sums slabs x C floats),
// so callers keep the slabs of a sample to a hundred or so; ops/groupnorm.py holds them to 128.
// stats: [N][G][2] (mean, rstd) for the backward.  -1 ineligible shape or null / misaligned tensor, -2 N, HW or
// slab_pixels below 1, -3 workspace too small; nothing is launched after a negative code.
DTM_API int dtm_groupnorm_fwd(const void* x, const float* gamma, const float* beta, void* y, float* stats, float* ws,
                              long ws_floats, int N, int HW, int C, int G, int slab_pixels, float eps, int relu,
                              int bf16, void* stream) {
  GnGeom g;
  const int rc = make_geom(N, HW, C, G, slab_pixels, &g);
  if (rc) return rc;
  if (!x || !y || !stats || !ws || !aligned16(x) || !aligned16(y)) return -1;
  if (ws_floats < dtm_groupnorm_ws_floats(N, HW, C, G, slab_pixels, 0)) return -3;
  const dim3 grid(g.slabs, N);
  hipStream_t st = (hipStream_t)stream;
  if (bf16) {
    hipLaunchKernelGGL(gn_stats_kernel<true>, grid, dim3(GN_T), 0, st, x, ws, g);
    hipLaunchKernelGGL(gn_apply_kernel<true>, grid, dim3(GN_T), 0, st, x, gamma, beta, y, stats, ws, g, eps, relu);
  } else {
    hipLaunchKernelGGL(gn_stats_kernel<false>, grid, dim3(GN_T), 0, st, x, ws, g);
    hipLaunchKernelGGL(gn_apply_kernel<false>, grid, dim3(GN_T), 0, st, x, gamma, beta, y, stats, ws, g, eps, relu);
  }
  return 0;
}

// dy: the gradient w.r.t. y; sums: [N][C][2] scratch; dgamma / dbeta: fp32 [C] or null.  Codes as the forward's.
DTM_API int dtm_groupnorm_bwd(const void* x, const void* dy, const float* gamma, const float* beta, const float* stats,
                              void* dx, float* dgamma, float* dbeta, float* ws, long ws_floats, float* sums, int N,
                              int HW, int C, int G, int slab_pixels, int relu, int bf16, void* stream) {
  GnGeom g;
  const int rc = make_geom(N, HW, C, G, slab_pixels, &g);
  if (rc) return rc;
  if (!x || !dy || !stats || !dx || !ws || !sums || !aligned16(x) || !aligned16(dy) || !aligned16(dx)) return -1;
  if (ws_floats < dtm_groupnorm_ws_floats(N, HW, C, G, slab_pixels, 1)) return -3;
  const dim3 grid(g.slabs, N);
  hipStream_t st = (hipStream_t)stream;
  if (bf16) {
    hipLaunchKernelGGL(gn_bwd_sums_kernel<true>, grid, dim3(GN_T), 0, st, x, dy, gamma, beta, stats, ws, g, relu);
    hipLaunchKernelGGL(gn_bwd_apply_kernel<true>, grid, dim3(GN_T), 0, st, x, dy, gamma, beta, stats, ws, dx, sums, g,
                       relu);
  } else {
    hipLaunchKernelGGL(gn_bwd_sums_kernel<false>, grid, dim3(GN_T), 0, st, x, dy, gamma, beta, stats, ws, g, relu);
    hipLaunchKernelGGL(gn_bwd_apply_kernel<false>, grid, dim3(GN_T), 0, st, x, dy, gamma, beta, stats, ws, dx, sums, g,
                       relu);
  }
  if (dgamma || dbeta)
    hipLaunchKernelGGL(gn_bwd_param_kernel, dim3((C + GN_T - 1) / GN_T), dim3(GN_T), 0, st, sums, dgamma, dbeta, N, C);
  return 0;
}
