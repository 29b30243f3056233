// Squeeze-and-excitation (Hu et al. 2018) on NHWC bf16 with an optional residual add and ReLU; fp32 math and fp32
// master weights.  For sample n (HW pixels, C channels, Cr hidden units):
//   s[n,c] = (1/HW) sum_hw x            z[n,j] = relu(w1[j,:] . s[n,:] + b1[j])
//   g[n,c] = sigmoid(w2[c,:] . z[n,:] + b2[c])         y = act(x * g[n,c] + residual)
// Eligible: C % 8 == 0, 8 <= C <= 4096, 1 <= Cr <= 256, 1 <= N <= 65535, HW >= 1.
//
// Work split of the passes over the big tensors, as groupnorm.hip: a sample's pixels are cut into slabs of
// slab_pixels consecutive pixels, the grid is (slabs, N); lane t owns the 16-byte column t % cols and the pixel lane
// t / cols (cols = C/8, in chunks of 256 columns when C/8 > 256), so every trip reads one contiguous run.  Pixel lanes
// are summed through LDS by col_tree8's fixed tree, slab records are merged in slab order.  The excitation MLP runs in
// blocks of 1024 lanes, one per SE_G consecutive samples: a weight row loaded once serves the whole sample group, whose
// squeezed vectors live in LDS.  No atomics, no flags, no waiting between blocks: every result keeps its bits.
//
// Forward:  se_squeeze_kernel   x -> sum_hw x per (n, slab, c);
//           se_gate_kernel      merges the slab records to s, FC1 (a wave owns hidden units, its lanes stride over C
//                               with 16-byte loads, xor butterfly), FC2 (a lane owns a channel and walks z from LDS),
//                               sigmoid; writes s, z, g for the backward;
//           se_scale_kernel     y = act(x * g + residual), the lane's eight gates held in registers.
// Backward: se_bwd_sums_kernel  dm = dy * [y > 0];  sum_hw dm * x per (n, slab, c);
//           se_gate_bwd_kernel  merges to dg;  da2 = dg g (1 - g);  dz = (w2^T da2) [z > 0];  ds = (w1^T dz) / HW;
//           se_wgrad_kernel     dw2 = sum_n da2 (x) z, db2 = sum_n da2, dw1 = sum_n dz (x) s, db1 = sum_n dz;
//           se_bwd_apply_kernel dx = dm * g + ds;  dresidual = dm (written only where it is not dy itself).
#include "nhwc8.h"

namespace dtm {
namespace {

constexpr int SE_T = 256;    // lanes per block of the slab kernels = columns per chunk
constexpr int SE_GT = 1024;  // lanes per block of the gate kernels
constexpr int SE_G = 4;      // samples per block of the gate kernels
constexpr int SE_CMAX = 4096, SE_CRMAX = 256;
// dynamic LDS of the gate kernels at the largest shape (floats): forward s + z, backward da2 + dz + the dz partials
constexpr int SE_GATE_LDS = SE_G * (SE_CMAX + SE_CRMAX);
constexpr int SE_GATE_BWD_LDS = SE_G * (SE_CMAX + SE_CRMAX) + SE_G * SE_GT;

struct SeGeom {
  int N, HW, C, C8, Cr, SP, slabs;
};

// One accumulator set through col_tree8: the lanes t < cols store their column's totals at out (their own pointer).
// Called by the whole block.
__device__ __forceinline__ void col_sum8(float (*red)[SE_T][8], const float (&s)[8], float* out, int cols) {
  const int t = threadIdx.x;
  if (!col_tree8<1, SE_T>(red, s, nullptr, cols)) {
    if (t < cols) {
      *(float4*)out = make_float4(s[0], s[1], s[2], s[3]);
      *(float4*)(out + 4) = make_float4(s[4], s[5], s[6], s[7]);
    }
    return;
  }
  if (t < cols) {
    *(float4*)out = make_float4(red[0][t][0], red[0][t][1], red[0][t][2], red[0][t][3]);
    *(float4*)(out + 4) = make_float4(red[0][t][4], red[0][t][5], red[0][t][6], red[0][t][7]);
  }
}

// ------------------------------------------------------------------------------------------------------------
// ws[n][slab][c] = sum of x over the slab's pixels
__global__ __launch_bounds__(SE_T) void se_squeeze_kernel(const bf16_t* __restrict__ x, float* __restrict__ ws,
                                                          SeGeom g) {
  __shared__ float red[1][SE_T][8];
  const int n = blockIdx.y, slab = blockIdx.x;
  const int p0 = slab * g.SP, p1 = min(g.HW, p0 + g.SP);
  const size_t base = (size_t)n * g.HW * g.C;
  float* rec = ws + ((size_t)n * g.slabs + slab) * g.C;
  for (int c0 = 0; c0 < g.C8; c0 += SE_T) {
    const Chunk k = make_chunk<SE_T>(c0, g.C8);
    float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (k.live) {
#pragma unroll 4
      for (int p = p0 + k.pl; p < p1; p += k.PL) {
        float v[8];
        ld8<true>(x, base + (size_t)p * g.C + k.c, v);
#pragma unroll
        for (int e = 0; e < 8; ++e) s[e] += v[e];
      }
    }
    col_sum8(red, s, rec + k.c, k.cc);
  }
}

// channel c of sample n: its slab records summed in slab order
__device__ __forceinline__ float merge_slabs(const float* __restrict__ ws, const SeGeom& g, int n, int c) {
  const float* r = ws + (size_t)n * g.slabs * g.C + c;
  float a = 0.f;
#pragma unroll 4
  for (int s = 0; s < g.slabs; ++s) a += r[(size_t)s * g.C];
  return a;
}

// One block per SE_G samples.  LDS: s [SE_G][C], z [SE_G][Cr].
__global__ __launch_bounds__(SE_GT) void se_gate_kernel(const float* __restrict__ ws, const float* __restrict__ w1,
                                                        const float* __restrict__ b1, const float* __restrict__ w2,
                                                        const float* __restrict__ b2, float* __restrict__ s_out,
                                                        float* __restrict__ z_out, float* __restrict__ g_out,
                                                        SeGeom g) {
  extern __shared__ float sm[];
  float* sS = sm;
  float* sZ = sm + SE_G * g.C;
  const int t = threadIdx.x, n0 = blockIdx.x * SE_G, ng = min(SE_G, g.N - n0);
  const int C = g.C, Cr = g.Cr;
  const float inv = 1.f / (float)g.HW;
  for (int i = t; i < SE_G * C; i += SE_GT) {
    const int gi = i / C, c = i - gi * C;
    float a = 0.f;
    if (gi < ng) {
      a = merge_slabs(ws, g, n0 + gi, c) * inv;
      s_out[(size_t)(n0 + gi) * C + c] = a;
    }
    sS[i] = a;
  }
  __syncthreads();
  // FC1: wave w owns the hidden units w, w + 16, ...; one row load serves the SE_G samples
  const int wave = t >> 6, lane = t & 63;
  for (int j = wave; j < Cr; j += SE_GT / 64) {
    const float* wr = w1 + (size_t)j * C;
    float acc[SE_G];
#pragma unroll
    for (int gi = 0; gi < SE_G; ++gi) acc[gi] = 0.f;
#pragma unroll 4  // several row loads in flight: the block is bound by the latency of its weight reads
    for (int c = lane * 4; c < C; c += 256) {
      const float4 w = *(const float4*)(wr + c);
#pragma unroll
      for (int gi = 0; gi < SE_G; ++gi) {
        const float4 v = *(const float4*)(sS + gi * C + c);
        acc[gi] = fmaf(w.x, v.x, acc[gi]);
        acc[gi] = fmaf(w.y, v.y, acc[gi]);
        acc[gi] = fmaf(w.z, v.z, acc[gi]);
        acc[gi] = fmaf(w.w, v.w, acc[gi]);
      }
    }
    const float bj = b1[j];
#pragma unroll
    for (int gi = 0; gi < SE_G; ++gi) {
      const float v = fmaxf(warp_sum(acc[gi]) + bj, 0.f);
      if (lane == 0) {
        sZ[gi * Cr + j] = v;
        if (gi < ng) z_out[(size_t)(n0 + gi) * Cr + j] = v;
      }
    }
  }
  __syncthreads();
  // FC2: a lane owns a channel, its w2 row is contiguous; z is an LDS broadcast
  for (int c = t; c < C; c += SE_GT) {
    const float* wr = w2 + (size_t)c * Cr;
    float acc[SE_G];
#pragma unroll
    for (int gi = 0; gi < SE_G; ++gi) acc[gi] = 0.f;
    int j = 0;
    if ((Cr & 3) == 0) {
#pragma unroll 4
      for (; j < Cr; j += 4) {
        const float4 w = *(const float4*)(wr + j);
#pragma unroll
        for (int gi = 0; gi < SE_G; ++gi) {
          const float4 v = *(const float4*)(sZ + gi * Cr + j);
          acc[gi] = fmaf(w.x, v.x, acc[gi]);
          acc[gi] = fmaf(w.y, v.y, acc[gi]);
          acc[gi] = fmaf(w.z, v.z, acc[gi]);
          acc[gi] = fmaf(w.w, v.w, acc[gi]);
        }
      }
    }
    for (; j < Cr; ++j) {
      const float w = wr[j];
#pragma unroll
      for (int gi = 0; gi < SE_G; ++gi) acc[gi] = fmaf(w, sZ[gi * Cr + j], acc[gi]);
    }
    const float bc = b2[c];
#pragma unroll
    for (int gi = 0; gi < SE_G; ++gi)
      if (gi < ng) g_out[(size_t)(n0 + gi) * C + c] = 1.f / (1.f + expf(-(acc[gi] + bc)));
  }
}

template <bool RES, bool RELU>
__global__ __launch_bounds__(SE_T) void se_scale_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ res,
                                                        const float* __restrict__ gate, bf16_t* __restrict__ y,
                                                        SeGeom g) {
  const int n = blockIdx.y, slab = blockIdx.x;
  const int p0 = slab * g.SP, p1 = min(g.HW, p0 + g.SP);
  const size_t base = (size_t)n * g.HW * g.C;
  for (int c0 = 0; c0 < g.C8; c0 += SE_T) {
    const Chunk k = make_chunk<SE_T>(c0, g.C8);
    if (!k.live) continue;
    float gv[8];
    ld8<false>(gate + (size_t)n * g.C + k.c, 0, gv);
#pragma unroll 2
    for (int p = p0 + k.pl; p < p1; p += k.PL) {
      const size_t off = base + (size_t)p * g.C + k.c;
      float v[8], r[8];
      ld8<true>(x, off, v);
      if (RES) ld8<true>(res, off, r);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        v[e] = RES ? fmaf(v[e], gv[e], r[e]) : v[e] * gv[e];
        if (RELU) v[e] = fmaxf(v[e], 0.f);
      }
      st8<true>(y, off, v);
    }
  }
}

// ws[n][slab][c] = sum of dm * x over the slab's pixels
template <bool RELU>
__global__ __launch_bounds__(SE_T) void se_bwd_sums_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ y,
                                                           const bf16_t* __restrict__ dy, float* __restrict__ ws,
                                                           SeGeom g) {
  __shared__ float red[1][SE_T][8];
  const int n = blockIdx.y, slab = blockIdx.x;
  const int p0 = slab * g.SP, p1 = min(g.HW, p0 + g.SP);
  const size_t base = (size_t)n * g.HW * g.C;
  float* rec = ws + ((size_t)n * g.slabs + slab) * g.C;
  for (int c0 = 0; c0 < g.C8; c0 += SE_T) {
    const Chunk k = make_chunk<SE_T>(c0, g.C8);
    float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (k.live) {
#pragma unroll 2
      for (int p = p0 + k.pl; p < p1; p += k.PL) {
        const size_t off = base + (size_t)p * g.C + k.c;
        float v[8], d[8], o[8];
        ld8<true>(x, off, v);
        ld8<true>(dy, off, d);
        if (RELU) ld8<true>(y, off, o);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          if (RELU && !(o[e] > 0.f)) d[e] = 0.f;
          s[e] = fmaf(d[e], v[e], s[e]);
        }
      }
    }
    col_sum8(red, s, rec + k.c, k.cc);
  }
}

// One block per SE_G samples (the forward's groups).  LDS: da2 [SE_G][C], dz [SE_G][Cr], red [PL][SE_G][Cr] with
// PL = SE_GT / Cr partial sums per hidden unit.  out: da2 [N][C], dz [N][Cr], ds [N][C].
__global__ __launch_bounds__(SE_GT) void se_gate_bwd_kernel(const float* __restrict__ ws, const float* __restrict__ w1,
                                                            const float* __restrict__ w2, const float* __restrict__ z,
                                                            const float* __restrict__ gate, float* __restrict__ da2_out,
                                                            float* __restrict__ dz_out, float* __restrict__ ds_out,
                                                            SeGeom g) {
  extern __shared__ float sm[];
  float* sA = sm;
  float* sD = sm + SE_G * g.C;
  float* red = sD + SE_G * g.Cr;
  const int t = threadIdx.x, n0 = blockIdx.x * SE_G, ng = min(SE_G, g.N - n0);
  const int C = g.C, Cr = g.Cr;
  for (int i = t; i < SE_G * C; i += SE_GT) {
    const int gi = i / C, c = i - gi * C;
    float a = 0.f;
    if (gi < ng) {
      const size_t o = (size_t)(n0 + gi) * C + c;
      const float gg = gate[o];
      a = merge_slabs(ws, g, n0 + gi, c) * gg * (1.f - gg);
      da2_out[o] = a;
    }
    sA[i] = a;
  }
  __syncthreads();
  // dz: lane (j, p) sums the channels p, p + PL, ... of column j of w2 (consecutive lanes read consecutive j)
  const int PL = SE_GT / Cr;
  {
    const int j = t % Cr, p = t / Cr;
    if (p < PL) {
      float acc[SE_G];
#pragma unroll
      for (int gi = 0; gi < SE_G; ++gi) acc[gi] = 0.f;
#pragma unroll 8
      for (int c = p; c < C; c += PL) {
        const float w = w2[(size_t)c * Cr + j];
#pragma unroll
        for (int gi = 0; gi < SE_G; ++gi) acc[gi] = fmaf(w, sA[gi * C + c], acc[gi]);
      }
#pragma unroll
      for (int gi = 0; gi < SE_G; ++gi) red[(p * SE_G + gi) * Cr + j] = acc[gi];
    }
  }
  __syncthreads();
  if (t < SE_G * Cr) {  // the partials in p order
    const int gi = t / Cr, j = t - gi * Cr;
    float a = 0.f;
    for (int p = 0; p < PL; ++p) a += red[(p * SE_G + gi) * Cr + j];
    if (gi < ng) {
      const size_t o = (size_t)(n0 + gi) * Cr + j;
      a = z[o] > 0.f ? a : 0.f;
      dz_out[o] = a;
    } else {
      a = 0.f;
    }
    sD[t] = a;
  }
  __syncthreads();
  // ds: a lane owns a channel and walks the rows of w1 (consecutive lanes read consecutive c)
  const float inv = 1.f / (float)g.HW;
  for (int c = t; c < C; c += SE_GT) {
    float acc[SE_G];
#pragma unroll
    for (int gi = 0; gi < SE_G; ++gi) acc[gi] = 0.f;
#pragma unroll 8
    for (int j = 0; j < Cr; ++j) {
      const float w = w1[(size_t)j * C + c];
#pragma unroll
      for (int gi = 0; gi < SE_G; ++gi) acc[gi] = fmaf(w, sD[gi * Cr + j], acc[gi]);
    }
#pragma unroll
    for (int gi = 0; gi < SE_G; ++gi)
      if (gi < ng) ds_out[(size_t)(n0 + gi) * C + c] = acc[gi] * inv;
  }
}

// blockIdx.y == 0: a tile of 256 consecutive elements of dw2 [C][Cr] and the db2 of the rows that begin in it;
// blockIdx.y == 1: the same of dw1 [Cr][C] and db1.  Every element sums over n in ascending order.
__global__ __launch_bounds__(SE_T) void se_wgrad_kernel(const float* __restrict__ da2, const float* __restrict__ dz,
                                                        const float* __restrict__ s, const float* __restrict__ z,
                                                        float* __restrict__ dw1, float* __restrict__ db1,
                                                        float* __restrict__ dw2, float* __restrict__ db2, int N, int C,
                                                        int Cr) {
  const int e = blockIdx.x * SE_T + threadIdx.x;
  if (e >= C * Cr) return;
  const bool second = blockIdx.y == 0;
  const int ld_row = second ? C : Cr, ld_col = second ? Cr : C;  // row operand da2 / dz, column operand z / s
  const int row = e / ld_col, col = e - row * ld_col;
  const float* a = (second ? da2 : dz) + row;
  const float* b = (second ? z : s) + col;
  float w = 0.f, bias = 0.f;
#pragma unroll 4
  for (int n = 0; n < N; ++n) {
    const float d = a[(size_t)n * ld_row];
    w = fmaf(d, b[(size_t)n * ld_col], w);
    bias += d;
  }
  (second ? dw2 : dw1)[e] = w;
  if (col == 0) (second ? db2 : db1)[row] = bias;
}

template <bool RELU, bool DRES>
__global__ __launch_bounds__(SE_T) void se_bwd_apply_kernel(const bf16_t* __restrict__ y, const bf16_t* __restrict__ dy,
                                                            const float* __restrict__ gate,
                                                            const float* __restrict__ ds, bf16_t* __restrict__ dx,
                                                            bf16_t* __restrict__ dres, SeGeom g) {
  const int n = blockIdx.y, slab = blockIdx.x;
  const int p0 = slab * g.SP, p1 = min(g.HW, p0 + g.SP);
  const size_t base = (size_t)n * g.HW * g.C;
  for (int c0 = 0; c0 < g.C8; c0 += SE_T) {
    const Chunk k = make_chunk<SE_T>(c0, g.C8);
    if (!k.live) continue;
    float gv[8], sv[8];
    ld8<false>(gate + (size_t)n * g.C + k.c, 0, gv);
    ld8<false>(ds + (size_t)n * g.C + k.c, 0, sv);
#pragma unroll 2
    for (int p = p0 + k.pl; p < p1; p += k.PL) {
      const size_t off = base + (size_t)p * g.C + k.c;
      float d[8], o[8], v[8];
      ld8<true>(dy, off, d);
      if (RELU) ld8<true>(y, off, o);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        if (RELU && !(o[e] > 0.f)) d[e] = 0.f;
        v[e] = fmaf(d[e], gv[e], sv[e]);
      }
      st8<true>(dx, off, v);
      if (DRES) st8<true>(dres, off, d);
    }
  }
}

// 0, or the entry points' negative code
int make_geom(int N, int HW, int C, int Cr, int slab_pixels, SeGeom* g) {
  if (C < 8 || C > SE_CMAX || C % 8 != 0 || Cr < 1 || Cr > SE_CRMAX) return -1;
  if (N < 1 || N > 65535 || HW < 1 || slab_pixels < 1) return -2;
  g->N = N; g->HW = HW; g->C = C; g->C8 = C / 8; g->Cr = Cr;
  g->SP = slab_pixels < HW ? slab_pixels : HW;
  g->slabs = (HW + g->SP - 1) / g->SP;
  return 0;
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// the gate kernels' LDS at the largest shapes passes the 64 KiB a launch gets unasked
bool gate_lds_ready() {
  static const bool ok =
      hipFuncSetAttribute((const void*)se_gate_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                          SE_GATE_LDS * (int)sizeof(float)) == hipSuccess &&
      hipFuncSetAttribute((const void*)se_gate_bwd_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                          SE_GATE_BWD_LDS * (int)sizeof(float)) == hipSuccess;
  return ok;
}

}  // namespace
}  // namespace dtm

using namespace dtm;

// floats of workspace that dtm_se_fwd (bwd == 0) or dtm_se_bwd needs; negative for a shape they refuse.
// Forward: the slab records [N][slabs][C].  Backward: the same, then da2 [N][C], dz [N][Cr], ds [N][C].
DTM_API long dtm_se_ws_floats(int N, int HW, int C, int Cr, int slab_pixels, int bwd) {
  SeGeom g;
  const int rc = make_geom(N, HW, C, Cr, slab_pixels, &g);
  if (rc) return rc;
  return (long)N * g.slabs * C + (bwd ? (long)N * (2 * C + Cr) : 0);
}

// x, res (or null), y: bf16 [N][HW][C]; w1 [Cr][C], b1 [Cr], w2 [C][Cr], b2 [C]: fp32; s [N][C], z [N][Cr], g [N][C]:
// fp32 outputs kept for the backward.  -1 ineligible shape or null / misaligned tensor, -2 N, HW or slab_pixels below
// 1, -3 workspace too small, -4 the device refuses the gate kernels' LDS; nothing is launched after a negative code.
// Callers keep the slabs of a sample to a hundred or so (the gate kernel merges them serially); ops/se.py holds them
// to 128.
DTM_API int dtm_se_fwd(const void* x, const void* res, const float* w1, const float* b1, const float* w2,
                       const float* b2, void* y, float* s, float* z, float* gate, float* ws, long ws_floats, int N,
                       int HW, int C, int Cr, int slab_pixels, int relu, void* stream) {
  SeGeom g;
  const int rc = make_geom(N, HW, C, Cr, slab_pixels, &g);
  if (rc) return rc;
  if (!x || !w1 || !b1 || !w2 || !b2 || !y || !s || !z || !gate || !ws) return -1;
  if (!aligned16(x) || !aligned16(res) || !aligned16(y) || !aligned16(w1) || !aligned16(w2) || !aligned16(s) ||
      !aligned16(z) || !aligned16(gate) || !aligned16(ws))
    return -1;
  if (ws_floats < dtm_se_ws_floats(N, HW, C, Cr, slab_pixels, 0)) return -3;
  if (!gate_lds_ready()) return -4;
  const dim3 grid(g.slabs, N);
  hipStream_t st = (hipStream_t)stream;
  const bf16_t *xb = (const bf16_t*)x, *rb = (const bf16_t*)res;
  bf16_t* yb = (bf16_t*)y;
  hipLaunchKernelGGL(se_squeeze_kernel, grid, dim3(SE_T), 0, st, xb, ws, g);
  hipLaunchKernelGGL(se_gate_kernel, dim3((N + SE_G - 1) / SE_G), dim3(SE_GT), SE_G * (C + Cr) * sizeof(float), st, ws,
                     w1, b1, w2, b2, s, z, gate, g);
  if (res && relu) hipLaunchKernelGGL((se_scale_kernel<true, true>), grid, dim3(SE_T), 0, st, xb, rb, gate, yb, g);
  else if (res) hipLaunchKernelGGL((se_scale_kernel<true, false>), grid, dim3(SE_T), 0, st, xb, rb, gate, yb, g);
  else if (relu) hipLaunchKernelGGL((se_scale_kernel<false, true>), grid, dim3(SE_T), 0, st, xb, rb, gate, yb, g);
  else hipLaunchKernelGGL((se_scale_kernel<false, false>), grid, dim3(SE_T), 0, st, xb, rb, gate, yb, g);
  return 0;
}

// y: the forward's output, read for the ReLU mask (unused without relu); dres: bf16 like dx, or null (without ReLU
// dresidual is dy itself and is never written); dw1, db1, dw2, db2: fp32, all four or none.  Codes as the forward's.
DTM_API int dtm_se_bwd(const void* x, const void* y, const void* dy, const float* w1, const float* w2, const float* s,
                       const float* z, const float* gate, void* dx, void* dres, float* dw1, float* db1, float* dw2,
                       float* db2, float* ws, long ws_floats, int N, int HW, int C, int Cr, int slab_pixels, int relu,
                       void* stream) {
  SeGeom g;
  const int rc = make_geom(N, HW, C, Cr, slab_pixels, &g);
  if (rc) return rc;
  if (!x || !dy || !w1 || !w2 || !s || !z || !gate || !dx || !ws || (relu && !y) || (dres && !relu)) return -1;
  const bool wgrad = dw1 && db1 && dw2 && db2;
  if (!wgrad && (dw1 || db1 || dw2 || db2)) return -1;
  if (!aligned16(x) || !aligned16(y) || !aligned16(dy) || !aligned16(dx) || !aligned16(dres) || !aligned16(w1) ||
      !aligned16(gate) || !aligned16(ws))
    return -1;
  if (ws_floats < dtm_se_ws_floats(N, HW, C, Cr, slab_pixels, 1)) return -3;
  if (!gate_lds_ready()) return -4;
  float* da2 = ws + (size_t)N * g.slabs * C;  // (N * slabs * C and N * C are multiples of 8 floats: ds stays aligned)
  float* ds = da2 + (size_t)N * C;
  float* dz = ds + (size_t)N * C;
  const dim3 grid(g.slabs, N);
  hipStream_t st = (hipStream_t)stream;
  const bf16_t *xb = (const bf16_t*)x, *yb = (const bf16_t*)y, *dyb = (const bf16_t*)dy;
  bf16_t *dxb = (bf16_t*)dx, *drb = (bf16_t*)dres;
  if (relu) hipLaunchKernelGGL(se_bwd_sums_kernel<true>, grid, dim3(SE_T), 0, st, xb, yb, dyb, ws, g);
  else hipLaunchKernelGGL(se_bwd_sums_kernel<false>, grid, dim3(SE_T), 0, st, xb, yb, dyb, ws, g);
  const int lds = SE_G * (C + Cr) + SE_G * (SE_GT / Cr) * Cr;
  hipLaunchKernelGGL(se_gate_bwd_kernel, dim3((N + SE_G - 1) / SE_G), dim3(SE_GT), lds * sizeof(float), st, ws, w1, w2,
                     z, gate, da2, dz, ds, g);
  if (wgrad)
    hipLaunchKernelGGL(se_wgrad_kernel, dim3((C * Cr + SE_T - 1) / SE_T, 2), dim3(SE_T), 0, st, da2, dz, s, z, dw1,
                       db1, dw2, db2, N, C, Cr);
  const dim3 blk(SE_T);
  if (relu && dres)
    hipLaunchKernelGGL((se_bwd_apply_kernel<true, true>), grid, blk, 0, st, yb, dyb, gate, ds, dxb, drb, g);
  else if (relu)
    hipLaunchKernelGGL((se_bwd_apply_kernel<true, false>), grid, blk, 0, st, yb, dyb, gate, ds, dxb, drb, g);
  else
    hipLaunchKernelGGL((se_bwd_apply_kernel<false, false>), grid, blk, 0, st, yb, dyb, gate, ds, dxb, drb, g);
  return 0;
}
