// LDS-tiled depthwise 2-D convolution for depth multiplier 1 (NHWC bf16, fp32 weights [R][S][C][1]): forward, input
// gradient and weight gradient for ANY C % 8 == 0, R, S <= 7, stride 1 or 2, dilation 1.  The second depthwise family
// next to depthwise.hip: that file's dw_*8 kernels need 256 % (C/8) == 0 and re-read their operands once per tap
// through the caches; every other width fell to its scalar kernels.  Here every global input byte is fetched once per
// block (plus the halo overlap of neighbouring tiles) with 16-byte loads into LDS, zero-filled where it is padding or
// past the image, so the tap loops carry no bounds tests.  No reduction over channels: VALU work, no MFMA.
//
// Work split.  A lane owns one 8-channel column (16 B of bf16).  The C/8 columns are cut into `slabs` slabs of
// cpb = ceil(ncols / ceil(ncols / 8)) <= 8 columns (96 -> 2 x 6, 144 -> 3 x 6, 264 -> 5 x 7 with a tail of 5, 24 -> 3):
// balanced, so the tail slab idles few lanes; a lane whose column lies past C leaves after the staging.  A block is one
// image x one spatial tile x one slab (forward, dgrad), or one slab x a strided list of (image, tile) items (wgrad).
//
// LDS layout: [tile row][tile column][cpb] 16-byte vectors, row pitch padded.  The 256 lanes are ordered column
// fastest, then tile row: lanes t .. t + cpb - 1 read one contiguous cpb * 16 B run, the next cpb lanes the same run
// one tile row (x stride) further.  gfx950's LDS has 64 banks of 4 B and serves a 16-byte ds_read to 16 lanes per
// pass (256 B), so the pitch (in vectors) is padded until stride * pitch = cpb (mod 16) - for an odd cpb at stride 2,
// cpb + 1: the 16 / cpb runs of one pass then tile the 64 banks without overlap.  A power-of-two pitch (8 columns x 16
// pixels = 2 KiB) would put every tile row on the same banks.
// LDS budget: every launch stays under the 64 KiB default dynamic limit (3x3, 8 columns: 26 KiB forward at stride 1;
// at stride 2 the 8-row tile's 73 KiB become 40 KiB at 4 rows), so two to four blocks share a CU's 160 KiB and one
// block's staging overlaps another's arithmetic.  pick_tile() halves the tile height until the tile fits.
//
// dwt_conv<S, ST> (forward; dgrad at stride 1 = the same correlation over dy with the taps flipped as they are staged
//   and pad R-1-ph): tile = TH (8) output rows x TXS strips of 4 output pixels; lane = (column, row ty, strip tx).
//   Per filter row r the lane takes the S taps' weights (staged fp32 in LDS) into S*8 registers and slides along W: each
//   of the 3*ST+S input vectors of the row is read from LDS once and feeds every (output j, tap s) pair that uses it,
//   so the four neighbours share reads (3x3 stride 1: 6 reads for 12 tap uses).  fp32 accumulation in (r, s) order per
//   output, one RNE bf16 16-byte store per output pixel.
// dwt_dgrad2<S> (dgrad at stride 2): the tile origin is shifted by (ph & 1, pw & 1) so that tile row ty needs exactly
//   the filter rows r = ty & 1, ty & 1 + 2, ... (a loop start, not a test per tap) and strip pixel j the taps
//   s = j (mod 2), resolved at compile time.  The dy halo is (TH/2 + (R-1)/2) x (2*TXS + (S-1)/2) pixels.  An input
//   pixel that no output touches keeps its +0 accumulator.
// dwt_wgrad<S, ST>: lane = (column, filter row r, pixel lane u), U = 256 / (cpb * R) pixel lanes.  A lane keeps the
//   S*8 fp32 sums of ITS filter row in registers across every tile of the block (the filter rows are spread over lanes
//   instead of looped, so nothing is reduced between rows or tiles), walks the tile's 4-pixel dy strips u, u + U, ...
//   with the same sliding window over the x halo, and x and dy are read from global memory once.  At the end of the
//   block the U pixel lanes are summed in ascending order through LDS and the block writes its [R*S*slab] part of one
//   workspace row; dtm_reduce_rows_det (one row chunk, fixed order, no atomics - dtm_reduce_rows may split tall slabs
//   over atomically combined chunks) adds the G rows into dw.  Bit-identical run to run.
//
// Resource usage (hipcc -O3, gfx950, -Rpass-analysis=kernel-resource-usage); none of the 35 instantiations uses
// scratch, the largest is dwt_conv<7,2> (two blocks of 4 waves per CU need <= 256 VGPRs):
//   kernel                VGPRs  scratch   kernel                VGPRs  scratch
//   dwt_conv<3,1>             79      0    dwt_wgrad<3,1>            81      0
//   dwt_conv<3,2>             73      0    dwt_wgrad<3,2>            81      0
//   dwt_conv<7,2>            127      0    dwt_wgrad<7,2>           113      0
//   dwt_dgrad2<3>            70       0    dwt_dgrad2<7>            83       0
#include "nhwc8.h"

namespace dtm {

struct DwArgs {
  int N, H, W, C, M, R, S, P, Q, stride, ph, pw, dil;
};

// one staged window / one launch's geometry (host-built, block-uniform)
struct TileP {
  int IH, IW;         // image that is staged (forward: x; dgrad: dy)
  int OH, OW;         // image that is written
  int C, cpb, R;      // channels, columns per slab, filter rows (filter columns: template S)
  int ph, pw;         // output o, tap r reads input row o * ST - ph + r
  int TH, th_shift;   // tile rows (power of two), log2
  int TXS, tiles_w;   // 4-pixel strips per tile row; tiles per image row
  int hrows, hcols, pitch;  // staged window and its padded row pitch, in 16-byte vectors
  int flip;           // stage the taps reversed (dgrad at stride 1)
  FastDiv d_cpb, d_row;     // / cpb, / (hcols * cpb)
};

struct WgP {
  int H, W, C, P, Q, R, ph, pw, cpb;
  int TH, tiles_w, tiles, items;  // dy tile: TH x 16 pixels; tiles per image; N * tiles
  int xrows, xcols, xpitch;       // x halo
  int U;                          // pixel lanes
  FastDiv d_cpb, d_xrow, d_dyrow, d_R;
};

// Stage the [rows][wcols] pixel window at (r0, c0) of one image (IH x IW x C, channels ch0 .. ch0 + cb*8) into
// lds[row * pitch + col * cpb + column]; pixels outside the image are zero, columns >= cb are left alone (no lane
// reads them).  All 256 lanes take part: consecutive lanes load consecutive 16-byte vectors of a pixel's slab.
__device__ __forceinline__ void stage_window(uint4* lds, const bf16_t* img, int IH, int IW, int C, int ch0, int cb,
                                             int cpb, int r0, int c0, int rows, int wcols, int pitch,
                                             const FastDiv& d_cpb, const FastDiv& d_row) {
  const int rowlen = wcols * cpb, total = rows * rowlen;
  for (int i = threadIdx.x; i < total; i += 256) {
    const int hr = (int)fdiv((uint32_t)i, d_row), rem = i - hr * rowlen;
    const int hc = (int)fdiv((uint32_t)rem, d_cpb), cg = rem - hc * cpb;
    if (cg >= cb) continue;
    const int h = r0 + hr, w = c0 + hc;
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if ((unsigned)h < (unsigned)IH && (unsigned)w < (unsigned)IW)
      v = *(const uint4*)(img + ((long)h * IW + w) * C + ch0 + cg * 8);
    lds[hr * pitch + rem] = v;
  }
}

// fp32 taps of the slab -> wl[tap][cpb * 8] (zero for the columns past C), reversed when flip
__device__ __forceinline__ void stage_taps(float* wl, const float* __restrict__ w, int taps, int C, int ch0, int cb,
                                           int cpb, int flip, const FastDiv& d_cpb) {
  const int total = taps * cpb * 8;
  for (int i = threadIdx.x; i < total; i += 256) {
    const int v = i >> 3, tap = (int)fdiv((uint32_t)v, d_cpb), cg = v - tap * cpb;
    const int src = flip ? taps - 1 - tap : tap;
    wl[i] = cg < cb ? w[(long)src * C + ch0 + cg * 8 + (i & 7)] : 0.f;
  }
}

template <int S, int ST>
__global__ __launch_bounds__(256) void dwt_conv(const bf16_t* __restrict__ in, const float* __restrict__ w,
                                                bf16_t* __restrict__ out, TileP p) {
  extern __shared__ uint4 lds[];
  float* wl = (float*)(lds + p.hrows * p.pitch);
  const int t = threadIdx.x, cpb = p.cpb;
  const int tile_h = blockIdx.x / p.tiles_w, tile_w = blockIdx.x - tile_h * p.tiles_w;
  const int ch0 = blockIdx.y * cpb * 8, cb = min(cpb, p.C / 8 - (int)blockIdx.y * cpb), n = blockIdx.z;
  const int oh0 = tile_h * p.TH, ow0 = tile_w * p.TXS * 4;
  stage_window(lds, in + (long)n * p.IH * p.IW * p.C, p.IH, p.IW, p.C, ch0, cb, cpb, oh0 * ST - p.ph,
               ow0 * ST - p.pw, p.hrows, p.hcols, p.pitch, p.d_cpb, p.d_row);
  stage_taps(wl, w, p.R * S, p.C, ch0, cb, cpb, p.flip, p.d_cpb);
  __syncthreads();
  const int pl = (int)fdiv((uint32_t)t, p.d_cpb), cg = t - pl * cpb;
  const int ty = pl & (p.TH - 1), tx = pl >> p.th_shift;
  const int oh = oh0 + ty, ow = ow0 + tx * 4;
  if (cg >= cb || tx >= p.TXS || oh >= p.OH || ow >= p.OW) return;
  float acc[4][8];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[j][e] = 0.f;
  constexpr int KW = 3 * ST + S;  // input vectors of one filter row under the 4-pixel strip
  for (int r = 0; r < p.R; ++r) {
    float wr[S][8];
#pragma unroll
    for (int s = 0; s < S; ++s) {
      const f32x4* q = (const f32x4*)(wl + ((r * S + s) * cpb + cg) * 8);
      const f32x4 a = q[0], b = q[1];
      wr[s][0] = a.x; wr[s][1] = a.y; wr[s][2] = a.z; wr[s][3] = a.w;
      wr[s][4] = b.x; wr[s][5] = b.y; wr[s][6] = b.z; wr[s][7] = b.w;
    }
    const uint4* row = lds + (ty * ST + r) * p.pitch + tx * 4 * ST * cpb + cg;
#pragma unroll
    for (int k = 0; k < KW; ++k) {
      float xv[8];
      unpack8(row[k * cpb], xv);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int s = k - j * ST;  // (compile time)
        if (s >= 0 && s < S) {
#pragma unroll
          for (int e = 0; e < 8; ++e) acc[j][e] += xv[e] * wr[s][e];
        }
      }
    }
  }
  bf16_t* o = out + (((long)n * p.OH + oh) * p.OW + ow) * p.C + ch0 + cg * 8;
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (ow + j < p.OW) st8<true>(o, (long)j * p.C, acc[j]);
}

// dgrad at stride 2.  p.IH x p.IW is dy (P x Q), p.OH x p.OW is dx (H x W); p.ph / p.pw are the forward pads.
// Tile origin (oh0, ow0) = tile * (TH, 4 * TXS) - (ph & 1, pw & 1): oh0 + ph and ow0 + pw are even.
template <int S>
__global__ __launch_bounds__(256) void dwt_dgrad2(const bf16_t* __restrict__ dy, const float* __restrict__ w,
                                                  bf16_t* __restrict__ dx, TileP p) {
  extern __shared__ uint4 lds[];
  float* wl = (float*)(lds + p.hrows * p.pitch);
  const int t = threadIdx.x, cpb = p.cpb;
  const int tile_h = blockIdx.x / p.tiles_w, tile_w = blockIdx.x - tile_h * p.tiles_w;
  const int ch0 = blockIdx.y * cpb * 8, cb = min(cpb, p.C / 8 - (int)blockIdx.y * cpb), n = blockIdx.z;
  const int oh0 = tile_h * p.TH - (p.ph & 1), ow0 = tile_w * p.TXS * 4 - (p.pw & 1);
  constexpr int SH = (S - 1) / 2;
  const int RH = (p.R - 1) / 2;
  stage_window(lds, dy + (long)n * p.IH * p.IW * p.C, p.IH, p.IW, p.C, ch0, cb, cpb, (oh0 + p.ph) / 2 - RH,
               (ow0 + p.pw) / 2 - SH, p.hrows, p.hcols, p.pitch, p.d_cpb, p.d_row);
  stage_taps(wl, w, p.R * S, p.C, ch0, cb, cpb, 0, p.d_cpb);
  __syncthreads();
  const int pl = (int)fdiv((uint32_t)t, p.d_cpb), cg = t - pl * cpb;
  const int ty = pl & (p.TH - 1), tx = pl >> p.th_shift;
  const int oh = oh0 + ty, ow = ow0 + tx * 4;
  if (cg >= cb || tx >= p.TXS || oh < 0 || oh >= p.OH || ow >= p.OW) return;
  float acc[4][8];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[j][e] = 0.f;
  constexpr int KW = SH + 2;  // dy columns (ow + pw) / 2 - SH .. + 1 under the 4-pixel strip
  for (int r = ty & 1; r < p.R; r += 2) {
    float wr[S][8];
#pragma unroll
    for (int s = 0; s < S; ++s) {
      const f32x4* q = (const f32x4*)(wl + ((r * S + s) * cpb + cg) * 8);
      const f32x4 a = q[0], b = q[1];
      wr[s][0] = a.x; wr[s][1] = a.y; wr[s][2] = a.z; wr[s][3] = a.w;
      wr[s][4] = b.x; wr[s][5] = b.y; wr[s][6] = b.z; wr[s][7] = b.w;
    }
    const uint4* row = lds + (((ty - r) >> 1) + RH) * p.pitch + tx * 2 * cpb + cg;  // (ty - r is even)
#pragma unroll
    for (int k = 0; k < KW; ++k) {
      float g[8];
      unpack8(row[k * cpb], g);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
#pragma unroll
        for (int s = 0; s < S; ++s) {
          if (((j - s) & 1) == 0 && (j - s) / 2 == k - SH) {  // (compile time) q = (ow + pw + j - s) / 2
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[j][e] += g[e] * wr[s][e];
          }
        }
      }
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (ow + j >= 0 && ow + j < p.OW)
      st8<true>(dx, (((long)n * p.OH + oh) * p.OW + ow + j) * p.C + ch0 + cg * 8, acc[j]);
}

template <int S, int ST>
__global__ __launch_bounds__(256) void dwt_wgrad(const bf16_t* __restrict__ x, const bf16_t* __restrict__ dy,
                                                 float* __restrict__ ws, WgP p) {
  extern __shared__ uint4 lds[];
  uint4* dys = lds + p.xrows * p.xpitch;  // [TH][16][cpb]
  float* red = (float*)lds;               // [256][S * 8], after the last tile
  const int t = threadIdx.x, cpb = p.cpb;
  const int ch0 = blockIdx.y * cpb * 8, cb = min(cpb, p.C / 8 - (int)blockIdx.y * cpb);
  const int v = (int)fdiv((uint32_t)t, p.d_cpb), cg = t - v * cpb;
  const int u = (int)fdiv((uint32_t)v, p.d_R), r = v - u * p.R;
  const bool active = cg < cb && u < p.U;
  float acc[S][8];
#pragma unroll
  for (int s = 0; s < S; ++s)
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[s][e] = 0.f;
  constexpr int KW = 3 * ST + S;
  for (int item = blockIdx.x; item < p.items; item += gridDim.x) {
    const int n = item / p.tiles, tl = item - n * p.tiles;
    const int tile_h = tl / p.tiles_w, tile_w = tl - tile_h * p.tiles_w;
    const int p0 = tile_h * p.TH, q0 = tile_w * 16;
    __syncthreads();  // the previous tile has been consumed
    stage_window(lds, x + (long)n * p.H * p.W * p.C, p.H, p.W, p.C, ch0, cb, cpb, p0 * ST - p.ph, q0 * ST - p.pw,
                 p.xrows, p.xcols, p.xpitch, p.d_cpb, p.d_xrow);
    stage_window(dys, dy + (long)n * p.P * p.Q * p.C, p.P, p.Q, p.C, ch0, cb, cpb, p0, q0, p.TH, 16, 16 * cpb,
                 p.d_cpb, p.d_dyrow);
    __syncthreads();
    if (active) {
      for (int unit = u; unit < p.TH * 4; unit += p.U) {
        const int ty = unit >> 2, tx = unit & 3;
        float g[4][8];
        const uint4* gp = dys + (ty * 16 + tx * 4) * cpb + cg;
#pragma unroll
        for (int j = 0; j < 4; ++j) unpack8(gp[j * cpb], g[j]);
        const uint4* row = lds + (ty * ST + r) * p.xpitch + tx * 4 * ST * cpb + cg;
#pragma unroll
        for (int k = 0; k < KW; ++k) {
          float xv[8];
          unpack8(row[k * cpb], xv);
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int s = k - j * ST;  // (compile time)
            if (s >= 0 && s < S) {
#pragma unroll
              for (int e = 0; e < 8; ++e) acc[s][e] += xv[e] * g[j][e];
            }
          }
        }
      }
    }
  }
  __syncthreads();
#pragma unroll
  for (int s = 0; s < S; ++s)
#pragma unroll
    for (int e = 0; e < 8; ++e) red[t * (S * 8) + s * 8 + e] = acc[s][e];  // (idle lanes hold zeros)
  __syncthreads();
  // one partial row per block: sum the pixel lanes u = 0 .. U-1 in that order
  float* out = ws + (size_t)blockIdx.x * p.R * S * p.C;
  const int total = p.R * S * cpb * 8;
  for (int o = t; o < total; o += 256) {
    const int e = o & 7, vv = o >> 3;
    const int tap = (int)fdiv((uint32_t)vv, p.d_cpb), c = vv - tap * cpb;
    if (c >= cb) continue;
    const int rr = tap / S, s = tap - rr * S;
    float sum = 0.f;
    for (int k = 0; k < p.U; ++k) sum += red[((k * p.R + rr) * cpb + c) * (S * 8) + s * 8 + e];
    out[(size_t)tap * p.C + ch0 + c * 8 + e] = sum;
  }
}

}  // namespace dtm
using namespace dtm;

static bool tile_ok(const DwArgs& a) {
  return a.M == 1 && a.C >= 8 && a.C % 8 == 0 && a.R >= 1 && a.R <= 7 && a.S >= 1 && a.S <= 7 &&
         (a.stride == 1 || a.stride == 2) && a.dil == 1 && a.N >= 1 && a.N <= 65535 && a.H >= 1 && a.W >= 1 &&
         a.P >= 1 && a.Q >= 1 && a.ph >= 0 && a.pw >= 0;
}
static bool ptr_ok(const void* p) { return p && ((uintptr_t)p & 15) == 0; }

static int cols_per_block(int C) {
  const int ncols = C / 8, slabs = (ncols + 7) / 8;
  return (ncols + slabs - 1) / slabs;
}
// smallest pitch >= n (16-byte vectors) with stride * pitch = cpb (mod 16); odd cpb at stride 2: cpb + 1
static int pad_pitch(int n, int cpb, int st) {
  const int tgt = cpb + ((st == 2 && (cpb & 1)) ? 1 : 0);
  while ((st * n - tgt) % 16 != 0) ++n;
  return n;
}
constexpr size_t LDS_MAX = 64 * 1024;

// tile of dwt_conv / dwt_dgrad2 for an OH x OW output: 0 when nothing fits (cannot happen for R, S <= 7)
static size_t pick_tile(TileP& p, int S, int st, bool dgrad2) {
  const int PL = 256 / p.cpb;
  int TH = 8, TXS = PL / TH;
  if (TXS > 8) TXS = 8;
  const int need = (p.OW + (dgrad2 ? 1 : 0) + 3) / 4;
  if (TXS > need) TXS = need;
  for (;; TH /= 2) {
    if (TH < 2) return 0;
    p.hrows = dgrad2 ? TH / 2 + (p.R - 1) / 2 : (TH - 1) * st + p.R;
    p.hcols = dgrad2 ? TXS * 2 + (S - 1) / 2 : (TXS * 4 - 1) * st + S;
    p.pitch = pad_pitch(p.hcols * p.cpb, p.cpb, dgrad2 ? 1 : st);
    const size_t bytes = (size_t)p.hrows * p.pitch * 16 + (size_t)p.R * S * p.cpb * 32;
    if (bytes <= LDS_MAX) {
      p.TH = TH;
      p.th_shift = TH == 8 ? 3 : (TH == 4 ? 2 : 1);
      p.TXS = TXS;
      p.d_cpb = make_fastdiv(p.cpb);
      p.d_row = make_fastdiv(p.hcols * p.cpb);
      return bytes;
    }
  }
}

template <int ST>
static void launch_conv(int S, dim3 g, size_t lds, hipStream_t st, const bf16_t* in, const float* w, bf16_t* out,
                        const TileP& p) {
#define DWT_CASE(S_) \
  case S_: hipLaunchKernelGGL((dwt_conv<S_, ST>), g, dim3(256), lds, st, in, w, out, p); break;
  switch (S) { DWT_CASE(1) DWT_CASE(2) DWT_CASE(3) DWT_CASE(4) DWT_CASE(5) DWT_CASE(6) DWT_CASE(7) }
#undef DWT_CASE
}
static void launch_dgrad2(int S, dim3 g, size_t lds, hipStream_t st, const bf16_t* dy, const float* w, bf16_t* dx,
                          const TileP& p) {
#define DWT_CASE(S_) \
  case S_: hipLaunchKernelGGL((dwt_dgrad2<S_>), g, dim3(256), lds, st, dy, w, dx, p); break;
  switch (S) { DWT_CASE(1) DWT_CASE(2) DWT_CASE(3) DWT_CASE(4) DWT_CASE(5) DWT_CASE(6) DWT_CASE(7) }
#undef DWT_CASE
}
template <int ST>
static void launch_wgrad(int S, dim3 g, size_t lds, hipStream_t st, const bf16_t* x, const bf16_t* dy, float* ws,
                         const WgP& p) {
#define DWT_CASE(S_) \
  case S_: hipLaunchKernelGGL((dwt_wgrad<S_, ST>), g, dim3(256), lds, st, x, dy, ws, p); break;
  switch (S) { DWT_CASE(1) DWT_CASE(2) DWT_CASE(3) DWT_CASE(4) DWT_CASE(5) DWT_CASE(6) DWT_CASE(7) }
#undef DWT_CASE
}

// (tile_ok is ops/depthwise.py's tile_eligible)  w: fp32 [R][S][C][1].  Non-zero, and nothing launched, for an ineligible geometry or a null / misaligned pointer.
DTM_API int dtm_depthwise_tile_fwd(const void* x, const float* w, void* y, const DwArgs* a, void* stream) {
  if (!a || !tile_ok(*a)) return -2;
  if (!ptr_ok(x) || !ptr_ok(w) || !ptr_ok(y)) return -3;
  TileP p = {};
  p.IH = a->H; p.IW = a->W; p.OH = a->P; p.OW = a->Q;
  p.C = a->C; p.cpb = cols_per_block(a->C); p.R = a->R; p.ph = a->ph; p.pw = a->pw;
  const size_t lds = pick_tile(p, a->S, a->stride, false);
  if (!lds) return -2;
  p.tiles_w = (p.OW + p.TXS * 4 - 1) / (p.TXS * 4);
  const int tiles_h = (p.OH + p.TH - 1) / p.TH, slabs = (a->C / 8 + p.cpb - 1) / p.cpb;
  const dim3 g(tiles_h * p.tiles_w, slabs, a->N);
  if (a->stride == 1) launch_conv<1>(a->S, g, lds, (hipStream_t)stream, (const bf16_t*)x, w, (bf16_t*)y, p);
  else launch_conv<2>(a->S, g, lds, (hipStream_t)stream, (const bf16_t*)x, w, (bf16_t*)y, p);
  return 0;
}

DTM_API int dtm_depthwise_tile_dgrad(const void* dy, const float* w, void* dx, const DwArgs* a, void* stream) {
  if (!a || !tile_ok(*a)) return -2;
  if (!ptr_ok(dy) || !ptr_ok(w) || !ptr_ok(dx)) return -3;
  TileP p = {};
  p.IH = a->P; p.IW = a->Q; p.OH = a->H; p.OW = a->W;
  p.C = a->C; p.cpb = cols_per_block(a->C); p.R = a->R;
  const int slabs = (a->C / 8 + p.cpb - 1) / p.cpb;
  if (a->stride == 1) {
    // dx[h] = sum_r' dy[h - (R-1-ph) + r'] * w[R-1-r']: the forward kernel over dy with flipped taps
    p.ph = a->R - 1 - a->ph; p.pw = a->S - 1 - a->pw; p.flip = 1;
    const size_t lds = pick_tile(p, a->S, 1, false);
    if (!lds) return -2;
    p.tiles_w = (p.OW + p.TXS * 4 - 1) / (p.TXS * 4);
    const dim3 g((p.OH + p.TH - 1) / p.TH * p.tiles_w, slabs, a->N);
    launch_conv<1>(a->S, g, lds, (hipStream_t)stream, (const bf16_t*)dy, w, (bf16_t*)dx, p);
  } else {
    p.ph = a->ph; p.pw = a->pw;
    const size_t lds = pick_tile(p, a->S, 2, true);
    if (!lds) return -2;
    p.tiles_w = (p.OW + (a->pw & 1) + p.TXS * 4 - 1) / (p.TXS * 4);
    const dim3 g((p.OH + (a->ph & 1) + p.TH - 1) / p.TH * p.tiles_w, slabs, a->N);
    launch_dgrad2(a->S, g, lds, (hipStream_t)stream, (const bf16_t*)dy, w, (bf16_t*)dx, p);
  }
  return 0;
}

// dw (fp32, [R][S][C][1]) += gradient
DTM_API int dtm_depthwise_tile_wgrad(const void* x, const void* dy, float* dw, const DwArgs* a, void* stream) {
  if (!a || !tile_ok(*a)) return -2;
  if (!ptr_ok(x) || !ptr_ok(dy) || !ptr_ok(dw)) return -3;
  hipStream_t st = (hipStream_t)stream;
  const int S = a->S, ST = a->stride;
  WgP p = {};
  p.H = a->H; p.W = a->W; p.C = a->C; p.P = a->P; p.Q = a->Q; p.R = a->R; p.ph = a->ph; p.pw = a->pw;
  p.cpb = cols_per_block(a->C);
  p.U = 256 / (p.cpb * p.R);
  p.xcols = 15 * ST + S;
  p.xpitch = pad_pitch(p.xcols * p.cpb, p.cpb, 1);
  const size_t red_bytes = (size_t)256 * S * 32;
  size_t lds = 0;
  for (p.TH = 8;; p.TH /= 2) {
    if (p.TH < 1) return -2;
    p.xrows = (p.TH - 1) * ST + p.R;
    lds = ((size_t)p.xrows * p.xpitch + (size_t)p.TH * 16 * p.cpb) * 16;
    if (lds <= LDS_MAX) break;
  }
  if (lds < red_bytes) lds = red_bytes;
  p.tiles_w = (p.Q + 15) / 16;
  p.tiles = (p.P + p.TH - 1) / p.TH * p.tiles_w;
  const long items = (long)a->N * p.tiles;
  if (items > 0x7fffffffL) return -2;
  p.items = (int)items;
  p.d_cpb = make_fastdiv(p.cpb);
  p.d_xrow = make_fastdiv(p.xcols * p.cpb);
  p.d_dyrow = make_fastdiv(16 * p.cpb);
  p.d_R = make_fastdiv(p.R);
  const int slabs = (a->C / 8 + p.cpb - 1) / p.cpb;
  int G = 2 * dtm_compute_cus() / slabs;  // two resident blocks per CU over all slabs
  if (G < 1) G = 1;
  if (G > p.items) G = p.items;
  const int width = a->R * S * a->C;
  float* ws = dtm_ws_get_stream((size_t)G * width, st);
  if (!ws) return -4;
  const dim3 g(G, slabs);
  if (ST == 1) launch_wgrad<1>(S, g, lds, st, (const bf16_t*)x, (const bf16_t*)dy, ws, p);
  else launch_wgrad<2>(S, g, lds, st, (const bf16_t*)x, (const bf16_t*)dy, ws, p);
  dtm_reduce_rows_det(ws, G, width, width, dw, st);
  return 0;
}
