// Grouped 3x3 convolution on the matrix units (NHWC bf16, fp32 master weights [C][3][3][D], D = C / groups input
// channels per filter; group g owns channels [gD, (g+1)D) of input AND output): forward, input gradient and weight
// gradient for D in {4, 8, 16, 32}, C % 16 == 0, stride 1 or 2, rate 1, top / left pad 0 or 1.  The op between the
// dense implicit GEMMs (conv_igemm.hip) and the depthwise VALU kernels (depthwise_tile.hip); it is bound by bytes
// (ResNeXt-50's 56x56x128 layer: 18 FLOP per activation byte), so the design is one read of the input, one write of
// the output, and v_mfma_f32_16x16x32_bf16 as cheap arithmetic even where most of it multiplies zeros.
//
// Columns.  The unit of work along channels is a column of 16 consecutive output channels = the 16 rows of one MFMA;
// one wave owns one column, a block of 4 waves a chunk of 64 channels (the tail chunk at C % 64 != 0 has 16 / 32 / 48
// and idles waves).  For D <= 16 a column is 16 / D whole groups and reads exactly its own 16 input channels: the
// 32-deep reduction of one MFMA is two taps x 16 channels (lane quarter fk = lane / 16 holds tap 2m + fk / 2,
// channels (fk & 1) * 8 .. + 7), 9 taps = 5 MFMAs with a zero tenth half.  For D = 32 a column is half a group and
// reads the group's 32 channels: one tap per MFMA, 9 MFMAs.  The weight operand is block-diagonal - (output channel,
// input channel) of different groups is zero - which wastes 75 % of the MFMA at D = 4 and 50 % at D = 8, on purpose.
//
// Weight fragments.  Every lane builds its 5 (9) fragments at block start straight from the fp32 master: one RNE
// rounding to bf16, zero off the diagonal, 20 (36) VGPRs for the block's life.  No host pack, no prep launch, no
// cached copy.
//
// gc_conv<D32, ST, TR> (forward; TR: dgrad at stride 1 = the same body over dy with the builder reading
//   w[k][2-r][2-s][c], the transpose within the group with flipped taps, and pad 2 - pad).  Block = one tile of TH x 16
//   output pixels (TH = 8 at stride 1, 4 at stride 2) x one chunk x one image.  The input halo tile goes to LDS once,
//   16-byte loads, zero where it is padding; pixel pitch = chunk bytes + 16 (144 B: the 16 pixels of one ds_read_b128
//   pass fall on 16 different bank quads at stride 1).  Weights are the MFMA's row operand, so a lane ends with 4
//   consecutive channels of one pixel: fp32 accumulation, one rounding, one 8-byte store.
// gc_dgrad2<D32> (dgrad at stride 2): tile = 8 x 32 dx pixels, origin shifted by (ph & 1, pw & 1); the 16 pixels of an
//   MFMA are one row's pixels of one column parity, and only the taps of that (row, column) parity class are issued
//   (4, 2, 2, 1 of the 9: again 5 / 9 fragments in all).  No dilated dy; every dx pixel is written, +0 where no
//   output reaches it.
// gc_wgrad<D32, ST>: dw[k][r][s][c] = sum_pixels dy[k] x[c]: per column and tap one 16 x 16 MFMA result over a 32-pixel
//   reduction (D = 32: two, for the halves of c), its diagonal blocks kept.  Both operands need 8 consecutive pixels
//   of one channel per lane, so x and dy tiles (TH x 32 outputs, TH = 4 / 2) are staged channel-major; at stride 2 x
//   is de-interleaved by column parity.  The three taps of a filter row come from one aligned 20-byte read shifted in
//   registers.  A wave keeps its 36 (72) accumulators over every tile the block walks; one partial row per block goes
//   to the stream's workspace and dtm_reduce_rows_det sums the rows in a fixed order: no atomics, bit-identical.
#include "common.h"

namespace dtm {

struct GcArgs {
  int N, H, W, C, D, P, Q, stride, ph, pw;
};

// one launch's geometry (host-built, block-uniform)
struct GcP {
  int IH, IW;        // image that is staged (forward: x; dgrad: dy)
  int OH, OW;        // image that is written
  int C, dsh;        // channels, log2(D)
  int ph, pw;        // gc_conv: output o, tap r reads staged row o * ST - ph + r; gc_dgrad2: the forward pads
  int TH, tiles_w;   // tile rows; tiles per image row
  int hrows, hcols;  // staged window, pixels
  FastDiv d_hcols;
};

struct GcWgP {
  int H, W, C, P, Q, dsh, ph, pw;
  int tiles_w, tiles, items;  // dy tile: TH x 32 pixels; tiles per image; N * tiles
  int width;                  // floats of dw = one workspace row
  FastDiv d_xcols, d_dycols;
};

__device__ __forceinline__ short8 as_s8(uint4 u) { return __builtin_bit_cast(short8, u); }

// 8 weights of row channel rc against the reduction channels kc0 .. kc0 + 7 at tap t (t < 0: none), bf16, zero where
// the two channels lie in different groups.  TR: rows are input channels (dgrad), w[kc][t][rc % D]
template <bool TR>
__device__ __forceinline__ short8 wfrag(const float* __restrict__ w, int dsh, int rc, int kc0, int t) {
  short8 f;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int kc = kc0 + e;
    float v = 0.f;
    if (t >= 0 && (rc >> dsh) == (kc >> dsh)) {
      const int dm = (1 << dsh) - 1;
      v = TR ? w[((long)(kc * 9 + t) << dsh) + (rc & dm)] : w[((long)(rc * 9 + t) << dsh) + (kc & dm)];
    }
    f[e] = (short)f2bf(v);
  }
  return f;
}

// Stage the [rows][cols] pixel window at (r0, c0) of one image, channels ch0 .. ch0 + cv * 8, pixel-major:
// lds[pixel * (cv + 1) + vector]; pixels outside the image are zero.
__device__ __forceinline__ void stage_halo(uint4* lds, const bf16_t* img, int IH, int IW, int C, int ch0, int cv,
                                           int r0, int c0, int rows, int cols, const FastDiv& d_cols) {
  const int total = rows * cols * 8;
  for (int i = threadIdx.x; i < total; i += 256) {
    const int pix = i >> 3, v = i & 7;
    if (v >= cv) continue;
    const int hr = (int)fdiv((uint32_t)pix, d_cols), hc = pix - hr * cols;
    const int h = r0 + hr, x = c0 + hc;
    uint4 val = make_uint4(0u, 0u, 0u, 0u);
    if ((unsigned)h < (unsigned)IH && (unsigned)x < (unsigned)IW)
      val = *(const uint4*)(img + ((long)h * IW + x) * C + ch0 + v * 8);
    lds[pix * (cv + 1) + v] = val;
  }
}

template <bool D32, int ST, bool TR>
__global__ __launch_bounds__(256) void gc_conv(const bf16_t* __restrict__ in, const float* __restrict__ w,
                                               bf16_t* __restrict__ out, GcP p) {
  extern __shared__ uint4 lds[];
  constexpr int NS = D32 ? 9 : 5;
  const int t = threadIdx.x, lane = t & 63, col = t >> 6, fr = lane & 15, fk = lane >> 4;
  const int ch0 = blockIdx.y * 64, CB = min(64, p.C - ch0), cv = CB >> 3, pv = cv + 1;
  const int n = blockIdx.z;
  const int tile_h = blockIdx.x / p.tiles_w, tile_w = blockIdx.x - tile_h * p.tiles_w;
  const int oh0 = tile_h * p.TH, ow0 = tile_w * 16;
  const bool live = col * 16 < CB;

  short8 wf[NS];
  int boff[NS];
  const int vofs = D32 ? (col >> 1) * 4 + fk : col * 2 + (fk & 1);
#pragma unroll
  for (int m = 0; m < NS; ++m) {
    const int tp = D32 ? m : 2 * m + (fk >> 1);  // position tap of this lane's half of the reduction
    const int tq = tp > 8 ? 8 : tp, r = tq / 3, s = tq - r * 3;
    boff[m] = (r * p.hcols + fr * ST + s) * pv + vofs;
    wf[m] = (short8){0, 0, 0, 0, 0, 0, 0, 0};
    if (live) wf[m] = wfrag<TR>(w, p.dsh, ch0 + col * 16 + fr, ch0 + vofs * 8, tp > 8 ? -1 : (TR ? 8 - tp : tp));
  }
  stage_halo(lds, in + (long)n * p.IH * p.IW * p.C, p.IH, p.IW, p.C, ch0, cv, oh0 * ST - p.ph, ow0 * ST - p.pw,
             p.hrows, p.hcols, p.d_hcols);
  __syncthreads();
  if (!live) return;
  const int ow = ow0 + fr;
  for (int ty = 0; ty < p.TH; ++ty) {
    const int oh = oh0 + ty;
    if (oh >= p.OH) break;
    const uint4* row = lds + ty * ST * p.hcols * pv;
    f32x4 acc = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int m = 0; m < NS; ++m) {
      uint4 b = row[boff[m]];
      if (!D32 && m == 4 && (fk >> 1)) b = make_uint4(0u, 0u, 0u, 0u);  // the tenth half-step
      acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[m], as_s8(b), acc, 0, 0, 0);
    }
    if (ow < p.OW)
      *(uint2*)(out + (((long)n * p.OH + oh) * p.OW + ow) * p.C + ch0 + col * 16 + fk * 4) =
          make_uint2(pack2bf(acc[0], acc[1]), pack2bf(acc[2], acc[3]));
  }
}

// dgrad at stride 2.  p.IH x p.IW is dy, p.OH x p.OW is dx.  Tile origin (oh0, ow0) = tile * (8, 32) - (ph & 1,
// pw & 1), so oh0 + ph and ow0 + pw are even: tile row ty is of row parity a = ty & 1 and needs the filter rows
// r = a (mod 2), pixel 2 * fr + b the taps s = b (mod 2).  dy window: rows (oh0 + ph) / 2 - 1 .. + 3, 17 columns from
// (ow0 + pw) / 2 - 1; dx row ty, tap r reads window row (ty - r) / 2 + 1, pixel 2j + b, tap s column j + (b - s) / 2 + 1.
// Fragment slots in class order (a, b) = (0,0) (0,1) (1,0) (1,1):
//   D <= 16: {0,2} {6,8} | {1,7} | {3,5} | {4,-}      D = 32: 0 2 6 8 | 1 7 | 3 5 | 4       (tap = 3r + s)
__device__ constexpr int DG2_TAP16[5][2] = {{0, 2}, {6, 8}, {1, 7}, {3, 5}, {4, -1}};
__device__ constexpr int DG2_TAP32[9] = {0, 2, 6, 8, 1, 7, 3, 5, 4};

template <bool D32>
__global__ __launch_bounds__(256) void gc_dgrad2(const bf16_t* __restrict__ dy, const float* __restrict__ w,
                                                 bf16_t* __restrict__ dx, GcP p) {
  extern __shared__ uint4 lds[];
  constexpr int NS = D32 ? 9 : 5;
  const int t = threadIdx.x, lane = t & 63, col = t >> 6, fr = lane & 15, fk = lane >> 4;
  const int ch0 = blockIdx.y * 64, CB = min(64, p.C - ch0), cv = CB >> 3, pv = cv + 1;
  const int n = blockIdx.z;
  const int tile_h = blockIdx.x / p.tiles_w, tile_w = blockIdx.x - tile_h * p.tiles_w;
  const int oh0 = tile_h * 8 - (p.ph & 1), ow0 = tile_w * 32 - (p.pw & 1);
  const bool live = col * 16 < CB;

  short8 wf[NS];
  int boff[NS];
  bool bzero[NS];
  const int vofs = D32 ? (col >> 1) * 4 + fk : col * 2 + (fk & 1);
#pragma unroll
  for (int m = 0; m < NS; ++m) {
    const int tp = D32 ? DG2_TAP32[m] : ((fk >> 1) ? DG2_TAP16[m][1] : DG2_TAP16[m][0]);
    const int tq = tp < 0 ? 4 : tp, r = tq / 3, s = tq - r * 3;
    // ((r & 1) - r) / 2 = -1 for r = 2, else 0
    boff[m] = ((1 - (r >> 1)) * 17 + fr + 1 - (s >> 1)) * pv + vofs;
    bzero[m] = tp < 0;
    wf[m] = (short8){0, 0, 0, 0, 0, 0, 0, 0};
    if (live) wf[m] = wfrag<true>(w, p.dsh, ch0 + col * 16 + fr, ch0 + vofs * 8, tp);
  }
  stage_halo(lds, dy + (long)n * p.IH * p.IW * p.C, p.IH, p.IW, p.C, ch0, cv, (oh0 + p.ph) / 2 - 1,
             (ow0 + p.pw) / 2 - 1, 5, 17, p.d_hcols);
  __syncthreads();
  if (!live) return;
  constexpr int S0[4] = {0, D32 ? 4 : 2, D32 ? 6 : 3, D32 ? 8 : 4};  // first slot of class a * 2 + b
  constexpr int S1[4] = {D32 ? 4 : 2, D32 ? 6 : 3, D32 ? 8 : 4, D32 ? 9 : 5};
  for (int tyh = 0; tyh < 4; ++tyh) {
    const uint4* row = lds + tyh * 17 * pv;
#pragma unroll
    for (int a = 0; a < 2; ++a) {
      const int oh = oh0 + 2 * tyh + a;
      if (oh < 0 || oh >= p.OH) continue;
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        f32x4 acc = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int m = S0[a * 2 + b]; m < S1[a * 2 + b]; ++m) {
          uint4 v = row[boff[m]];
          if (bzero[m]) v = make_uint4(0u, 0u, 0u, 0u);
          acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[m], as_s8(v), acc, 0, 0, 0);
        }
        const int ow = ow0 + 2 * fr + b;
        if (ow >= 0 && ow < p.OW)
          *(uint2*)(dx + (((long)n * p.OH + oh) * p.OW + ow) * p.C + ch0 + col * 16 + fk * 4) =
              make_uint2(pack2bf(acc[0], acc[1]), pack2bf(acc[2], acc[3]));
      }
    }
  }
}

// ---- weight gradient ----
// Channel-major LDS tiles of 2-byte elements: xs[channel][XCHP], dys[channel][DCHP].  Row pitch of x: 40 pixels
// (34 used at stride 1); at stride 2 a row is two parity planes of 40 (even window columns first: 33 + 32 used).  The
// channel pitches are odd multiples of 8 elements, so the 16 channels of one ds_read_b128 pass fall on 16 different
// bank quads.
template <int ST> struct WgGeom {
  static constexpr int TH = ST == 1 ? 4 : 2;
  static constexpr int XROWS = (TH - 1) * ST + 3, XCOLS = 31 * ST + 3;
  static constexpr int XROWP = ST == 1 ? 40 : 80;
  static constexpr int XCHP = (XROWS * XROWP / 8) % 2 ? XROWS * XROWP : XROWS * XROWP + 8;
  static constexpr int DCHP = TH * 32 + 8;
};

// Stage the [rows][cols] pixel window at (r0, c0) transposed: dst[channel * chp + hr * rowp + column slot], column
// slot = hc (DEINT: (hc & 1) * 40 + hc / 2); zero outside the image
template <bool DEINT>
__device__ __forceinline__ void stage_T(bf16_t* dst, const bf16_t* img, int IH, int IW, int C, int ch0, int cv, int r0,
                                        int c0, int rows, int cols, int rowp, int chp, const FastDiv& d_cols) {
  const int total = rows * cols * 8;
  for (int i = threadIdx.x; i < total; i += 256) {
    const int pix = i >> 3, v = i & 7;
    if (v >= cv) continue;
    const int hr = (int)fdiv((uint32_t)pix, d_cols), hc = pix - hr * cols;
    const int h = r0 + hr, x = c0 + hc;
    uint4 val = make_uint4(0u, 0u, 0u, 0u);
    if ((unsigned)h < (unsigned)IH && (unsigned)x < (unsigned)IW)
      val = *(const uint4*)(img + ((long)h * IW + x) * C + ch0 + v * 8);
    bf16_t* q = dst + v * 8 * chp + hr * rowp + (DEINT ? (hc & 1) * 40 + (hc >> 1) : hc);
    q[0] = (bf16_t)val.x; q[chp] = (bf16_t)(val.x >> 16);
    q[2 * chp] = (bf16_t)val.y; q[3 * chp] = (bf16_t)(val.y >> 16);
    q[4 * chp] = (bf16_t)val.z; q[5 * chp] = (bf16_t)(val.z >> 16);
    q[6 * chp] = (bf16_t)val.w; q[7 * chp] = (bf16_t)(val.w >> 16);
  }
}

template <bool D32, int ST>
__global__ __launch_bounds__(256) void gc_wgrad(const bf16_t* __restrict__ x, const bf16_t* __restrict__ dy,
                                                float* __restrict__ ws, GcWgP p) {
  extern __shared__ uint4 lds[];
  typedef WgGeom<ST> G;
  constexpr int NH = D32 ? 2 : 1;
  const int t = threadIdx.x, lane = t & 63, col = t >> 6, fr = lane & 15, fk = lane >> 4;
  const int ch0 = blockIdx.y * 64, CB = min(64, p.C - ch0), cv = CB >> 3;
  bf16_t* xs = (bf16_t*)lds;
  bf16_t* dys = xs + 64 * G::XCHP;
  const bool live = col * 16 < CB;
  f32x4 acc[NH][9];
#pragma unroll
  for (int h = 0; h < NH; ++h)
#pragma unroll
    for (int k = 0; k < 9; ++k) acc[h][k] = (f32x4){0.f, 0.f, 0.f, 0.f};

  for (int item = blockIdx.x; item < p.items; item += gridDim.x) {
    const int n = item / p.tiles, tl = item - n * p.tiles;
    const int tile_h = tl / p.tiles_w, tile_w = tl - tile_h * p.tiles_w;
    const int p0 = tile_h * G::TH, q0 = tile_w * 32;
    __syncthreads();  // the previous tile has been consumed
    stage_T<ST == 2>(xs, x + (long)n * p.H * p.W * p.C, p.H, p.W, p.C, ch0, cv, p0 * ST - p.ph, q0 * ST - p.pw,
                     G::XROWS, G::XCOLS, G::XROWP, G::XCHP, p.d_xcols);
    stage_T<false>(dys, dy + (long)n * p.P * p.Q * p.C, p.P, p.Q, p.C, ch0, cv, p0, q0, G::TH, 32, 32, G::DCHP,
                   p.d_dycols);
    __syncthreads();
    if (live) {
#pragma unroll
      for (int ty = 0; ty < G::TH; ++ty) {
        const short8 a = as_s8(*(const uint4*)(dys + (col * 16 + fr) * G::DCHP + ty * 32 + fk * 8));
#pragma unroll
        for (int h = 0; h < NH; ++h) {
          const int cl = D32 ? (col >> 1) * 32 + h * 16 + fr : col * 16 + fr;
#pragma unroll
          for (int r = 0; r < 3; ++r) {
            const bf16_t* q = xs + cl * G::XCHP + (ty * ST + r) * G::XROWP + fk * 8;
            const uint4 d = *(const uint4*)q;
            const uint32_t d4 = *(const uint32_t*)(q + 8);
            // elements 1 .. 8 of the aligned run
            const uint4 sh = make_uint4((d.x >> 16) | (d.y << 16), (d.y >> 16) | (d.z << 16),
                                        (d.z >> 16) | (d.w << 16), (d.w >> 16) | (d4 << 16));
            uint4 b1, b2;
            if (ST == 1) {
              b1 = sh;
              b2 = make_uint4(d.y, d.z, d.w, d4);
            } else {
              b1 = *(const uint4*)(q + 40);  // the odd plane
              b2 = sh;
            }
            acc[h][r * 3 + 0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, as_s8(d), acc[h][r * 3 + 0], 0, 0, 0);
            acc[h][r * 3 + 1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, as_s8(b1), acc[h][r * 3 + 1], 0, 0, 0);
            acc[h][r * 3 + 2] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, as_s8(b2), acc[h][r * 3 + 2], 0, 0, 0);
          }
        }
      }
    }
  }
  if (!live) return;
  // lane holds (output channel 4 * fk + j, input channel fr) of the column for each tap: keep the diagonal blocks
  float* out = ws + (size_t)blockIdx.x * p.width;
  const int dm = (1 << p.dsh) - 1;
#pragma unroll
  for (int h = 0; h < NH; ++h)
#pragma unroll
    for (int tap = 0; tap < 9; ++tap)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int kl = fk * 4 + j, k = ch0 + col * 16 + kl;
        if (D32) out[((size_t)(k * 9 + tap) << 5) + h * 16 + fr] = acc[h][tap][j];
        else if ((kl >> p.dsh) == (fr >> p.dsh)) out[((size_t)(k * 9 + tap) << p.dsh) + (fr & dm)] = acc[h][tap][j];
      }
}

}  // namespace dtm
using namespace dtm;

// (ops/groupconv.py's eligible)
static int gc_ok(const GcArgs& a) {
  const bool d = a.D == 4 || a.D == 8 || a.D == 16 || a.D == 32;
  return d && a.C >= 16 && a.C % 16 == 0 && a.C % a.D == 0 && (a.stride == 1 || a.stride == 2) && a.N >= 1 &&
         a.N <= 65535 && a.H >= 1 && a.W >= 1 && a.P >= 1 && a.Q >= 1 && (a.ph == 0 || a.ph == 1) &&
         (a.pw == 0 || a.pw == 1) && (long)a.C * 9 * a.D < 0x7fffffffL;
}
static bool gc_ptr_ok(const void* p) { return p && ((uintptr_t)p & 15) == 0; }
static int gc_dsh(int D) { return D == 4 ? 2 : D == 8 ? 3 : D == 16 ? 4 : 5; }
static size_t gc_halo_bytes(const GcP& p) {
  const int cv = (p.C < 64 ? p.C : 64) / 8;
  return (size_t)p.hrows * p.hcols * (cv + 1) * 16;
}

// x / dy -> y / dx through gc_conv: `in` is IH x IW, `out` OH x OW, pads of the correlation
template <bool TR>
static int gc_launch_conv(const void* in, const float* w, void* out, const GcArgs& a, int IH, int IW, int OH, int OW,
                          int st, int ph, int pw, hipStream_t s) {
  GcP p = {};
  p.IH = IH; p.IW = IW; p.OH = OH; p.OW = OW; p.C = a.C; p.dsh = gc_dsh(a.D); p.ph = ph; p.pw = pw;
  p.TH = st == 1 ? 8 : 4;
  p.hrows = (p.TH - 1) * st + 3;
  p.hcols = 15 * st + 3;
  p.d_hcols = make_fastdiv(p.hcols);
  p.tiles_w = (OW + 15) / 16;
  const long tiles = (long)((OH + p.TH - 1) / p.TH) * p.tiles_w;
  if (tiles > 0x7fffffffL) return -2;
  const dim3 g((unsigned)tiles, (a.C + 63) / 64, a.N);
  const size_t lds = gc_halo_bytes(p);
  const bf16_t* i = (const bf16_t*)in;
  bf16_t* o = (bf16_t*)out;
  if (a.D == 32) {
    if (st == 1) hipLaunchKernelGGL((gc_conv<true, 1, TR>), g, dim3(256), lds, s, i, w, o, p);
    else hipLaunchKernelGGL((gc_conv<true, 2, false>), g, dim3(256), lds, s, i, w, o, p);
  } else {
    if (st == 1) hipLaunchKernelGGL((gc_conv<false, 1, TR>), g, dim3(256), lds, s, i, w, o, p);
    else hipLaunchKernelGGL((gc_conv<false, 2, false>), g, dim3(256), lds, s, i, w, o, p);
  }
  return 0;
}

// w: fp32 [C][3][3][D].  Non-zero, and nothing launched, for an ineligible geometry or a null / misaligned pointer.
DTM_API int dtm_groupconv_fwd(const void* x, const float* w, void* y, const GcArgs* a, void* stream) {
  if (!a || !gc_ok(*a)) return -2;
  if (!gc_ptr_ok(x) || !gc_ptr_ok(w) || !gc_ptr_ok(y)) return -3;
  return gc_launch_conv<false>(x, w, y, *a, a->H, a->W, a->P, a->Q, a->stride, a->ph, a->pw, (hipStream_t)stream);
}

DTM_API int dtm_groupconv_dgrad(const void* dy, const float* w, void* dx, const GcArgs* a, void* stream) {
  if (!a || !gc_ok(*a)) return -2;
  if (!gc_ptr_ok(dy) || !gc_ptr_ok(w) || !gc_ptr_ok(dx)) return -3;
  hipStream_t s = (hipStream_t)stream;
  if (a->stride == 1)  // dx[h] = sum_r' dy[h - (2 - ph) + r'] * w[2 - r']
    return gc_launch_conv<true>(dy, w, dx, *a, a->P, a->Q, a->H, a->W, 1, 2 - a->ph, 2 - a->pw, s);
  GcP p = {};
  p.IH = a->P; p.IW = a->Q; p.OH = a->H; p.OW = a->W; p.C = a->C; p.dsh = gc_dsh(a->D); p.ph = a->ph; p.pw = a->pw;
  p.TH = 8; p.hrows = 5; p.hcols = 17;
  p.d_hcols = make_fastdiv(17);
  p.tiles_w = (p.OW + (a->pw & 1) + 31) / 32;
  const long tiles = (long)((p.OH + (a->ph & 1) + 7) / 8) * p.tiles_w;
  if (tiles > 0x7fffffffL) return -2;
  const dim3 g((unsigned)tiles, (a->C + 63) / 64, a->N);
  const size_t lds = gc_halo_bytes(p);
  if (a->D == 32) hipLaunchKernelGGL((gc_dgrad2<true>), g, dim3(256), lds, s, (const bf16_t*)dy, w, (bf16_t*)dx, p);
  else hipLaunchKernelGGL((gc_dgrad2<false>), g, dim3(256), lds, s, (const bf16_t*)dy, w, (bf16_t*)dx, p);
  return 0;
}

// dw (fp32, [C][3][3][D]) += gradient
DTM_API int dtm_groupconv_wgrad(const void* x, const void* dy, float* dw, const GcArgs* a, void* stream) {
  if (!a || !gc_ok(*a)) return -2;
  if (!gc_ptr_ok(x) || !gc_ptr_ok(dy) || !gc_ptr_ok(dw)) return -3;
  hipStream_t s = (hipStream_t)stream;
  const int ST = a->stride, TH = ST == 1 ? 4 : 2;
  GcWgP p = {};
  p.H = a->H; p.W = a->W; p.C = a->C; p.P = a->P; p.Q = a->Q; p.dsh = gc_dsh(a->D); p.ph = a->ph; p.pw = a->pw;
  p.tiles_w = (a->Q + 31) / 32;
  p.tiles = (a->P + TH - 1) / TH * p.tiles_w;
  const long items = (long)a->N * p.tiles;
  if (items > 0x7fffffffL) return -2;
  p.items = (int)items;
  p.width = a->C * 9 * a->D;
  p.d_xcols = make_fastdiv(31 * ST + 3);
  p.d_dycols = make_fastdiv(32);
  const int chunks = (a->C + 63) / 64;
  int G = 2 * dtm_compute_cus() / chunks;  // two resident blocks per CU over all chunks
  if (G < 1) G = 1;
  if (G > p.items) G = p.items;
  float* ws = dtm_ws_get_stream((size_t)G * p.width, s);
  if (!ws) return -4;
  const dim3 g(G, chunks);
  const bf16_t* xi = (const bf16_t*)x;
  const bf16_t* gi = (const bf16_t*)dy;
  if (ST == 1) {
    const size_t lds = (size_t)64 * (WgGeom<1>::XCHP + WgGeom<1>::DCHP) * 2;
    if (a->D == 32) hipLaunchKernelGGL((gc_wgrad<true, 1>), g, dim3(256), lds, s, xi, gi, ws, p);
    else hipLaunchKernelGGL((gc_wgrad<false, 1>), g, dim3(256), lds, s, xi, gi, ws, p);
  } else {
    const size_t lds = (size_t)64 * (WgGeom<2>::XCHP + WgGeom<2>::DCHP) * 2;
    if (a->D == 32) hipLaunchKernelGGL((gc_wgrad<true, 2>), g, dim3(256), lds, s, xi, gi, ws, p);
    else hipLaunchKernelGGL((gc_wgrad<false, 2>), g, dim3(256), lds, s, xi, gi, ws, p);
  }
  dtm_reduce_rows_det(ws, G, p.width, p.width, dw, s);
  return 0;
}
