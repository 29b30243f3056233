// RandAugment on uint8 NHWC batches (ops/randaugment.py holds the definitions and their numpy form, the bit-for-bit
// oracle of this file).  A plan is int32[B][N][12]: per image and layer
//   [op, i0, i1, i2, i3, bits(f0) .. bits(f5), fill]          (fill = r | g<<8 | b<<16)
// and the layers are applied in order.  The op is data, so every image of a batch can run another op.
//
// dtm_randaugment issues, in stream order and with no host decision in between, one memset of the histogram scratch
// and, per layer, two launches:
//   ra_stats_kernel   blocks of an image whose op needs no statistics exit at once (grid.y is the image: the op is
//                     uniform per block).  The others count r, g, b (AutoContrast, Equalize) or grey (Contrast) of the
//                     layer's INPUT in per-wave LDS histograms (LDS integer atomics) and add their non-empty bins to
//                     the image's global bins with integer atomics: the sums do not depend on the arrival order, so
//                     the result is bit-identical from run to run (the arrangement of summary.hip).
//   ra_apply_kernel   a block forms what its op needs once in LDS (the three 256-entry LUTs of ops 0 to 6, Contrast's
//                     mean from the grey histogram), then writes its pixels.  Layer l reads what layer l - 1 wrote
//                     (two uint8 ping-pong buffers); layer 0 reads the source, quantising a float source on read; the
//                     last layer writes the destination kind itself.
// Memory-bound: 3 B read per pixel in a stats pass that runs, 3 B read + 3 B written per inner layer.
//
// A thread handles units of 4 pixels = 12 elements.  The image bases may sit at any element of a larger buffer
// (rows of 299 x 299 x 3 make them odd): where an image's base is 4-byte aligned the 12 elements move as one 12-, 24-
// or 48-byte access, otherwise element by element; the unit's values are the same either way.
// Every fp32 / fp64 operation of the definitions is rounded on its own: contraction is off for the whole file.
#include "common.h"

#pragma clang fp contract(off)

namespace dtm {

enum { RA_IDENTITY = 0, RA_AUTOCONTRAST, RA_EQUALIZE, RA_INVERT, RA_POSTERIZE, RA_SOLARIZE, RA_SOLARIZE_ADD, RA_COLOR,
       RA_CONTRAST, RA_BRIGHTNESS, RA_SHARPNESS, RA_AFFINE, RA_CUTOUT };
enum { RA_U8 = 0, RA_F32 = 1, RA_BF16 = 2 };
constexpr int RA_REC = 12;

template <int K> struct RaElem;
template <> struct RaElem<RA_U8> { using T = uint8_t; };
template <> struct RaElem<RA_F32> { using T = float; };
template <> struct RaElem<RA_BF16> { using T = bf16_t; };

template <typename T>
struct alignas(4) RaPack {  // 12 elements: 12, 24 or 48 bytes
  T v[12];
};

struct RaArgs {
  const void* in;        // the layer's input batch
  void* out;             // the layer's output batch
  const int* plan;       // [B][N][12]
  uint32_t* hist;        // this layer's [B][4][256] bins: r, g, b, grey
  int B, H, W, N, layer;
  uint32_t npix;         // H * W < 2^31
  FastDiv dw;            // / W
  float in_scale, in_shift, out_scale, out_shift;
};

// a source element as the byte layer 0 reads: rint(min(max((y * s + b) * 255, 0), 255)), a NaN reads as 0
__device__ __forceinline__ uint32_t ra_quant(float y, float s, float b) {
  float t = y * s;
  t = t + b;
  t = t * 255.f;
  t = t > 0.f ? t : 0.f;
  t = t < 255.f ? t : 255.f;
  return (uint32_t)rintf(t);
}

template <int K>
__device__ __forceinline__ uint32_t ra_in(typename RaElem<K>::T e, float s, float b) {
  if constexpr (K == RA_U8) return e;
  else if constexpr (K == RA_F32) return ra_quant(e, s, b);
  else return ra_quant(bf2f(e), s, b);
}

template <int K>
__device__ __forceinline__ typename RaElem<K>::T ra_out(uint32_t v, float s, float b) {
  if constexpr (K == RA_U8) {
    return (uint8_t)v;
  } else {
    float t = (float)v * s;
    t = t + b;
    if constexpr (K == RA_F32) return t;
    else return f2bf(t);
  }
}

// elements [e0, e0 + cnt) of an image as bytes (cnt <= 12; the rest reads as 0)
template <int K>
__device__ __forceinline__ void ra_load12(const typename RaElem<K>::T* img, size_t e0, int cnt, bool wide, float s,
                                          float b, uint32_t* v) {
  using T = typename RaElem<K>::T;
  if (wide && cnt == 12) {
    const RaPack<T> pk = *reinterpret_cast<const RaPack<T>*>(img + e0);
#pragma unroll
    for (int j = 0; j < 12; ++j) v[j] = ra_in<K>(pk.v[j], s, b);
  } else {
#pragma unroll
    for (int j = 0; j < 12; ++j) v[j] = j < cnt ? ra_in<K>(img[e0 + j], s, b) : 0u;
  }
}

template <int K>
__device__ __forceinline__ void ra_store12(typename RaElem<K>::T* img, size_t e0, int cnt, bool wide, float s, float b,
                                           const uint32_t* r) {
  using T = typename RaElem<K>::T;
  if (wide && cnt == 12) {
    RaPack<T> pk;
#pragma unroll
    for (int j = 0; j < 12; ++j) pk.v[j] = ra_out<K>(r[j], s, b);
    *reinterpret_cast<RaPack<T>*>(img + e0) = pk;
  } else {
#pragma unroll
    for (int j = 0; j < 12; ++j)
      if (j < cnt) img[e0 + j] = ra_out<K>(r[j], s, b);
  }
}

__device__ __forceinline__ uint32_t ra_grey(uint32_t r, uint32_t g, uint32_t b) {
  return (19595u * r + 38470u * g + 7471u * b + 32768u) >> 16;
}

// a + f * (b - a) with three roundings; 0 if t <= 0, 255 if t >= 255, else truncated
__device__ __forceinline__ uint32_t ra_blend(uint32_t a, uint32_t b, float f) {
  const float fa = (float)a;
  float t = (float)b - fa;
  t = f * t;
  t = fa + t;
  return t <= 0.f ? 0u : t >= 255.f ? 255u : (uint32_t)t;
}

__device__ __forceinline__ bool ra_needs_stats(int op) {
  return op == RA_AUTOCONTRAST || op == RA_EQUALIZE || op == RA_CONTRAST;
}

// grid (blocks per image, images)
template <int IK>
__global__ __launch_bounds__(256) void ra_stats_kernel(RaArgs a) {
  using TI = typename RaElem<IK>::T;
  __shared__ uint32_t hist[4][3][256];  // one histogram set per wave: fewer lanes collide on a narrow image
  const int tid = threadIdx.x, wave = tid >> 6;
  const size_t n = (size_t)a.npix * 3;
  const uint32_t nunits = (a.npix + 3u) >> 2;
  for (int b = blockIdx.y; b < a.B; b += gridDim.y) {
    const int op = a.plan[((size_t)b * a.N + a.layer) * RA_REC];
    if (!ra_needs_stats(op)) continue;
    __syncthreads();  // the histograms of the previous image have been read
    for (int i = tid; i < 4 * 3 * 256; i += 256) (&hist[0][0][0])[i] = 0u;
    __syncthreads();
    const TI* img = (const TI*)a.in + (size_t)b * n;
    const bool wide = ((uintptr_t)img & 3u) == 0;
    const bool grey = op == RA_CONTRAST;
    for (uint32_t u = blockIdx.x * 256u + tid; u < nunits; u += gridDim.x * 256u) {
      const uint32_t p0 = u * 4u;
      const int cntp = (int)(a.npix - p0 < 4u ? a.npix - p0 : 4u);
      uint32_t v[12];
      ra_load12<IK>(img, (size_t)p0 * 3, cntp * 3, wide, a.in_scale, a.in_shift, v);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (j < cntp) {
          if (grey) {
            atomicAdd(&hist[wave][0][ra_grey(v[3 * j], v[3 * j + 1], v[3 * j + 2])], 1u);
          } else {
            atomicAdd(&hist[wave][0][v[3 * j]], 1u);
            atomicAdd(&hist[wave][1][v[3 * j + 1]], 1u);
            atomicAdd(&hist[wave][2][v[3 * j + 2]], 1u);
          }
        }
      }
    }
    __syncthreads();
    uint32_t* gb = a.hist + (size_t)b * 4 * 256;
    for (int c = 0; c < (grey ? 1 : 3); ++c) {
      const uint32_t h = hist[0][c][tid] + hist[1][c][tid] + hist[2][c][tid] + hist[3][c][tid];
      if (h) atomicAdd(&gb[(grey ? 3 : c) * 256 + tid], h);
    }
  }
}

// grid (blocks per image, images)
template <int IK, int OK>
__global__ __launch_bounds__(256) void ra_apply_kernel(RaArgs a) {
  using TI = typename RaElem<IK>::T;
  using TO = typename RaElem<OK>::T;
  __shared__ uint32_t sa[3][256], sb[3][256];  // the prefix sums of Equalize
  __shared__ uint8_t lut[3][256];
  __shared__ int lo[3], hi[3];
  __shared__ unsigned long long gsum;
  const int tid = threadIdx.x;
  const size_t n = (size_t)a.npix * 3;
  const uint32_t nunits = (a.npix + 3u) >> 2;
  const int H = a.H, W = a.W;
  for (int b = blockIdx.y; b < a.B; b += gridDim.y) {
    // the record: the same addresses in every lane
    const int* rec = a.plan + ((size_t)b * a.N + a.layer) * RA_REC;
    const int op = rec[0];
    const int i0 = rec[1], i1 = rec[2], i2 = rec[3], i3 = rec[4];
    const float f0 = __int_as_float(rec[5]);
    const uint32_t fillw = (uint32_t)rec[11];
    const uint32_t fill[3] = {fillw & 255u, (fillw >> 8) & 255u, (fillw >> 16) & 255u};
    const uint32_t* gh = a.hist + (size_t)b * 4 * 256;
    uint32_t mean = 0u;

    __syncthreads();  // the LDS tables of the previous image have been read
    if (op == RA_AUTOCONTRAST || op == RA_EQUALIZE) {
      uint32_t h[3];
      if (tid < 3) { lo[tid] = 256; hi[tid] = -1; }
#pragma unroll
      for (int c = 0; c < 3; ++c) { h[c] = gh[c * 256 + tid]; sa[c][tid] = h[c]; }
      __syncthreads();
#pragma unroll
      for (int c = 0; c < 3; ++c)
        if (h[c]) { atomicMin(&lo[c], tid); atomicMax(&hi[c], tid); }
      uint32_t (*src)[256] = sa, (*dst)[256] = sb;
      if (op == RA_EQUALIZE) {  // inclusive prefix sums (8 steps: the result is back in sa)
        for (int d = 1; d < 256; d <<= 1) {
#pragma unroll
          for (int c = 0; c < 3; ++c) dst[c][tid] = src[c][tid] + (tid >= d ? src[c][tid - d] : 0u);
          __syncthreads();
          uint32_t (*t)[256] = src; src = dst; dst = t;
        }
      }
      __syncthreads();
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const int l = lo[c], hh = hi[c];
        uint32_t r = (uint32_t)tid;
        if (hh > l) {
          if (op == RA_AUTOCONTRAST) {
            const double scale = 255.0 / (double)(hh - l);
            const double offset = -(double)l * scale;
            double val = (double)tid * scale;
            val = val + offset;
            r = val < 0.0 ? 0u : val > 255.0 ? 255u : (uint32_t)val;
          } else {
            const uint32_t step = (a.npix - gh[c * 256 + hh]) / 255u;
            if (step) {
              const uint32_t q = (step / 2u + (src[c][tid] - h[c])) / step;
              r = q < 255u ? q : 255u;
            }
          }
        }
        lut[c][tid] = (uint8_t)r;
      }
    } else if (op <= RA_SOLARIZE_ADD) {
      const uint32_t v = (uint32_t)tid;
      uint32_t r = v;
      if (op == RA_INVERT) r = 255u - v;
      else if (op == RA_POSTERIZE) r = v & ~((1u << (8 - i0)) - 1u) & 255u;
      else if (op == RA_SOLARIZE) r = (int)v < i0 ? v : 255u - v;
      else if (op == RA_SOLARIZE_ADD) r = v < 128u ? (v + (uint32_t)i0 < 255u ? v + (uint32_t)i0 : 255u) : v;
      lut[0][tid] = lut[1][tid] = lut[2][tid] = (uint8_t)r;
    } else if (op == RA_CONTRAST) {
      if (tid == 0) gsum = 0ull;
      __syncthreads();
      const unsigned long long part = (unsigned long long)tid * gh[3 * 256 + tid];
      if (part) atomicAdd(&gsum, part);  // an integer sum: the order does not matter
      __syncthreads();
      mean = (uint32_t)((2ull * gsum + a.npix) / (2ull * a.npix));
    }
    __syncthreads();

    const TI* in = (const TI*)a.in + (size_t)b * n;
    TO* out = (TO*)a.out + (size_t)b * n;
    const bool wide_in = ((uintptr_t)in & 3u) == 0, wide_out = ((uintptr_t)out & 3u) == 0;
    const float is = a.in_scale, ib = a.in_shift;
    float m[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) m[k] = __int_as_float(rec[5 + k]);
    const float fW = (float)W, fH = (float)H;

    for (uint32_t u = blockIdx.x * 256u + tid; u < nunits; u += gridDim.x * 256u) {
      const uint32_t p0 = u * 4u;
      const int cntp = (int)(a.npix - p0 < 4u ? a.npix - p0 : 4u);
      const size_t e0 = (size_t)p0 * 3;
      uint32_t v[12], r[12];
      if (op != RA_AFFINE) ra_load12<IK>(in, e0, cntp * 3, wide_in, is, ib, v);
      if (op <= RA_SOLARIZE_ADD) {
#pragma unroll
        for (int j = 0; j < 12; ++j) r[j] = lut[j % 3][v[j]];
      } else if (op == RA_COLOR) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const uint32_t g = ra_grey(v[3 * j], v[3 * j + 1], v[3 * j + 2]);
#pragma unroll
          for (int c = 0; c < 3; ++c) r[3 * j + c] = ra_blend(g, v[3 * j + c], f0);
        }
      } else if (op == RA_CONTRAST || op == RA_BRIGHTNESS) {
#pragma unroll
        for (int j = 0; j < 12; ++j) r[j] = ra_blend(mean, v[j], f0);  // (Brightness: mean is 0)
      } else {  // the ops that need the pixel's position
        uint32_t y = fdiv(p0, a.dw);
        uint32_t x = p0 - y * (uint32_t)W;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (j < cntp) {
            if (op == RA_SHARPNESS) {
              const bool border = y == 0u || x == 0u || y == (uint32_t)H - 1u || x == (uint32_t)W - 1u;
#pragma unroll
              for (int c = 0; c < 3; ++c) {
                uint32_t d = v[3 * j + c];
                if (!border) {
                  uint32_t s = 4u * d;
                  for (int dy = -1; dy <= 1; ++dy)
                    for (int dx = -1; dx <= 1; ++dx)
                      s += ra_in<IK>(in[((size_t)(y + dy) * W + (x + dx)) * 3 + c], is, ib);
                  d = (s + 6u) / 13u;
                }
                r[3 * j + c] = ra_blend(d, v[3 * j + c], f0);
              }
            } else if (op == RA_AFFINE) {
              const float xf = (float)x + 0.5f, yf = (float)y + 0.5f;
              float xin = m[0] * xf, t = m[1] * yf;
              xin = xin + t;
              xin = xin + m[2];
              float yin = m[3] * xf;
              t = m[4] * yf;
              yin = yin + t;
              yin = yin + m[5];
              // tested on the floats, before any conversion: false for a NaN and for any magnitude
              const bool ok = xin >= 0.f && xin < fW && yin >= 0.f && yin < fH;
              if (ok) {
                int xi = (int)xin, yi = (int)yin;
                xi = xi < W - 1 ? xi : W - 1;  // (float(W) can round up past 2^24)
                yi = yi < H - 1 ? yi : H - 1;
                const size_t e = ((size_t)yi * W + xi) * 3;
#pragma unroll
                for (int c = 0; c < 3; ++c) r[3 * j + c] = ra_in<IK>(in[e + c], is, ib);
              } else {
#pragma unroll
                for (int c = 0; c < 3; ++c) r[3 * j + c] = fill[c];
              }
            } else {  // RA_CUTOUT
              const bool inside = (int)y >= i0 && (int)y < i1 && (int)x >= i2 && (int)x < i3;
#pragma unroll
              for (int c = 0; c < 3; ++c) r[3 * j + c] = inside ? fill[c] : v[3 * j + c];
            }
          }
          if (++x == (uint32_t)W) { x = 0u; ++y; }
        }
      }
      ra_store12<OK>(out, e0, cntp * 3, wide_out, a.out_scale, a.out_shift, r);
    }
  }
}

template <int IK>
static void ra_launch_apply(int ok, dim3 grid, hipStream_t st, const RaArgs& a) {
  if (ok == RA_U8) hipLaunchKernelGGL((ra_apply_kernel<IK, RA_U8>), grid, dim3(256), 0, st, a);
  else if (ok == RA_F32) hipLaunchKernelGGL((ra_apply_kernel<IK, RA_F32>), grid, dim3(256), 0, st, a);
  else hipLaunchKernelGGL((ra_apply_kernel<IK, RA_BF16>), grid, dim3(256), 0, st, a);
}

}  // namespace dtm
using namespace dtm;

// src: B images of H*W*3 elements of src_kind (0 uint8, 1 fp32, 2 bf16), contiguous; plan: int32[B][N][12] on the
// device; buf0, buf1: B*H*W*3 bytes each; scratch: uint32[N][B][4][256]; dst: as src, of dst_kind, not overlapping
// src.  One memset and 2 N launches on ``stream``; nothing is allocated or read back.
// Returns -1 for a null pointer, a kind outside 0..2 or a float source / destination misaligned for its element size,
// -2 for B, H, W < 1 or H*W >= 2^31, -3 for N < 1; nothing is launched then.
DTM_API int dtm_randaugment(const void* src, int src_kind, float in_scale, float in_shift, const int* plan, int B,
                            int H, int W, int N, void* buf0, void* buf1, void* scratch, void* dst, int dst_kind,
                            float out_scale, float out_shift, void* stream) {
  if (!src || !plan || !buf0 || !buf1 || !scratch || !dst) return -1;
  if (src_kind < 0 || src_kind > 2 || dst_kind < 0 || dst_kind > 2) return -1;
  const uintptr_t es_in = src_kind == RA_U8 ? 1 : src_kind == RA_F32 ? 4 : 2;
  const uintptr_t es_out = dst_kind == RA_U8 ? 1 : dst_kind == RA_F32 ? 4 : 2;
  if (((uintptr_t)src & (es_in - 1)) || ((uintptr_t)dst & (es_out - 1)) || ((uintptr_t)plan & 3) ||
      ((uintptr_t)scratch & 3))
    return -1;
  if (B < 1 || H < 1 || W < 1 || (long)H * W >= (1L << 31)) return -2;
  if (N < 1) return -3;
  hipStream_t st = (hipStream_t)stream;
  const long npix = (long)H * W;
  const long units = (npix + 3) / 4;
  long bx = (units + 255) / 256;                            // one unit per lane ...
  const long cap = (8L * dtm_compute_cus() + B - 1) / B;    // ... up to 8 blocks per CU over the batch
  if (bx > cap) bx = cap;
  if (bx < 1) bx = 1;
  const dim3 grid((unsigned)bx, (unsigned)(B > 65535 ? 65535 : B));
  const size_t hist_words = (size_t)B * 4 * 256;
  if (hipMemsetAsync(scratch, 0, sizeof(uint32_t) * hist_words * N, st) != hipSuccess) return -4;
  void* bufs[2] = {buf0, buf1};
  for (int l = 0; l < N; ++l) {
    RaArgs a;
    a.in = l == 0 ? src : bufs[(l - 1) & 1];
    a.out = l == N - 1 ? dst : bufs[l & 1];
    a.plan = plan;
    a.hist = (uint32_t*)scratch + hist_words * l;
    a.B = B; a.H = H; a.W = W; a.N = N; a.layer = l;
    a.npix = (uint32_t)npix;
    a.dw = make_fastdiv((uint32_t)W);
    a.in_scale = in_scale; a.in_shift = in_shift; a.out_scale = out_scale; a.out_shift = out_shift;
    const int ik = l == 0 ? src_kind : RA_U8, ok = l == N - 1 ? dst_kind : RA_U8;
    if (ik == RA_U8) {
      hipLaunchKernelGGL(ra_stats_kernel<RA_U8>, grid, dim3(256), 0, st, a);
      ra_launch_apply<RA_U8>(ok, grid, st, a);
    } else if (ik == RA_F32) {
      hipLaunchKernelGGL(ra_stats_kernel<RA_F32>, grid, dim3(256), 0, st, a);
      ra_launch_apply<RA_F32>(ok, grid, st, a);
    } else {
      hipLaunchKernelGGL(ra_stats_kernel<RA_BF16>, grid, dim3(256), 0, st, a);
      ra_launch_apply<RA_BF16>(ok, grid, st, a);
    }
  }
  return hipGetLastError() == hipSuccess ? 0 : -5;
}
