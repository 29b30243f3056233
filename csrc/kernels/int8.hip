// 8-bit integer inference for fake-quantised models (ops/int8.py, compat/quantize.py with QuantConfig(integer=True)).
//
// One integer layer (forward only, NHWC, dilation 1):
//   acc[n,p,q,k] = sum over the in-bounds taps (r, s) and c of (a - z_a) * (w - z_w)        int32, exact
//   t = s_a * s_w;  r = fma((float)acc, t, bias[k]);  r = act(r)                             fp32, every rounding spelled out
//   code = clamp(rint(r * inv_o) + z_o, 0, 255)                                               the arithmetic of fq_apply
// with a: uint8 activation codes, w: uint8 weight codes, (s, z) from the quantiser records of fakequant.hip (8 words:
// scale, inv_scale, zero point, qmin, qmax as fp32).  Optionally the dequantised (code - z_o) * s_o is written too, in
// bf16 or fp32: the bits fq_apply gives r.
//
// q8_convert_kernel   bf16 / fp32 -> codes through a record and codes -> bf16 / fp32: 16 codes per 16-byte access over
//                     the body, a scalar head and tail (the body needs both tensors 16-byte aligned at one element;
//                     otherwise element by element).
// q8_prepare_kernel   folded fp32 weights [K][R*S][C] -> shifted signed codes w' = code - 128 as rows
//                     [Kp][row bytes]: R*S taps of Cp = roundup(C, 16) channels (padding channels hold z_w, so they
//                     contribute 0 whatever the activation padding holds), the row zero-filled to a multiple of 64
//                     bytes, Kp = roundup(K, 64) with zero rows; and sum_k w' per row.  Once per weights version.
// q8_conv_kernel      implicit GEMM on v_mfma_i32_16x16x64_i8.  A wave owns 32 pixels x 64 output channels: per
//                     64-deep step it holds 4 weight fragments (MFMA A operand: 16 channels x 64) and 2 pixel
//                     fragments (B operand: 64 x 16 pixels), 8 MFMAs.  A lane's 16-byte fragment is ONE 16-channel
//                     chunk of one tap, loaded straight from global memory into the operand registers (the next step's
//                     six loads are issued before this step's MFMAs); the four waves of a block form 64 pixels x 128
//                     channels and share their fragments through L1.  Operands are shifted to signed with x ^ 0x80:
//                       sum (a' - z_a')(w' - z_w') = sum a'w' - z_w' * sum a' - z_a' * sum w' + n * z_a' * z_w'
//                     which holds only if a padded tap holds z_a', so out-of-bounds taps are FILLED with z_a' on load
//                     (not zero); chunks past the end of the reduction are 0 on both sides.  sum a' per pixel comes
//                     from the pixel fragments the wave holds (sdot4 with 0x01010101, then the four lanes that share
//                     the pixel), sum w' from the prepare step.  Epilogue: the 4 x 4 packed codes of a pixel are
//                     gathered from the four lanes that hold them (ds_bpermute) so one lane stores 16 codes with one
//                     16-byte store when K % 16 == 0.  No atomics, no split-K.
// q8_depthwise_kernel multiplier 1, integer VALU: a lane owns 16 channels x a strip of 4 output pixels of one row;
//                     for S == 3 the input row window of the strip is loaded once per kernel row and reused by the
//                     three taps and the four outputs; (a - z_a)(w - z_w) directly in int32; the same epilogue.
#include "common.h"

#pragma clang fp contract(off)

namespace dtm {

typedef int int32x4 __attribute__((ext_vector_type(4)));

constexpr int Q8_THREADS = 256;
constexpr int Q8_MAX_GRID = 2048;
constexpr int Q8_MAX_REDUCE = 32768;  // R*S*C: |acc| <= 255 * 254 * 32768 < 2^31
constexpr int Q8_TILE_M = 64, Q8_TILE_K = 128, Q8_WAVE_K = 64;
constexpr int Q8_DW_TQ = 4;

struct Q8Desc {
  int N, H, W, C, K, R, S, P, Q, stride, pad_h, pad_w;  // C: channels of the (padded) activation, a multiple of 16
};

struct Q8Out {
  float t, inv_o, zp_o, s_o;
  int act, deq;  // act 0 none, 1 relu, 2 relu6; deq 0 none, 1 bf16, 2 fp32
};

__device__ __forceinline__ float q8_requant(int acc, float bias, const Q8Out& o) {
  float r = __fmaf_rn((float)acc, o.t, bias);
  if (o.act >= 1) r = fmaxf(r, 0.f);
  if (o.act == 2) r = fminf(r, 6.f);
  const float q = __fadd_rn(rintf(__fmul_rn(r, o.inv_o)), o.zp_o);
  return fminf(fmaxf(q, 0.f), 255.f);
}
__device__ __forceinline__ float q8_deq(float code, const Q8Out& o) {
  return __fmul_rn(__fsub_rn(code, o.zp_o), o.s_o);
}
__device__ __forceinline__ Q8Out q8_out(const int* rec_a, const int* rec_w, const int* rec_o, int act, int deq) {
  const float* fo = (const float*)rec_o;
  Q8Out o;
  o.t = __fmul_rn(((const float*)rec_a)[0], ((const float*)rec_w)[0]);
  o.s_o = fo[0]; o.inv_o = fo[1]; o.zp_o = fo[2];
  o.act = act; o.deq = deq;
  return o;
}

// 16 codes of one pixel (channels k0 .. k0 + 15 of K, packed in memory order) -> codes and the dequantised copy
__device__ __forceinline__ void q8_store16(const int32x4 pk, long pix, int k0, int K, bool vec, uint8_t* codes,
                                           void* deq, const Q8Out& o) {
  const long at = pix * K + k0;
  if (vec) {
    *(int32x4*)(codes + at) = pk;
    if (o.deq == 1) {
      int32x4 lo, hi;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const uint32_t u = (uint32_t)pk[j];
        const uint32_t p0 = pack2bf(q8_deq((float)(u & 255u), o), q8_deq((float)((u >> 8) & 255u), o));
        const uint32_t p1 = pack2bf(q8_deq((float)((u >> 16) & 255u), o), q8_deq((float)(u >> 24), o));
        if (j < 2) { lo[2 * j] = (int)p0; lo[2 * j + 1] = (int)p1; }
        else { hi[2 * (j - 2)] = (int)p0; hi[2 * (j - 2) + 1] = (int)p1; }
      }
      int32x4* d = (int32x4*)((bf16_t*)deq + at);
      d[0] = lo; d[1] = hi;
    } else if (o.deq == 2) {
      f32x4* d = (f32x4*)((float*)deq + at);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const uint32_t u = (uint32_t)pk[j];
        f32x4 v;
        v[0] = q8_deq((float)(u & 255u), o); v[1] = q8_deq((float)((u >> 8) & 255u), o);
        v[2] = q8_deq((float)((u >> 16) & 255u), o); v[3] = q8_deq((float)(u >> 24), o);
        d[j] = v;
      }
    }
    return;
  }
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    if (k0 + e < K) {
      const uint32_t c = ((uint32_t)pk[e >> 2] >> (8 * (e & 3))) & 255u;
      codes[at + e] = (uint8_t)c;
      if (o.deq == 1) ((bf16_t*)deq)[at + e] = f2bf(q8_deq((float)c, o));
      else if (o.deq == 2) ((float*)deq)[at + e] = q8_deq((float)c, o);
    }
  }
}

// ---- quantize / dequantize ----------------------------------------------------------------------------------------
struct Q8Rec {
  float scale, inv, zp, qmin, qmax;
};
__device__ __forceinline__ Q8Rec q8_load_rec(const int* rec) {
  const float* f = (const float*)rec;
  Q8Rec r;
  r.scale = f[0]; r.inv = f[1]; r.zp = f[2]; r.qmin = f[3]; r.qmax = f[4];
  return r;
}
__device__ __forceinline__ uint32_t q8_code(float x, const Q8Rec& r) {
  return (uint32_t)fminf(fmaxf(__fadd_rn(rintf(__fmul_rn(x, r.inv)), r.zp), r.qmin), r.qmax);
}
__device__ __forceinline__ float q8_value(uint32_t c, const Q8Rec& r) {
  return __fmul_rn(__fsub_rn((float)c, r.zp), r.scale);
}

// TO_CODES: f (bf16 / fp32) -> u8; else u8 -> f.  VEC: f + head elements and u8 + head bytes are both 16-byte aligned
template <bool BF16, bool TO_CODES, bool VEC>
__global__ __launch_bounds__(Q8_THREADS) void q8_convert_kernel(void* __restrict__ fbuf, uint8_t* __restrict__ u8,
                                                                long n, const int* __restrict__ rec) {
  const Q8Rec r = q8_load_rec(rec);
  bf16_t* fb = (bf16_t*)fbuf;
  float* ff = (float*)fbuf;
  const long gtid = (long)blockIdx.x * Q8_THREADS + threadIdx.x, gsz = (long)gridDim.x * Q8_THREADS;
  auto one = [&](long i) {
    if (TO_CODES) u8[i] = (uint8_t)q8_code(BF16 ? bf2f(fb[i]) : ff[i], r);
    else if (BF16) fb[i] = f2bf(q8_value(u8[i], r));
    else ff[i] = q8_value(u8[i], r);
  };
  if (!VEC) {
    for (long i = gtid; i < n; i += gsz) one(i);
    return;
  }
  long head = (long)((16u - (unsigned)((uintptr_t)u8 & 15u)) & 15u);
  if (head > n) head = n;
  const long nvec = (n - head) / 16, tail0 = head + nvec * 16;
  if (gtid < head) one(gtid);  // (head < 16 <= Q8_THREADS: block 0)
  for (long i = gtid; i < nvec; i += gsz) {
    const long e0 = head + i * 16;
    float v[16];
    int32x4 pk;
    if (TO_CODES) {
      if (BF16) {
        const short8* xv = (const short8*)(fb + e0);
        const short8 a = xv[0], b = xv[1];
#pragma unroll
        for (int e = 0; e < 8; ++e) { v[e] = bf2f((bf16_t)a[e]); v[8 + e] = bf2f((bf16_t)b[e]); }
      } else {
        const f32x4* xv = (const f32x4*)(ff + e0);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const f32x4 a = xv[j];
#pragma unroll
          for (int e = 0; e < 4; ++e) v[4 * j + e] = a[e];
        }
      }
#pragma unroll
      for (int j = 0; j < 4; ++j)
        pk[j] = (int)(q8_code(v[4 * j], r) | (q8_code(v[4 * j + 1], r) << 8) | (q8_code(v[4 * j + 2], r) << 16) |
                      (q8_code(v[4 * j + 3], r) << 24));
      *(int32x4*)(u8 + e0) = pk;
    } else {
      pk = *(const int32x4*)(u8 + e0);
#pragma unroll
      for (int e = 0; e < 16; ++e) v[e] = q8_value(((uint32_t)pk[e >> 2] >> (8 * (e & 3))) & 255u, r);
      if (BF16) {
        short8 a, b;
#pragma unroll
        for (int e = 0; e < 8; ++e) { a[e] = (short)f2bf(v[e]); b[e] = (short)f2bf(v[8 + e]); }
        short8* yv = (short8*)(fb + e0);
        yv[0] = a; yv[1] = b;
      } else {
        f32x4* yv = (f32x4*)(ff + e0);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          f32x4 a;
#pragma unroll
          for (int e = 0; e < 4; ++e) a[e] = v[4 * j + e];
          yv[j] = a;
        }
      }
    }
  }
  if (tail0 + gtid < n) one(tail0 + gtid);  // (tail < 16)
}

// ---- weights ----------------------------------------------------------------------------------------------------
__host__ __device__ static inline int q8_round_up(int v, int m) { return (v + m - 1) / m * m; }
static int q8_row_bytes(int R, int S, int C) { return q8_round_up(R * S * q8_round_up(C, 16), 64); }
static int q8_rows(int K) { return q8_round_up(K, Q8_WAVE_K); }

// one block per prepared row k < Kp
__global__ __launch_bounds__(Q8_THREADS) void q8_prepare_kernel(const float* __restrict__ w,
                                                                const int* __restrict__ rec_w,
                                                                int8_t* __restrict__ w8, int* __restrict__ wsum, int K,
                                                                int RS, int C, int Cp, int row_bytes) {
  __shared__ int red[Q8_THREADS / 64];
  const Q8Rec r = q8_load_rec(rec_w);
  const int k = blockIdx.x;
  int sum = 0;
  for (int j = threadIdx.x; j < row_bytes; j += Q8_THREADS) {
    const int rs = j / Cp, c = j - rs * Cp;
    int v = 0;
    if (k < K && rs < RS) {
      const uint32_t code = c < C ? q8_code(w[((long)k * RS + rs) * C + c], r) : (uint32_t)r.zp;
      v = (int)code - 128;
    }
    w8[(long)k * row_bytes + j] = (int8_t)v;
    sum += v;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = sum;
  __syncthreads();
  if (threadIdx.x == 0) {
    int s = 0;
#pragma unroll
    for (int i = 0; i < Q8_THREADS / 64; ++i) s += red[i];
    wsum[k] = s;
  }
}

// ---- implicit-GEMM conv -------------------------------------------------------------------------------------------
// PW: 1x1, stride 1, no padding (every tap in bounds, the chunk walk is a pointer increment)
template <bool PW>
__global__ __launch_bounds__(Q8_THREADS) void q8_conv_kernel(const uint8_t* __restrict__ a,
                                                             const int8_t* __restrict__ w8,
                                                             const int* __restrict__ wsum,
                                                             const float* __restrict__ bias,
                                                             const int* __restrict__ rec_a,
                                                             const int* __restrict__ rec_w,
                                                             const int* __restrict__ rec_o, uint8_t* __restrict__ codes,
                                                             void* __restrict__ deq, Q8Desc d, int act, int deq_dtype) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, row16 = lane & 15, g = lane >> 4;
  const int M = d.N * d.P * d.Q;
  const int mbase = blockIdx.x * Q8_TILE_M + (wave & 1) * 32;
  const int kbase = blockIdx.y * Q8_TILE_K + (wave >> 1) * Q8_WAVE_K;
  if (mbase >= M || kbase >= q8_round_up(d.K, Q8_WAVE_K)) return;  // (wave-uniform: the shuffles below stay whole)
  const int C16 = d.C >> 4, n16 = d.R * d.S * C16, row_bytes = q8_round_up(n16 * 16, 64), steps = row_bytes >> 6;
  const int za = (int)((const float*)rec_a)[2], zw = (int)((const float*)rec_w)[2];
  const int fill = (int)(((uint32_t)(za ^ 0x80) & 255u) * 0x01010101u);

  // the lane's pixel of each of the two pixel fragments
  const uint8_t* abase[2];
  int ih0[2], iw0[2];
  bool valid[2];
#pragma unroll
  for (int pt = 0; pt < 2; ++pt) {
    const int m = mbase + pt * 16 + row16;
    valid[pt] = m < M;
    const int mm = valid[pt] ? m : 0;
    const int q = mm % d.Q, pq = mm / d.Q, p = pq % d.P, n = pq / d.P;
    ih0[pt] = p * d.stride - d.pad_h;
    iw0[pt] = q * d.stride - d.pad_w;
    abase[pt] = a + (long)n * d.H * d.W * d.C;
  }
  // the lane's chunk of the reduction: chunk cq = step * 4 + g  ->  tap (r, s), channel chunk c16
  int cq = g, c16 = g % C16, s = (g / C16) % d.S, r = (g / C16) / d.S;
  const int8_t* wp = w8 + (long)(kbase + row16) * row_bytes + g * 16;
  const long wtile = (long)16 * row_bytes;

  auto load_a = [&](int pt) -> int32x4 {
    int32x4 v = {0, 0, 0, 0};
    if (cq < n16 && valid[pt]) {
      const int ih = ih0[pt] + r, iw = iw0[pt] + s;
      if (PW || ((unsigned)ih < (unsigned)d.H && (unsigned)iw < (unsigned)d.W)) {
        v = *(const int32x4*)(abase[pt] + ((long)ih * d.W + iw) * d.C + c16 * 16);
        v ^= (int)0x80808080;
      } else {
        v = int32x4{fill, fill, fill, fill};
      }
    }
    return v;
  };
  auto advance = [&]() {
    cq += 4;
    c16 += 4;
    wp += 64;
    while (c16 >= C16) {
      c16 -= C16;
      if (++s == d.S) { s = 0; ++r; }
    }
  };

  int32x4 acc[2][4];
#pragma unroll
  for (int pt = 0; pt < 2; ++pt)
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[pt][t] = int32x4{0, 0, 0, 0};
  int asum[2] = {0, 0};

  int32x4 af[2], wf[4];
  af[0] = load_a(0); af[1] = load_a(1);
#pragma unroll
  for (int t = 0; t < 4; ++t) wf[t] = *(const int32x4*)(wp + t * wtile);
  for (int step = 0; step < steps; ++step) {
    int32x4 an[2] = {af[0], af[1]}, wn[4] = {wf[0], wf[1], wf[2], wf[3]};
    if (step + 1 < steps) {  // the next step's fragments, in flight during this step's MFMAs
      advance();
      an[0] = load_a(0); an[1] = load_a(1);
#pragma unroll
      for (int t = 0; t < 4; ++t) wn[t] = *(const int32x4*)(wp + t * wtile);
    }
#pragma unroll
    for (int pt = 0; pt < 2; ++pt) {
#pragma unroll
      for (int j = 0; j < 4; ++j) asum[pt] = __builtin_amdgcn_sdot4(af[pt][j], 0x01010101, asum[pt], false);
#pragma unroll
      for (int t = 0; t < 4; ++t)
        acc[pt][t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(wf[t], af[pt], acc[pt][t], 0, 0, 0);
    }
    af[0] = an[0]; af[1] = an[1];
#pragma unroll
    for (int t = 0; t < 4; ++t) wf[t] = wn[t];
  }

  // D: lane holds pixel row16, channels kbase + t * 16 + g * 4 + i
  const Q8Out o = q8_out(rec_a, rec_w, rec_o, act, deq_dtype);
  const uint32_t zas = (uint32_t)(za - 128), zws = (uint32_t)(zw - 128);
  const uint32_t nzz = (uint32_t)(d.R * d.S * d.C) * zas * zws;
  const bool vec = (d.K & 15) == 0;
#pragma unroll
  for (int pt = 0; pt < 2; ++pt) {
    int sa = asum[pt];
    sa += __shfl_xor(sa, 16, 64);
    sa += __shfl_xor(sa, 32, 64);
    uint32_t pk[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int kc = kbase + t * 16 + g * 4;
      const int32x4 ws = *(const int32x4*)(wsum + kc);
      uint32_t p = 0;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const uint32_t full = (uint32_t)acc[pt][t][i] - zws * (uint32_t)sa - zas * (uint32_t)ws[i] + nzz;
        const float b = (kc + i < d.K) ? bias[kc + i] : 0.f;
        p |= (uint32_t)q8_requant((int)full, b, o) << (8 * i);
      }
      pk[t] = p;
    }
    // lane (row16, g) gathers tile t == g: the 4 dwords held by lanes row16 + 16 * j
    int32x4 out = {0, 0, 0, 0};
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int v = __shfl((int)pk[t], row16 + 16 * j, 64);
        if (g == t) out[j] = v;
      }
    const int m = mbase + pt * 16 + row16, k0 = kbase + g * 16;
    if (m < M && k0 < d.K) q8_store16(out, m, k0, d.K, vec, codes, deq, o);
  }
}

// ---- depthwise ----------------------------------------------------------------------------------------------------
struct Q8Dw {
  int N, H, W, C, Cp, R, S, P, Q, stride, pad_h, pad_w;  // C: real channels (outputs), Cp: channels of the padded input
};

// S3: S == 3, the strip's input row window lives in registers; else every tap is loaded where it is used
template <int STRIDE, bool S3>
__global__ __launch_bounds__(Q8_THREADS) void q8_depthwise_kernel(const uint8_t* __restrict__ a,
                                                                  const int8_t* __restrict__ w8,
                                                                  const float* __restrict__ bias,
                                                                  const int* __restrict__ rec_a,
                                                                  const int* __restrict__ rec_w,
                                                                  const int* __restrict__ rec_o,
                                                                  uint8_t* __restrict__ codes, void* __restrict__ deq,
                                                                  Q8Dw d, int act, int deq_dtype) {
  constexpr int TQ = Q8_DW_TQ, WW = (TQ - 1) * STRIDE + 3;
  const int C16 = d.Cp >> 4, QT = (d.Q + TQ - 1) / TQ;
  const long items = (long)d.N * d.P * QT * C16;
  const long idx = (long)blockIdx.x * Q8_THREADS + threadIdx.x;
  if (idx >= items) return;
  const int c16 = (int)(idx % C16);
  long rest = idx / C16;
  const int qt = (int)(rest % QT);
  rest /= QT;
  const int p = (int)(rest % d.P), n = (int)(rest / d.P);
  const int q0 = qt * TQ, iw_first = q0 * STRIDE - d.pad_w;
  const int za = (int)((const float*)rec_a)[2], zws = (int)((const float*)rec_w)[2] - 128;
  const uint8_t* an = a + (long)n * d.H * d.W * d.Cp + c16 * 16;

  int acc[TQ][16];
#pragma unroll
  for (int t = 0; t < TQ; ++t)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[t][e] = 0;

  auto tap = [&](int t, const int32x4 av, const int32x4 wv) {
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int x = (int)(((uint32_t)av[e >> 2] >> (8 * (e & 3))) & 255u) - za;
      const int w = (int)(int8_t)(((uint32_t)wv[e >> 2] >> (8 * (e & 3))) & 255u) - zws;
      acc[t][e] += x * w;
    }
  };
  for (int r = 0; r < d.R; ++r) {
    const int ih = p * STRIDE - d.pad_h + r;
    if ((unsigned)ih >= (unsigned)d.H) continue;  // a padded row adds 0
    const uint8_t* arow = an + (long)ih * d.W * d.Cp;
    const int8_t* wrow = w8 + (long)r * d.S * d.Cp + c16 * 16;
    if (S3) {
      int32x4 win[WW];
#pragma unroll
      for (int j = 0; j < WW; ++j) {
        const int iw = iw_first + j;
        win[j] = int32x4{0, 0, 0, 0};
        if ((unsigned)iw < (unsigned)d.W) win[j] = *(const int32x4*)(arow + (long)iw * d.Cp);
      }
#pragma unroll
      for (int s = 0; s < 3; ++s) {
        const int32x4 wv = *(const int32x4*)(wrow + (long)s * d.Cp);
#pragma unroll
        for (int t = 0; t < TQ; ++t) {
          const int iw = iw_first + t * STRIDE + s;
          if ((unsigned)iw < (unsigned)d.W) tap(t, win[t * STRIDE + s], wv);  // a padded column adds 0
        }
      }
    } else {
      for (int s = 0; s < d.S; ++s) {
        const int32x4 wv = *(const int32x4*)(wrow + (long)s * d.Cp);
#pragma unroll
        for (int t = 0; t < TQ; ++t) {
          const int iw = iw_first + t * STRIDE + s;
          if ((unsigned)iw < (unsigned)d.W) tap(t, *(const int32x4*)(arow + (long)iw * d.Cp), wv);
        }
      }
    }
  }

  const Q8Out o = q8_out(rec_a, rec_w, rec_o, act, deq_dtype);
  const bool vec = (d.C & 15) == 0;
  const int k0 = c16 * 16;
  float b[16];
#pragma unroll
  for (int e = 0; e < 16; ++e) b[e] = (k0 + e < d.C) ? bias[k0 + e] : 0.f;
#pragma unroll
  for (int t = 0; t < TQ; ++t) {
    const int q = q0 + t;
    if (q >= d.Q) break;
    int32x4 pk;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      uint32_t u = 0;
#pragma unroll
      for (int i = 0; i < 4; ++i) u |= (uint32_t)q8_requant(acc[t][4 * j + i], b[4 * j + i], o) << (8 * i);
      pk[j] = (int)u;
    }
    q8_store16(pk, ((long)n * d.P + p) * d.Q + q, k0, d.C, vec, codes, deq, o);
  }
}

static int q8_grid(long n) {
  const long per_block = (long)Q8_THREADS * 4 * 16;
  long g = (n + per_block - 1) / per_block;
  if (g < 1) g = 1;
  if (g > Q8_MAX_GRID) g = Q8_MAX_GRID;
  return (int)g;
}
static bool q8_bad(const void* p, unsigned mask) { return !p || ((uintptr_t)p & mask); }

template <bool TO_CODES>
static int q8_convert(void* f, int dtype, void* u8, long n, const void* rec, hipStream_t st) {
  if (!dtm_device_ok()) return -9;
  if (n < 1 || (dtype != 0 && dtype != 1)) return -3;
  if (q8_bad(f, dtype == 1 ? 1u : 3u) || !u8 || q8_bad(rec, 3u)) return -1;
  const long head = (long)((16u - (unsigned)((uintptr_t)u8 & 15u)) & 15u);
  const bool vec = (((uintptr_t)f + (uintptr_t)head * (dtype == 1 ? 2u : 4u)) & 15u) == 0;
  const dim3 grid((unsigned)q8_grid(n)), block(Q8_THREADS);
  const int* r = (const int*)rec;
  uint8_t* u = (uint8_t*)u8;
  if (dtype == 1) {
    if (vec) hipLaunchKernelGGL((q8_convert_kernel<true, TO_CODES, true>), grid, block, 0, st, f, u, n, r);
    else hipLaunchKernelGGL((q8_convert_kernel<true, TO_CODES, false>), grid, block, 0, st, f, u, n, r);
  } else {
    if (vec) hipLaunchKernelGGL((q8_convert_kernel<false, TO_CODES, true>), grid, block, 0, st, f, u, n, r);
    else hipLaunchKernelGGL((q8_convert_kernel<false, TO_CODES, false>), grid, block, 0, st, f, u, n, r);
  }
  return hipGetLastError() == hipSuccess ? 0 : -4;
}

// shared argument checks of the two layer entry points; esz: bytes per element of the dequantised copy
static int q8_check_layer(const void* a, const void* w8, const void* bias, const void* rec_a, const void* rec_w,
                          const void* rec_o, const void* codes, const void* deq, int deq_dtype, int act, bool vec) {
  if (q8_bad(a, 15u) || q8_bad(w8, 15u) || q8_bad(bias, 3u) || q8_bad(rec_a, 3u) || q8_bad(rec_w, 3u) ||
      q8_bad(rec_o, 3u) || q8_bad(codes, vec ? 15u : 0u))
    return -1;
  if (deq_dtype != 0 && q8_bad(deq, vec ? 15u : (deq_dtype == 1 ? 1u : 3u))) return -1;
  if (deq_dtype < 0 || deq_dtype > 2 || act < 0 || act > 2) return -3;
  return 0;
}

}  // namespace dtm

using namespace dtm;

DTM_API int dtm_q8_max_reduce() { return Q8_MAX_REDUCE; }
// prepared weights of a [K][R][S][C] layer: dtm_q8_weight_rows(K) rows of dtm_q8_weight_row_bytes(R, S, C) bytes
DTM_API int dtm_q8_weight_rows(int K) { return K < 1 ? -3 : q8_rows(K); }
DTM_API int dtm_q8_weight_row_bytes(int R, int S, int C) { return (R < 1 || S < 1 || C < 1) ? -3 : q8_row_bytes(R, S, C); }

// x: n contiguous bf16 (dtype 1) or fp32 (0) elements -> n codes through the record rec
DTM_API int dtm_q8_quantize(const void* x, int dtype, void* codes, long n, const void* rec, void* stream) {
  return q8_convert<true>(const_cast<void*>(x), dtype, codes, n, rec, (hipStream_t)stream);
}
DTM_API int dtm_q8_dequantize(const void* codes, void* y, int dtype, long n, const void* rec, void* stream) {
  return q8_convert<false>(y, dtype, const_cast<void*>(codes), n, rec, (hipStream_t)stream);
}

// w: fp32 [K][R][S][C] (a depthwise filter [R][S][C] is K == 1) -> w8 [rows][row bytes] int8, wsum [rows] int32
DTM_API int dtm_q8_prepare_weights(const void* w, const void* rec_w, void* w8, void* wsum, int K, int R, int S, int C,
                                   void* stream) {
  if (!dtm_device_ok()) return -9;
  if (K < 1 || R < 1 || S < 1 || C < 1) return -3;
  if ((long)R * S * q8_round_up(C, 16) > Q8_MAX_REDUCE) return -2;
  if (q8_bad(w, 3u) || q8_bad(rec_w, 3u) || q8_bad(w8, 15u) || q8_bad(wsum, 15u)) return -1;
  hipLaunchKernelGGL(q8_prepare_kernel, dim3((unsigned)q8_rows(K)), dim3(Q8_THREADS), 0, (hipStream_t)stream,
                     (const float*)w, (const int*)rec_w, (int8_t*)w8, (int*)wsum, K, R * S, C, q8_round_up(C, 16),
                     q8_row_bytes(R, S, C));
  return hipGetLastError() == hipSuccess ? 0 : -4;
}

// a: codes [N][H][W][C], C % 16 == 0 (padding channels hold any code: their prepared weights are z_w); w8 / wsum: the
// prepared weights of [K][R][S][C]; bias: fp32 [K]; codes: [N][P][Q][K]; deq: the same shape in bf16 (deq_dtype 1) or
// fp32 (2), or unused (0).  act: 0 none, 1 relu, 2 relu6.
DTM_API int dtm_q8_conv(const void* a, const void* w8, const void* wsum, const void* bias, const void* rec_a,
                        const void* rec_w, const void* rec_o, void* codes, void* deq, int deq_dtype, int act,
                        const Q8Desc* dp, void* stream) {
  if (!dtm_device_ok()) return -9;
  if (!dp) return -1;
  const Q8Desc d = *dp;
  if (d.N < 1 || d.H < 1 || d.W < 1 || d.C < 1 || d.K < 1 || d.R < 1 || d.S < 1 || d.P < 1 || d.Q < 1 ||
      d.stride < 1 || d.pad_h < 0 || d.pad_w < 0 || (d.C & 15))
    return -3;
  if ((long)d.R * d.S * d.C > Q8_MAX_REDUCE) return -2;
  const long M = (long)d.N * d.P * d.Q;
  if (M * d.K >= (1L << 31) || (long)d.N * d.H * d.W * d.C >= (1L << 31)) return -3;
  // the last tap of the last output must not pass the input by more than the padding covers: taps are bounds-checked
  // in the kernel, so any geometry is safe; P and Q only decide how many pixels are written
  const int rc = q8_check_layer(a, w8, bias, rec_a, rec_w, rec_o, codes, deq, deq_dtype, act, (d.K & 15) == 0);
  if (rc) return rc;
  if (q8_bad(wsum, 15u)) return -1;
  const dim3 grid((unsigned)((M + Q8_TILE_M - 1) / Q8_TILE_M), (unsigned)((q8_rows(d.K) + Q8_TILE_K - 1) / Q8_TILE_K));
  const bool pw = d.R == 1 && d.S == 1 && d.stride == 1 && d.pad_h == 0 && d.pad_w == 0 && d.P == d.H && d.Q == d.W;
  if (pw)
    hipLaunchKernelGGL(q8_conv_kernel<true>, grid, dim3(Q8_THREADS), 0, (hipStream_t)stream, (const uint8_t*)a,
                       (const int8_t*)w8, (const int*)wsum, (const float*)bias, (const int*)rec_a, (const int*)rec_w,
                       (const int*)rec_o, (uint8_t*)codes, deq, d, act, deq_dtype);
  else
    hipLaunchKernelGGL(q8_conv_kernel<false>, grid, dim3(Q8_THREADS), 0, (hipStream_t)stream, (const uint8_t*)a,
                       (const int8_t*)w8, (const int*)wsum, (const float*)bias, (const int*)rec_a, (const int*)rec_w,
                       (const int*)rec_o, (uint8_t*)codes, deq, d, act, deq_dtype);
  return hipGetLastError() == hipSuccess ? 0 : -4;
}

// a: codes [N][H][W][Cp], Cp = roundup(C, 16); w8: the prepared weights of the [R][S][C] filter; bias: fp32 [C];
// codes (and deq): [N][P][Q][C].  stride 1 or 2.
DTM_API int dtm_q8_depthwise(const void* a, const void* w8, const void* bias, const void* rec_a, const void* rec_w,
                             const void* rec_o, void* codes, void* deq, int deq_dtype, int act, const Q8Dw* dp,
                             void* stream) {
  if (!dtm_device_ok()) return -9;
  if (!dp) return -1;
  const Q8Dw d = *dp;
  if (d.N < 1 || d.H < 1 || d.W < 1 || d.C < 1 || d.R < 1 || d.S < 1 || d.P < 1 || d.Q < 1 || d.pad_h < 0 ||
      d.pad_w < 0 || d.Cp != q8_round_up(d.C, 16) || (d.stride != 1 && d.stride != 2))
    return -3;
  if ((long)d.R * d.S * d.Cp > Q8_MAX_REDUCE) return -2;
  if ((long)d.N * d.P * d.Q * d.C >= (1L << 31) || (long)d.N * d.H * d.W * d.Cp >= (1L << 31)) return -3;
  const int rc = q8_check_layer(a, w8, bias, rec_a, rec_w, rec_o, codes, deq, deq_dtype, act, (d.C & 15) == 0);
  if (rc) return rc;
  const long items = (long)d.N * d.P * ((d.Q + Q8_DW_TQ - 1) / Q8_DW_TQ) * (d.Cp / 16);
  const dim3 grid((unsigned)((items + Q8_THREADS - 1) / Q8_THREADS)), block(Q8_THREADS);
  hipStream_t st = (hipStream_t)stream;
#define Q8_DW_LAUNCH(ST, S3)                                                                                       \
  hipLaunchKernelGGL((q8_depthwise_kernel<ST, S3>), grid, block, 0, st, (const uint8_t*)a, (const int8_t*)w8,      \
                     (const float*)bias, (const int*)rec_a, (const int*)rec_w, (const int*)rec_o, (uint8_t*)codes, \
                     deq, d, act, deq_dtype)
  if (d.stride == 1) { if (d.S == 3) Q8_DW_LAUNCH(1, true); else Q8_DW_LAUNCH(1, false); }
  else { if (d.S == 3) Q8_DW_LAUNCH(2, true); else Q8_DW_LAUNCH(2, false); }
#undef Q8_DW_LAUNCH
  return hipGetLastError() == hipSuccess ? 0 : -4;
}
