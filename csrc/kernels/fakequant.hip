// Fake quantisation (TF FakeQuantWithMinMaxVars) of one contiguous fp32 or bf16 tensor as small device passes whose
// state lives in device memory, so a whole quantised training step can be captured into a hipGraph and replayed
// across the quant_delay boundary (ops/fakequant.py, compat/quantize.py with QuantConfig(fused=True)).
//
// Per quantiser: two 0-d fp32 range variables vmin / vmax (checkpointed), a record of 8 four-byte words
//   [0] scale  [1] inv_scale  [2] zero point  [3] qmin  [4] qmax   (fp32)
//   [5] active  [6] nonfinite_batches  [7] 0                        (int32)
// and a scratch table of one (min, max, nonfinite_seen) fp32 partial per block of the range pass (stride 4 floats).
// Per QuantConfig: one int64 step counter (training forwards seen).
//
// fq_range_kernel     min / max of the finite elements and "a NaN or +-Inf was seen" of x[0..n), x starting at any
//                     element: 16-byte loads over the aligned body, a scalar head and tail, grid-stride over a bounded
//                     grid; wave64 butterfly, then the block's four waves through LDS; one partial per block with plain
//                     stores.  min / max are order-independent, so the result is exact and no atomics are needed.
// fq_finalize_kernel  ONE block folds the partials and updates the range variables:
//                       WEIGHTS    vmin = min(lo, 0), vmax = max(hi, 0)                         (last value)
//                       ACT_TRAIN  vmin = vmin * d + (1 - d) * min(lo, 0), vmax likewise        (moving average)
//                       FROZEN     read only (no range pass)
//                     A batch with a non-finite element leaves vmin / vmax alone and adds 1 to nonfinite_batches (the
//                     step then quantises with the stored range) - the one deliberate difference from the torch-op path
//                     of compat/quantize.py, where such a batch poisons the range for the rest of the run.
//                     Then the record from vmin / vmax, operation by operation the arithmetic of
//                     compat.quantize.fake_quant (every fp32 operation spelled out, nothing contracted):
//                       lo = min(vmin, 0), hi = max(vmax, 0), scale = (hi - lo) / (qmax - qmin), 1 unless > 1e-12,
//                       zp = clamp(rint(qmin - lo / scale), qmin, qmax), inv_scale = 1 / scale,
//                       active = (mode == FROZEN && !training_cfg) || step >= quant_delay   (step: the device counter)
// fq_apply_kernel     y = active ? (clamp(rint(x * inv_scale) + zp, qmin, qmax) - zp) * scale : x (bit for bit); NaN
//                     stays NaN, +-Inf clamps to the range ends; a bf16 result is rounded to nearest even.
// fq_apply_bwd_kernel dx = active ? (qmin <= q && q <= qmax ? dy : 0) : dy, q recomputed from the saved x.
//                     Both take the 16-byte path (scalar head and tail) when all their tensors share one misalignment
//                     and an element-wise path otherwise.
// fq_advance_kernel   one thread: counter += 1.
// Stream order is the only synchronisation between the passes.
#include <float.h>

#include "common.h"

#pragma clang fp contract(off)

namespace dtm {

constexpr int FQ_THREADS = 256;
constexpr int FQ_MAX_GRID = 2048;
constexpr int FQ_VECS_PER_THREAD = 4;  // the grid is sized for this many 16-byte loads per thread before it is capped
constexpr int FQ_REC_WORDS = 8;
constexpr int FQ_PARTIAL_STRIDE = 4;

enum : int { FQ_WEIGHTS = 0, FQ_ACT_TRAIN = 1, FQ_FROZEN = 2 };

template <bool BF16>
struct FqElem {
  typedef float type;
  static constexpr int PER_VEC = 4;
};
template <>
struct FqElem<true> {
  typedef bf16_t type;
  static constexpr int PER_VEC = 8;
};

// elements in front of the first 16-byte boundary of p (at most n)
template <bool BF16>
__device__ __forceinline__ long fq_head(const void* p, long n) {
  const long h = (long)(((16u - (unsigned)((uintptr_t)p & 15u)) & 15u) / (unsigned)sizeof(typename FqElem<BF16>::type));
  return h < n ? h : n;
}

template <bool BF16>
__global__ __launch_bounds__(FQ_THREADS) void fq_range_kernel(const void* __restrict__ xin, long n,
                                                              float* __restrict__ partials) {
  typedef typename FqElem<BF16>::type T;
  constexpr int PV = FqElem<BF16>::PER_VEC;
  __shared__ float red[FQ_THREADS / 64][3];
  const T* x = (const T*)xin;
  const long head = fq_head<BF16>(x, n), nvec = (n - head) / PV, tail0 = head + nvec * PV;
  const long gtid = (long)blockIdx.x * FQ_THREADS + threadIdx.x, gsz = (long)gridDim.x * FQ_THREADS;
  float lo = INFINITY, hi = -INFINITY;
  bool bad = false;
  auto visit = [&](float v) {
    if (fabsf(v) <= FLT_MAX) { lo = fminf(lo, v); hi = fmaxf(hi, v); }
    else bad = true;
  };
  if (gtid < head) visit(BF16 ? bf2f((bf16_t)x[gtid]) : (float)x[gtid]);  // (head < PV <= FQ_THREADS: block 0)
  if (BF16) {
    const short8* xv = (const short8*)(x + head);
    for (long i = gtid; i < nvec; i += gsz) {
      const short8 w = xv[i];
#pragma unroll
      for (int e = 0; e < 8; ++e) visit(bf2f((bf16_t)w[e]));
    }
  } else {
    const f32x4* xv = (const f32x4*)(x + head);
    for (long i = gtid; i < nvec; i += gsz) {
      const f32x4 w = xv[i];
#pragma unroll
      for (int e = 0; e < 4; ++e) visit(w[e]);
    }
  }
  if (tail0 + gtid < n) visit(BF16 ? bf2f((bf16_t)x[tail0 + gtid]) : (float)x[tail0 + gtid]);  // (tail < PV)
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    lo = fminf(lo, __shfl_xor(lo, o, 64));
    hi = fmaxf(hi, __shfl_xor(hi, o, 64));
  }
  const bool wbad = __any(bad) != 0;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (lane == 0) { red[wv][0] = lo; red[wv][1] = hi; red[wv][2] = wbad ? 1.f : 0.f; }
  __syncthreads();
  if (threadIdx.x == 0) {
    float b = 0.f;
#pragma unroll
    for (int w = 0; w < FQ_THREADS / 64; ++w) {
      lo = fminf(lo, red[w][0]);
      hi = fmaxf(hi, red[w][1]);
      b = fmaxf(b, red[w][2]);
    }
    float* p = partials + (long)blockIdx.x * FQ_PARTIAL_STRIDE;
    p[0] = lo; p[1] = hi; p[2] = b;
  }
}

__global__ __launch_bounds__(FQ_THREADS) void fq_finalize_kernel(const float* __restrict__ partials, int nparts,
                                                                 float* __restrict__ vmin, float* __restrict__ vmax,
                                                                 int* __restrict__ rec,
                                                                 const long long* __restrict__ counter, int mode,
                                                                 float d, float omd, int qmin_i, int qmax_i,
                                                                 long long quant_delay, int training_cfg) {
  __shared__ float red[FQ_THREADS / 64][3];
  float lo = INFINITY, hi = -INFINITY, b = 0.f;
  for (int i = threadIdx.x; i < nparts; i += FQ_THREADS) {
    const float* p = partials + (long)i * FQ_PARTIAL_STRIDE;
    lo = fminf(lo, p[0]);
    hi = fmaxf(hi, p[1]);
    b = fmaxf(b, p[2]);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    lo = fminf(lo, __shfl_xor(lo, o, 64));
    hi = fmaxf(hi, __shfl_xor(hi, o, 64));
    b = fmaxf(b, __shfl_xor(b, o, 64));
  }
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (lane == 0) { red[wv][0] = lo; red[wv][1] = hi; red[wv][2] = b; }
  __syncthreads();
  if (threadIdx.x != 0) return;
#pragma unroll
  for (int w = 0; w < FQ_THREADS / 64; ++w) {
    lo = fminf(lo, red[w][0]);
    hi = fmaxf(hi, red[w][1]);
    b = fmaxf(b, red[w][2]);
  }
  float mn = *vmin, mx = *vmax;
  int nonfinite = rec[6];
  if (mode != FQ_FROZEN) {
    if (b != 0.f) {
      nonfinite += 1;  // the range variables keep their values; the step quantises with them
    } else {
      const float lo0 = lo < 0.f ? lo : 0.f, hi0 = hi > 0.f ? hi : 0.f;
      if (mode == FQ_WEIGHTS) {
        mn = lo0;
        mx = hi0;
      } else {
        mn = __fadd_rn(__fmul_rn(mn, d), __fmul_rn(omd, lo0));
        mx = __fadd_rn(__fmul_rn(mx, d), __fmul_rn(omd, hi0));
      }
      *vmin = mn;
      *vmax = mx;
    }
  }
  const float qmin = (float)qmin_i, qmax = (float)qmax_i;
  const float l = mn < 0.f ? mn : 0.f, h = mx > 0.f ? mx : 0.f;  // (a NaN restored from a checkpoint: 0)
  float scale = __fdiv_rn(__fsub_rn(h, l), (float)(qmax_i - qmin_i));
  if (!(scale > 1e-12f)) scale = 1.0f;
  const float zp = fminf(fmaxf(rintf(__fsub_rn(qmin, __fdiv_rn(l, scale))), qmin), qmax);
  const bool active = (mode == FQ_FROZEN && !training_cfg) || *counter >= quant_delay;
  float* recf = (float*)rec;
  recf[0] = scale;
  recf[1] = __fdiv_rn(1.0f, scale);
  recf[2] = zp;
  recf[3] = qmin;
  recf[4] = qmax;
  rec[5] = active ? 1 : 0;
  rec[6] = nonfinite;
  rec[7] = 0;
}

struct FqRec {
  float scale, inv, zp, qmin, qmax;
  int active;
};
__device__ __forceinline__ FqRec fq_load_rec(const int* rec) {
  const float* f = (const float*)rec;
  FqRec r;
  r.scale = f[0]; r.inv = f[1]; r.zp = f[2]; r.qmin = f[3]; r.qmax = f[4];
  r.active = rec[5];
  return r;
}
__device__ __forceinline__ float fq_q(float x, const FqRec& r) {
  return __fadd_rn(rintf(__fmul_rn(x, r.inv)), r.zp);
}
__device__ __forceinline__ float fq_fwd(float x, const FqRec& r) {
  if (x != x) return x;  // (fmaxf / fminf would drop the NaN)
  const float q = fminf(fmaxf(fq_q(x, r), r.qmin), r.qmax);
  return __fmul_rn(__fsub_rn(q, r.zp), r.scale);
}
__device__ __forceinline__ bool fq_inside(float x, const FqRec& r) {
  const float q = fq_q(x, r);
  return r.qmin <= q && q <= r.qmax;  // (false for a NaN and for +-Inf)
}

// y = f(x) element-wise; VEC: x and y share one misalignment (16-byte body, scalar head and tail)
template <bool BF16, bool VEC>
__global__ __launch_bounds__(FQ_THREADS) void fq_apply_kernel(const void* __restrict__ xin, void* __restrict__ yout,
                                                              long n, const int* __restrict__ rec) {
  typedef typename FqElem<BF16>::type T;
  constexpr int PV = FqElem<BF16>::PER_VEC;
  const T* x = (const T*)xin;
  T* y = (T*)yout;
  const FqRec r = fq_load_rec(rec);
  const long gtid = (long)blockIdx.x * FQ_THREADS + threadIdx.x, gsz = (long)gridDim.x * FQ_THREADS;
  auto one = [&](long i) {
    if (!r.active) { y[i] = x[i]; return; }
    if (BF16) y[i] = (T)f2bf(fq_fwd(bf2f((bf16_t)x[i]), r));
    else y[i] = (T)fq_fwd((float)x[i], r);
  };
  if (!VEC) {
    for (long i = gtid; i < n; i += gsz) one(i);
    return;
  }
  const long head = fq_head<BF16>(x, n), nvec = (n - head) / PV, tail0 = head + nvec * PV;
  if (gtid < head) one(gtid);
  if (BF16) {
    const short8* xv = (const short8*)(x + head);
    short8* yv = (short8*)(y + head);
    for (long i = gtid; i < nvec; i += gsz) {
      short8 w = xv[i];
      if (r.active) {
#pragma unroll
        for (int e = 0; e < 8; ++e) w[e] = (short)f2bf(fq_fwd(bf2f((bf16_t)w[e]), r));
      }
      yv[i] = w;
    }
  } else {
    const f32x4* xv = (const f32x4*)(x + head);
    f32x4* yv = (f32x4*)(y + head);
    for (long i = gtid; i < nvec; i += gsz) {
      f32x4 w = xv[i];
      if (r.active) {
#pragma unroll
        for (int e = 0; e < 4; ++e) w[e] = fq_fwd(w[e], r);
      }
      yv[i] = w;
    }
  }
  if (tail0 + gtid < n) one(tail0 + gtid);
}

template <bool BF16, bool VEC>
__global__ __launch_bounds__(FQ_THREADS) void fq_apply_bwd_kernel(const void* __restrict__ xin,
                                                                  const void* __restrict__ dyin,
                                                                  void* __restrict__ dxout, long n,
                                                                  const int* __restrict__ rec) {
  typedef typename FqElem<BF16>::type T;
  constexpr int PV = FqElem<BF16>::PER_VEC;
  const T* x = (const T*)xin;
  const T* dy = (const T*)dyin;
  T* dx = (T*)dxout;
  const FqRec r = fq_load_rec(rec);
  const long gtid = (long)blockIdx.x * FQ_THREADS + threadIdx.x, gsz = (long)gridDim.x * FQ_THREADS;
  auto one = [&](long i) {
    const float xv = BF16 ? bf2f((bf16_t)x[i]) : (float)x[i];
    dx[i] = (!r.active || fq_inside(xv, r)) ? dy[i] : (T)0;
  };
  if (!VEC) {
    for (long i = gtid; i < n; i += gsz) one(i);
    return;
  }
  const long head = fq_head<BF16>(x, n), nvec = (n - head) / PV, tail0 = head + nvec * PV;
  if (gtid < head) one(gtid);
  if (BF16) {
    const short8* xv = (const short8*)(x + head);
    const short8* gv = (const short8*)(dy + head);
    short8* ov = (short8*)(dx + head);
    for (long i = gtid; i < nvec; i += gsz) {
      short8 g = gv[i];
      if (r.active) {
        const short8 w = xv[i];
#pragma unroll
        for (int e = 0; e < 8; ++e) g[e] = fq_inside(bf2f((bf16_t)w[e]), r) ? g[e] : (short)0;
      }
      ov[i] = g;
    }
  } else {
    const f32x4* xv = (const f32x4*)(x + head);
    const f32x4* gv = (const f32x4*)(dy + head);
    f32x4* ov = (f32x4*)(dx + head);
    for (long i = gtid; i < nvec; i += gsz) {
      f32x4 g = gv[i];
      if (r.active) {
        const f32x4 w = xv[i];
#pragma unroll
        for (int e = 0; e < 4; ++e) g[e] = fq_inside(w[e], r) ? g[e] : 0.f;
      }
      ov[i] = g;
    }
  }
  if (tail0 + gtid < n) one(tail0 + gtid);
}

__global__ void fq_advance_kernel(long long* counter) { *counter += 1; }

static int fq_grid(long n, int dtype) {
  const long per_block = (long)FQ_THREADS * FQ_VECS_PER_THREAD * (dtype == 1 ? 8 : 4);
  long g = (n + per_block - 1) / per_block;
  if (g < 1) g = 1;
  if (g > FQ_MAX_GRID) g = FQ_MAX_GRID;
  return (int)g;
}

static bool fq_bad_tensor(const void* p, int dtype) { return !p || ((uintptr_t)p & (dtype == 1 ? 1u : 3u)); }

}  // namespace dtm

using namespace dtm;

DTM_API int dtm_fq_rec_words() { return FQ_REC_WORDS; }
DTM_API int dtm_fq_partial_stride() { return FQ_PARTIAL_STRIDE; }
DTM_API int dtm_fq_threads() { return FQ_THREADS; }
// blocks of the range / apply passes over n elements (dtype 0 = fp32, 1 = bf16) = partials the range pass writes
DTM_API int dtm_fq_grid(long n, int dtype) { return (n < 1 || (dtype != 0 && dtype != 1)) ? -1 : fq_grid(n, dtype); }

// x: n >= 1 contiguous elements aligned to the element size; partials: >= dtm_fq_grid(n, dtype) * stride floats
DTM_API int dtm_fq_range(const void* x, int dtype, long n, void* partials, void* stream) {
  if (!dtm_device_ok()) return -9;
  if (n < 1 || (dtype != 0 && dtype != 1)) return -1;
  if (fq_bad_tensor(x, dtype) || !partials || ((uintptr_t)partials & 3u)) return -3;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)fq_grid(n, dtype)), block(FQ_THREADS);
  if (dtype == 1) hipLaunchKernelGGL(fq_range_kernel<true>, grid, block, 0, st, x, n, (float*)partials);
  else hipLaunchKernelGGL(fq_range_kernel<false>, grid, block, 0, st, x, n, (float*)partials);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

// mode 0 WEIGHTS, 1 ACT_TRAIN (both fold nparts >= 1 partials), 2 FROZEN (nparts == 0, partials unused).  d and
// one_minus_d: the moving-average decay and 1 - decay (formed in double by the caller), both rounded to fp32.
DTM_API int dtm_fq_finalize(const void* partials, int nparts, void* vmin, void* vmax, void* rec, const void* counter,
                            int mode, float d, float one_minus_d, int bits, int narrow, long quant_delay,
                            int training_cfg, void* stream) {
  if (!dtm_device_ok()) return -9;
  if (mode < FQ_WEIGHTS || mode > FQ_FROZEN || bits < 2 || bits > 16) return -1;
  if (mode == FQ_FROZEN ? nparts != 0 : (nparts < 1 || nparts > FQ_MAX_GRID || !partials)) return -1;
  if (!vmin || !vmax || !rec || !counter) return -3;
  if (((uintptr_t)vmin & 3u) || ((uintptr_t)vmax & 3u) || ((uintptr_t)rec & 3u) || ((uintptr_t)counter & 7u) ||
      ((uintptr_t)partials & 3u))
    return -3;
  hipLaunchKernelGGL(fq_finalize_kernel, dim3(1), dim3(FQ_THREADS), 0, (hipStream_t)stream, (const float*)partials,
                     nparts, (float*)vmin, (float*)vmax, (int*)rec, (const long long*)counter, mode, d, one_minus_d,
                     narrow ? 1 : 0, (1 << bits) - 1, (long long)quant_delay, training_cfg);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

DTM_API int dtm_fq_apply(const void* x, void* y, int dtype, long n, const void* rec, void* stream) {
  if (!dtm_device_ok()) return -9;
  if (n < 1 || (dtype != 0 && dtype != 1)) return -1;
  if (fq_bad_tensor(x, dtype) || fq_bad_tensor(y, dtype) || !rec || ((uintptr_t)rec & 3u)) return -3;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)fq_grid(n, dtype)), block(FQ_THREADS);
  const bool vec = (((uintptr_t)x ^ (uintptr_t)y) & 15u) == 0;
  const int* r = (const int*)rec;
  if (dtype == 1) {
    if (vec) hipLaunchKernelGGL((fq_apply_kernel<true, true>), grid, block, 0, st, x, y, n, r);
    else hipLaunchKernelGGL((fq_apply_kernel<true, false>), grid, block, 0, st, x, y, n, r);
  } else {
    if (vec) hipLaunchKernelGGL((fq_apply_kernel<false, true>), grid, block, 0, st, x, y, n, r);
    else hipLaunchKernelGGL((fq_apply_kernel<false, false>), grid, block, 0, st, x, y, n, r);
  }
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

DTM_API int dtm_fq_apply_bwd(const void* x, const void* dy, void* dx, int dtype, long n, const void* rec,
                             void* stream) {
  if (!dtm_device_ok()) return -9;
  if (n < 1 || (dtype != 0 && dtype != 1)) return -1;
  if (fq_bad_tensor(x, dtype) || fq_bad_tensor(dy, dtype) || fq_bad_tensor(dx, dtype) || !rec ||
      ((uintptr_t)rec & 3u))
    return -3;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)fq_grid(n, dtype)), block(FQ_THREADS);
  const bool vec = ((((uintptr_t)x ^ (uintptr_t)dy) | ((uintptr_t)x ^ (uintptr_t)dx)) & 15u) == 0;
  const int* r = (const int*)rec;
  if (dtype == 1) {
    if (vec) hipLaunchKernelGGL((fq_apply_bwd_kernel<true, true>), grid, block, 0, st, x, dy, dx, n, r);
    else hipLaunchKernelGGL((fq_apply_bwd_kernel<true, false>), grid, block, 0, st, x, dy, dx, n, r);
  } else {
    if (vec) hipLaunchKernelGGL((fq_apply_bwd_kernel<false, true>), grid, block, 0, st, x, dy, dx, n, r);
    else hipLaunchKernelGGL((fq_apply_bwd_kernel<false, false>), grid, block, 0, st, x, dy, dx, n, r);
  }
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

DTM_API int dtm_fq_advance(void* counter, void* stream) {
  if (!dtm_device_ok()) return -9;
  if (!counter || ((uintptr_t)counter & 7u)) return -3;
  hipLaunchKernelGGL(fq_advance_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, (long long*)counter);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}
