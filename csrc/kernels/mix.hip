// Mixup / CutMix of one NHWC batch in one launch (ops/mix.py): out[r] is row r of x blended with, or patched from,
// row partner[r] of the same batch, as the batch's plan says.  The plan is data: one 32-byte record per row,
//   [partner, bits(w_pix), bits(w_lab), y0, y1, x0, x1, 0]          (int32; the weights are fp32 bit patterns)
// so a captured launch replays whatever kind of mixing the record of the step holds.  Per element of row r, with
// a = x[r], b = x[partner] and w = w_pix:
//   inside the box [y0, y1) x [x0, x1)     the bits of b
//   outside it, w == 1                     the bits of a
//   otherwise                              fp32 (w * a) + ((1 - w) * b), each product and the sum rounded on its own,
//                                          rounded to the storage type with f2bf
// The first two are bit copies: a NaN or an Inf of the source that does not contribute never reaches out.
// The records are trusted (the Python wrapper validates the host copy): 0 <= partner < B, box inside the image.
//
// Memory-bound: 3 element sizes per blended element (two reads, one write), 2 per copied or patched one.  A row may
// start at any element (a batch is a view into a larger buffer, and rows of 299 x 299 x 3 bf16 are no multiple of 16
// bytes).  Where the row of out and the source rows it reads agree modulo 16 bytes, the body moves 16 bytes per lane
// with an up-to-7-element head and tail done by the row's first block; a vector that lies on one side of the box
// loads only the source it takes.  Otherwise every access is a coalesced element access.  With C = 3 a vector
// straddles pixels and box edges, so the box test is per element: element e of a row is inside when
// e / (W*C) is in [y0, y1) and e % (W*C) is in [x0*C, x1*C) - one division per vector, then increments.
#include "common.h"

namespace dtm {

template <typename U>
struct MixElem;
template <>
struct MixElem<uint16_t> {  // bf16
  static constexpr int VEC = 8;
  static __device__ __forceinline__ float to_f(uint32_t v) { return __uint_as_float(v << 16); }
  static __device__ __forceinline__ uint32_t from_f(float f) { return (uint32_t)f2bf(f); }
  static __device__ __forceinline__ uint32_t get(const uint4& v, int j) {
    const uint32_t wd = j < 2 ? v.x : j < 4 ? v.y : j < 6 ? v.z : v.w;
    return (j & 1) ? wd >> 16 : wd & 0xffffu;
  }
  static __device__ __forceinline__ uint4 pack(const uint32_t* e) {
    return make_uint4(e[0] | (e[1] << 16), e[2] | (e[3] << 16), e[4] | (e[5] << 16), e[6] | (e[7] << 16));
  }
};
template <>
struct MixElem<uint32_t> {  // fp32
  static constexpr int VEC = 4;
  static __device__ __forceinline__ float to_f(uint32_t v) { return __uint_as_float(v); }
  static __device__ __forceinline__ uint32_t from_f(float f) { return __float_as_uint(f); }
  static __device__ __forceinline__ uint32_t get(const uint4& v, int j) {
    return j == 0 ? v.x : j == 1 ? v.y : j == 2 ? v.z : v.w;
  }
  static __device__ __forceinline__ uint4 pack(const uint32_t* e) { return make_uint4(e[0], e[1], e[2], e[3]); }
};

// (w * a) + (omw * b) with three roundings.  Plain operators under contract(off): the __fmul_rn / __fadd_rn of the
// HIP headers are plain operators too, and after inlining the compiler may contract them into one fma.
template <typename U>
__device__ __forceinline__ uint32_t mix_blend(uint32_t a, uint32_t b, float w, float omw) {
#pragma clang fp contract(off)
  const float pa = w * MixElem<U>::to_f(a);
  const float pb = omw * MixElem<U>::to_f(b);
  const float s = pa + pb;
  return MixElem<U>::from_f(s);
}

template <typename U>
__device__ __forceinline__ uint32_t mix_one(uint32_t a, uint32_t b, bool inbox, bool copy_a, float w, float omw) {
  return inbox ? b : copy_a ? a : mix_blend<U>(a, b, w, omw);
}

struct MixBox {
  uint32_t y0, y1, q0, q1;  // rows [y0, y1), positions within an image row [q0, q1) = [x0*C, x1*C)
  bool any;
  __device__ __forceinline__ bool in(uint32_t y, uint32_t q) const { return y >= y0 && y < y1 && q >= q0 && q < q1; }
};

// n: elements per row (H*W*C < 2^31); wc = W*C with its magic divisor; grid (blocks per row, rows)
template <typename U>
__global__ __launch_bounds__(256) void mix_images_kernel(const U* __restrict__ x, U* __restrict__ out,
                                                         const int* __restrict__ plan, int B, uint32_t n, uint32_t wc,
                                                         FastDiv dwc, int C) {
  using E = MixElem<U>;
  constexpr int VEC = E::VEC;
  const uint32_t tid = blockIdx.x * 256u + threadIdx.x, nthr = gridDim.x * 256u;
  for (int r = blockIdx.y; r < B; r += gridDim.y) {
    // the record: the same addresses in every lane, read once per wave
    const int* rec = plan + (long)r * 8;
    const int partner = rec[0];
    const float w = __int_as_float(rec[1]);
    const int y0 = rec[3], y1 = rec[4], x0 = rec[5], x1 = rec[6];
    MixBox box;
    box.any = y1 > y0 && x1 > x0;
    box.y0 = (uint32_t)y0; box.y1 = (uint32_t)y1; box.q0 = (uint32_t)(x0 * C); box.q1 = (uint32_t)(x1 * C);
    const bool copy_a = w == 1.f;
    float omw;
    {
#pragma clang fp contract(off)
      omw = 1.f - w;
    }
    const U* __restrict__ pa = x + (long)r * n;
    const U* __restrict__ pb = x + (long)partner * n;
    U* __restrict__ po = out + (long)r * n;
    const bool uses_b = box.any || !copy_a;

    auto scalar = [&](uint32_t e) {
      bool in = false;
      if (box.any) {
        const uint32_t y = fdiv(e, dwc);
        in = box.in(y, e - y * wc);
      }
      uint32_t a = 0u, b = 0u;
      if (!in) a = pa[e];
      if (in || !copy_a) b = pb[e];
      po[e] = (U)mix_one<U>(a, b, in, copy_a, w, omw);
    };

    const uintptr_t ao = (uintptr_t)po, aa = (uintptr_t)pa, ab = (uintptr_t)pb;
    const bool vec = ((ao ^ aa) & 15u) == 0 && (!uses_b || ((ao ^ ab) & 15u) == 0);
    if (!vec) {
      for (uint32_t e = tid; e < n; e += nthr) scalar(e);
      continue;
    }
    uint32_t head = (uint32_t)(((16u - (uint32_t)(ao & 15u)) & 15u) / sizeof(U));
    head = head < n ? head : n;
    const uint32_t nvec = (n - head) / VEC, tail0 = head + nvec * VEC;
    const uint4* __restrict__ av = reinterpret_cast<const uint4*>(pa + head);
    const uint4* __restrict__ bv = reinterpret_cast<const uint4*>(pb + head);
    uint4* __restrict__ ov = reinterpret_cast<uint4*>(po + head);
    for (uint32_t v = tid; v < nvec; v += nthr) {
      uint32_t mask = 0u;
      if (box.any) {
        const uint32_t e0 = head + v * VEC;
        uint32_t y = fdiv(e0, dwc);
        uint32_t q = e0 - y * wc;
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
          mask |= (uint32_t)box.in(y, q) << j;
          if (++q == wc) { q = 0u; ++y; }
        }
      }
      // a vector that lies on one side of the box (or a row that only copies) loads one source
      const bool need_a = mask != (1u << VEC) - 1u;
      const bool need_b = mask != 0u || !copy_a;
      uint4 va = make_uint4(0u, 0u, 0u, 0u), vb = va;
      if (need_a) va = av[v];
      if (need_b) vb = bv[v];
      uint32_t res[VEC];
#pragma unroll
      for (int j = 0; j < VEC; ++j)
        res[j] = mix_one<U>(E::get(va, j), E::get(vb, j), (mask >> j) & 1u, copy_a, w, omw);
      ov[v] = E::pack(res);
    }
    if (blockIdx.x == 0) {  // head and tail: fewer than VEC elements each
      if (threadIdx.x < head) scalar(threadIdx.x);
      if (tail0 + threadIdx.x < n) scalar(tail0 + threadIdx.x);
    }
  }
}

}  // namespace dtm
using namespace dtm;

// x, out: B rows of H*W*C elements (bf16 or fp32), contiguous, not overlapping; plan: B records of 8 int32 on the
// device.  One launch on ``stream``; nothing is allocated or read back, so the launch can be captured into a
// hipGraph.  Returns -1 for a bad argument, -2 where x and out overlap.
DTM_API int dtm_mix_images(const void* x, void* out, const int* plan, int B, int H, int W, int C, int bf16,
                           void* stream) {
  if (!x || !out || !plan || B < 1 || H < 1 || W < 1 || C < 1) return -1;
  const long n = (long)H * W * C;
  if (n >= (1L << 31) || (long)W * C >= (1L << 31)) return -1;
  const size_t es = bf16 ? 2 : 4;
  const uintptr_t px = (uintptr_t)x, po = (uintptr_t)out;
  if ((px & (es - 1)) || (po & (es - 1)) || ((uintptr_t)plan & 3)) return -1;
  const size_t bytes = (size_t)B * n * es;
  if (px < po + bytes && po < px + bytes) return -2;
  const long vecs = (n * (long)es + 15) / 16;
  long bpr = (vecs + 255) / 256;                             // one 16-byte vector per lane ...
  const long cap = (8L * dtm_compute_cus() + B - 1) / B;     // ... up to 8 blocks per CU over the batch
  if (bpr > cap) bpr = cap;
  if (bpr < 1) bpr = 1;
  const dim3 grid((unsigned)bpr, (unsigned)(B > 65535 ? 65535 : B)), block(256);
  const uint32_t wc = (uint32_t)(W * C);
  const FastDiv dwc = make_fastdiv(wc);
  hipStream_t st = (hipStream_t)stream;
  if (bf16)
    hipLaunchKernelGGL(mix_images_kernel<uint16_t>, grid, block, 0, st, (const uint16_t*)x, (uint16_t*)out, plan, B,
                       (uint32_t)n, wc, dwc, C);
  else
    hipLaunchKernelGGL(mix_images_kernel<uint32_t>, grid, block, 0, st, (const uint32_t*)x, (uint32_t*)out, plan, B,
                       (uint32_t)n, wc, dwc, C);
  return 0;
}
