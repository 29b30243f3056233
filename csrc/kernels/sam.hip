// Sharpness-aware minimisation (Foret et al. 2021) and its scale-invariant variant ASAM (Kwon et al. 2021): the
// perturbation of the weights between the two passes of a micro-batch, and its undoing (ops/sam.py, engine.TrainStep).
//   SAM :  S = sum over all rows of g*g        scale = rho / (sqrt(S) + 1e-12)    e = scale * g
//   ASAM:  S = sum of (|p|*g)^2                scale = rho / (sqrt(S) + 1e-12)    e = ((scale * p) * p) * g
//   p_hat = p + e
// S is an fp64 sum in a fixed order, scale is formed in fp64 and rounded once, e and p_hat are fp32 with one rounding
// per operation in the order written and no fused multiply-add, so the torch-op form on CPU tensors gives the same
// bits (the kernel's oracle) and the 16-byte and the 4-byte path agree element by element.
//
// One table of SamTensor rows and the 8192-element chunk list (the layout style of the optimizer's tables).  A row
// with g == nullptr is backup-only (a BN moving mean / variance: the descent forward's in-place update is undone).
// Four launches in stream order, no host decision, float atomic, flag or inter-block wait between them:
//   1 sam_norm_kernel      one block per chunk row -> one fp64 record (backup-only rows: 0)
//   2 sam_finalize_kernel  one block: records summed per tensor (lane l takes records l, l+64, ... in chunk order,
//                          then a xor butterfly), the per-tensor sums the same way in tensor order -> {sqrt(S), scale}
//   3 sam_perturb_kernel   backup = p (bit copy); p = p_hat; pcopy = bf16(p_hat); g = +0 (the zero-grad of the
//                          descent pass); backup-only rows: backup = p
//   4 sam_restore_kernel   p = backup (bit copy); pcopy = bf16(p) (the optimizer's own conversion); g is not touched
// Bytes per element with the bf16 copy: norm 4 (ASAM 8); perturb 8 read + 14 written; restore 4 read + 6 written.
// 16-byte accesses (8 for the bf16 copy) where all arrays a launch touches reach a 16-byte boundary together, with a
// scalar head and tail; coalesced 4-byte accesses otherwise (gradients are views into the flat buffer at any offset).
// The walk and the fixed-order sums are chunk_walk.h's.
#include "chunk_walk.h"

namespace dtm {

struct SamTensor {
  float* p;
  float* g;       // nullptr: backup-only row
  float* backup;  // allocated at p's own offset from a 16-byte boundary
  bf16_t* pcopy;  // optional bf16 compute copy
  long n;
};
constexpr int SAM_CHUNK = 8192;
constexpr int SAM_FIN_THREADS = 1024;

template <bool ADAPTIVE>
__device__ __forceinline__ double sam_term(float p, float g) {
#pragma clang fp contract(off)
  const float x = ADAPTIVE ? fabsf(p) * g : g;
  return (double)x * (double)x;
}

template <bool ADAPTIVE>
__global__ __launch_bounds__(256) void sam_norm_kernel(const SamTensor* __restrict__ tens,
                                                       const ChunkRow* __restrict__ chunks, double* __restrict__ recs) {
  const int tid = threadIdx.x;
  const ChunkRow c = chunks[blockIdx.x];
  const SamTensor t = tens[c.t];
  double a[1] = {0.0};
  if (t.g) {
    const float* pp = t.p + c.start;  // (read by ASAM only)
    const float* gp = t.g + c.start;
    const WalkPlan w =
        walk_plan(4, (uintptr_t)gp, chunk_len(t.n, c.start, SAM_CHUNK), !ADAPTIVE || same16(gp, pp));
    const f32x4* pv = (const f32x4*)(pp + w.head);
    const f32x4* gv = (const f32x4*)(gp + w.head);
    walk<256, 4>(
        w, tid, [&](int i) { a[0] += sam_term<ADAPTIVE>(ADAPTIVE ? pp[i] : 0.f, gp[i]); },
        [&](int i, int) {
          const f32x4 gw = gv[i];
          f32x4 pw = {0.f, 0.f, 0.f, 0.f};
          if constexpr (ADAPTIVE) pw = pv[i];
#pragma unroll
          for (int e = 0; e < 4; ++e) a[0] += sam_term<ADAPTIVE>(pw[e], gw[e]);
        });
  }
  block_sum_f64(a, tid);
  if (tid == 0) recs[blockIdx.x] = a[0];
}

__global__ __launch_bounds__(SAM_FIN_THREADS) void sam_finalize_kernel(const ChunkSpan* __restrict__ meta, int ntens,
                                                                       const double* __restrict__ recs,
                                                                       double* __restrict__ tsum, double rho,
                                                                       float* __restrict__ out) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  double s[1];
  for (int t = wv; t < ntens; t += SAM_FIN_THREADS / 64) {  // one wave per tensor
    record_sum(recs, meta[t], lane, s);
    if (lane == 0) tsum[t] = s[0];
  }
  __syncthreads();
  if (wv == 0) {  // the per-tensor sums the same way, in tensor order
    record_sum((const double*)tsum, ChunkSpan{0, ntens}, lane, s);
    if (lane == 0) {
      const double nrm = sqrt(s[0]);
      out[0] = (float)nrm;
      out[1] = (float)(rho / (nrm + 1e-12));
    }
  }
}

// p_hat of one element: one rounding per operation, in the order written
template <bool ADAPTIVE>
__device__ __forceinline__ float sam_phat(float p, float g, float scale) {
#pragma clang fp contract(off)
  float e;
  if constexpr (ADAPTIVE) {
    const float a = scale * p;
    const float b = a * p;
    e = b * g;
  } else {
    e = scale * g;
  }
  const float r = p + e;
  return r;
}

template <bool ADAPTIVE>
__global__ __launch_bounds__(256) void sam_perturb_kernel(const SamTensor* __restrict__ tens,
                                                          const ChunkRow* __restrict__ chunks,
                                                          const float* __restrict__ rec) {
  const int tid = threadIdx.x;
  const ChunkRow c = chunks[blockIdx.x];
  const SamTensor t = tens[c.t];
  const int len = chunk_len(t.n, c.start, SAM_CHUNK);
  float* pp = t.p + c.start;
  float* bp = t.backup + c.start;
  if (!t.g) {  // backup-only row: a bit copy
    const uint32_t* src = (const uint32_t*)pp;
    uint32_t* dst = (uint32_t*)bp;
    for (int i = tid; i < len; i += 256) dst[i] = src[i];
    return;
  }
  const float scale = rec[1];
  float* gp = t.g + c.start;
  bf16_t* cp = t.pcopy ? t.pcopy + c.start : nullptr;

  const WalkPlan w = walk_plan(4, (uintptr_t)pp, len, same16(pp, gp, bp) && copy8_ok(cp, (uintptr_t)pp));
  f32x4* pv = (f32x4*)(pp + w.head);
  f32x4* gv = (f32x4*)(gp + w.head);
  uint4* bv = (uint4*)(bp + w.head);
  walk<256, 4>(
      w, tid,
      [&](int i) {
        const float p = pp[i];
        const float r = sam_phat<ADAPTIVE>(p, gp[i], scale);
        ((uint32_t*)bp)[i] = __float_as_uint(p);
        pp[i] = r;
        if (cp) cp[i] = f2bf(r);
        gp[i] = 0.f;
      },
      [&](int i, int) {
        const f32x4 pw = pv[i], gw = gv[i];
        f32x4 rw;
#pragma unroll
        for (int e = 0; e < 4; ++e) rw[e] = sam_phat<ADAPTIVE>(pw[e], gw[e], scale);
        bv[i] = make_uint4(__float_as_uint(pw[0]), __float_as_uint(pw[1]), __float_as_uint(pw[2]),
                           __float_as_uint(pw[3]));
        pv[i] = rw;
        if (cp) store_bf16x4(cp + w.head, i, rw);
        gv[i] = f32x4{0.f, 0.f, 0.f, 0.f};
      });
}

__global__ __launch_bounds__(256) void sam_restore_kernel(const SamTensor* __restrict__ tens,
                                                          const ChunkRow* __restrict__ chunks) {
  const int tid = threadIdx.x;
  const ChunkRow c = chunks[blockIdx.x];
  const SamTensor t = tens[c.t];
  uint32_t* pp = (uint32_t*)(t.p + c.start);
  const uint32_t* bp = (const uint32_t*)(t.backup + c.start);
  bf16_t* cp = (t.g && t.pcopy) ? t.pcopy + c.start : nullptr;

  const WalkPlan w = walk_plan(4, (uintptr_t)pp, chunk_len(t.n, c.start, SAM_CHUNK),
                               same16(pp, bp) && copy8_ok(cp, (uintptr_t)pp));
  uint4* pv = (uint4*)(pp + w.head);
  const uint4* bv = (const uint4*)(bp + w.head);
  walk<256, 4>(
      w, tid,
      [&](int i) {
        const uint32_t b = bp[i];
        pp[i] = b;
        if (cp) cp[i] = f2bf(__uint_as_float(b));
      },
      [&](int i, int) {
        const uint4 b = bv[i];
        pv[i] = b;
        if (cp)
          store_bf16x4(cp + w.head, i,
                       f32x4{__uint_as_float(b.x), __uint_as_float(b.y), __uint_as_float(b.z), __uint_as_float(b.w)});
      });
}

}  // namespace dtm
using namespace dtm;

DTM_API int dtm_sam_chunk_size() { return SAM_CHUNK; }
DTM_API int dtm_sam_tensor_bytes() { return (int)sizeof(SamTensor); }
DTM_API int dtm_sam_chunk_bytes() { return (int)sizeof(ChunkRow); }
DTM_API int dtm_sam_meta_bytes() { return (int)sizeof(ChunkSpan); }
// scratch: one fp64 record per chunk row, then one fp64 sum per tensor
DTM_API long dtm_sam_scratch_bytes(int num_chunks, int ntens) {
  return 8L * ((long)(num_chunks > 0 ? num_chunks : 0) + (long)(ntens > 0 ? ntens : 0));
}

// Launches 1-3.  tensors / chunks / meta: the device tables; scratch: dtm_sam_scratch_bytes; out: two fp32
// {sqrt(S), scale}.  Nothing is allocated or read back, so the launches can be captured into a hipGraph.  Returns a
// negative code and launches nothing for a bad argument (rho <= 0 or not finite: -2; an empty table: -3).
DTM_API int dtm_sam_perturb(const void* tensors_dev, const void* chunks_dev, int num_chunks, const void* meta_dev,
                            int ntens, double rho, int adaptive, void* scratch, void* out, void* stream) {
  if (!(rho > 0.0) || !(rho <= 1.7976931348623157e308)) return -2;
  if (num_chunks <= 0 || ntens <= 0) return -3;
  if (!tensors_dev || !chunks_dev || !meta_dev || !scratch || !out) return -1;
  hipStream_t st = (hipStream_t)stream;
  const SamTensor* tens = (const SamTensor*)tensors_dev;
  const ChunkRow* chunks = (const ChunkRow*)chunks_dev;
  double* recs = (double*)scratch;
  double* tsum = recs + num_chunks;
  const dim3 grid((unsigned)num_chunks), block(256);
  if (adaptive) hipLaunchKernelGGL(sam_norm_kernel<true>, grid, block, 0, st, tens, chunks, recs);
  else hipLaunchKernelGGL(sam_norm_kernel<false>, grid, block, 0, st, tens, chunks, recs);
  hipLaunchKernelGGL(sam_finalize_kernel, dim3(1), dim3(SAM_FIN_THREADS), 0, st, (const ChunkSpan*)meta_dev, ntens,
                     (const double*)recs, tsum, rho, (float*)out);
  if (adaptive) hipLaunchKernelGGL(sam_perturb_kernel<true>, grid, block, 0, st, tens, chunks, (const float*)out);
  else hipLaunchKernelGGL(sam_perturb_kernel<false>, grid, block, 0, st, tens, chunks, (const float*)out);
  return 0;
}

// Launch 4.  The same argument checks as dtm_sam_perturb (rho is the configuration's: a restore belongs to a perturb).
DTM_API int dtm_sam_restore(const void* tensors_dev, const void* chunks_dev, int num_chunks, double rho,
                            void* stream) {
  if (!(rho > 0.0) || !(rho <= 1.7976931348623157e308)) return -2;
  if (num_chunks <= 0) return -3;
  if (!tensors_dev || !chunks_dev) return -1;
  hipLaunchKernelGGL(sam_restore_kernel, dim3((unsigned)num_chunks), dim3(256), 0, (hipStream_t)stream,
                     (const SamTensor*)tensors_dev, (const ChunkRow*)chunks_dev);
  return 0;
}
