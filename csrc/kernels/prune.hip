// Gradual magnitude pruning (ops/prune.py): an exact k-th-magnitude selection over every pruned weight tensor and the
// mask apply, as multi-tensor launches beside the optimizer's.
//
// Key of an element: bits(w) & 0x7fffffff read as an unsigned integer (-0 == +0, denormals order, Inf / NaN largest).
// Per tensor of n elements at sparsity s: z = floor(double(s) * n); z == 0: the mask is all ones and tau = 0; else
// tau = the z-th smallest key (1-based) and mask = key > tau (ties at tau are all pruned).
//
// Select: a radix select on the 31-bit key, most significant digit first, 11 + 10 + 10 bits.  Per digit two launches:
//   hist  one block per chunk row: counts, in an LDS histogram, the digit of every element whose higher digits equal
//         the prefix found so far, then adds its non-empty bins into the tensor's global histogram (uint32 adds:
//         integer sums do not depend on the order, so the result is the same bits in every run);
//   scan  one block per tensor: finds the bin where the running count crosses the remaining rank, records the
//         extended prefix and the rank inside that bin, and clears the histogram for the next digit.
// After the last digit the prefix is tau.  Stream order is the only synchronisation between the launches.
// On an update step the masks so far are applied first (the apply kernel in its ``pre`` mode, which exits at once
// otherwise): the optimizer has just moved the pruned coordinates off zero, and the selection must see them as the
// zeros they are, so that they are its smallest keys and a mask only ever shrinks.
// Apply (one launch): with the record's update flag set it forms mask = key > tau, stores it (four mask bytes per
// lane in one 32-bit store) and counts the kept elements (one integer add per wave); in both cases it then writes
// w = mask ? w : +0 to the weight, its bf16 compute copy and its EMA shadow.
//
// Everything a step decides lives in the 16-byte device record {double sparsity, int update, int pad}: with
// update == 0 every select kernel exits at once and apply only applies, so one captured graph serves every step.
//
// A tensor may start at any element of a larger buffer: chunk 0 takes the up-to-3-element head in front of the
// first 16-byte boundary with 4-byte accesses, every chunk then moves 16 bytes per lane, the last one ends with a
// 4-byte tail.  A row whose bf16 copy, shadow or mask does not reach its boundary together with the weight has
// vec = 0 and uses 4-byte (2-, 1-byte) accesses throughout.
#include "common.h"

namespace dtm {

constexpr int PR_CHUNK = 8192;   // elements per chunk row (a multiple of 4)
constexpr int PR_BINS = 2048;    // histogram row per tensor (the widest digit)
constexpr int PR_THREADS = 256;

struct PruneTensor {  // 64 bytes
  uint32_t* w;
  bf16_t* w16;       // or null
  uint32_t* shadow;  // or null
  uint8_t* mask;
  long n;
  int chunk0, nchunks;
  int vec;           // 16-byte path allowed
  int pad[3];
};
struct PruneChunk { int t, pad; };  // 8 bytes
struct PruneRec { double sparsity; int update, pad; };
static_assert(sizeof(PruneTensor) == 64 && sizeof(PruneChunk) == 8 && sizeof(PruneRec) == 16, "table layout");

__host__ __device__ __forceinline__ int pr_head(const void* w, long n) {
  const int h = (int)(((16 - ((uintptr_t)w & 15)) & 15) >> 2);
  return h > n ? (int)n : h;
}

// Runs fs(i) over the 4-byte elements and fv(i) over the 16-byte groups (i = first element) of chunk j of tensor T.
template <class FS, class FV>
__device__ __forceinline__ void pr_for_chunk(const PruneTensor& T, int j, FS fs, FV fv) {
  const int tid = threadIdx.x;
  const int head = pr_head(T.w, T.n);
  const long vlo = head + (long)j * PR_CHUNK;  // 16-byte aligned
  long hi = vlo + PR_CHUNK;
  if (hi > T.n) hi = T.n;
  if (!T.vec) {
    for (long i = (j == 0 ? 0 : vlo) + tid; i < hi; i += PR_THREADS) fs(i);
    return;
  }
  if (j == 0 && tid < head) fs((long)tid);
  if (vlo >= hi) return;
  const long nvec = (hi - vlo) >> 2;
  for (long v = tid; v < nvec; v += PR_THREADS) fv(vlo + (v << 2));
  const long t0 = vlo + (nvec << 2);
  if (t0 + tid < hi) fs(t0 + tid);
}

__global__ __launch_bounds__(PR_THREADS) void prune_init_kernel(const PruneTensor* __restrict__ tens,
                                                                const PruneRec* __restrict__ rec,
                                                                uint2* __restrict__ state, uint32_t* __restrict__ hist,
                                                                uint32_t* __restrict__ tau, int* __restrict__ kept,
                                                                int* __restrict__ z) {
  if (rec->update == 0) return;
  const int t = blockIdx.x;
  for (int b = threadIdx.x; b < PR_BINS; b += PR_THREADS) hist[(long)t * PR_BINS + b] = 0u;
  if (threadIdx.x == 0) {
    const int zz = (int)floor(rec->sparsity * (double)tens[t].n);
    z[t] = zz;
    state[t] = make_uint2(0u, (uint32_t)zz);
    kept[t] = 0;
    if (zz == 0) tau[t] = 0u;
  }
}

// digit = (key >> shift) & (2^bits - 1); counted where key >> (shift + bits) == the prefix so far
// Keys that are exactly 0 (what pruning leaves behind: half the tensor at sparsity 0.5, all in bin 0 of every digit)
// are counted in a register and added once per wave instead of one LDS add each.  Measured on ResNet-50's 25.5 M
// weights (profiles/prune_bench.log): the first digit's launch on half-zero weights 0.052 -> 0.026 ms, on dense
// N(0, 0.05^2) weights 0.0258 -> 0.0266 ms.  Plain LDS adds otherwise: one sub-histogram per wave (0.031 ms) and a
// ballot / match on equal digits before the add (0.37 ms) both lost to them on dense and on few-exponent weights.
__global__ __launch_bounds__(PR_THREADS) void prune_hist_kernel(const PruneTensor* __restrict__ tens,
                                                                const PruneChunk* __restrict__ chunks,
                                                                const PruneRec* __restrict__ rec,
                                                                const uint2* __restrict__ state,
                                                                const int* __restrict__ z, uint32_t* __restrict__ hist,
                                                                int shift, int bits) {
  if (rec->update == 0) return;
  const int t = chunks[blockIdx.x].t;
  if (z[t] == 0) return;
  __shared__ uint32_t h[PR_BINS];
  const PruneTensor T = tens[t];
  const int nb = 1 << bits;
  const uint32_t prefix = state[t].x, dmask = (uint32_t)nb - 1u;
  const int hs = shift + bits;  // <= 31, and key < 2^31: digit 0 compares 0 with the prefix 0
  for (int b = threadIdx.x; b < nb; b += PR_THREADS) h[b] = 0u;
  __syncthreads();
  uint32_t zeros = 0u;
  auto add = [&](uint32_t bitsw) {
    const uint32_t key = bitsw & 0x7fffffffu;
    if (key == 0u) { ++zeros; return; }
    if ((key >> hs) == prefix) atomicAdd(&h[(key >> shift) & dmask], 1u);
  };
  pr_for_chunk(
      T, blockIdx.x - T.chunk0, [&](long i) { add(T.w[i]); },
      [&](long i) {
        const uint4 x = *reinterpret_cast<const uint4*>(T.w + i);
        add(x.x); add(x.y); add(x.z); add(x.w);
      });
  if (prefix == 0u) {  // (a key of 0 has every higher digit 0)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) zeros += __shfl_xor(zeros, o, 64);
    if ((threadIdx.x & 63) == 0 && zeros != 0u) atomicAdd(&h[0], zeros);
  }
  __syncthreads();
  for (int b = threadIdx.x; b < nb; b += PR_THREADS) {
    const uint32_t c = h[b];
    if (c != 0u) atomicAdd(&hist[(long)t * PR_BINS + b], c);
  }
}

// one block per tensor: the bin with  count before it < rank <= count through it  (rank is 1-based)
__global__ __launch_bounds__(PR_THREADS) void prune_scan_kernel(const PruneRec* __restrict__ rec,
                                                                const int* __restrict__ z, uint2* __restrict__ state,
                                                                uint32_t* __restrict__ hist, uint32_t* __restrict__ tau,
                                                                int bits, int last) {
  if (rec->update == 0) return;
  const int t = blockIdx.x, tid = threadIdx.x;
  if (z[t] == 0) return;
  const uint2 st = state[t];
  const int per = (1 << bits) / PR_THREADS;  // 8 or 4 consecutive bins per lane
  uint32_t c[PR_BINS / PR_THREADS];
  uint32_t sum = 0u;
  uint32_t* row = hist + (long)t * PR_BINS + tid * per;
#pragma unroll
  for (int k = 0; k < PR_BINS / PR_THREADS; ++k) {
    c[k] = 0u;
    if (k < per) { c[k] = row[k]; row[k] = 0u; }
    sum += c[k];
  }
  __shared__ uint32_t s[PR_THREADS];
  s[tid] = sum;
  __syncthreads();  // (also: every lane has read state[t] before the one store below)
  for (int off = 1; off < PR_THREADS; off <<= 1) {
    const uint32_t v = tid >= off ? s[tid - off] : 0u;
    __syncthreads();
    s[tid] += v;
    __syncthreads();
  }
  uint32_t run = s[tid] - sum;
#pragma unroll
  for (int k = 0; k < PR_BINS / PR_THREADS; ++k) {
    if (k < per && run < st.y && st.y <= run + c[k]) {
      const uint32_t p = (st.x << bits) | (uint32_t)(tid * per + k);
      state[t] = make_uint2(p, st.y - run);
      if (last) tau[t] = p;
    }
    run += c[k];
  }
}

__device__ __forceinline__ uint32_t pr_keep(uint32_t bitsw, uint32_t ta, bool all) {
  return (all || (bitsw & 0x7fffffffu) > ta) ? 1u : 0u;
}

__global__ __launch_bounds__(PR_THREADS) void prune_apply_kernel(const PruneTensor* __restrict__ tens,
                                                                 const PruneChunk* __restrict__ chunks,
                                                                 const PruneRec* __restrict__ rec,
                                                                 const uint32_t* __restrict__ tau,
                                                                 int* __restrict__ kept, const int* __restrict__ z,
                                                                 int pre) {
  if (pre && rec->update == 0) return;
  const int t = chunks[blockIdx.x].t;
  const PruneTensor T = tens[t];
  const bool upd = !pre && rec->update != 0;  // pre: the stored masks, applied in front of an update's selection
  uint32_t ta = 0u;
  bool all = false;
  if (upd) { ta = tau[t]; all = z[t] == 0; }
  int cnt = 0;
  pr_for_chunk(
      T, blockIdx.x - T.chunk0,
      [&](long i) {
        uint32_t m;
        if (upd) {
          m = pr_keep(T.w[i], ta, all);
          T.mask[i] = (uint8_t)m;
          cnt += (int)m;
        } else {
          m = T.mask[i];
        }
        if (m == 0u) {
          T.w[i] = 0u;
          if (T.w16) T.w16[i] = 0;
          if (T.shadow) T.shadow[i] = 0u;
        }
      },
      [&](long i) {
        uint4* wp = reinterpret_cast<uint4*>(T.w + i);
        uint32_t* mp = reinterpret_cast<uint32_t*>(T.mask + i);
        uint4 x;
        uint32_t mm;
        if (upd) {
          x = *wp;
          mm = pr_keep(x.x, ta, all) | (pr_keep(x.y, ta, all) << 8) | (pr_keep(x.z, ta, all) << 16) |
               (pr_keep(x.w, ta, all) << 24);
          *mp = mm;
          cnt += __popc(mm);
        } else {
          mm = *mp;
          if (mm == 0x01010101u) return;
          x = *wp;
        }
        if (mm == 0x01010101u) return;
        const bool k0 = (mm & 0xffu) != 0u, k1 = (mm & 0xff00u) != 0u, k2 = (mm & 0xff0000u) != 0u,
                   k3 = (mm & 0xff000000u) != 0u;
        x.x = k0 ? x.x : 0u; x.y = k1 ? x.y : 0u; x.z = k2 ? x.z : 0u; x.w = k3 ? x.w : 0u;
        *wp = x;
        if (T.w16) {
          uint2* bp = reinterpret_cast<uint2*>(T.w16 + i);
          uint2 b = *bp;
          b.x &= (k0 ? 0x0000ffffu : 0u) | (k1 ? 0xffff0000u : 0u);
          b.y &= (k2 ? 0x0000ffffu : 0u) | (k3 ? 0xffff0000u : 0u);
          *bp = b;
        }
        if (T.shadow) {
          uint4* sp = reinterpret_cast<uint4*>(T.shadow + i);
          uint4 s = *sp;
          s.x = k0 ? s.x : 0u; s.y = k1 ? s.y : 0u; s.z = k2 ? s.z : 0u; s.w = k3 ? s.w : 0u;
          *sp = s;
        }
      });
  if (upd) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
    if ((threadIdx.x & 63) == 0 && cnt != 0) atomicAdd(&kept[t], cnt);
  }
}

}  // namespace dtm
using namespace dtm;

DTM_API int dtm_prune_tensor_bytes() { return (int)sizeof(PruneTensor); }
DTM_API int dtm_prune_chunk_bytes() { return (int)sizeof(PruneChunk); }
DTM_API int dtm_prune_rec_bytes() { return (int)sizeof(PruneRec); }
DTM_API int dtm_prune_chunk_size() { return PR_CHUNK; }
DTM_API int dtm_prune_hist_bins() { return PR_BINS; }

// chunk rows of a tensor of n fp32 elements that starts at address w; -2: n outside [1, 2^31)
DTM_API long dtm_prune_num_chunks(const void* w, long n) {
  if (n < 1 || n >= (1L << 31)) return -2;
  const long body = n - pr_head(w, n);
  return body <= 0 ? 1 : (body + PR_CHUNK - 1) / PR_CHUNK;
}

// Fills one host row of the device record.  -3 (and the row untouched): sparsity outside [0, 1) or NaN.
DTM_API int dtm_prune_fill_record(void* row, double sparsity, int update) {
  if (!row) return -1;
  if (!(sparsity >= 0.0 && sparsity < 1.0)) return -3;
  PruneRec r;
  r.sparsity = sparsity;
  r.update = update ? 1 : 0;
  r.pad = 0;
  *reinterpret_cast<PruneRec*>(row) = r;
  return 0;
}

static int pr_check(const void* tens, int ntens, const void* chunks, int nchunks, const void* rec, long max_n) {
  if (!tens || !chunks || !rec || ntens < 1 || nchunks < ntens) return -1;
  if (max_n < 1 || max_n >= (1L << 31)) return -2;  // counts are uint32, z and kept int32
  return 0;
}

static const int PR_SHIFT[3] = {20, 10, 0}, PR_BITS[3] = {11, 10, 10};

static void pr_launch_hist(int nchunks, hipStream_t st, const PruneTensor* T, const PruneChunk* C, const PruneRec* R,
                           const uint2* state, const int* z, uint32_t* hist, int d) {
  const dim3 grid((unsigned)nchunks), block(PR_THREADS);
  hipLaunchKernelGGL(prune_hist_kernel, grid, block, 0, st, T, C, R, state, z, hist, PR_SHIFT[d], PR_BITS[d]);
}

// One histogram launch of digit ``digit`` alone (tools/prune_bench.py times it); ``state`` and ``z`` as a select left
// them.
DTM_API int dtm_prune_hist_stage(const void* tens, int ntens, const void* chunks, int nchunks, const void* rec,
                                 const void* state, const void* z, void* hist, int digit, long max_n, void* stream) {
  const int rc = pr_check(tens, ntens, chunks, nchunks, rec, max_n);
  if (rc != 0) return rc;
  if (!state || !z || !hist || digit < 0 || digit > 2) return -1;
  pr_launch_hist(nchunks, (hipStream_t)stream, (const PruneTensor*)tens, (const PruneChunk*)chunks,
                 (const PruneRec*)rec, (const uint2*)state, (const int*)z, (uint32_t*)hist, digit);
  return 0;
}

// The select stages: 7 launches that exit at once when the record's update flag is 0.  state: ntens x 8 bytes,
// hist: ntens x 2048 uint32, tau: ntens uint32, kept / z: ntens int32; max_n: the largest element count in the
// table.  Nothing is allocated or read back.  Returns -1 for a bad argument, -2 for max_n >= 2^31 (nothing launched).
DTM_API int dtm_prune_select(const void* tens, int ntens, const void* chunks, int nchunks, const void* rec, void* state,
                             void* hist, void* tau, void* kept, void* z, long max_n, void* stream) {
  const int rc = pr_check(tens, ntens, chunks, nchunks, rec, max_n);
  if (rc != 0) return rc;
  if (!state || !hist || !tau || !kept || !z) return -1;
  hipStream_t st = (hipStream_t)stream;
  const PruneTensor* T = (const PruneTensor*)tens;
  const PruneRec* R = (const PruneRec*)rec;
  hipLaunchKernelGGL(prune_init_kernel, dim3((unsigned)ntens), dim3(PR_THREADS), 0, st, T, R, (uint2*)state,
                     (uint32_t*)hist, (uint32_t*)tau, (int*)kept, (int*)z);
  for (int d = 0; d < 3; ++d) {
    pr_launch_hist(nchunks, st, T, (const PruneChunk*)chunks, R, (const uint2*)state, (const int*)z, (uint32_t*)hist,
                   d);
    hipLaunchKernelGGL(prune_scan_kernel, dim3((unsigned)ntens), dim3(PR_THREADS), 0, st, R, (const int*)z,
                       (uint2*)state, (uint32_t*)hist, (uint32_t*)tau, PR_BITS[d], d == 2 ? 1 : 0);
  }
  return 0;
}

// Mask write (update flag set) + apply, one launch.  ``pre`` != 0: the launch in front of the select stages instead,
// which applies the stored masks when the update flag is set and exits at once when it is not.  Same return codes
// as dtm_prune_select.
DTM_API int dtm_prune_apply(const void* tens, int ntens, const void* chunks, int nchunks, const void* rec,
                            const void* tau, void* kept, const void* z, long max_n, int pre, void* stream) {
  const int rc = pr_check(tens, ntens, chunks, nchunks, rec, max_n);
  if (rc != 0) return rc;
  if (!tau || !kept || !z) return -1;
  hipLaunchKernelGGL(prune_apply_kernel, dim3((unsigned)nchunks), dim3(PR_THREADS), 0, (hipStream_t)stream,
                     (const PruneTensor*)tens, (const PruneChunk*)chunks, (const PruneRec*)rec, (const uint32_t*)tau,
                     (int*)kept, (const int*)z, pre ? 1 : 0);
  return 0;
}
