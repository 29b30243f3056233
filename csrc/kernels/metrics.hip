// Streaming evaluation metrics of one batch of logits [B][C] (fp32 or bf16, rows contiguous) against labels [B]
// (int32 or int64): top-1 / top-k counts by the tf.nn.in_top_k rule, the argmax accuracy of tf.metrics.accuracy,
// the softmax cross-entropy, per-class support / correct / predicted counts and an optional confusion matrix,
// ADDED to one device record in two launches with nothing for the host to wait for.
//
// Per row r, x = logits[r], t = labels[r]:
//   valid       0 <= t < C; an invalid row is counted in `skipped` only
//   finite_row  every x[c] is finite
//   greater     #{c : x[c] > x[t]};  in_top_k(k) = isfinite(x[t]) && greater < k  (in_top_k_kernel's rule: ties at
//               the boundary are in, a NaN elsewhere in the row is not greater)
//   pred        argmax, the lowest index among equal maxima (finite rows only)
//   loss        log(sum_c exp(x[c] - m)) + m - x[t], m = max_c x[c] (finite rows only).  The exp-sum and its log are
//               fp32; the last two terms are combined in fp64 (m - x[t] can exceed FLT_MAX for finite fp32 logits)
//               and the row's loss is kept as fp64.
// A valid row that is not finite counts in `nonfinite`, examples, top1, topk and support, and in nothing else.
//
// Record (int64 words): [0] examples [1] skipped [2] nonfinite [3] loss_rows [4] top1 [5] topk [6] argmax_correct
//   [7] loss_sum (fp64 bits), then support[C], top1_correct[C], predicted[C] and, optionally, confusion[C][C]
//   (row = label, column = pred).
//
// eval_metrics_rows_kernel: one wave per row, four rows per block.  Reads x[t] first, then the row twice (the
//   second time from cache) with 16-byte loads over the aligned body and a scalar head and tail (rows start at any
//   element: odd C, views).  Adds the per-class counts with INTEGER atomics (order-independent) and writes the row's
//   fp64 loss and a flag word with plain stores.
// eval_metrics_finalize_kernel: ONE block sums the flag bits and, thread-strided then by a fixed butterfly and a
//   fixed order over the waves, the fp64 row losses, and adds the batch totals to the record's header - the block's
//   thread 0 is the header's only writer, ordered by the stream, so no atomics and no floating-point atomics at
//   all: the record is bit-identical from run to run.
#include <float.h>
#include <limits.h>

#include "chunk_walk.h"

namespace dtm {

constexpr int METRICS_HEADER = 8;  // int64 words in front of the per-class arrays
constexpr int METRICS_MAX_CLASSES = 65536;
constexpr int METRICS_MAX_CONFUSION_CLASSES = 4096;  // 128 MB of int64
constexpr int METRICS_MAX_BATCH = 65536;
constexpr int METRICS_FIN_THREADS = 1024;

enum : unsigned {
  MF_VALID = 1u, MF_FINITE = 2u, MF_TOP1 = 4u, MF_TOPK = 8u, MF_ARGMAX = 16u,
};

template <typename T>
__global__ __launch_bounds__(256) void eval_metrics_rows_kernel(const void* __restrict__ logits,
                                                                const void* __restrict__ labels, int lab64, int B,
                                                                int C, int k, int confusion,
                                                                unsigned long long* __restrict__ rec,
                                                                double* __restrict__ rowloss,
                                                                unsigned* __restrict__ flags) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= B) return;
  const long long t = lab64 ? ((const long long*)labels)[row] : (long long)((const int*)labels)[row];
  if (t < 0 || t >= C) {  // (wave-uniform)
    if (lane == 0) { flags[row] = 0u; rowloss[row] = 0.0; }
    return;
  }
  const T* xrow = (const T*)logits + (long)row * C;
  const float xt = elem_f32(xrow[t]);

  float m = -INFINITY;
  int idx = INT_MAX, greater = 0;
  bool fin = true;
  visit_row<64>(xrow, C, lane, [&](int c, float v) {  // each lane its own share of the row, in increasing c
    fin = fin && fabsf(v) <= FLT_MAX;
    greater += v > xt ? 1 : 0;
    if (v > m) { m = v; idx = c; }  // strictly greater, c increasing: the lane's lowest index of its maximum
  });
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    greater += __shfl_xor(greater, o, 64);
    const float om = __shfl_xor(m, o, 64);
    const int oi = __shfl_xor(idx, o, 64);
    if (om > m || (om == m && oi < idx)) { m = om; idx = oi; }
  }
  const bool finite_row = __all(fin) != 0;
  const bool xt_fin = fabsf(xt) <= FLT_MAX;
  const bool top1 = xt_fin && greater < 1, topk = xt_fin && greater < k;

  double loss = 0.0;
  if (finite_row) {  // (wave-uniform)
    float s = 0.f;
    visit_row<64>(xrow, C, lane, [&](int, float v) { s += expf(v - m); });
    s = warp_sum(s);  // fixed order: the lane's elements in index order, then the xor butterfly
    loss = (double)logf(s) + ((double)m - (double)xt);
  }
  if (lane == 0) {
    const unsigned long long one = 1ull;
    unsigned long long* cls = rec + METRICS_HEADER;
    atomicAdd(cls + t, one);                                // support
    if (top1) atomicAdd(cls + C + t, one);                  // top1_correct
    if (finite_row) {
      atomicAdd(cls + 2 * (long)C + idx, one);              // predicted
      if (confusion) atomicAdd(cls + 3 * (long)C + t * C + idx, one);
    }
    flags[row] = MF_VALID | (finite_row ? MF_FINITE : 0u) | (top1 ? MF_TOP1 : 0u) | (topk ? MF_TOPK : 0u) |
                 (finite_row && idx == (int)t ? MF_ARGMAX : 0u);
    rowloss[row] = loss;
  }
}

__global__ __launch_bounds__(METRICS_FIN_THREADS) void eval_metrics_finalize_kernel(
    const double* __restrict__ rowloss, const unsigned* __restrict__ flags, int B,
    unsigned long long* __restrict__ rec) {
  constexpr int NW = METRICS_FIN_THREADS / 64;
  __shared__ double rl[NW];
  __shared__ int rc[NW][5];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  double loss = 0.0;
  int cnt[5] = {0, 0, 0, 0, 0};  // valid, finite, top1, topk, argmax_correct
  for (int r = tid; r < B; r += METRICS_FIN_THREADS) {
    const unsigned f = flags[r];
    loss += rowloss[r];  // (0.0 for a row without a loss)
#pragma unroll
    for (int b = 0; b < 5; ++b) cnt[b] += (int)((f >> b) & 1u);
  }
  loss = wave_sum_f64(loss);
#pragma unroll
  for (int b = 0; b < 5; ++b) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt[b] += __shfl_xor(cnt[b], o, 64);
  }
  if (lane == 0) {
    rl[wv] = loss;
#pragma unroll
    for (int b = 0; b < 5; ++b) rc[wv][b] = cnt[b];
  }
  __syncthreads();
  if (tid == 0) {
    double s = 0.0;
    int c[5] = {0, 0, 0, 0, 0};
    for (int w = 0; w < NW; ++w) {  // wave order
      s += rl[w];
      for (int b = 0; b < 5; ++b) c[b] += rc[w][b];
    }
    rec[0] += (unsigned long long)c[0];        // examples
    rec[1] += (unsigned long long)(B - c[0]);  // skipped
    rec[2] += (unsigned long long)(c[0] - c[1]);  // nonfinite
    rec[3] += (unsigned long long)c[1];        // loss_rows
    rec[4] += (unsigned long long)c[2];        // top1
    rec[5] += (unsigned long long)c[3];        // topk
    rec[6] += (unsigned long long)c[4];        // argmax_correct
    double* ls = (double*)(rec + 7);
    *ls = *ls + s;
  }
}

}  // namespace dtm

using namespace dtm;

DTM_API int dtm_metrics_header_words() { return METRICS_HEADER; }
DTM_API int dtm_metrics_max_classes() { return METRICS_MAX_CLASSES; }
DTM_API int dtm_metrics_max_confusion_classes() { return METRICS_MAX_CONFUSION_CLASSES; }
DTM_API int dtm_metrics_max_batch() { return METRICS_MAX_BATCH; }

// logits [B][C] rows contiguous, aligned to the element size only; dtype 0 = fp32, 1 = bf16; labels int32 (lab64 = 0)
// or int64; rec: the record above (8-byte aligned); rowloss [>= B] fp64 and flags [>= B] uint32 scratch.
// B == 0 is a no-op; any other violation of a limit returns a negative code and launches nothing.
DTM_API int dtm_eval_metrics(const void* logits, int dtype, const void* labels, int lab64, int B, int C, int k,
                             int confusion, void* rec, void* rowloss, void* flags, void* stream) {
  if (!dtm_device_ok()) return -9;
  if (B == 0) return 0;
  if (B < 0 || B > METRICS_MAX_BATCH || C < 1 || C > METRICS_MAX_CLASSES || k < 1 || k > C) return -1;
  if (confusion && C > METRICS_MAX_CONFUSION_CLASSES) return -1;
  if (dtype != 0 && dtype != 1) return -1;
  if (!logits || !labels || !rec || !rowloss || !flags) return -1;
  if (((uintptr_t)logits & (dtype == 1 ? 1u : 3u)) || ((uintptr_t)labels & (lab64 ? 7u : 3u)) ||
      ((uintptr_t)rec & 7u) || ((uintptr_t)rowloss & 7u) || ((uintptr_t)flags & 3u))
    return -3;
  hipStream_t st = (hipStream_t)stream;
  const unsigned grid = (unsigned)((B + 3) / 4);
  if (dtype == 1)
    hipLaunchKernelGGL(eval_metrics_rows_kernel<bf16_t>, dim3(grid), dim3(256), 0, st, logits, labels, lab64, B, C, k,
                       confusion, (unsigned long long*)rec, (double*)rowloss, (unsigned*)flags);
  else
    hipLaunchKernelGGL(eval_metrics_rows_kernel<float>, dim3(grid), dim3(256), 0, st, logits, labels, lab64, B, C, k,
                       confusion, (unsigned long long*)rec, (double*)rowloss, (unsigned*)flags);
  hipLaunchKernelGGL(eval_metrics_finalize_kernel, dim3(1), dim3(METRICS_FIN_THREADS), 0, st,
                     (const double*)rowloss, (const unsigned*)flags, B, (unsigned long long*)rec);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}
