// Fused softmax cross-entropy (+label smoothing), its two-label and distillation variants, the backward of the
// per-row loss into the padded FC operand and the scalar training loss.
//
// Replaces SoftmaxCrossEntropyWithLogits / sparse variant and slim cross_entropy_loss
// with label smoothing y*(1-eps) + eps/K (reference
// inception/slim/losses.py:142-174, cnn/cifar10.py:298-306).
#include "common.h"

namespace dtm {

template <typename T>
__device__ __forceinline__ float ldf(const T* p, long i);
template <>
__device__ __forceinline__ float ldf<float>(const float* p, long i) { return p[i]; }
template <>
__device__ __forceinline__ float ldf<bf16_t>(const bf16_t* p, long i) { return bf2f(p[i]); }

// one block per row; labels int32; out_loss[row]; dlogits fp32 or bf16 (same type as logits)
// MIX (dtm_softmax_xent_mix): the row has two labels, la = labels[row] and lb = labels[partner], with weights wl and
// 1 - wl from the row's mixing record (mix.hip: [partner, bits(w_pix), bits(w_lab), ...], 8 int32), and the target
//   t_k = off + (on - off) * (wl * [k == la] + (1 - wl) * [k == lb]).
// A target weight of exactly 1 or 0 takes the plain kernel's own expressions, so a row with wl == 1 gets the bits
// softmax_xent_kernel gives it with labels[row]; an out-of-range label contributes nothing, on either side.
// DISTILL (dtm_softmax_xent_distill): a soft-target term against the teacher's row z at temperature T (Hinton et al.
// 2015), with pT = softmax(x / T), q = softmax(z / T) and hard the loss above:
//   kl   = sum_k q_k (log q_k - log pT_k)
//   loss = (1 - a) * hard + a * T^2 * kl,   dlogits_k = gscale * ((1 - a) * (p_k - t_k) + a * T * (pT_k - q_k)).
// The teacher's terms ride in the same three passes (its maximum with the row's; its sums with the row's).  With
//   A = sum_k e^((z_k - mz) / T) * ((z_k - mz) - (x_k - m)),  Zq = sum_k e^((z_k - mz) / T),
//   Zp = sum_k e^((x_k - m) / T)
// kl = (A / Zq) / T - log Zq + log Zp: the row maxima cancel in the sum instead of in the result.  Every hard-loss
// expression is the one above and the two terms are combined as (1 - a) * u + a * v, so a == 0 with a finite teacher
// row gives the bits of the plain (MIX: the mixed) kernel.  A non-finite teacher logit is not special-cased: the
// row's loss and gradient are non-finite and the step's NaN guard skips the update.
template <typename T, bool MIX, bool DISTILL = false>
__device__ __forceinline__ void softmax_xent_body(const T* __restrict__ logits, const int* __restrict__ labels,
                                                  float* __restrict__ loss, T* __restrict__ dlogits, int K,
                                                  float smoothing, float gscale, const float* row_weight, int ldx,
                                                  const int* __restrict__ plan, const T* __restrict__ teacher = nullptr,
                                                  int ldt = 0, float* __restrict__ kl_out = nullptr, float alpha = 0.f,
                                                  float temperature = 1.f) {
  __shared__ float red[DISTILL ? 20 : 8];
  const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const T* x = logits + (long)row * ldx;  // (ldx: row pitch - an FC's padded output read in place)
  const T* z = DISTILL ? teacher + (long)row * ldt : nullptr;
  const float rT = 1.f / temperature;
  float m = -INFINITY, mz = -INFINITY;
  for (int k = tid; k < K; k += 256) {
    m = fmaxf(m, ldf(x, k));
    if constexpr (DISTILL) mz = fmaxf(mz, ldf(z, k));
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  if (lane == 0) red[wv] = m;
  if constexpr (DISTILL) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mz = fmaxf(mz, __shfl_xor(mz, o, 64));
    if (lane == 0) red[4 + wv] = mz;
  }
  __syncthreads();
  m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  if constexpr (DISTILL) mz = fmaxf(fmaxf(red[4], red[5]), fmaxf(red[6], red[7]));
  __syncthreads();
  float s = 0.f, sx = 0.f;
  float zp = 0.f, zq = 0.f, za = 0.f;  // DISTILL: Zp, Zq, A
  for (int k = tid; k < K; k += 256) {
    float v = ldf(x, k);
    s += __expf(v - m);
    sx += v;
    if constexpr (DISTILL) {
      const float dz = ldf(z, k) - mz, dx = v - m;
      const float eq = __expf(dz * rT);
      zp += __expf(dx * rT);
      zq += eq;
      za += eq * (dz - dx);
    }
  }
  s = warp_sum(s);
  sx = warp_sum(sx);
  if (lane == 0) { red[wv] = s; red[4 + wv] = sx; }
  if constexpr (DISTILL) {
    zp = warp_sum(zp);
    zq = warp_sum(zq);
    za = warp_sum(za);
    if (lane == 0) { red[8 + wv] = zp; red[12 + wv] = zq; red[16 + wv] = za; }
  }
  __syncthreads();
  s = red[0] + red[1] + red[2] + red[3];
  sx = red[4] + red[5] + red[6] + red[7];
  const float lse = m + __logf(s);
  float lzp = 0.f, lzq = 0.f, kl = 0.f;
  if constexpr (DISTILL) {  // the four waves in a fixed order, as above
    zp = (red[8] + red[9]) + (red[10] + red[11]);
    zq = (red[12] + red[13]) + (red[14] + red[15]);
    za = (red[16] + red[17]) + (red[18] + red[19]);
    lzp = logf(zp);
    lzq = logf(zq);
    kl = (za / zq) * rT - lzq + lzp;
  }
  const float oma = 1.f - alpha;
  const int lab = labels[row];
  int lab2 = -1;
  float wl = 1.f;
  if constexpr (MIX) {
    lab2 = labels[plan[(long)row * 8]];
    wl = __int_as_float(plan[(long)row * 8 + 2]);
  }
  const float on = 1.f - smoothing + smoothing / K, off = smoothing / K;
  const float w = row_weight ? row_weight[row] : 1.f;
  if (tid == 0) {
    float xl = (lab >= 0 && lab < K) ? ldf(x, lab) : 0.f;
    if constexpr (MIX) {
      const float xl2 = (lab2 >= 0 && lab2 < K) ? ldf(x, lab2) : 0.f;
      if (wl != 1.f) xl = wl * xl + (1.f - wl) * xl2;
    }
    // -sum_k t_k log p_k = lse - sum_k t_k x_k
    const float hard = w * (lse - (off * sx + (on - off) * xl));
    if constexpr (DISTILL) {
      loss[row] = oma * hard + (alpha * temperature * temperature) * kl;
      if (kl_out) kl_out[row] = kl;
    } else {
      loss[row] = hard;
    }
  }
  if (dlogits) {
    T* d = dlogits + (long)row * K;
    for (int k = tid; k < K; k += 256) {
      const float v = ldf(x, k);
      float p = __expf(v - lse);
      float t = (k == lab) ? on : off;
      if constexpr (MIX) {
        const float m = (k == lab ? wl : 0.f) + (k == lab2 ? 1.f - wl : 0.f);  // the target's share of "on"
        t = m == 1.f ? on : m == 0.f ? off : off + (on - off) * m;
      }
      float g = p - t;
      if constexpr (DISTILL) {
        const float pT = __expf((v - m) * rT - lzp), q = __expf((ldf(z, k) - mz) * rT - lzq);
        g = oma * g + (alpha * temperature) * (pT - q);
      }
      float gv = g * gscale * w;
      if constexpr (sizeof(T) == 4) d[k] = gv;
      else d[k] = f2bf(gv);
    }
  }
}

template <typename T>
__global__ __launch_bounds__(256) void softmax_xent_kernel(const T* __restrict__ logits, const int* __restrict__ labels,
                                                           float* __restrict__ loss, T* __restrict__ dlogits, int K,
                                                           float smoothing, float gscale, const float* row_weight,
                                                           int ldx) {
  softmax_xent_body<T, false>(logits, labels, loss, dlogits, K, smoothing, gscale, row_weight, ldx, nullptr);
}

template <typename T>
__global__ __launch_bounds__(256) void softmax_xent_mix_kernel(const T* __restrict__ logits,
                                                               const int* __restrict__ labels,
                                                               const int* __restrict__ plan, float* __restrict__ loss,
                                                               T* __restrict__ dlogits, int K, float smoothing,
                                                               float gscale, int ldx) {
  softmax_xent_body<T, true>(logits, labels, loss, dlogits, K, smoothing, gscale, nullptr, ldx, plan);
}

template <typename T, bool MIX>
__global__ __launch_bounds__(256) void softmax_xent_distill_kernel(
    const T* __restrict__ logits, const T* __restrict__ teacher, int ldt, const int* __restrict__ labels,
    const int* __restrict__ plan, float* __restrict__ loss, float* __restrict__ kl, T* __restrict__ dlogits, int K,
    float smoothing, float alpha, float temperature, float gscale, int ldx) {
  softmax_xent_body<T, MIX, true>(logits, labels, loss, dlogits, K, smoothing, gscale, nullptr, ldx, plan, teacher, ldt,
                                  kl, alpha, temperature);
}

// Backward of the per-row loss: out[r][c] = dl[r][c] * gl[r * gstride] for c < N, 0 for N <= c < ldo (the zero
// columns of the padded logits operand of the FC backward, written here instead of a zero fill + copy).  One pass in
// place of the float cast, broadcast multiply and bf16 cast autograd would launch; gstride 0: one scale for every row.
template <typename T>
__global__ __launch_bounds__(256) void scale_rows_pad_kernel(const T* __restrict__ dl, const float* __restrict__ gl,
                                                             int gstride, T* __restrict__ out, int B, int N,
                                                             int ldo) {
  // rows grid-stride over blockIdx.y (grid.y <= 65535 whatever the batch)
  for (int r = blockIdx.y; r < B; r += gridDim.y) {
    const float g = gl[(long)r * gstride];
    const T* src = dl + (long)r * N;
    T* dst = out + (long)r * ldo;
    for (int c = blockIdx.x * 256 + threadIdx.x; c < ldo; c += gridDim.x * 256) {
      const float v = c < N ? ldf(src, c) * g : 0.f;
      if constexpr (sizeof(T) == 2) dst[c] = f2bf(v);
      else dst[c] = v;
    }
  }
}

// The scalar training loss from up to 4 per-row loss vectors: out = sum_h w_h * sum_r loss[h][r] (w_h = the head's
// weight / batch: the mean, the aux-head weight and the batch weight in one launch, one block, fixed order).
struct LossW {
  float w[4];
};
__global__ __launch_bounds__(256) void loss_combine_kernel(const float* __restrict__ loss, int heads, int B, LossW lw,
                                                           float* __restrict__ out) {
  __shared__ float red[4];
  float acc = 0.f;
  for (int h = 0; h < heads; ++h) {
    float s = 0.f;
    for (int r = threadIdx.x; r < B; r += 256) s += loss[(long)h * B + r];
    acc += s * lw.w[h];
  }
  acc = warp_sum(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) out[0] = (red[0] + red[1]) + (red[2] + red[3]);
}

}  // namespace dtm
using namespace dtm;

DTM_API int dtm_scale_rows_pad(const void* dl, int bf16, const float* gl, int gstride, void* out, int B, int N, int ldo,
                               void* stream) {
  if (B <= 0 || N <= 0 || ldo < N) return -1;
  const int bx = (ldo + 255) / 256 > 8 ? 8 : (ldo + 255) / 256;
  const int by = B > 65535 ? 65535 : B;
  if (bf16)
    hipLaunchKernelGGL(scale_rows_pad_kernel<bf16_t>, dim3(bx, by), dim3(256), 0, (hipStream_t)stream,
                       (const bf16_t*)dl, gl, gstride, (bf16_t*)out, B, N, ldo);
  else
    hipLaunchKernelGGL(scale_rows_pad_kernel<float>, dim3(bx, by), dim3(256), 0, (hipStream_t)stream,
                       (const float*)dl, gl, gstride, (float*)out, B, N, ldo);
  return 0;
}

DTM_API void dtm_softmax_xent(const void* logits, int logits_bf16, const int* labels, float* loss, void* dlogits,
                              int B, int K, float smoothing, float gscale, const float* row_weight, int ldx,
                              void* stream) {
  if (ldx < K) ldx = K;
  if (logits_bf16)
    hipLaunchKernelGGL(softmax_xent_kernel<bf16_t>, dim3(B), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)logits,
                       labels, loss, (bf16_t*)dlogits, K, smoothing, gscale, row_weight, ldx);
  else
    hipLaunchKernelGGL(softmax_xent_kernel<float>, dim3(B), dim3(256), 0, (hipStream_t)stream, (const float*)logits,
                       labels, loss, (float*)dlogits, K, smoothing, gscale, row_weight, ldx);
}

// The two-label loss of a mixed batch (softmax_xent_body<T, true>): plan is the batch's device record of mix.hip, B
// rows of 8 int32, trusted (0 <= partner < B).  Returns -1 for a bad argument.
DTM_API int dtm_softmax_xent_mix(const void* logits, int logits_bf16, const int* labels, const int* plan, float* loss,
                                 void* dlogits, int B, int K, float smoothing, float gscale, int ldx, void* stream) {
  if (!logits || !labels || !plan || !loss || B < 1 || K < 1) return -1;
  if (ldx < K) ldx = K;
  if (logits_bf16)
    hipLaunchKernelGGL(softmax_xent_mix_kernel<bf16_t>, dim3(B), dim3(256), 0, (hipStream_t)stream,
                       (const bf16_t*)logits, labels, plan, loss, (bf16_t*)dlogits, K, smoothing, gscale, ldx);
  else
    hipLaunchKernelGGL(softmax_xent_mix_kernel<float>, dim3(B), dim3(256), 0, (hipStream_t)stream,
                       (const float*)logits, labels, plan, loss, (float*)dlogits, K, smoothing, gscale, ldx);
  return 0;
}

// The distillation loss of the main head (softmax_xent_body<T, MIX, true>): teacher is a [B][K] block of the
// student's dtype at pitch ldt, read in place like the student's at ldx; plan null: one label per row, else the
// two-label target of dtm_softmax_xent_mix.  kl (optional) receives the row's unweighted KL(q || pT).  Returns -1 for
// a bad pointer or size, -2 for temperature <= 0 or alpha outside [0, 1] (NaN included); nothing is launched then.
template <typename T>
static void launch_xent_distill(const void* logits, const void* teacher, int ldt, const int* labels, const int* plan,
                                float* loss, float* kl, void* dlogits, int B, int K, float smoothing, float alpha,
                                float temperature, float gscale, int ldx, hipStream_t stream) {
  if (plan)
    hipLaunchKernelGGL((softmax_xent_distill_kernel<T, true>), dim3(B), dim3(256), 0, stream, (const T*)logits,
                       (const T*)teacher, ldt, labels, plan, loss, kl, (T*)dlogits, K, smoothing, alpha, temperature,
                       gscale, ldx);
  else
    hipLaunchKernelGGL((softmax_xent_distill_kernel<T, false>), dim3(B), dim3(256), 0, stream, (const T*)logits,
                       (const T*)teacher, ldt, labels, plan, loss, kl, (T*)dlogits, K, smoothing, alpha, temperature,
                       gscale, ldx);
}

DTM_API int dtm_softmax_xent_distill(const void* logits, int logits_bf16, const void* teacher, int ldt,
                                     const int* labels, const int* plan, float* loss, float* kl, void* dlogits, int B,
                                     int K, float smoothing, float alpha, float temperature, float gscale, int ldx,
                                     void* stream) {
  if (!logits || !teacher || !labels || !loss || B < 1 || B > 65535 || K < 1) return -1;
  if (!(temperature > 0.f) || !(alpha >= 0.f && alpha <= 1.f)) return -2;
  if (ldx < K) ldx = K;
  if (ldt < K) ldt = K;
  if (logits_bf16)
    launch_xent_distill<bf16_t>(logits, teacher, ldt, labels, plan, loss, kl, dlogits, B, K, smoothing, alpha,
                                temperature, gscale, ldx, (hipStream_t)stream);
  else
    launch_xent_distill<float>(logits, teacher, ldt, labels, plan, loss, kl, dlogits, B, K, smoothing, alpha,
                               temperature, gscale, ldx, (hipStream_t)stream);
  return 0;
}

DTM_API int dtm_loss_combine(const float* loss, int heads, int B, const float* w, float* out, void* stream) {
  if (heads < 1 || heads > 4 || B < 1) return -1;
  LossW lw{};
  for (int h = 0; h < heads; ++h) lw.w[h] = w[h];
  hipLaunchKernelGGL(loss_combine_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, loss, heads, B, lw, out);
  return 0;
}
