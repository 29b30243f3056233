// Fused softmax cross-entropy (+label smoothing) and multi-tensor optimizer kernels.
//
// Loss: replaces SoftmaxCrossEntropyWithLogits / sparse variant and slim cross_entropy_loss
// with label smoothing y*(1-eps) + eps/K (reference
// inception/slim/losses.py:142-174, cnn/cifar10.py:298-306).
//
// Optimizer: one launch updates every parameter tensor (chunk table built once on the host),
// with TF 1.x update rules:
//   SGD            p -= lr*g
//   Momentum       a = mu*a + g;  p -= lr*a            (use_nesterov=False)
//   RMSProp (TF)   ms = rho*ms + (1-rho)*g^2;  mom = mu*mom + lr*g/sqrt(ms+eps);  p -= mom
//   LARS           the Momentum update with the rate lr*lr_scale[t] (trust ratio from the norm pass below)
//   Adam           its own entry point and kernel (dtm_multi_tensor_adam, below the norm pass)
// with g = grad*grad_scale + wd*p (coupled L2, the gradient of wd*sum(p^2)/2), optionally times the
// clip-by-global-norm factor of the norm pass, an optional
// fused ExponentialMovingAverage shadow update (decay already min'd with (1+n)/(10+n) on the
// host) and a bf16 copy-out of the updated weight for the next forward.
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

struct OptTensor {
  float* p;
  const float* g;
  float* s1;      // momentum accumulator / RMSProp mom
  float* s2;      // RMSProp ms
  bf16_t* pcopy;  // optional bf16 copy of the updated weight
  float* ema;     // optional EMA shadow
  long n;
  float wd;
  float lr_mult;
};
struct OptChunk {
  int t;
  int pad;
  long start;
};
struct OptHyper {
  int kind;  // 0 sgd, 1 momentum, 2 rmsprop
  float lr, mu, rho, eps, grad_scale, ema_decay;
  int use_ema;
  const int* skip_flag;  // optional: non-zero -> skip the update (non-finite gradients)
  const float* dyn;      // optional device scalars [lr, ema_decay, grad_scale] (graph-replay safe)
  const float* lr_scale;  // optional per-tensor rate factor (LARS trust ratio) written by the norm pass
  const float* gclip;     // optional scalar gradient factor (clip by global norm) written by the norm pass
};
constexpr int OPT_CHUNK = 8192;

__global__ __launch_bounds__(256) void multi_tensor_opt_kernel(const OptTensor* __restrict__ tens,
                                                               const OptChunk* __restrict__ chunks, OptHyper h) {
  if (h.skip_flag && *h.skip_flag) return;
  const OptChunk c = chunks[blockIdx.x];
  const OptTensor t = tens[c.t];
  const long end = min(t.n, c.start + (long)OPT_CHUNK);
  float lr = (h.dyn ? h.dyn[0] : h.lr) * t.lr_mult;
  if (h.lr_scale) lr *= h.lr_scale[c.t];
  const float gclip = h.gclip ? h.gclip[0] : 1.f;
  const float ema_decay = h.dyn ? h.dyn[1] : h.ema_decay;
  const float grad_scale = h.dyn ? h.dyn[2] : h.grad_scale;
  if (!t.g) {  // EMA-only row (BN moving statistics): shadow -= (1-d)(shadow - value)
    if (h.use_ema && t.ema)
      for (long i = c.start + threadIdx.x; i < end; i += 256) t.ema[i] -= (1.f - ema_decay) * (t.ema[i] - t.p[i]);
    return;
  }
  for (long i = c.start + threadIdx.x; i < end; i += 256) {
    float p = t.p[i];
    float g = t.g[i] * grad_scale + t.wd * p;
    if (h.gclip) g *= gclip;
    if (h.kind == 0) {
      p -= lr * g;
    } else if (h.kind == 1) {
      float a = h.mu * t.s1[i] + g;
      t.s1[i] = a;
      p -= lr * a;
    } else {
      float ms = h.rho * t.s2[i] + (1.f - h.rho) * g * g;
      t.s2[i] = ms;
      float mom = h.mu * t.s1[i] + lr * g * rsqrtf(ms + h.eps);
      t.s1[i] = mom;
      p -= mom;
    }
    t.p[i] = p;
    if (t.pcopy) t.pcopy[i] = f2bf(p);
    if (h.use_ema && t.ema) t.ema[i] -= (1.f - ema_decay) * (t.ema[i] - p);
  }
}

// ---- multi-tensor norm pass (LARS trust ratios, clipping by global norm) -------------------------------------
// The L2 norms of every weight and every reduced gradient in two launches over the optimizer's own tables, with no
// float atomics, flags or inter-block waiting: the kernel boundary is the only synchronisation, and every sum has a
// fixed order, so the results are bit-identical run to run and rank to rank (replicas that derived different trust
// ratios from the same all-reduced gradient would drift apart).
//   launch 1: one block per OptChunk row -> one record {sum p^2, sum gs^2, sum ge^2} (fp64), with
//             gs = g*grad_scale and ge = g*grad_scale + wd*p, the update kernel's own fp32 expressions;
//   launch 2: one block; per tensor the records are summed (lane l takes records l, l+64, ... in chunk order, then a
//             xor butterfly over the wave), then the per-tensor sum ge^2 the same way in tensor order:
//     norms[t]    = {|p|, |gs|, |ge|}
//     lr_scale[t] = eeta*|p| / (|gs| + wd_t*|p| + eps)  if tensor t is adapted, |p| > 0 and |gs| > 0, else 1   (LARS)
//     gclip       = clip / max(sqrt(sum_t sum ge^2), clip)  if clip > 0, else 1            (tf.clip_by_global_norm)
struct NormRec {
  double p2, gs2, ge2;
};
struct NormMeta {  // per tensor, beside the 64-byte OptTensor: its rows of the chunk table and the LARS flag
  int chunk0, nchunks, adapt, pad;
};
struct NormHyper {
  float grad_scale, eeta, eps, clip;
  const float* dyn;  // optional device scalars [lr, ema_decay, grad_scale], as OptHyper::dyn
};

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ void norm_add(NormRec& a, float p, float g, float grad_scale, float wd) {
  const float gs = g * grad_scale;
  const float ge = g * grad_scale + wd * p;
  a.p2 += (double)p * (double)p;
  a.gs2 += (double)gs * (double)gs;
  a.ge2 += (double)ge * (double)ge;
}

__global__ __launch_bounds__(256) void multi_tensor_norm_kernel(const OptTensor* __restrict__ tens,
                                                                const OptChunk* __restrict__ chunks, NormHyper h,
                                                                NormRec* __restrict__ recs) {
  __shared__ double red[4][3];
  const int tid = threadIdx.x;
  const OptChunk c = chunks[blockIdx.x];
  const OptTensor t = tens[c.t];
  NormRec a = {0.0, 0.0, 0.0};
  if (t.g) {  // (an EMA-only row writes a zero record)
    const float grad_scale = h.dyn ? h.dyn[2] : h.grad_scale;
    const long rem = t.n - c.start;
    const int len = (int)(rem < (long)OPT_CHUNK ? (rem > 0 ? rem : 0) : (long)OPT_CHUNK);
    const float* pp = t.p + c.start;
    const float* gp = t.g + c.start;
    if ((((uintptr_t)pp ^ (uintptr_t)gp) & 15u) == 0) {
      // weight and gradient reach a 16-byte boundary together: a scalar head up to it, 16-byte loads over the
      // body, a scalar tail (gradients are views into the flat all-reduce buffer at any element offset)
      int head = (int)(((16u - (unsigned)((uintptr_t)gp & 15u)) & 15u) >> 2);
      head = head < len ? head : len;
      const int nvec = (len - head) >> 2, tail0 = head + (nvec << 2);
      if (tid < head) norm_add(a, pp[tid], gp[tid], grad_scale, t.wd);
      const f32x4* pv = (const f32x4*)(pp + head);
      const f32x4* gv = (const f32x4*)(gp + head);
      for (int i = tid; i < nvec; i += 256) {
        const f32x4 pw = pv[i], gw = gv[i];
#pragma unroll
        for (int e = 0; e < 4; ++e) norm_add(a, pw[e], gw[e], grad_scale, t.wd);
      }
      if (tail0 + tid < len) norm_add(a, pp[tail0 + tid], gp[tail0 + tid], grad_scale, t.wd);
    } else {  // the two are offset against each other within 16 bytes: coalesced 4-byte loads
      for (int i = tid; i < len; i += 256) norm_add(a, pp[i], gp[i], grad_scale, t.wd);
    }
  }
  // fixed order: xor butterfly over each wave, then the four waves in LDS
  a.p2 = wave_sum_f64(a.p2);
  a.gs2 = wave_sum_f64(a.gs2);
  a.ge2 = wave_sum_f64(a.ge2);
  if ((tid & 63) == 0) {
    red[tid >> 6][0] = a.p2; red[tid >> 6][1] = a.gs2; red[tid >> 6][2] = a.ge2;
  }
  __syncthreads();
  if (tid == 0) {
    NormRec r;
    r.p2 = (red[0][0] + red[1][0]) + (red[2][0] + red[3][0]);
    r.gs2 = (red[0][1] + red[1][1]) + (red[2][1] + red[3][1]);
    r.ge2 = (red[0][2] + red[1][2]) + (red[2][2] + red[3][2]);
    recs[blockIdx.x] = r;
  }
}

constexpr int NORM_FIN_THREADS = 1024;
__global__ __launch_bounds__(NORM_FIN_THREADS) void multi_tensor_norm_finalize_kernel(
    const OptTensor* __restrict__ tens, const NormMeta* __restrict__ meta, int ntens,
    const NormRec* __restrict__ recs, NormHyper h, double* __restrict__ tsum, float* __restrict__ norms,
    float* __restrict__ lr_scale, float* __restrict__ gclip) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (int t = wv; t < ntens; t += NORM_FIN_THREADS / 64) {  // one wave per tensor
    const NormMeta m = meta[t];
    double p2 = 0.0, gs2 = 0.0, ge2 = 0.0;
    for (int j = lane; j < m.nchunks; j += 64) {
      const NormRec r = recs[m.chunk0 + j];
      p2 += r.p2; gs2 += r.gs2; ge2 += r.ge2;
    }
    p2 = wave_sum_f64(p2);
    gs2 = wave_sum_f64(gs2);
    ge2 = wave_sum_f64(ge2);
    if (lane == 0) {
      const double pn = sqrt(p2), gn = sqrt(gs2);
      norms[3 * t] = (float)pn;
      norms[3 * t + 1] = (float)gn;
      norms[3 * t + 2] = (float)sqrt(ge2);
      double s = 1.0;
      if (m.adapt && pn > 0.0 && gn > 0.0) s = (double)h.eeta * pn / (gn + (double)tens[t].wd * pn + (double)h.eps);
      lr_scale[t] = (float)s;
      tsum[t] = ge2;
    }
  }
  __syncthreads();
  if (wv == 0) {
    double s = 0.0;
    for (int t = lane; t < ntens; t += 64) s += tsum[t];
    s = wave_sum_f64(s);
    if (lane == 0) gclip[0] = h.clip > 0.f ? (float)((double)h.clip / fmax(sqrt(s), (double)h.clip)) : 1.f;
  }
}

// ---- Adam (TF 1.x AdamOptimizer: no Nesterov, no AMSGrad) ---------------------------------------------------------
//   m = b1*m + (1-b1)*g;  v = b2*v + (1-b2)*g*g;  p -= lr*lr_mult * sqrt(1-b2^t)/(1-b1^t) * m / (sqrt(v) + eps)
// over the same OptTensor rows (s1 = m, s2 = v) and OptChunk list, g as above.  t is the number of APPLIED updates:
// the NaN guard skips an update on the device without the host knowing, and the step may be a replayed hipGraph, so
// t and the two correction terms live in a 16-byte device record that a one-thread launch in front of the update
// advances (stream order is the only synchronisation; nothing but the record's contents changes between replays).
struct AdamState {
  int t;      // applied updates so far
  float bc1;  // 1 - b1^t        } from t in fp64, rounded once
  float bc2;  // sqrt(1 - b2^t)  }
  int pad;
};
struct AdamHyper {
  float b1, omb1, b2, omb2, eps;  // omb = 1 - b, rounded from the fp64 difference (1 - 0.999f is 1.3e-5 off 0.001)
  int use_ema;
  const int* skip_flag;
  const float* dyn;    // device scalars [lr, ema_decay, grad_scale]
  const float* gclip;  // optional clip-by-global-norm factor of the norm pass
  const AdamState* state;
};

__global__ void adam_advance_kernel(AdamState* st, const int* skip_flag, double b1, double b2) {
  if (skip_flag && *skip_flag) return;
  const int t = st->t + 1;
  double p1 = 1.0, p2 = 1.0, q1 = b1, q2 = b2;  // b^t by squaring: no product carried from step to step
  for (int e = t; e > 0; e >>= 1) {
    if (e & 1) { p1 *= q1; p2 *= q2; }
    q1 *= q1; q2 *= q2;
  }
  st->t = t;
  st->bc1 = (float)(1.0 - p1);
  st->bc2 = (float)sqrt(1.0 - p2);
}

// One element.  Every operation is spelled out (no contraction left to the compiler), so the 16-byte and the 4-byte
// path of the kernel below give the same bits for the same element.
__device__ __forceinline__ void adam_elem(float& p, float graw, float& m, float& v, float wd, float grad_scale,
                                          bool clip, float gclip, float alpha, const AdamHyper& h) {
  float g = __fmaf_rn(graw, grad_scale, __fmul_rn(wd, p));
  if (clip) g = __fmul_rn(g, gclip);
  m = __fmaf_rn(h.b1, m, __fmul_rn(h.omb1, g));
  v = __fmaf_rn(h.b2, v, __fmul_rn(__fmul_rn(h.omb2, g), g));
  p = __fmaf_rn(-alpha, __fdiv_rn(m, __fadd_rn(__fsqrt_rn(v), h.eps)), p);
}
__device__ __forceinline__ float ema_elem(float e, float p, float omd) {  // e -= (1-d)(e - p)
  return __fmaf_rn(-omd, __fsub_rn(e, p), e);
}

// 30 B per element (+2 B bf16 copy, +8 B EMA): 16-byte accesses where weight, gradient, m, v (and the shadow; the
// bf16 copy at 8 bytes) reach a 16-byte boundary together, with a scalar head and tail, as the norm pass does;
// coalesced 4-byte accesses otherwise (gradients are views into the flat bucket buffer at any element offset).
__global__ __launch_bounds__(256) void multi_tensor_adam_kernel(const OptTensor* __restrict__ tens,
                                                                const OptChunk* __restrict__ chunks, AdamHyper h) {
  if (h.skip_flag && *h.skip_flag) return;
  const int tid = threadIdx.x;
  const OptChunk c = chunks[blockIdx.x];
  const OptTensor t = tens[c.t];
  const long rem = t.n - c.start;
  const int len = (int)(rem < (long)OPT_CHUNK ? (rem > 0 ? rem : 0) : (long)OPT_CHUNK);
  const float ema_decay = h.dyn[1], grad_scale = h.dyn[2];
  if (!t.g) {  // EMA-only row (BN moving statistics), as in multi_tensor_opt_kernel
    if (h.use_ema && t.ema) {
      const float* bp = t.p + c.start;
      float* sp = t.ema + c.start;
      for (int i = tid; i < len; i += 256) sp[i] -= (1.f - ema_decay) * (sp[i] - bp[i]);
    }
    return;
  }
  const AdamState s = *h.state;
  const float alpha = __fdiv_rn(__fmul_rn(__fmul_rn(h.dyn[0], t.lr_mult), s.bc2), s.bc1);
  const float omd = 1.f - ema_decay;
  const bool clip = h.gclip != nullptr;
  const float gclip = clip ? h.gclip[0] : 1.f;
  float* pp = t.p + c.start;
  const float* gp = t.g + c.start;
  float* mp = t.s1 + c.start;
  float* vp = t.s2 + c.start;
  float* ep = (h.use_ema && t.ema) ? t.ema + c.start : nullptr;
  bf16_t* cp = t.pcopy ? t.pcopy + c.start : nullptr;

  auto scalar = [&](int i) {
    float p = pp[i], m = mp[i], v = vp[i];
    adam_elem(p, gp[i], m, v, t.wd, grad_scale, clip, gclip, alpha, h);
    pp[i] = p; mp[i] = m; vp[i] = v;
    if (cp) cp[i] = f2bf(p);
    if (ep) ep[i] = ema_elem(ep[i], p, omd);
  };

  const uintptr_t pa = (uintptr_t)pp;
  uintptr_t off = (pa ^ (uintptr_t)gp) | (pa ^ (uintptr_t)mp) | (pa ^ (uintptr_t)vp);
  if (ep) off |= pa ^ (uintptr_t)ep;
  const int head16 = (int)(((16u - (unsigned)(pa & 15u)) & 15u) >> 2);  // elements up to the 16-byte boundary
  if ((off & 15u) == 0 && (!cp || ((uintptr_t)(cp + head16) & 7u) == 0)) {
    const int head = head16 < len ? head16 : len;
    const int nvec = (len - head) >> 2, tail0 = head + (nvec << 2);
    if (tid < head) scalar(tid);
    f32x4* pv = (f32x4*)(pp + head);
    const f32x4* gv = (const f32x4*)(gp + head);
    f32x4* mv = (f32x4*)(mp + head);
    f32x4* vv = (f32x4*)(vp + head);
    for (int i = tid; i < nvec; i += 256) {
      f32x4 pw = pv[i], mw = mv[i], vw = vv[i];
      const f32x4 gw = gv[i];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float p = pw[e], m = mw[e], v = vw[e];
        adam_elem(p, gw[e], m, v, t.wd, grad_scale, clip, gclip, alpha, h);
        pw[e] = p; mw[e] = m; vw[e] = v;
      }
      pv[i] = pw; mv[i] = mw; vv[i] = vw;
      if (cp) ((uint2*)(cp + head))[i] = make_uint2(pack2bf(pw[0], pw[1]), pack2bf(pw[2], pw[3]));
      if (ep) {
        f32x4* ev = (f32x4*)(ep + head);
        f32x4 ew = ev[i];
#pragma unroll
        for (int e = 0; e < 4; ++e) ew[e] = ema_elem(ew[e], pw[e], omd);
        ev[i] = ew;
      }
    }
    if (tail0 + tid < len) scalar(tail0 + tid);
  } else {
    for (int i = tid; i < len; i += 256) scalar(i);
  }
}

// ---- LAMB (You et al. 2020: Adam's direction, decoupled weight decay, LARS's per-tensor trust ratio) --------------
//   m = b1*m + (1-b1)*gs;  v = b2*v + (1-b2)*gs*gs;  r = (m/bc1) / (sqrt(v)/bc2 + eps) + wd_t*p     (gs = g*grad_scale)
//   phi[t] = |p| / |r|  if tensor t is adapted, |p| > 0 and |r| > 0, else 1;   p -= (lr*lr_mult[t]*phi[t]) * r
// |r| needs the moments AFTER they took this step's gradient, so the pass has launches of its own over the Adam
// tables (s1 = m, s2 = v, the AdamState record) and the norm pass's side table and scratch:
//   launch 1: adam_advance_kernel;
//   launch 2: one block per OptChunk row: m, v updated and stored, one record {sum p^2, sum gs^2, sum r^2} (fp64, the
//             norm pass's fixed order) per row;
//   launch 3: one block, one wave per tensor: norms[t] = {|p|, |r|, |gs|}, lr_scale[t] = phi[t];
//   launch 4: one block per OptChunk row: r again from the stored p, m, v (p has not changed in between, so these
//             are the bits launch 2 reduced), then p, its bf16 copy and the EMA shadow.
// No float atomics, flags or inter-block waiting; every launch leaves at once on the skip flag.
struct LambHyper {
  float b1, omb1, b2, omb2, eps;
  int use_ema;
  const int* skip_flag;
  const float* dyn;  // device scalars [lr, ema_decay, grad_scale]
  const AdamState* state;
  const float* lr_scale;  // phi per tensor (launch 4)
};

// One element, every operation spelled out (as adam_elem): launches 2 and 4 and both access paths of each form r
// here, from the same p, m, v.
__device__ __forceinline__ float lamb_gs(float graw, float grad_scale) { return __fmul_rn(graw, grad_scale); }
__device__ __forceinline__ void lamb_moments(float g, float& m, float& v, const LambHyper& h) {
  m = __fmaf_rn(h.b1, m, __fmul_rn(h.omb1, g));
  v = __fmaf_rn(h.b2, v, __fmul_rn(__fmul_rn(h.omb2, g), g));
}
// (sqrtf, not __fsqrt_rn: the intrinsic is the native root, good to 1 ulp, while sqrtf is correctly rounded like the
// quotients - so a host evaluation with IEEE fp32 operations reproduces r)
__device__ __forceinline__ float lamb_dir(float p, float m, float v, float wd, float bc1, float bc2, float eps) {
  return __fmaf_rn(wd, p, __fdiv_rn(__fdiv_rn(m, bc1), __fadd_rn(__fdiv_rn(sqrtf(v), bc2), eps)));
}
// (NormRec::ge2 carries sum r^2 here: r takes the place of the effective gradient)
__device__ __forceinline__ void lamb_acc(NormRec& a, float p, float gs, float r) {
  a.p2 += (double)p * (double)p;
  a.gs2 += (double)gs * (double)gs;
  a.ge2 += (double)r * (double)r;
}

// 16 B read + 8 B written per element: 16-byte accesses where weight, gradient, m and v reach a 16-byte boundary
// together, with a scalar head and tail; coalesced 4-byte accesses otherwise.
__global__ __launch_bounds__(256) void multi_tensor_lamb_moments_kernel(const OptTensor* __restrict__ tens,
                                                                        const OptChunk* __restrict__ chunks,
                                                                        LambHyper h, NormRec* __restrict__ recs) {
  if (h.skip_flag && *h.skip_flag) return;  // m, v and the records stay
  __shared__ double red[4][3];
  const int tid = threadIdx.x;
  const OptChunk c = chunks[blockIdx.x];
  const OptTensor t = tens[c.t];
  NormRec a = {0.0, 0.0, 0.0};
  if (t.g) {  // (an EMA-only row writes a zero record)
    const long rem = t.n - c.start;
    const int len = (int)(rem < (long)OPT_CHUNK ? (rem > 0 ? rem : 0) : (long)OPT_CHUNK);
    const float grad_scale = h.dyn[2];
    const AdamState s = *h.state;
    const float* pp = t.p + c.start;
    const float* gp = t.g + c.start;
    float* mp = t.s1 + c.start;
    float* vp = t.s2 + c.start;

    auto scalar = [&](int i) {
      const float p = pp[i], g = lamb_gs(gp[i], grad_scale);
      float m = mp[i], v = vp[i];
      lamb_moments(g, m, v, h);
      mp[i] = m; vp[i] = v;
      lamb_acc(a, p, g, lamb_dir(p, m, v, t.wd, s.bc1, s.bc2, h.eps));
    };

    const uintptr_t pa = (uintptr_t)pp;
    const uintptr_t off = (pa ^ (uintptr_t)gp) | (pa ^ (uintptr_t)mp) | (pa ^ (uintptr_t)vp);
    if ((off & 15u) == 0) {
      int head = (int)(((16u - (unsigned)(pa & 15u)) & 15u) >> 2);  // elements up to the 16-byte boundary
      head = head < len ? head : len;
      const int nvec = (len - head) >> 2, tail0 = head + (nvec << 2);
      if (tid < head) scalar(tid);
      const f32x4* pv = (const f32x4*)(pp + head);
      const f32x4* gv = (const f32x4*)(gp + head);
      f32x4* mv = (f32x4*)(mp + head);
      f32x4* vv = (f32x4*)(vp + head);
      for (int i = tid; i < nvec; i += 256) {
        const f32x4 pw = pv[i], gw = gv[i];
        f32x4 mw = mv[i], vw = vv[i];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float g = lamb_gs(gw[e], grad_scale);
          float m = mw[e], v = vw[e];
          lamb_moments(g, m, v, h);
          mw[e] = m; vw[e] = v;
          lamb_acc(a, pw[e], g, lamb_dir(pw[e], m, v, t.wd, s.bc1, s.bc2, h.eps));
        }
        mv[i] = mw; vv[i] = vw;
      }
      if (tail0 + tid < len) scalar(tail0 + tid);
    } else {
      for (int i = tid; i < len; i += 256) scalar(i);
    }
  }
  // fixed order: xor butterfly over each wave, then the four waves in LDS (as multi_tensor_norm_kernel)
  a.p2 = wave_sum_f64(a.p2);
  a.gs2 = wave_sum_f64(a.gs2);
  a.ge2 = wave_sum_f64(a.ge2);
  if ((tid & 63) == 0) {
    red[tid >> 6][0] = a.p2; red[tid >> 6][1] = a.gs2; red[tid >> 6][2] = a.ge2;
  }
  __syncthreads();
  if (tid == 0) {
    NormRec r;
    r.p2 = (red[0][0] + red[1][0]) + (red[2][0] + red[3][0]);
    r.gs2 = (red[0][1] + red[1][1]) + (red[2][1] + red[3][1]);
    r.ge2 = (red[0][2] + red[1][2]) + (red[2][2] + red[3][2]);
    recs[blockIdx.x] = r;
  }
}

__global__ __launch_bounds__(NORM_FIN_THREADS) void multi_tensor_lamb_finalize_kernel(
    const NormMeta* __restrict__ meta, int ntens, const NormRec* __restrict__ recs, const int* skip_flag,
    float* __restrict__ norms, float* __restrict__ lr_scale) {
  if (skip_flag && *skip_flag) return;  // the previous step's outputs stay
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (int t = wv; t < ntens; t += NORM_FIN_THREADS / 64) {  // one wave per tensor
    const NormMeta m = meta[t];
    double p2 = 0.0, gs2 = 0.0, r2 = 0.0;
    for (int j = lane; j < m.nchunks; j += 64) {
      const NormRec r = recs[m.chunk0 + j];
      p2 += r.p2; gs2 += r.gs2; r2 += r.ge2;
    }
    p2 = wave_sum_f64(p2);
    gs2 = wave_sum_f64(gs2);
    r2 = wave_sum_f64(r2);
    if (lane == 0) {
      const double pn = sqrt(p2), rn = sqrt(r2);
      norms[3 * t] = (float)pn;
      norms[3 * t + 1] = (float)rn;
      norms[3 * t + 2] = (float)sqrt(gs2);
      lr_scale[t] = (m.adapt && pn > 0.0 && rn > 0.0) ? (float)(pn / rn) : 1.f;  // (a NaN norm fails both tests)
    }
  }
}

// 12 B read + 6 B written per element with the bf16 copy (+8 B EMA): 16-byte accesses where weight, m, v (and the
// shadow; the bf16 copy at 8 bytes) reach a 16-byte boundary together, as multi_tensor_adam_kernel chooses.
__global__ __launch_bounds__(256) void multi_tensor_lamb_apply_kernel(const OptTensor* __restrict__ tens,
                                                                      const OptChunk* __restrict__ chunks,
                                                                      LambHyper h) {
  if (h.skip_flag && *h.skip_flag) return;
  const int tid = threadIdx.x;
  const OptChunk c = chunks[blockIdx.x];
  const OptTensor t = tens[c.t];
  const long rem = t.n - c.start;
  const int len = (int)(rem < (long)OPT_CHUNK ? (rem > 0 ? rem : 0) : (long)OPT_CHUNK);
  const float ema_decay = h.dyn[1];
  if (!t.g) {  // EMA-only row (BN moving statistics), as in multi_tensor_opt_kernel
    if (h.use_ema && t.ema) {
      const float* bp = t.p + c.start;
      float* sp = t.ema + c.start;
      for (int i = tid; i < len; i += 256) sp[i] -= (1.f - ema_decay) * (sp[i] - bp[i]);
    }
    return;
  }
  const AdamState s = *h.state;
  const float step = __fmul_rn(__fmul_rn(h.dyn[0], t.lr_mult), h.lr_scale[c.t]);
  const float omd = 1.f - ema_decay;
  float* pp = t.p + c.start;
  const float* mp = t.s1 + c.start;
  const float* vp = t.s2 + c.start;
  float* ep = (h.use_ema && t.ema) ? t.ema + c.start : nullptr;
  bf16_t* cp = t.pcopy ? t.pcopy + c.start : nullptr;

  auto elem = [&](float p, float m, float v) {
    return __fmaf_rn(-step, lamb_dir(p, m, v, t.wd, s.bc1, s.bc2, h.eps), p);
  };
  auto scalar = [&](int i) {
    const float p = elem(pp[i], mp[i], vp[i]);
    pp[i] = p;
    if (cp) cp[i] = f2bf(p);
    if (ep) ep[i] = ema_elem(ep[i], p, omd);
  };

  const uintptr_t pa = (uintptr_t)pp;
  uintptr_t off = (pa ^ (uintptr_t)mp) | (pa ^ (uintptr_t)vp);
  if (ep) off |= pa ^ (uintptr_t)ep;
  const int head16 = (int)(((16u - (unsigned)(pa & 15u)) & 15u) >> 2);  // elements up to the 16-byte boundary
  if ((off & 15u) == 0 && (!cp || ((uintptr_t)(cp + head16) & 7u) == 0)) {
    const int head = head16 < len ? head16 : len;
    const int nvec = (len - head) >> 2, tail0 = head + (nvec << 2);
    if (tid < head) scalar(tid);
    f32x4* pv = (f32x4*)(pp + head);
    const f32x4* mv = (const f32x4*)(mp + head);
    const f32x4* vv = (const f32x4*)(vp + head);
    for (int i = tid; i < nvec; i += 256) {
      f32x4 pw = pv[i];
      const f32x4 mw = mv[i], vw = vv[i];
#pragma unroll
      for (int e = 0; e < 4; ++e) pw[e] = elem(pw[e], mw[e], vw[e]);
      pv[i] = pw;
      if (cp) ((uint2*)(cp + head))[i] = make_uint2(pack2bf(pw[0], pw[1]), pack2bf(pw[2], pw[3]));
      if (ep) {
        f32x4* ev = (f32x4*)(ep + head);
        f32x4 ew = ev[i];
#pragma unroll
        for (int e = 0; e < 4; ++e) ew[e] = ema_elem(ew[e], pw[e], omd);
        ev[i] = ew;
      }
    }
    if (tail0 + tid < len) scalar(tail0 + tid);
  } else {
    for (int i = tid; i < len; i += 256) scalar(i);
  }
}

__global__ void check_finite_kernel(const float* __restrict__ x, long n, int* __restrict__ flag) {
  bool bad = false;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    float v = x[i];
    bad |= !(fabsf(v) <= 3.4e38f);
  }
  if (__any(bad) && (threadIdx.x & 63) == 0) atomicOr(flag, 1);
}

__global__ void f32_to_bf16_kernel(const float* __restrict__ x, bf16_t* __restrict__ y, long n) {
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) y[i] = f2bf(x[i]);
}
__global__ void scale_kernel(float* __restrict__ x, long n, float s) {
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) x[i] *= s;
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

DTM_API int dtm_opt_chunk_size() { return OPT_CHUNK; }
DTM_API int dtm_opt_tensor_bytes() { return (int)sizeof(OptTensor); }
DTM_API int dtm_opt_chunk_bytes() { return (int)sizeof(OptChunk); }

// lr_scale [ntens] / gclip [1]: the outputs of dtm_multi_tensor_norms (either may be null: factor 1)
DTM_API void dtm_multi_tensor_opt_scaled(const void* tensors_dev, const void* chunks_dev, int num_chunks, int kind,
                                         float lr, float mu, float rho, float eps, float grad_scale, float ema_decay,
                                         int use_ema, const int* skip_flag, const float* dyn, const float* lr_scale,
                                         const float* gclip, void* stream) {
  OptHyper h;
  h.dyn = dyn;
  h.kind = kind; h.lr = lr; h.mu = mu; h.rho = rho; h.eps = eps; h.grad_scale = grad_scale;
  h.ema_decay = ema_decay; h.use_ema = use_ema; h.skip_flag = skip_flag;
  h.lr_scale = lr_scale; h.gclip = gclip;
  if (num_chunks <= 0) return;
  hipLaunchKernelGGL(multi_tensor_opt_kernel, dim3(num_chunks), dim3(256), 0, (hipStream_t)stream,
                     (const OptTensor*)tensors_dev, (const OptChunk*)chunks_dev, h);
}

DTM_API void dtm_multi_tensor_opt(const void* tensors_dev, const void* chunks_dev, int num_chunks, int kind, float lr,
                                  float mu, float rho, float eps, float grad_scale, float ema_decay, int use_ema,
                                  const int* skip_flag, const float* dyn, void* stream) {
  dtm_multi_tensor_opt_scaled(tensors_dev, chunks_dev, num_chunks, kind, lr, mu, rho, eps, grad_scale, ema_decay,
                              use_ema, skip_flag, dyn, nullptr, nullptr, stream);
}

DTM_API int dtm_adam_state_bytes() { return (int)sizeof(AdamState); }

// The Adam step over the optimizer's tables (as dtm_multi_tensor_opt; s1 = m, s2 = v): a one-thread launch advances
// the device record ``state`` (AdamState, zeroed by the owner before the first step) unless *skip_flag, then the
// update reads it.  dyn: device scalars [lr, ema_decay, grad_scale]; gclip: the norm pass's clip factor or null.
// Nothing is allocated, uploaded or read back: the two launches can be captured into a hipGraph.
DTM_API int dtm_multi_tensor_adam(const void* tensors_dev, const void* chunks_dev, int num_chunks, double b1,
                                  double b2, double eps, int use_ema, const int* skip_flag, const float* dyn,
                                  const float* gclip, void* state, void* stream) {
  if (num_chunks < 0 || !dyn || !state || !(b1 >= 0.0 && b1 < 1.0) || !(b2 >= 0.0 && b2 < 1.0)) return -1;
  if (num_chunks > 0 && (!tensors_dev || !chunks_dev)) return -1;
  AdamHyper h;
  h.b1 = (float)b1; h.omb1 = (float)(1.0 - b1); h.b2 = (float)b2; h.omb2 = (float)(1.0 - b2); h.eps = (float)eps;
  h.use_ema = use_ema; h.skip_flag = skip_flag; h.dyn = dyn; h.gclip = gclip; h.state = (const AdamState*)state;
  hipLaunchKernelGGL(adam_advance_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, (AdamState*)state, skip_flag, b1,
                     b2);
  if (num_chunks > 0)
    hipLaunchKernelGGL(multi_tensor_adam_kernel, dim3(num_chunks), dim3(256), 0, (hipStream_t)stream,
                       (const OptTensor*)tensors_dev, (const OptChunk*)chunks_dev, h);
  return 0;
}

DTM_API int dtm_opt_norm_meta_bytes() { return (int)sizeof(NormMeta); }
// bytes of the norm pass's scratch: one record per chunk row, then one fp64 sum per tensor
DTM_API long dtm_opt_norm_scratch_bytes(int num_chunks, int ntens) {
  return (long)sizeof(NormRec) * (num_chunks > 0 ? num_chunks : 0) + (long)sizeof(double) * (ntens > 0 ? ntens : 0);
}

// The two-launch norm pass over the optimizer's tables (tensors_dev / chunks_dev as dtm_multi_tensor_opt; meta_dev:
// ntens NormMeta rows; the chunk rows of a tensor are contiguous and in order).  Writes norms [ntens][3], lr_scale
// [ntens], gclip [1]; nothing is allocated or uploaded, so the pass can be captured into a hipGraph.
DTM_API int dtm_multi_tensor_norms(const void* tensors_dev, const void* chunks_dev, int num_chunks,
                                   const void* meta_dev, int ntens, const float* dyn, float grad_scale, float eeta,
                                   float eps, float clip, void* scratch, float* norms, float* lr_scale, float* gclip,
                                   void* stream) {
  if (num_chunks < 0 || ntens <= 0 || !tensors_dev || !meta_dev || !scratch || !norms || !lr_scale || !gclip)
    return -1;
  if (num_chunks > 0 && !chunks_dev) return -1;
  NormHyper h;
  h.grad_scale = grad_scale; h.eeta = eeta; h.eps = eps; h.clip = clip; h.dyn = dyn;
  NormRec* recs = (NormRec*)scratch;
  double* tsum = (double*)(recs + num_chunks);
  if (num_chunks > 0)
    hipLaunchKernelGGL(multi_tensor_norm_kernel, dim3(num_chunks), dim3(256), 0, (hipStream_t)stream,
                       (const OptTensor*)tensors_dev, (const OptChunk*)chunks_dev, h, recs);
  hipLaunchKernelGGL(multi_tensor_norm_finalize_kernel, dim3(1), dim3(NORM_FIN_THREADS), 0, (hipStream_t)stream,
                     (const OptTensor*)tensors_dev, (const NormMeta*)meta_dev, ntens, (const NormRec*)recs, h, tsum,
                     norms, lr_scale, gclip);
  return 0;
}

// The LAMB step over the optimizer's tables (s1 = m, s2 = v; meta_dev / scratch / norms / lr_scale as
// dtm_multi_tensor_norms, state / dyn as dtm_multi_tensor_adam): four launches in stream order - the state advance,
// the moments pass with the per-row records, the per-tensor finalize (norms [ntens][3] = {|p|, |r|, |gs|}, lr_scale
// [ntens] = phi) and the apply pass.  Nothing is allocated, uploaded or read back, so the step can be captured into a
// hipGraph.  Returns -1 for a bad count or a null table, -2 for a beta outside [0, 1) or eps < 0 (NaN included);
// nothing is launched then.
DTM_API int dtm_multi_tensor_lamb(const void* tensors_dev, const void* chunks_dev, int num_chunks,
                                  const void* meta_dev, int ntens, double b1, double b2, double eps, int use_ema,
                                  const int* skip_flag, const float* dyn, void* state, void* scratch, float* norms,
                                  float* lr_scale, void* stream) {
  if (num_chunks < 0 || ntens < 0 || !dyn || !state) return -1;
  if (ntens > 0 && (!tensors_dev || !meta_dev || !scratch || !norms || !lr_scale)) return -1;
  if (num_chunks > 0 && (!chunks_dev || ntens == 0)) return -1;
  if (!(b1 >= 0.0 && b1 < 1.0) || !(b2 >= 0.0 && b2 < 1.0) || !(eps >= 0.0)) return -2;
  LambHyper h;
  h.b1 = (float)b1; h.omb1 = (float)(1.0 - b1); h.b2 = (float)b2; h.omb2 = (float)(1.0 - b2); h.eps = (float)eps;
  h.use_ema = use_ema; h.skip_flag = skip_flag; h.dyn = dyn; h.state = (const AdamState*)state;
  h.lr_scale = lr_scale;
  NormRec* recs = (NormRec*)scratch;
  hipLaunchKernelGGL(adam_advance_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, (AdamState*)state, skip_flag, b1,
                     b2);
  if (num_chunks > 0)
    hipLaunchKernelGGL(multi_tensor_lamb_moments_kernel, dim3(num_chunks), dim3(256), 0, (hipStream_t)stream,
                       (const OptTensor*)tensors_dev, (const OptChunk*)chunks_dev, h, recs);
  if (ntens > 0)
    hipLaunchKernelGGL(multi_tensor_lamb_finalize_kernel, dim3(1), dim3(NORM_FIN_THREADS), 0, (hipStream_t)stream,
                       (const NormMeta*)meta_dev, ntens, (const NormRec*)recs, skip_flag, norms, lr_scale);
  if (num_chunks > 0)
    hipLaunchKernelGGL(multi_tensor_lamb_apply_kernel, dim3(num_chunks), dim3(256), 0, (hipStream_t)stream,
                       (const OptTensor*)tensors_dev, (const OptChunk*)chunks_dev, h);
  return 0;
}

DTM_API void dtm_check_finite(const float* x, long n, int* flag, void* stream) {
  long b = (n + 255) / 256;
  if (b > 2048) b = 2048;
  if (b < 1) b = 1;
  hipLaunchKernelGGL(check_finite_kernel, dim3((int)b), dim3(256), 0, (hipStream_t)stream, x, n, flag);
}
DTM_API void dtm_f32_to_bf16(const float* x, void* y, long n, void* stream) {
  long b = (n + 255) / 256;
  if (b > 4096) b = 4096;
  if (b < 1) b = 1;
  hipLaunchKernelGGL(f32_to_bf16_kernel, dim3((int)b), dim3(256), 0, (hipStream_t)stream, x, (bf16_t*)y, n);
}
DTM_API void dtm_scale(float* x, long n, float s, void* stream) {
  long b = (n + 255) / 256;
  if (b > 4096) b = 4096;
  if (b < 1) b = 1;
  hipLaunchKernelGGL(scale_kernel, dim3((int)b), dim3(256), 0, (hipStream_t)stream, x, n, s);
}
