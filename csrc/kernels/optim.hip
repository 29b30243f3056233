// Multi-tensor optimizer kernels: one launch updates every parameter tensor (chunk table built once on the host),
// with TF 1.x update rules:
//   SGD            p -= lr*g
//   Momentum       a = mu*a + g;  p -= lr*a            (use_nesterov=False)
//   RMSProp (TF)   ms = rho*ms + (1-rho)*g^2;  mom = mu*mom + lr*g/sqrt(ms+eps);  p -= mom
//   LARS           the Momentum update with the rate lr*lr_scale[t] (trust ratio from the norm pass below)
//   Adam, LAMB     their own entry points and kernels (dtm_multi_tensor_adam / _lamb, below the norm pass)
// with g = grad*grad_scale + wd*p (coupled L2, the gradient of wd*sum(p^2)/2), optionally times the
// clip-by-global-norm factor of the norm pass, an optional
// fused ExponentialMovingAverage shadow update (decay already min'd with (1+n)/(10+n) on the
// host) and a bf16 copy-out of the updated weight for the next forward.
// The row walk (scalar head, 16-byte body, scalar tail, or scalar throughout) and the fixed-order fp64 sums of the
// norm, Adam and LAMB kernels are chunk_walk.h's; the per-element math is in the small functions beside each kernel.
#include "chunk_walk.h"

namespace dtm {

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
                                                               const ChunkRow* __restrict__ chunks, OptHyper h) {
  if (h.skip_flag && *h.skip_flag) return;
  const ChunkRow c = chunks[blockIdx.x];
  const OptTensor t = tens[c.t];
  const long end = min(t.n, c.start + (long)OPT_CHUNK);
  float lr = (h.dyn ? h.dyn[0] : h.lr) * t.lr_mult;
  if (h.lr_scale) lr *= h.lr_scale[c.t];
  const float gclip = h.gclip ? h.gclip[0] : 1.f;
  const float ema_decay = h.dyn ? h.dyn[1] : h.ema_decay;
  const float grad_scale = h.dyn ? h.dyn[2] : h.grad_scale;
  if (!t.g) {  // EMA-only row (BN moving statistics)
    if (h.use_ema && t.ema)
      ema_only_row(t.ema + c.start, t.p + c.start, chunk_len(t.n, c.start, OPT_CHUNK), ema_decay, threadIdx.x);
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
//   launch 1: one block per chunk row -> one record {sum p^2, sum gs^2, sum ge^2} (fp64), with
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
  ChunkSpan rows;
  int adapt, pad;
};
struct NormHyper {
  float grad_scale, eeta, eps, clip;
  const float* dyn;  // optional device scalars [lr, ema_decay, grad_scale], as OptHyper::dyn
};

__device__ __forceinline__ void norm_add(NormRec& a, float p, float g, float grad_scale, float wd) {
  const float gs = g * grad_scale;
  const float ge = g * grad_scale + wd * p;
  a.p2 += (double)p * (double)p;
  a.gs2 += (double)gs * (double)gs;
  a.ge2 += (double)ge * (double)ge;
}

// the block's record from its threads' partial sums, in block_sum_f64's fixed order
__device__ __forceinline__ void store_norm_rec(NormRec* __restrict__ recs, const NormRec& a, int tid) {
  double v[3] = {a.p2, a.gs2, a.ge2};
  block_sum_f64(v, tid);
  if (tid == 0) recs[blockIdx.x] = NormRec{v[0], v[1], v[2]};
}

__global__ __launch_bounds__(256) void multi_tensor_norm_kernel(const OptTensor* __restrict__ tens,
                                                                const ChunkRow* __restrict__ chunks, NormHyper h,
                                                                NormRec* __restrict__ recs) {
  const int tid = threadIdx.x;
  const ChunkRow c = chunks[blockIdx.x];
  const OptTensor t = tens[c.t];
  NormRec a = {0.0, 0.0, 0.0};
  if (t.g) {  // (an EMA-only row writes a zero record)
    const float grad_scale = h.dyn ? h.dyn[2] : h.grad_scale;
    const float* pp = t.p + c.start;
    const float* gp = t.g + c.start;
    // (gradients are views into the flat all-reduce buffer at any element offset)
    const WalkPlan w = walk_plan(4, (uintptr_t)gp, chunk_len(t.n, c.start, OPT_CHUNK), same16(gp, pp));
    const f32x4* pv = (const f32x4*)(pp + w.head);
    const f32x4* gv = (const f32x4*)(gp + w.head);
    walk<256, 4>(
        w, tid, [&](int i) { norm_add(a, pp[i], gp[i], grad_scale, t.wd); },
        [&](int i, int) {
          const f32x4 pw = pv[i], gw = gv[i];
#pragma unroll
          for (int e = 0; e < 4; ++e) norm_add(a, pw[e], gw[e], grad_scale, t.wd);
        });
  }
  store_norm_rec(recs, a, tid);
}

constexpr int NORM_FIN_THREADS = 1024;
__global__ __launch_bounds__(NORM_FIN_THREADS) void multi_tensor_norm_finalize_kernel(
    const OptTensor* __restrict__ tens, const NormMeta* __restrict__ meta, int ntens,
    const NormRec* __restrict__ recs, NormHyper h, double* __restrict__ tsum, float* __restrict__ norms,
    float* __restrict__ lr_scale, float* __restrict__ gclip) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (int t = wv; t < ntens; t += NORM_FIN_THREADS / 64) {  // one wave per tensor
    const NormMeta m = meta[t];
    double s[3];  // p2, gs2, ge2
    record_sum(recs, m.rows, lane, s);
    if (lane == 0) {
      const double pn = sqrt(s[0]), gn = sqrt(s[1]);
      norms[3 * t] = (float)pn;
      norms[3 * t + 1] = (float)gn;
      norms[3 * t + 2] = (float)sqrt(s[2]);
      double r = 1.0;
      if (m.adapt && pn > 0.0 && gn > 0.0) r = (double)h.eeta * pn / (gn + (double)tens[t].wd * pn + (double)h.eps);
      lr_scale[t] = (float)r;
      tsum[t] = s[2];
    }
  }
  __syncthreads();
  if (wv == 0) {  // the per-tensor sums the same way, in tensor order
    double s[1];
    record_sum((const double*)tsum, ChunkSpan{0, ntens}, lane, s);
    if (lane == 0) gclip[0] = h.clip > 0.f ? (float)((double)h.clip / fmax(sqrt(s[0]), (double)h.clip)) : 1.f;
  }
}

// ---- Adam (TF 1.x AdamOptimizer: no Nesterov, no AMSGrad) ---------------------------------------------------------
//   m = b1*m + (1-b1)*g;  v = b2*v + (1-b2)*g*g;  p -= lr*lr_mult * sqrt(1-b2^t)/(1-b1^t) * m / (sqrt(v) + eps)
// over the same OptTensor rows (s1 = m, s2 = v) and chunk list, g as above.  t is the number of APPLIED updates:
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

// The updated weight(s) into the optional bf16 copy cp and the optional EMA shadow ep of the row (Adam, LAMB): element
// i, or group i of the body that starts at element head.
__device__ __forceinline__ void copy_and_ema(float p, int i, bf16_t* cp, float* ep, float omd) {
  if (cp) cp[i] = f2bf(p);
  if (ep) ep[i] = ema_elem(ep[i], p, omd);
}
__device__ __forceinline__ void copy_and_ema4(const f32x4& pw, int i, int head, bf16_t* cp, float* ep, float omd) {
  if (cp) store_bf16x4(cp + head, i, pw);
  if (ep) {
    f32x4* ev = (f32x4*)(ep + head);
    f32x4 ew = ev[i];
#pragma unroll
    for (int e = 0; e < 4; ++e) ew[e] = ema_elem(ew[e], pw[e], omd);
    ev[i] = ew;
  }
}

// 30 B per element (+2 B bf16 copy, +8 B EMA): 16-byte accesses where weight, gradient, m, v (and the shadow; the
// bf16 copy at 8 bytes) reach a 16-byte boundary together, with a scalar head and tail, as the norm pass does;
// coalesced 4-byte accesses otherwise (gradients are views into the flat bucket buffer at any element offset).
__global__ __launch_bounds__(256) void multi_tensor_adam_kernel(const OptTensor* __restrict__ tens,
                                                                const ChunkRow* __restrict__ chunks, AdamHyper h) {
  if (h.skip_flag && *h.skip_flag) return;
  const int tid = threadIdx.x;
  const ChunkRow c = chunks[blockIdx.x];
  const OptTensor t = tens[c.t];
  const int len = chunk_len(t.n, c.start, OPT_CHUNK);
  const float ema_decay = h.dyn[1], grad_scale = h.dyn[2];
  if (!t.g) {  // EMA-only row (BN moving statistics), as in multi_tensor_opt_kernel
    if (h.use_ema && t.ema) ema_only_row(t.ema + c.start, t.p + c.start, len, ema_decay, tid);
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

  const bool vec_ok = same16(pp, gp, mp, vp) && (!ep || same16(pp, ep)) && copy8_ok(cp, (uintptr_t)pp);
  const WalkPlan w = walk_plan(4, (uintptr_t)pp, len, vec_ok);
  f32x4* pv = (f32x4*)(pp + w.head);
  const f32x4* gv = (const f32x4*)(gp + w.head);
  f32x4* mv = (f32x4*)(mp + w.head);
  f32x4* vv = (f32x4*)(vp + w.head);
  walk<256, 4>(
      w, tid,
      [&](int i) {
        float p = pp[i], m = mp[i], v = vp[i];
        adam_elem(p, gp[i], m, v, t.wd, grad_scale, clip, gclip, alpha, h);
        pp[i] = p; mp[i] = m; vp[i] = v;
        copy_and_ema(p, i, cp, ep, omd);
      },
      [&](int i, int) {
        f32x4 pw = pv[i], mw = mv[i], vw = vv[i];
        const f32x4 gw = gv[i];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float p = pw[e], m = mw[e], v = vw[e];
          adam_elem(p, gw[e], m, v, t.wd, grad_scale, clip, gclip, alpha, h);
          pw[e] = p; mw[e] = m; vw[e] = v;
        }
        pv[i] = pw; mv[i] = mw; vv[i] = vw;
        copy_and_ema4(pw, i, w.head, cp, ep, omd);
      });
}

// ---- LAMB (You et al. 2020: Adam's direction, decoupled weight decay, LARS's per-tensor trust ratio) --------------
//   m = b1*m + (1-b1)*gs;  v = b2*v + (1-b2)*gs*gs;  r = (m/bc1) / (sqrt(v)/bc2 + eps) + wd_t*p     (gs = g*grad_scale)
//   phi[t] = |p| / |r|  if tensor t is adapted, |p| > 0 and |r| > 0, else 1;   p -= (lr*lr_mult[t]*phi[t]) * r
// |r| needs the moments AFTER they took this step's gradient, so the pass has launches of its own over the Adam
// tables (s1 = m, s2 = v, the AdamState record) and the norm pass's side table and scratch:
//   launch 1: adam_advance_kernel;
//   launch 2: one block per chunk row: m, v updated and stored, one record {sum p^2, sum gs^2, sum r^2} (fp64, the
//             norm pass's fixed order) per row;
//   launch 3: one block, one wave per tensor: norms[t] = {|p|, |r|, |gs|}, lr_scale[t] = phi[t];
//   launch 4: one block per chunk row: r again from the stored p, m, v (p has not changed in between, so these
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
                                                                        const ChunkRow* __restrict__ chunks,
                                                                        LambHyper h, NormRec* __restrict__ recs) {
  if (h.skip_flag && *h.skip_flag) return;  // m, v and the records stay
  const int tid = threadIdx.x;
  const ChunkRow c = chunks[blockIdx.x];
  const OptTensor t = tens[c.t];
  NormRec a = {0.0, 0.0, 0.0};
  if (t.g) {  // (an EMA-only row writes a zero record)
    const float grad_scale = h.dyn[2];
    const AdamState s = *h.state;
    const float* pp = t.p + c.start;
    const float* gp = t.g + c.start;
    float* mp = t.s1 + c.start;
    float* vp = t.s2 + c.start;
    const WalkPlan w = walk_plan(4, (uintptr_t)pp, chunk_len(t.n, c.start, OPT_CHUNK), same16(pp, gp, mp, vp));
    const f32x4* pv = (const f32x4*)(pp + w.head);
    const f32x4* gv = (const f32x4*)(gp + w.head);
    f32x4* mv = (f32x4*)(mp + w.head);
    f32x4* vv = (f32x4*)(vp + w.head);
    walk<256, 4>(
        w, tid,
        [&](int i) {
          const float p = pp[i], g = lamb_gs(gp[i], grad_scale);
          float m = mp[i], v = vp[i];
          lamb_moments(g, m, v, h);
          mp[i] = m; vp[i] = v;
          lamb_acc(a, p, g, lamb_dir(p, m, v, t.wd, s.bc1, s.bc2, h.eps));
        },
        [&](int i, int) {
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
        });
  }
  store_norm_rec(recs, a, tid);  // (as multi_tensor_norm_kernel)
}

__global__ __launch_bounds__(NORM_FIN_THREADS) void multi_tensor_lamb_finalize_kernel(
    const NormMeta* __restrict__ meta, int ntens, const NormRec* __restrict__ recs, const int* skip_flag,
    float* __restrict__ norms, float* __restrict__ lr_scale) {
  if (skip_flag && *skip_flag) return;  // the previous step's outputs stay
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (int t = wv; t < ntens; t += NORM_FIN_THREADS / 64) {  // one wave per tensor
    const NormMeta m = meta[t];
    double s[3];  // p2, gs2, r2
    record_sum(recs, m.rows, lane, s);
    if (lane == 0) {
      const double pn = sqrt(s[0]), rn = sqrt(s[2]);
      norms[3 * t] = (float)pn;
      norms[3 * t + 1] = (float)rn;
      norms[3 * t + 2] = (float)sqrt(s[1]);
      lr_scale[t] = (m.adapt && pn > 0.0 && rn > 0.0) ? (float)(pn / rn) : 1.f;  // (a NaN norm fails both tests)
    }
  }
}

// 12 B read + 6 B written per element with the bf16 copy (+8 B EMA): 16-byte accesses where weight, m, v (and the
// shadow; the bf16 copy at 8 bytes) reach a 16-byte boundary together, as multi_tensor_adam_kernel chooses.
__global__ __launch_bounds__(256) void multi_tensor_lamb_apply_kernel(const OptTensor* __restrict__ tens,
                                                                      const ChunkRow* __restrict__ chunks,
                                                                      LambHyper h) {
  if (h.skip_flag && *h.skip_flag) return;
  const int tid = threadIdx.x;
  const ChunkRow c = chunks[blockIdx.x];
  const OptTensor t = tens[c.t];
  const int len = chunk_len(t.n, c.start, OPT_CHUNK);
  const float ema_decay = h.dyn[1];
  if (!t.g) {  // EMA-only row (BN moving statistics), as in multi_tensor_opt_kernel
    if (h.use_ema && t.ema) ema_only_row(t.ema + c.start, t.p + c.start, len, ema_decay, tid);
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
  const bool vec_ok = same16(pp, mp, vp) && (!ep || same16(pp, ep)) && copy8_ok(cp, (uintptr_t)pp);
  const WalkPlan w = walk_plan(4, (uintptr_t)pp, len, vec_ok);
  f32x4* pv = (f32x4*)(pp + w.head);
  const f32x4* mv = (const f32x4*)(mp + w.head);
  const f32x4* vv = (const f32x4*)(vp + w.head);
  walk<256, 4>(
      w, tid,
      [&](int i) {
        const float p = elem(pp[i], mp[i], vp[i]);
        pp[i] = p;
        copy_and_ema(p, i, cp, ep, omd);
      },
      [&](int i, int) {
        f32x4 pw = pv[i];
        const f32x4 mw = mv[i], vw = vv[i];
#pragma unroll
        for (int e = 0; e < 4; ++e) pw[e] = elem(pw[e], mw[e], vw[e]);
        pv[i] = pw;
        copy_and_ema4(pw, i, w.head, cp, ep, omd);
      });
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

}  // namespace dtm
using namespace dtm;

DTM_API int dtm_opt_chunk_size() { return OPT_CHUNK; }
DTM_API int dtm_opt_tensor_bytes() { return (int)sizeof(OptTensor); }
DTM_API int dtm_opt_chunk_bytes() { return (int)sizeof(ChunkRow); }

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
                     (const OptTensor*)tensors_dev, (const ChunkRow*)chunks_dev, h);
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
                       (const OptTensor*)tensors_dev, (const ChunkRow*)chunks_dev, h);
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
                       (const OptTensor*)tensors_dev, (const ChunkRow*)chunks_dev, h, recs);
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
                       (const OptTensor*)tensors_dev, (const ChunkRow*)chunks_dev, h, recs);
  if (ntens > 0)
    hipLaunchKernelGGL(multi_tensor_lamb_finalize_kernel, dim3(1), dim3(NORM_FIN_THREADS), 0, (hipStream_t)stream,
                       (const NormMeta*)meta_dev, ntens, (const NormRec*)recs, skip_flag, norms, lr_scale);
  if (num_chunks > 0)
    hipLaunchKernelGGL(multi_tensor_lamb_apply_kernel, dim3(num_chunks), dim3(256), 0, (hipStream_t)stream,
                       (const OptTensor*)tensors_dev, (const ChunkRow*)chunks_dev, h);
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
