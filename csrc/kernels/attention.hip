// Fused multi-head self-attention on bf16 rows [N][L][heads * D] (NHWC with L = H * W), D in {32, 64, 128}, fp32
// arithmetic on v_mfma_f32_16x16x32_bf16.  Per sample n and head h (channel h * D + c is component c of head h):
//   S = scale Q K^T      m_i = max_j S_ij      P_ij = exp(S_ij - m_i)      l_i = sum_j P_ij
//   O = (P V) / l  (one bf16 rounding)         lse_i = m_i + log l_i  (fp32, kept for the backward)
//   delta_i = sum_c dO_ic O_ic      P = exp(S - lse)      dV = P^T dO      dP = dO V^T      dS = P (dP - delta)
//   dQ = scale dS K                 dK = scale dS^T Q
// P and dS enter their second matrix product rounded to bf16 (they are MFMA operands); l is summed from the unrounded
// P.  S, P, dP and dS live in registers only.  Each tensor has its own row pitch in elements (a multiple of 8, rows
// of one sample L apart, 16-byte aligned base), so q, k, v may be the thirds of one fused qkv row.
//
// Work split.  Every MFMA kernel has an owner side, 64 rows of one (n, head) per block of 4 waves, 16 rows per wave,
// whose operand fragments stay in registers for the whole block, and a walked side, whose 64-row tiles go through LDS:
// 16-byte global loads of tile t + 1 are in flight in registers while tile t is multiplied, then stored into the
// other of two LDS buffers; one barrier per tile.  Grid (ceil(L / 64), heads, N).  Rows >= L of a tile are staged as
// zeros and never stored.
//
// The logits are computed with the walked side on the MFMA's row side, so that lane (li = lane % 16, g = lane / 16)
// ends with the four values (walked rows 16 j + 4 g + 0..3) x (owner row li) of each 16-row subtile j.  An MFMA's
// reduction index may be permuted as long as both operands agree, so the eight values of subtiles 2 jj and 2 jj + 1
// are, after exp and rounding, this lane's B operand of the second product over walked rows 32 jj .. 32 jj + 31
// (slot 8 g + e is row 32 jj + 16 (e / 4) + 4 g + e % 4), and the matching A operand, the walked tile transposed, is
// two ds_read_b64_tr_b16 of rows 32 jj + 4 g .. and 32 jj + 16 + 4 g ...  The second product is computed transposed
// too (O^T = V^T P^T): its accumulators are four consecutive channels of owner row li, so the softmax statistics of
// a row, its rescaling and its 8-byte stores never leave the lane; a row's max and sum cross the four 16-lane groups
// by two xor shuffles in a fixed order.  Tiles read by rows only have a pitch of D + 8 elements (the 16 lanes of a
// 16-byte fragment read fall on 16 distinct bank quads), tiles read transposed D + 16 (the 32 lanes of an 8-byte
// transposed read cover the 64 banks once).
//
//   mhsa_fwd_kernel<D>      owner Q, walks (K, V): online softmax, m, l and O in fp32, rescaled by exp(m_old - m_new);
//                           keys >= L get -inf logits.  Writes o and lse.
//   mhsa_delta_kernel       delta from dO and o.
//   mhsa_bwd_dkv_kernel<D>  owner (K, V), walks (Q, dO, lse, delta): here the owner is on the MFMA's column side of
//                           S and dP, the same lane pattern with queries and keys exchanged; query rows >= L carry
//                           lse = +inf, so P = 0.  dK and dV accumulate in registers and are written once.
//   mhsa_bwd_dq_kernel<D>   owner (Q, dO, lse, delta), walks (K, V); keys >= L get -inf logits.  Writes dq.
// No atomics, no flags, no waiting between blocks, a fixed summation order: every output keeps its bits.  LDS per
// block: forward 2 (64 (D + 8) + 64 (D + 16)) * 2 B = 70 KiB at D = 128, backward up to 73 KiB, asked for through
// hipFuncAttributeMaxDynamicSharedMemorySize.
#include "common.h"

namespace dtm {
namespace {

constexpr int AT_T = 256;  // lanes per block
constexpr int AT_R = 64;   // rows per tile
constexpr int AT_LMAX = 4096;
typedef __attribute__((address_space(3))) short4v lds_s4;

struct AttnGeom {
  int N, L, heads;
  long pq, pk, pv;  // row pitches of q, k, v in elements
  float scale;
};

__device__ __forceinline__ short8 as_s8(uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
  return __builtin_bit_cast(short8, make_uint4(a, b, c, d));
}
__device__ __forceinline__ short8 zero_s8() { return (short8){0, 0, 0, 0, 0, 0, 0, 0}; }
// the lane's eight values of two subtiles as one bf16 operand
__device__ __forceinline__ short8 pack8(const f32x4& a, const f32x4& b) {
  return as_s8(pack2bf(a[0], a[1]), pack2bf(a[2], a[3]), pack2bf(b[0], b[1]), pack2bf(b[2], b[3]));
}

// This lane's 16-byte chunks of the 64 x D tile whose first row is row0 (base: row 0 of the sample, at the head's
// first channel); rows >= L are zeros.
template <int D>
__device__ __forceinline__ void tile_load(uint4 (&r)[D / 32], const bf16_t* __restrict__ base, long pitch, int row0,
                                          int L) {
  constexpr int CPR = D / 8;
#pragma unroll
  for (int i = 0; i < D / 32; ++i) {
    const int c = threadIdx.x + AT_T * i, row = row0 + c / CPR;
    r[i] = row < L ? *(const uint4*)(base + (size_t)row * pitch + (c % CPR) * 8) : make_uint4(0u, 0u, 0u, 0u);
  }
}
template <int D, int PITCH>
__device__ __forceinline__ void tile_store(bf16_t* tile, const uint4 (&r)[D / 32]) {
  constexpr int CPR = D / 8;
#pragma unroll
  for (int i = 0; i < D / 32; ++i) {
    const int c = threadIdx.x + AT_T * i;
    *(uint4*)(tile + (c / CPR) * PITCH + (c % CPR) * 8) = r[i];
  }
}
// A row's D / 32 operand fragments straight from global memory (zeros for a row >= L)
template <int D>
__device__ __forceinline__ void row_frags(short8 (&f)[D / 32], const bf16_t* __restrict__ base, long pitch, int row,
                                          int L, int g) {
#pragma unroll
  for (int kk = 0; kk < D / 32; ++kk)
    f[kk] = row < L ? *(const short8*)(base + (size_t)row * pitch + kk * 32 + 8 * g) : zero_s8();
}
__device__ __forceinline__ short8 frag_row(const bf16_t* tile, int pitch, int row, int col) {
  return *(const short8*)(tile + row * pitch + col);
}
// The transposed operand of the permuted reduction: column c0 + li, rows k0 .. k0 + 3 and k0 + 16 .. k0 + 19
// (k0 = 32 jj + 4 g); the 16 lanes of a group address rows k0 + tq, columns c0 + 4 tp ..
__device__ __forceinline__ short8 frag_tr(const bf16_t* tile, int pitch, int k0, int c0, int tq, int tp) {
  const bf16_t* p = tile + (k0 + tq) * pitch + c0 + 4 * tp;
  const short4v lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4*)p);
  const short4v hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4*)(p + 16 * pitch));
  return (short8){lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}
// four consecutive channels of one row, one rounding each
__device__ __forceinline__ void store4(bf16_t* p, const f32x4& a, float s) {
  *(uint2*)p = make_uint2(pack2bf(a[0] * s, a[1] * s), pack2bf(a[2] * s, a[3] * s));
}
__device__ __forceinline__ float group_max(float v) {
  v = fmaxf(v, __shfl_xor(v, 16, 64));
  return fmaxf(v, __shfl_xor(v, 32, 64));
}
__device__ __forceinline__ float group_sum(float v) {
  v += __shfl_xor(v, 16, 64);
  return v + __shfl_xor(v, 32, 64);
}

struct Lane {
  int wave, li, g, tq, tp;
};
__device__ __forceinline__ Lane make_lane() {
  const int lane = threadIdx.x & 63;
  Lane t;
  t.wave = threadIdx.x >> 6; t.li = lane & 15; t.g = lane >> 4; t.tq = t.li >> 2; t.tp = t.li & 3;
  return t;
}

// ------------------------------------------------------------------------------------------------------------
template <int D>
__global__ __launch_bounds__(AT_T) void mhsa_fwd_kernel(const bf16_t* __restrict__ q, const bf16_t* __restrict__ k,
                                                        const bf16_t* __restrict__ v, bf16_t* __restrict__ o,
                                                        float* __restrict__ lse, AttnGeom a) {
  constexpr int KP = D + 8, VP = D + 16, KT = AT_R * KP, BUF = KT + AT_R * VP, NK = D / 32, NC = D / 16;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  bf16_t* lds = (bf16_t*)smem;
  const Lane t = make_lane();
  const int h = blockIdx.y, n = blockIdx.z, L = a.L;
  const int row = blockIdx.x * AT_R + t.wave * 16 + t.li;
  const bf16_t* kb = k + (size_t)n * L * a.pk + h * D;
  const bf16_t* vb = v + (size_t)n * L * a.pv + h * D;
  short8 qf[NK];
  row_frags<D>(qf, q + (size_t)n * L * a.pq + h * D, a.pq, row, L, t.g);
  f32x4 acc[NC];
#pragma unroll
  for (int ct = 0; ct < NC; ++ct) acc[ct] = (f32x4){0.f, 0.f, 0.f, 0.f};
  float m = -INFINITY, l = 0.f;  // l: this lane's keys only, until the end

  const int nt = (L + AT_R - 1) / AT_R;
  uint4 kr[NK], vr[NK];
  tile_load<D>(kr, kb, a.pk, 0, L);
  tile_load<D>(vr, vb, a.pv, 0, L);
  tile_store<D, KP>(lds, kr);
  tile_store<D, VP>(lds + KT, vr);
  __syncthreads();
  for (int it = 0; it < nt; ++it) {
    const bf16_t* kt = lds + (it & 1) * BUF;
    const bf16_t* vt = kt + KT;
    const bool more = it + 1 < nt;
    if (more) {
      tile_load<D>(kr, kb, a.pk, (it + 1) * AT_R, L);
      tile_load<D>(vr, vb, a.pv, (it + 1) * AT_R, L);
    }
    f32x4 s[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      s[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kk = 0; kk < NK; ++kk)
        s[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag_row(kt, KP, 16 * j + t.li, 32 * kk + 8 * t.g), qf[kk],
                                                       s[j], 0, 0, 0);
    }
    float mx = -INFINITY;
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int key = it * AT_R + 16 * j + 4 * t.g + i;
        s[j][i] = key < L ? s[j][i] * a.scale : -INFINITY;
        mx = fmaxf(mx, s[j][i]);
      }
    const float mn = fmaxf(m, group_max(mx));  // finite: key it * 64 of every tile is below L
    const float alpha = __expf(m - mn);
    m = mn;
    float ps = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        s[j][i] = __expf(s[j][i] - mn);
        ps += s[j][i];
      }
    l = l * alpha + ps;
    const short8 pf[2] = {pack8(s[0], s[1]), pack8(s[2], s[3])};
#pragma unroll
    for (int ct = 0; ct < NC; ++ct) {
      acc[ct] *= alpha;
#pragma unroll
      for (int jj = 0; jj < 2; ++jj)
        acc[ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag_tr(vt, VP, 32 * jj + 4 * t.g, 16 * ct, t.tq, t.tp),
                                                          pf[jj], acc[ct], 0, 0, 0);
    }
    if (more) {
      bf16_t* nb = lds + ((it + 1) & 1) * BUF;  // last read before the previous barrier
      tile_store<D, KP>(nb, kr);
      tile_store<D, VP>(nb + KT, vr);
    }
    __syncthreads();
  }
  l = group_sum(l);
  if (row < L) {
    const float inv = 1.f / l;
    bf16_t* orow = o + ((size_t)n * L + row) * ((size_t)a.heads * D) + h * D + 4 * t.g;
#pragma unroll
    for (int ct = 0; ct < NC; ++ct) store4(orow + 16 * ct, acc[ct], inv);
    if (t.g == 0) lse[((size_t)n * a.heads + h) * L + row] = m + __logf(l);
  }
}

// delta[n][h][row] = sum_c dO * o; dO and o are contiguous, so lane idx owns elements 8 idx .. 8 idx + 7 and the
// D / 8 lanes of one (row, head) are neighbours within a wave.
template <int D>
__global__ __launch_bounds__(AT_T) void mhsa_delta_kernel(const bf16_t* __restrict__ dO, const bf16_t* __restrict__ o,
                                                          float* __restrict__ delta, size_t total, int L, int heads) {
  const size_t idx = (size_t)blockIdx.x * AT_T + threadIdx.x;
  float s = 0.f;
  if (idx < total) {
    const uint4 x = *(const uint4*)(dO + idx * 8), y = *(const uint4*)(o + idx * 8);
    const uint32_t xw[4] = {x.x, x.y, x.z, x.w}, yw[4] = {y.x, y.y, y.z, y.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) s += lo_bf(xw[j]) * lo_bf(yw[j]) + hi_bf(xw[j]) * hi_bf(yw[j]);
  }
#pragma unroll
  for (int d = 1; d < D / 8; d <<= 1) s += __shfl_xor(s, d, 64);
  if (idx < total && idx % (D / 8) == 0) {
    const size_t rh = idx / (D / 8), r = rh / heads;  // r = n * L + row
    delta[((r / L) * heads + rh % heads) * L + r % L] = s;
  }
}

// Owner: 64 keys.  LDS buffer: the Q tile and the dO tile (both also read transposed), then lse[64], delta[64].
template <int D>
__global__ __launch_bounds__(AT_T) void mhsa_bwd_dkv_kernel(const bf16_t* __restrict__ q, const bf16_t* __restrict__ k,
                                                            const bf16_t* __restrict__ v,
                                                            const bf16_t* __restrict__ dO,
                                                            const float* __restrict__ lse,
                                                            const float* __restrict__ delta, bf16_t* __restrict__ dk,
                                                            bf16_t* __restrict__ dv, AttnGeom a) {
  constexpr int TP = D + 16, TT = AT_R * TP, BUF = 2 * TT + 4 * AT_R, NK = D / 32, NC = D / 16;  // in bf16 elements
  extern __shared__ __attribute__((aligned(16))) char smem[];
  bf16_t* lds = (bf16_t*)smem;
  const Lane t = make_lane();
  const int h = blockIdx.y, n = blockIdx.z, L = a.L;
  const int row = blockIdx.x * AT_R + t.wave * 16 + t.li;
  const size_t HD = (size_t)a.heads * D;
  const bf16_t* qb = q + (size_t)n * L * a.pq + h * D;
  const bf16_t* ob = dO + (size_t)n * L * HD + h * D;
  const float* sl = lse + ((size_t)n * a.heads + h) * L;
  const float* sd = delta + ((size_t)n * a.heads + h) * L;
  short8 kf[NK], vf[NK];
  row_frags<D>(kf, k + (size_t)n * L * a.pk + h * D, a.pk, row, L, t.g);
  row_frags<D>(vf, v + (size_t)n * L * a.pv + h * D, a.pv, row, L, t.g);
  f32x4 ak[NC], av[NC];
#pragma unroll
  for (int ct = 0; ct < NC; ++ct) ak[ct] = av[ct] = (f32x4){0.f, 0.f, 0.f, 0.f};

  // lanes 0 .. 63 carry the tile's lse (+inf for a query >= L: P = 0), lanes 64 .. 127 its delta
  const int tid = threadIdx.x;
  auto stat_load = [&](int row0) -> float {
    const int r = row0 + (tid & 63);
    if (tid < 64) return r < L ? sl[r] : INFINITY;
    return (tid < 128 && r < L) ? sd[r] : 0.f;
  };
  auto stat_store = [&](bf16_t* buf, float x) {
    if (tid < 128) ((float*)(buf + 2 * TT))[tid] = x;
  };
  const int nt = (L + AT_R - 1) / AT_R;
  uint4 qr[NK], dr[NK];
  float sr;
  tile_load<D>(qr, qb, a.pq, 0, L);
  tile_load<D>(dr, ob, (long)HD, 0, L);
  sr = stat_load(0);
  tile_store<D, TP>(lds, qr);
  tile_store<D, TP>(lds + TT, dr);
  stat_store(lds, sr);
  __syncthreads();
  for (int it = 0; it < nt; ++it) {
    const bf16_t* qt = lds + (it & 1) * BUF;
    const bf16_t* dt = qt + TT;
    const float* st = (const float*)(qt + 2 * TT);
    const bool more = it + 1 < nt;
    if (more) {
      tile_load<D>(qr, qb, a.pq, (it + 1) * AT_R, L);
      tile_load<D>(dr, ob, (long)HD, (it + 1) * AT_R, L);
      sr = stat_load((it + 1) * AT_R);
    }
    f32x4 p[4], ds[4];  // lane: queries 16 j + 4 g + i of key li
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      f32x4 s = (f32x4){0.f, 0.f, 0.f, 0.f}, dp = s;
#pragma unroll
      for (int kk = 0; kk < NK; ++kk) {
        const int col = 32 * kk + 8 * t.g;
        s = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag_row(qt, TP, 16 * j + t.li, col), kf[kk], s, 0, 0, 0);
        dp = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag_row(dt, TP, 16 * j + t.li, col), vf[kk], dp, 0, 0, 0);
      }
      const float4 ls = *(const float4*)(st + 16 * j + 4 * t.g), dl = *(const float4*)(st + AT_R + 16 * j + 4 * t.g);
      const float lsv[4] = {ls.x, ls.y, ls.z, ls.w}, dlv[4] = {dl.x, dl.y, dl.z, dl.w};
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        p[j][i] = __expf(s[i] * a.scale - lsv[i]);
        ds[j][i] = p[j][i] * (dp[i] - dlv[i]);
      }
    }
    const short8 pf[2] = {pack8(p[0], p[1]), pack8(p[2], p[3])};
    const short8 df[2] = {pack8(ds[0], ds[1]), pack8(ds[2], ds[3])};
#pragma unroll
    for (int ct = 0; ct < NC; ++ct)
#pragma unroll
      for (int jj = 0; jj < 2; ++jj) {
        const int k0 = 32 * jj + 4 * t.g;
        av[ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag_tr(dt, TP, k0, 16 * ct, t.tq, t.tp), pf[jj], av[ct], 0,
                                                         0, 0);
        ak[ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag_tr(qt, TP, k0, 16 * ct, t.tq, t.tp), df[jj], ak[ct], 0,
                                                         0, 0);
      }
    if (more) {
      bf16_t* nb = lds + ((it + 1) & 1) * BUF;
      tile_store<D, TP>(nb, qr);
      tile_store<D, TP>(nb + TT, dr);
      stat_store(nb, sr);
    }
    __syncthreads();
  }
  if (row < L) {
    const size_t off = ((size_t)n * L + row) * HD + h * D + 4 * t.g;
#pragma unroll
    for (int ct = 0; ct < NC; ++ct) {
      store4(dk + off + 16 * ct, ak[ct], a.scale);
      store4(dv + off + 16 * ct, av[ct], 1.f);
    }
  }
}

// Owner: 64 queries.  LDS buffer: the K tile (also read transposed), the V tile (read by rows only).
template <int D>
__global__ __launch_bounds__(AT_T) void mhsa_bwd_dq_kernel(const bf16_t* __restrict__ q, const bf16_t* __restrict__ k,
                                                           const bf16_t* __restrict__ v, const bf16_t* __restrict__ dO,
                                                           const float* __restrict__ lse,
                                                           const float* __restrict__ delta, bf16_t* __restrict__ dq,
                                                           AttnGeom a) {
  constexpr int KP = D + 16, VP = D + 8, KT = AT_R * KP, BUF = KT + AT_R * VP, NK = D / 32, NC = D / 16;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  bf16_t* lds = (bf16_t*)smem;
  const Lane t = make_lane();
  const int h = blockIdx.y, n = blockIdx.z, L = a.L;
  const int row = blockIdx.x * AT_R + t.wave * 16 + t.li;
  const size_t HD = (size_t)a.heads * D;
  const bf16_t* kb = k + (size_t)n * L * a.pk + h * D;
  const bf16_t* vb = v + (size_t)n * L * a.pv + h * D;
  short8 qf[NK], of[NK];
  row_frags<D>(qf, q + (size_t)n * L * a.pq + h * D, a.pq, row, L, t.g);
  row_frags<D>(of, dO + (size_t)n * L * HD + h * D, (long)HD, row, L, t.g);
  const size_t si = ((size_t)n * a.heads + h) * L + row;
  const float ls = row < L ? lse[si] : INFINITY, dl = row < L ? delta[si] : 0.f;
  f32x4 acc[NC];
#pragma unroll
  for (int ct = 0; ct < NC; ++ct) acc[ct] = (f32x4){0.f, 0.f, 0.f, 0.f};

  const int nt = (L + AT_R - 1) / AT_R;
  uint4 kr[NK], vr[NK];
  tile_load<D>(kr, kb, a.pk, 0, L);
  tile_load<D>(vr, vb, a.pv, 0, L);
  tile_store<D, KP>(lds, kr);
  tile_store<D, VP>(lds + KT, vr);
  __syncthreads();
  for (int it = 0; it < nt; ++it) {
    const bf16_t* kt = lds + (it & 1) * BUF;
    const bf16_t* vt = kt + KT;
    const bool more = it + 1 < nt;
    if (more) {
      tile_load<D>(kr, kb, a.pk, (it + 1) * AT_R, L);
      tile_load<D>(vr, vb, a.pv, (it + 1) * AT_R, L);
    }
    f32x4 ds[4];  // lane: keys 16 j + 4 g + i of query li
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      f32x4 s = (f32x4){0.f, 0.f, 0.f, 0.f}, dp = s;
#pragma unroll
      for (int kk = 0; kk < NK; ++kk) {
        const int col = 32 * kk + 8 * t.g;
        s = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag_row(kt, KP, 16 * j + t.li, col), qf[kk], s, 0, 0, 0);
        dp = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag_row(vt, VP, 16 * j + t.li, col), of[kk], dp, 0, 0, 0);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int key = it * AT_R + 16 * j + 4 * t.g + i;
        const float pv = __expf((key < L ? s[i] * a.scale : -INFINITY) - ls);
        ds[j][i] = pv * (dp[i] - dl);
      }
    }
    const short8 df[2] = {pack8(ds[0], ds[1]), pack8(ds[2], ds[3])};
#pragma unroll
    for (int ct = 0; ct < NC; ++ct)
#pragma unroll
      for (int jj = 0; jj < 2; ++jj)
        acc[ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag_tr(kt, KP, 32 * jj + 4 * t.g, 16 * ct, t.tq, t.tp),
                                                          df[jj], acc[ct], 0, 0, 0);
    if (more) {
      bf16_t* nb = lds + ((it + 1) & 1) * BUF;
      tile_store<D, KP>(nb, kr);
      tile_store<D, VP>(nb + KT, vr);
    }
    __syncthreads();
  }
  if (row < L) {
    bf16_t* drow = dq + ((size_t)n * L + row) * HD + h * D + 4 * t.g;
#pragma unroll
    for (int ct = 0; ct < NC; ++ct) store4(drow + 16 * ct, acc[ct], a.scale);
  }
}

// ------------------------------------------------------------------------------------------------------------
constexpr int fwd_lds(int D) { return 2 * (AT_R * (D + 8) + AT_R * (D + 16)) * 2; }
constexpr int dkv_lds(int D) { return 2 * (2 * AT_R * (D + 16) + 4 * AT_R) * 2; }

template <int D>
bool lds_ready() {
  static const bool ok =
      hipFuncSetAttribute((const void*)mhsa_fwd_kernel<D>, hipFuncAttributeMaxDynamicSharedMemorySize, fwd_lds(D)) ==
          hipSuccess &&
      hipFuncSetAttribute((const void*)mhsa_bwd_dq_kernel<D>, hipFuncAttributeMaxDynamicSharedMemorySize,
                          fwd_lds(D)) == hipSuccess &&
      hipFuncSetAttribute((const void*)mhsa_bwd_dkv_kernel<D>, hipFuncAttributeMaxDynamicSharedMemorySize,
                          dkv_lds(D)) == hipSuccess;
  return ok;
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// 0, or the entry points' negative code
int make_geom(int N, int L, int heads, int d, long pq, long pk, long pv, float scale, AttnGeom* g) {
  if (d != 32 && d != 64 && d != 128) return -1;
  if (N < 1 || heads < 1 || L < 1 || L > AT_LMAX || (long)N * heads > 65535) return -2;
  const long w = (long)heads * d;
  if (pq < w || pk < w || pv < w || pq % 8 || pk % 8 || pv % 8) return -1;
  g->N = N; g->L = L; g->heads = heads; g->pq = pq; g->pk = pk; g->pv = pv; g->scale = scale;
  return 0;
}

template <int D>
int launch_fwd(const bf16_t* q, const bf16_t* k, const bf16_t* v, bf16_t* o, float* lse, const AttnGeom& g,
               hipStream_t st) {
  if (!lds_ready<D>()) return -4;
  const dim3 grid((g.L + AT_R - 1) / AT_R, g.heads, g.N);
  hipLaunchKernelGGL(mhsa_fwd_kernel<D>, grid, dim3(AT_T), fwd_lds(D), st, q, k, v, o, lse, g);
  return 0;
}

template <int D>
int launch_bwd(const bf16_t* q, const bf16_t* k, const bf16_t* v, const bf16_t* o, const bf16_t* dO, const float* lse,
               float* delta, bf16_t* dq, bf16_t* dk, bf16_t* dv, const AttnGeom& g, hipStream_t st) {
  if (!lds_ready<D>()) return -4;
  const dim3 grid((g.L + AT_R - 1) / AT_R, g.heads, g.N);
  const size_t total = (size_t)g.N * g.L * g.heads * (D / 8);
  hipLaunchKernelGGL(mhsa_delta_kernel<D>, dim3((unsigned)((total + AT_T - 1) / AT_T)), dim3(AT_T), 0, st, dO, o,
                     delta, total, g.L, g.heads);
  hipLaunchKernelGGL(mhsa_bwd_dkv_kernel<D>, grid, dim3(AT_T), dkv_lds(D), st, q, k, v, dO, lse, delta, dk, dv, g);
  hipLaunchKernelGGL(mhsa_bwd_dq_kernel<D>, grid, dim3(AT_T), fwd_lds(D), st, q, k, v, dO, lse, delta, dq, g);
  return 0;
}

}  // namespace
}  // namespace dtm

using namespace dtm;

// q, k, v: bf16 rows of pitch pq, pk, pv elements (the head-major heads * d channels at the row's start), N * L rows
// each; o: bf16 [N][L][heads * d] contiguous; lse: fp32 [N][heads][L].  -1: d outside {32, 64, 128}, a null or
// misaligned pointer, a pitch below heads * d or no multiple of 8; -2: N, heads or L below 1, L above 4096 or
// N * heads above 65535; -4: the device refuses the LDS.  Nothing is launched after a negative code.
DTM_API int dtm_mhsa_fwd(const void* q, const void* k, const void* v, void* o, float* lse, long pq, long pk, long pv,
                         int N, int L, int heads, int d, float scale, void* stream) {
  AttnGeom g;
  const int rc = make_geom(N, L, heads, d, pq, pk, pv, scale, &g);
  if (rc) return rc;
  if (!q || !k || !v || !o || !lse) return -1;
  if (!aligned16(q) || !aligned16(k) || !aligned16(v) || !aligned16(o) || !aligned16(lse)) return -1;
  const bf16_t *qb = (const bf16_t*)q, *kb = (const bf16_t*)k, *vb = (const bf16_t*)v;
  hipStream_t st = (hipStream_t)stream;
  if (d == 32) return launch_fwd<32>(qb, kb, vb, (bf16_t*)o, lse, g, st);
  if (d == 64) return launch_fwd<64>(qb, kb, vb, (bf16_t*)o, lse, g, st);
  return launch_fwd<128>(qb, kb, vb, (bf16_t*)o, lse, g, st);
}

// o, dO, dq, dk, dv: bf16 [N][L][heads * d] contiguous; lse: the forward's; delta: fp32 [N][heads][L] workspace.
// Codes as the forward's.
DTM_API int dtm_mhsa_bwd(const void* q, const void* k, const void* v, const void* o, const void* dO, const float* lse,
                         float* delta, void* dq, void* dk, void* dv, long pq, long pk, long pv, int N, int L,
                         int heads, int d, float scale, void* stream) {
  AttnGeom g;
  const int rc = make_geom(N, L, heads, d, pq, pk, pv, scale, &g);
  if (rc) return rc;
  if (!q || !k || !v || !o || !dO || !lse || !delta || !dq || !dk || !dv) return -1;
  if (!aligned16(q) || !aligned16(k) || !aligned16(v) || !aligned16(o) || !aligned16(dO) || !aligned16(lse) ||
      !aligned16(delta) || !aligned16(dq) || !aligned16(dk) || !aligned16(dv))
    return -1;
  const bf16_t *qb = (const bf16_t*)q, *kb = (const bf16_t*)k, *vb = (const bf16_t*)v, *ob = (const bf16_t*)o,
               *gb = (const bf16_t*)dO;
  bf16_t *dqb = (bf16_t*)dq, *dkb = (bf16_t*)dk, *dvb = (bf16_t*)dv;
  hipStream_t st = (hipStream_t)stream;
  if (d == 32) return launch_bwd<32>(qb, kb, vb, ob, gb, lse, delta, dqb, dkb, dvb, g, st);
  if (d == 64) return launch_bwd<64>(qb, kb, vb, ob, gb, lse, delta, dqb, dkb, dvb, g, st);
  return launch_bwd<128>(qb, kb, vb, ob, gb, lse, delta, dqb, dkb, dvb, g, st);
}
