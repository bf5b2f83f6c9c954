// Shared core of the paged-attention kernels in paged_attn.hip: every formula
// whose bits the kernels must agree on is written here exactly once, so the
// fast kernels equal their oracle kernels by construction.  The kernels keep
// what really differs between them: when loads are issued, where the K/V
// fragments come from, and where the partials meet.
//
// Lane roles (wave of 64): col = lane & 15, hi = lane >> 4.  A score tile
// (MFMA C layout) holds key position pt*16 + hi*4 + r of score COLUMN col (a
// GQA head in decode, a q row in prefill); an output tile holds dim
// dt*16 + col of output ROW hi*4 + r.
#pragma once

#include "common.h"

#define QSA_PAGE 64

using bf16x8_a = __attribute__((ext_vector_type(8))) short;
using f32x4_a = __attribute__((ext_vector_type(4))) float;
using u32x4_a = __attribute__((ext_vector_type(4))) unsigned int;

// Lane exchange is bare ds_bpermute on byte addresses (lane * 4): the same
// data movement as __shfl/__shfl_xor without their per-call range check,
// which costs VALU work and registers in the page loop.
__device__ __forceinline__ float qsa_bperm_f(int byte_addr, float v) {
  return __builtin_bit_cast(
      float, __builtin_amdgcn_ds_bpermute(byte_addr, __builtin_bit_cast(int, v)));
}
__device__ __forceinline__ unsigned int qsa_bperm_u(int byte_addr,
                                                   unsigned int v) {
  return (unsigned int)__builtin_amdgcn_ds_bpermute(byte_addr, (int)v);
}

// A lane's exchange partners, computed once per kernel from (col, hi).
struct qsa_lanes {
  int x16, x32;      // lane ^ 16, lane ^ 32: the other hi groups of the column
  int arow;          // lane hi*16 + hi*4 (+ r): holds output row hi*4 + r's column
  int src_a, src_b;  // P repack sources: (col, (2*hi)&3) and (col, (2*hi+1)&3)
  bool lo;           // hi < 2: repack takes the half's first tile, else second
};
__device__ __forceinline__ qsa_lanes qsa_lanes_of(int col, int hi) {
  const int lane4 = (hi * 16 + col) * 4;
  return {lane4 ^ 64, lane4 ^ 128, hi * (16 + 4) * 4,
          (col + (((2 * hi) & 3) << 4)) * 4,
          (col + (((2 * hi + 1) & 3) << 4)) * 4, hi < 2};
}

// Q B-fragments: lane holds Q[column col][k = ks*32 + hi*8 + e].
template <int D>
__device__ __forceinline__ void qsa_load_q(const unsigned short* qrow, int hi,
                                           bf16x8_a (&qf)[D / 32]) {
#pragma unroll
  for (int ks = 0; ks < D / 32; ++ks)
    qf[ks] = *reinterpret_cast<const bf16x8_a*>(qrow + ks * 32 + hi * 8);
}

// Scores of one page, K fragments straight from global memory: 4 pos-tiles
// x D/32 MFMAs.  A-frag: lane holds K[pos = pt*16 + col][k = ks*32 + hi*8 + e];
// K layout element (pos, k) at ((k/8)*64 + pos)*8 + k%8, i.e. 16 B at
// ((ks*4 + hi)*64 + pos)*8.
template <int D>
__device__ __forceinline__ void qsa_scores_global(
    const unsigned short* kbase, const bf16x8_a (&qf)[D / 32], int col, int hi,
    f32x4_a (&sc)[4]) {
#pragma unroll
  for (int pt = 0; pt < 4; ++pt) {
    f32x4_a acc = {0.f, 0.f, 0.f, 0.f};
    const int pos = pt * 16 + col;
#pragma unroll
    for (int ks = 0; ks < D / 32; ++ks) {
      const bf16x8_a kf = *reinterpret_cast<const bf16x8_a*>(
          kbase + (((long long)(ks * 4 + hi) * QSA_PAGE) + pos) * 8);
      acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[ks], acc, 0, 0, 0);
    }
    sc[pt] = acc;
  }
}

// Mask and scale one page's scores in place; returns the lane-local max.
// A key survives when it is inside the page's valid prefix, (CAUSAL) not
// after the column's absolute q position qabs, and the column's row exists.
// page_pos0 = the page's first absolute key position.  Decode is the
// non-causal case with every row existing.
template <bool CAUSAL>
__device__ __forceinline__ float qsa_mask_scale(
    f32x4_a (&sc)[4], float scale, int hi, int nvalid, int page_pos0, int qabs,
    bool row_ok) {
  float pagemax = -3.0e38f;
#pragma unroll
  for (int pt = 0; pt < 4; ++pt) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int kpos = pt * 16 + hi * 4 + r;
      const bool ok = (kpos < nvalid) &&
                      (!CAUSAL || page_pos0 + kpos <= qabs) && row_ok;
      const float v = ok ? sc[pt][r] * scale : -3.0e38f;
      sc[pt][r] = v;
      pagemax = fmaxf(pagemax, v);
    }
  }
  return pagemax;
}

// Column reduce across the 4 hi groups: two xor hops.
template <bool MAX>
__device__ __forceinline__ float qsa_col_reduce(const qsa_lanes& L, float v) {
  const float a = qsa_bperm_f(L.x16, v);
  v = MAX ? fmaxf(v, a) : v + a;
  const float b = qsa_bperm_f(L.x32, v);
  return MAX ? fmaxf(v, b) : v + b;
}

// Online-softmax page update from the column-reduced pagemax: rescales
// o_acc, advances (m, lsum) and leaves P = exp(sc - m) (masked -> 0) as the
// two PV A-fragments pa[half].  Callers that may skip a fully masked page do
// so (wave-uniformly) BEFORE this call.
template <int DTILES>
__device__ __forceinline__ void qsa_page_update(
    const qsa_lanes& L, const f32x4_a (&sc)[4], float pagemax, float& m,
    float& lsum, f32x4_a (&o_acc)[DTILES], bf16x8_a (&pa)[2]) {
  const float m_new = fmaxf(m, pagemax);
  float alpha = __expf(m - m_new);
  if (m <= -3.0e38f) alpha = 0.f;
  m = m_new;
  // o_acc element (dt, r) belongs to OUTPUT ROW hi*4 + r, while alpha lives
  // per score COLUMN: fetch each row's own alpha from the lane holding that
  // column — the lane's own alpha mis-scales other rows' history whenever
  // per-row maxima diverge across pages
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const float alpha_r = qsa_bperm_f(L.arow + r * 4, alpha);
#pragma unroll
    for (int dt = 0; dt < DTILES; ++dt) o_acc[dt][r] *= alpha_r;
  }
  unsigned int ppk[8];   // tile pt -> 2 uints (4 bf16 = positions r0..3)
  float psum = 0.f;
#pragma unroll
  for (int pt = 0; pt < 4; ++pt) {
    float p[4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
      p[r] = (sc[pt][r] > -1.0e38f) ? __expf(sc[pt][r] - m_new) : 0.f;
    psum += p[0] + p[1] + p[2] + p[3];
    ppk[pt * 2] = f32x2_to_bf16x2(p[0], p[1]);
    ppk[pt * 2 + 1] = f32x2_to_bf16x2(p[2], p[3]);
  }
  lsum = lsum * alpha + qsa_col_reduce<false>(L, psum);
  // P repack: the PV A-fragment needs lane (col, hi) to hold
  // P[col][pos = half*32 + hi*8 + e], i.e. tile half*2 + (hi>>1), packed
  // pairs of source lanes src_a and src_b.  The register index must be
  // compile-time, so both candidate tiles are exchanged and lo selects.
#pragma unroll
  for (int half = 0; half < 2; ++half) {
    const int tA = half * 4, tB = half * 4 + 2;   // ppk index of tile, hi<2 / hi>=2
    const unsigned int a0A = qsa_bperm_u(L.src_a, ppk[tA]);
    const unsigned int a1A = qsa_bperm_u(L.src_a, ppk[tA + 1]);
    const unsigned int b0A = qsa_bperm_u(L.src_b, ppk[tA]);
    const unsigned int b1A = qsa_bperm_u(L.src_b, ppk[tA + 1]);
    const unsigned int a0B = qsa_bperm_u(L.src_a, ppk[tB]);
    const unsigned int a1B = qsa_bperm_u(L.src_a, ppk[tB + 1]);
    const unsigned int b0B = qsa_bperm_u(L.src_b, ppk[tB]);
    const unsigned int b1B = qsa_bperm_u(L.src_b, ppk[tB + 1]);
    const u32x4_a pu = {L.lo ? a0A : a0B, L.lo ? a1A : a1B,
                        L.lo ? b0A : b0B, L.lo ? b1A : b1B};
    pa[half] = __builtin_bit_cast(bf16x8_a, pu);
  }
}

// Store one split's fp32 partials: o rows (head = hi*4 + r < R) at
// po + head*o_stride when write_o, and (m, l) of head = lane < R at
// pml + lane*ml_stride.  Strides in floats; global memory or LDS.
template <int DTILES>
__device__ __forceinline__ void qsa_store_partials(
    const f32x4_a (&o_acc)[DTILES], float m, float lsum, bool write_o,
    float* po, int o_stride, float* pml, int ml_stride, int R, int lane) {
  const int col = lane & 15, hi = lane >> 4;
  if (write_o) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int head = hi * 4 + r;
      if (head < R) {
#pragma unroll
        for (int dt = 0; dt < DTILES; ++dt)
          po[head * o_stride + dt * 16 + col] = o_acc[dt][r];
      }
    }
  }
  if (lane < R)
    *reinterpret_cast<float2*>(pml + lane * ml_stride) = make_float2(m, lsum);
}

// Merge one (head, d) over NS splits: split s's (m, l) at ml + s*ml_stride,
// its o at o[s*o_stride].  Empty splits (l <= 0) do not take part.
__device__ __forceinline__ float qsa_merge_splits(
    int NS, const float* ml, int ml_stride, const float* o, int o_stride) {
  float M = -3.0e38f;
  for (int s = 0; s < NS; ++s)
    if (ml[s * ml_stride + 1] > 0.f) M = fmaxf(M, ml[s * ml_stride]);
  float L = 0.f, acc = 0.f;
  for (int s = 0; s < NS; ++s) {
    const float ls = ml[s * ml_stride + 1];
    if (ls <= 0.f) continue;
    const float w = __expf(ml[s * ml_stride] - M);
    L += w * ls;
    acc += w * o[s * o_stride];
  }
  return (L > 0.f) ? acc / L : 0.f;
}

// Prefill epilogue of one 16-row block: per-row 1/l (fetched from the lane
// holding the row's column) and bf16 store of rows qr < nrows to
// orow0 + qr*row_stride.
template <int DTILES>
__device__ __forceinline__ void qsa_prefill_store(
    const qsa_lanes& L, const f32x4_a (&o_acc)[DTILES], float lsum,
    unsigned short* orow0, int row_stride, int nrows, int col, int hi) {
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int qr = hi * 4 + r;
    const float lr = qsa_bperm_f(L.arow + r * 4, lsum);
    const float inv = (lr > 0.f) ? 1.f / lr : 0.f;
    if (qr < nrows) {
      unsigned short* orow = orow0 + (long long)qr * row_stride;
#pragma unroll
      for (int dt = 0; dt < DTILES; ++dt)
        orow[dt * 16 + col] = f32_to_bf16(o_acc[dt][r] * inv);
    }
  }
}

// RoPE of 8 consecutive dims (a) and their +D/2 partners (b), 2 bf16 per
// uint; cosr/sinr point at the row's table entries for those 8 dims.  The
// scalar kernels qsa_rope_kv_append and qsa_rope_kernel are its oracle.
__device__ __forceinline__ void qsa_rope8(uint4& a, uint4& b,
                                          const float* cosr, const float* sinr) {
  float c[8], s[8];
  *reinterpret_cast<float4*>(c) = *reinterpret_cast<const float4*>(cosr);
  *reinterpret_cast<float4*>(c + 4) = *reinterpret_cast<const float4*>(cosr + 4);
  *reinterpret_cast<float4*>(s) = *reinterpret_cast<const float4*>(sinr);
  *reinterpret_cast<float4*>(s + 4) = *reinterpret_cast<const float4*>(sinr + 4);
  unsigned int* au = reinterpret_cast<unsigned int*>(&a);
  unsigned int* bu = reinterpret_cast<unsigned int*>(&b);
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float2 x0 = bf16x2_to_f32x2(au[e]);
    const float2 x1 = bf16x2_to_f32x2(bu[e]);
    const float c0 = c[2 * e], c1 = c[2 * e + 1];
    const float s0 = s[2 * e], s1 = s[2 * e + 1];
    au[e] = (unsigned int)f32_to_bf16(x0.x * c0 - x1.x * s0) |
            ((unsigned int)f32_to_bf16(x0.y * c1 - x1.y * s1) << 16);
    bu[e] = (unsigned int)f32_to_bf16(x0.x * s0 + x1.x * c0) |
            ((unsigned int)f32_to_bf16(x0.y * s1 + x1.y * c1) << 16);
  }
}
