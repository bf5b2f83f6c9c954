// Shared core of the weight-streaming GEMM kernels (skinny_gemm.hip,
// skinny_gemm_fp8.hip, gemm_fp8_batch.hip): the dequantisation, the two
// packed weight layouts, the clamped activation rows, the skinny kernel body
// and the guarded store are written here exactly once, so the bf16 and fp8
// skinny kernels run the same loop by construction and every fp8 kernel
// reads the same stream.  The .hip files keep what really differs: which
// configurations exist, which one a shape gets, and the batch kernel's LDS
// pipeline.
//
// Lane roles (wave of 64) in mfma_f32_16x16x32_bf16: an A fragment holds
// A[row lane&15][k = (lane>>4)*8 + e], a B fragment W[col lane&15][same k],
// the C tile row (lane>>4)*4 + r of column lane&15.
#pragma once

#include "common.h"

using bf16x8 = __attribute__((ext_vector_type(8))) short;
using f32x2v = __attribute__((ext_vector_type(2))) float;
using f32x4 = __attribute__((ext_vector_type(4))) float;
using u32x4 = __attribute__((ext_vector_type(4))) unsigned int;

#define QSA_KCH 256  // k per wave-iteration: 4 k-blocks of 64, 8 MFMA k-steps

// 8 fp8 (OCP e4m3) bytes, as 2 dwords, -> bf16x8 fragment:
//   v_cvt_pk_f32_fp8 (2 fp8 -> 2 f32, exact)
//   v_perm_b32       (pack the two f32 high halves -> 2 bf16)
// The f32 -> bf16 TRUNCATION is exact: e4m3 has 3 mantissa bits, bf16 has 8,
// and every e4m3 value (normals and denormals) is exactly representable in
// bf16 -- the dequantised operand is bit-exact, so the MFMA math matches a
// bf16 kernel running on the dequantised weights.
__device__ __forceinline__ bf16x8 fp8x8_to_bf16x8(unsigned int a,
                                                  unsigned int b) {
  f32x2v f01 = __builtin_amdgcn_cvt_pk_f32_fp8(a, false);
  f32x2v f23 = __builtin_amdgcn_cvt_pk_f32_fp8(a, true);
  f32x2v f45 = __builtin_amdgcn_cvt_pk_f32_fp8(b, false);
  f32x2v f67 = __builtin_amdgcn_cvt_pk_f32_fp8(b, true);
  union { unsigned int u; float f; } u0, u1;
  union { unsigned int u[4]; bf16x8 v; } out;
  u0.f = f01.x; u1.f = f01.y;
  out.u[0] = __builtin_amdgcn_perm(u1.u, u0.u, 0x07060302u);
  u0.f = f23.x; u1.f = f23.y;
  out.u[1] = __builtin_amdgcn_perm(u1.u, u0.u, 0x07060302u);
  u0.f = f45.x; u1.f = f45.y;
  out.u[2] = __builtin_amdgcn_perm(u1.u, u0.u, 0x07060302u);
  u0.f = f67.x; u1.f = f67.y;
  out.u[3] = __builtin_amdgcn_perm(u1.u, u0.u, 0x07060302u);
  return out.v;
}

// One 16-byte weight load, plain or nontemporal (each weight byte is read
// once per step, so it need not displace L2 lines).
template <bool NT, class V>
__device__ __forceinline__ V qsa_load16(const V* p) {
  if (NT) return __builtin_nontemporal_load(p);
  return *reinterpret_cast<const V*>(__builtin_assume_aligned(p, 16));
}

// ---- the two weight-stream layouts -----------------------------------------
// Both are n-tile-major (16 output columns), then k-block-major, so that one
// wave instruction reads one contiguous 1 KiB block, perfectly coalesced.
// Each gives: the lane's base for n-tile nt, the offset of 64-k block kb from
// it, the load of a block, and the two 32-k B fragments of a loaded block.
// (Everything is static and takes the kernel's own pointer, so that the
// compiler keeps what it knows about a __restrict__ argument.)

// fp8 "fragment-pair-major" [N/16, K/64, 16, 4, 2, 8] (column, lane>>4,
// k-half, 8 codes): a lane's 16 B at byte (lane&15)*64 + (lane>>4)*16 of
// block (nt, kb) cover its 8 codes for BOTH 32-k fragments of the block --
// full-width dwordx4 loads on a byte stream, one load per lane per 64 k.
// Packed by dispatch.pack_weight_fp8.  scale: one f32 per output channel
// (s[n] = max|W[n,:]| / 448, W8A16), applied once in the epilogue.
struct qsa_fp8_stream {
  static constexpr bool kLoadW = true, kLoadA = true, kScaled = true;
  using block = u32x4;
  const u32x4* w;
  const float* scale;
  static __device__ __forceinline__ const u32x4* lane_base(
      const u32x4* w, int nt, long long K, int lane) {
    return w + ((long long)nt * (K >> 6)) * 64 +
           (long long)((lane & 15) * 4 + (lane >> 4));
  }
  static __device__ __forceinline__ long long block_off(long long kb) {
    return kb * 64;
  }
  template <bool NT>
  static __device__ __forceinline__ block load(const u32x4* blk) {
    return qsa_load16<NT>(blk);
  }
  static __device__ __forceinline__ void frags(const block& b, bf16x8& w0,
                                               bf16x8& w1) {
    w0 = fp8x8_to_bf16x8(b.x, b.y);   // k .. +32
    w1 = fp8x8_to_bf16x8(b.z, b.w);   // +32 .. +64
  }
};

// bf16 "fragment-major" [N/16, K/32, 16, 32]: a lane's 16 B at element
// (lane&15)*32 + (lane>>4)*8 of the 512-element block (nt, kk = 2*kb + half)
// are one B fragment -- two loads per lane per 64 k.  Packed by
// pack_weight_frag.  VARIANT is the ablation of tools/kernel_bench.py:
// 1 = W stream + MFMA only (no A loads), 2 = A loads + MFMA only.
template <int VARIANT>
struct qsa_bf16_stream {
  static constexpr bool kLoadW = VARIANT != 2, kLoadA = VARIANT != 1,
                        kScaled = false;
  struct block { bf16x8 lo, hi; };
  const unsigned short* w;
  static __device__ __forceinline__ const unsigned short* lane_base(
      const unsigned short* w, int nt, long long K, int lane) {
    return w + (long long)nt * (K >> 5) * 512 +
           (long long)((lane & 15) * 32 + (lane >> 4) * 8);
  }
  static __device__ __forceinline__ long long block_off(long long kb) {
    return kb * 1024;
  }
  template <bool NT>
  static __device__ __forceinline__ block load(const unsigned short* blk) {
    const bf16x8* p = reinterpret_cast<const bf16x8*>(blk);
    return {qsa_load16<NT>(p), qsa_load16<NT>(p + 64)};
  }
  static __device__ __forceinline__ void frags(const block& b, bf16x8& w0,
                                               bf16x8& w1) {
    w0 = b.lo;
    w1 = b.hi;
  }
};

// ---- activations and the store ---------------------------------------------

// Base of activation row `row`.  Out-of-batch rows CLAMP to
// row M-1 and load garbage that is never stored (per-row MFMA outputs are
// independent; the store is guarded).  A conditional `ok ? load : zero` here
// would be the guide's .s-level trap (c): hipcc branches around each load
// and drains vmcnt(0) per element -- measured 1.5-2.5x on the skinny kernel.
__device__ __forceinline__ const unsigned short* qsa_a_row(
    const unsigned short* A, int row, int M, long long lda) {
  return A + (long long)min(row, M - 1) * lda;
}

// The one rounding of an output: f32 -> bf16, nearest-even, rows < M only.
__device__ __forceinline__ void qsa_store_c(unsigned short* Cbf, int row,
                                            int ncol, int M, int N, float v) {
  if (row < M) Cbf[(long long)row * N + ncol] = f32_to_bf16(v);
}

// ---- the skinny kernel body -------------------------------------------------
// One workgroup per TILES 16-column n-tiles; WAVES waves SPLIT K inside the
// workgroup (wave w takes the 256-k chunks w, w + WAVES, ...), partial
// accumulators meet in LDS, wave 0 reduces, scales and stores.  No global
// split-K, no atomics, no epilogue kernel.
//
// A (M x K, <= 1 MB, L2-resident: every workgroup re-reads it) loads
// fragment-shaped straight to VGPRs, once per k-block for all TILES MFMA
// streams; MT 16-row m-tiles multiply only the A fragments and the
// accumulators.  The weight stream, its layout and the dequantisation are
// shared by all m-tiles.
//
// One output element accumulates over K in an order fixed by WAVES alone
// (chunks wave, wave + WAVES, ... in sequence, k ascending in 32-k MFMA steps
// inside a chunk, then the waves from 0.f in index order), and an MFMA output
// row depends on its own A row only -- so for a given WAVES a row's output
// bits do not depend on the stream's format, MT, TILES or the other rows.
template <class Stream, int WAVES, int TILES, bool NT, int MT>
__device__ __forceinline__ void qsa_skinny_body(
    const unsigned short* __restrict__ A, const Stream W,
    unsigned short* __restrict__ Cbf, int M, int N, long long K,
    long long lda) {
  const int nt0 = blockIdx.x * TILES;     // first 16-col n-tile
  const int wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const long long kchunks = K / QSA_KCH;  // K % 256 == 0

  f32x4 acc[MT][TILES];
#pragma unroll
  for (int m = 0; m < MT; ++m) {
#pragma unroll
    for (int t = 0; t < TILES; ++t) acc[m][t] = {0.f, 0.f, 0.f, 0.f};
  }

  const unsigned short* abase[MT];
#pragma unroll
  for (int m = 0; m < MT; ++m)
    abase[m] = qsa_a_row(A, 16 * m + (lane & 15), M, lda) + (lane >> 4) * 8;

  decltype(W.w) wbase[TILES];
#pragma unroll
  for (int t = 0; t < TILES; ++t)
    wbase[t] = Stream::lane_base(W.w, nt0 + t, K, lane);

  const bf16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
  for (long long c = wave; c < kchunks; c += WAVES) {
    const long long k0 = c * QSA_KCH;
#pragma unroll
    for (int s = 0; s < 4; ++s) {     // 4 k-blocks x 64 k = 256 k
      const long long kb = (k0 >> 6) + s;
      typename Stream::block q[TILES];
      if (Stream::kLoadW) {
#pragma unroll
        for (int t = 0; t < TILES; ++t)
          q[t] = Stream::template load<NT>(wbase[t] + Stream::block_off(kb));
      }
      const long long ak = k0 + s * 64;
      bf16x8 a0[MT], a1[MT];
#pragma unroll
      for (int m = 0; m < MT; ++m) {
        a0[m] = a1[m] = zero8;
        if (Stream::kLoadA) {
          a0[m] = *reinterpret_cast<const bf16x8*>(abase[m] + ak);
          a1[m] = *reinterpret_cast<const bf16x8*>(abase[m] + ak + 32);
        }
      }
#pragma unroll
      for (int t = 0; t < TILES; ++t) {
        bf16x8 w0 = zero8, w1 = zero8;
        if (Stream::kLoadW) Stream::frags(q[t], w0, w1);
#pragma unroll
        for (int m = 0; m < MT; ++m)
          acc[m][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              a0[m], w0, acc[m][t], 0, 0, 0);
#pragma unroll
        for (int m = 0; m < MT; ++m)
          acc[m][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              a1[m], w1, acc[m][t], 0, 0, 0);
      }
    }
  }

  // ---- cross-wave K-reduction in LDS (+ per-channel scale) --------------
  __shared__ float red[WAVES][64][4 * MT];
#pragma unroll
  for (int t = 0; t < TILES; ++t) {
    if (t > 0) __syncthreads();   // reuse the LDS slab per tile
#pragma unroll
    for (int m = 0; m < MT; ++m) {
#pragma unroll
      for (int r = 0; r < 4; ++r) red[wave][lane][4 * m + r] = acc[m][t][r];
    }
    __syncthreads();
    if (wave == 0) {
      const int ncol = (nt0 + t) * 16 + (lane & 15);
      const int mrow = (lane >> 4) * 4;
      float s;
      if constexpr (Stream::kScaled) s = W.scale[ncol];
#pragma unroll
      for (int m = 0; m < MT; ++m) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float v = 0.f;
#pragma unroll
          for (int wv = 0; wv < WAVES; ++wv) v += red[wv][lane][4 * m + r];
          if constexpr (Stream::kScaled) v *= s;
          qsa_store_c(Cbf, 16 * m + mrow + r, ncol, M, N, v);
        }
      }
    }
  }
}
