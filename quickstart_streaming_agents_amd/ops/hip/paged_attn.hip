// Paged-attention DECODE for CDNA4 (gfx950) — the K4 hot op, on MFMA.
//
// Replaces the reference's managed-LLM call (ML_PREDICT 'llm_textgen_model',
// terraform/core/main.tf:461) with on-GPU batched decode attention over a
// paged KV cache resident in 288 GB HBM3E.
//
// Design (flash-decoding, one WAVE per (batch b, kv head, context split)):
//   - All R GQA query heads of a kv head compute TOGETHER on the matrix
//     cores: scores via mfma_f32_16x16x32_bf16 with A = K-tile
//     [16 pos x 32 k] and B = Q [32 k x 16 heads] (heads pad to 16), PV
//     via A = P [16 heads x 32 pos] (packed bf16, redistributed with 8
//     cross-lane shuffles) and B = V^T [32 pos x 16 dims].  A VALU
//     decode kernel pays ~16 VALU per 16 B of KV; this pays ~1 MFMA per
//     1 KiB plus the online-softmax tail.
//   - K cache layout [page, kvh, D/8, 64, 8] (d-major x8): the A-fragment
//     read (lane = pos x k-slice) is one fully coalesced 1 KiB wave load.
//   - V cache layout [page, kvh, D, 64] (TRANSPOSED, pos minor): the PV
//     B-fragment read (lane = dim x pos-slice) is also one coalesced 1 KiB
//     wave load.  Every KV byte is read exactly ONCE per (b, kvh) — the
//     per-head VALU design re-read it R times.
//   - Context splits fill the chip (grid = B*KVH*NS >= ~2k waves);
//     unnormalized partials (o, m, l) merge in qsa_attn_reduce.
//   - What the model runs is qsa_paged_attn_mfma_fused: this decomposition
//     and arithmetic, bit for bit, with RoPE and the KV append folded in,
//     the page's K/V fragment loads issued in batches one stage ahead of
//     the MFMAs that consume them, and the splits merged inside the
//     workgroup when NS <= 4.  qsa_rope_kv_append + qsa_paged_attn_mfma +
//     qsa_attn_reduce remain as its oracle (QSA_DECODE_V1=1 runs them).
//
// The online softmax runs per head-column in registers: column max/sum
// reduce with two shfl_xor hops (the 4 hi-lane groups of a column).
//
// Also in this file: the KV-cache writers (decode append, prefill scatter,
// and the fused prefill rope + scatter qsa_rope_kv_scatter) and the two
// varlen PREFILL attention kernels: qsa_paged_attn_prefill (one wave per
// 16 q rows x head, fragments from global memory; the bit-exactness oracle
// and the path for shapes the tiled kernel does not cover) and
// qsa_paged_attn_prefill_tiled (one workgroup per 32/64 q rows x 4 heads,
// K/V pages double-buffered in LDS; what LlamaModel prefill runs).
#include "common.h"

#define QSA_PAGE 64

using bf16x8_a = __attribute__((ext_vector_type(8))) short;
using f32x4_a = __attribute__((ext_vector_type(4))) float;
using u32x4_a = __attribute__((ext_vector_type(4))) unsigned int;

template <int D>
__global__ void __launch_bounds__(256)
qsa_paged_attn_mfma(const unsigned short* __restrict__ q,   // [B, QH, D]
                    const unsigned short* __restrict__ kc,  // [P, KVH, D/8, 64, 8]
                    const unsigned short* __restrict__ vc,  // [P, KVH, D, 64]
                    const int* __restrict__ block_table,    // [B, max_pages]
                    const int* __restrict__ seq_lens,       // [B]
                    float* __restrict__ part_o,              // [B, QH, NS, D]
                    float* __restrict__ part_ml,             // [B, QH, NS, 2]
                    float scale, int B, int QH, int KVH, int max_pages,
                    long long qstride, int NS) {
  constexpr int KSTEPS = D / 32;      // QK^T k-steps (4 for D=128)
  constexpr int DTILES = D / 16;      // PV d-tiles (8 for D=128)
  const int wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const int nsb = (NS + 3) / 4;       // split-blocks per (b, kvh)
  const int bk = blockIdx.x / nsb;
  const int split = (blockIdx.x % nsb) * 4 + wave;
  const int b = bk / KVH;
  const int kvh = bk % KVH;
  const int R = QH / KVH;
  if (split >= NS) return;

  const int seqlen = seq_lens[b];
  const int npages = (seqlen + QSA_PAGE - 1) / QSA_PAGE;
  const int chunk = (npages + NS - 1) / NS;
  const int p0 = split * chunk;
  const int p1 = min(npages, p0 + chunk);
  const int col = lane & 15;          // head col (scores) / dim col (PV)
  const int hi = lane >> 4;           // 4 hi-lane groups

  // every (head) slot writes its partial, real or empty
  float* pml_base = part_ml + (((long long)b * QH + kvh * R) * NS + split) * 2;
  if (seqlen <= 0 || p0 >= npages) {
    if (lane < R)
      *reinterpret_cast<float2*>(pml_base + (long long)lane * NS * 2) =
          make_float2(-3.0e38f, 0.f);
    return;
  }

  // ---- Q B-fragments: lane holds Q[head=col][k = ks*32 + hi*8 + e] ----
  const int qh_l = kvh * R + min(col, R - 1);   // clamp: pad heads compute
  const unsigned short* qrow = q + (long long)b * qstride + (long long)qh_l * D;
  bf16x8_a qf[KSTEPS];
#pragma unroll
  for (int ks = 0; ks < KSTEPS; ++ks)
    qf[ks] = *reinterpret_cast<const bf16x8_a*>(qrow + ks * 32 + hi * 8);

  float m = -3.0e38f, lsum = 0.f;
  f32x4_a o_acc[DTILES];
#pragma unroll
  for (int dt = 0; dt < DTILES; ++dt)
    o_acc[dt] = (f32x4_a){0.f, 0.f, 0.f, 0.f};

  const int* btab = block_table + (long long)b * max_pages;
  for (int pi = p0; pi < p1; ++pi) {
    const int page = btab[pi];
    const unsigned short* kbase =
        kc + ((((long long)page * KVH + kvh) * (D / 8)) * QSA_PAGE) * 8;
    const unsigned short* vbase =
        vc + (((long long)page * KVH + kvh) * D) * QSA_PAGE;
    const int nvalid = min(seqlen - pi * QSA_PAGE, QSA_PAGE);

    // ---- scores: 4 pos-tiles x KSTEPS MFMAs ---------------------------
    // A-frag: lane holds K[pos = pt*16 + col][k = ks*32 + hi*8 + e];
    // K layout element (pos, k) at ((k/8)*64 + pos)*8 + k%8 ->
    // 16 B at ((ks*4 + hi)*64 + pos)*8.
    f32x4_a sc[4];
#pragma unroll
    for (int pt = 0; pt < 4; ++pt) {
      f32x4_a acc = {0.f, 0.f, 0.f, 0.f};
      const int pos = pt * 16 + col;
#pragma unroll
      for (int ks = 0; ks < KSTEPS; ++ks) {
        const bf16x8_a kf = *reinterpret_cast<const bf16x8_a*>(
            kbase + (((long long)(ks * 4 + hi) * QSA_PAGE) + pos) * 8);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[ks], acc,
                                                      0, 0, 0);
      }
      sc[pt] = acc;
    }
    // scale + mask invalid positions; C layout: row pos = hi*4 + r,
    // col head = lane&15 -> lane's r-th value is position pt*16 + hi*4 + r
    float pagemax = -3.0e38f;
#pragma unroll
    for (int pt = 0; pt < 4; ++pt) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int pos = pt * 16 + hi * 4 + r;
        float v = (pos < nvalid) ? sc[pt][r] * scale : -3.0e38f;
        sc[pt][r] = v;
        pagemax = fmaxf(pagemax, v);
      }
    }
    // column (per-head) max across the 4 hi groups
    pagemax = fmaxf(pagemax, __shfl_xor(pagemax, 16, QSA_WAVE));
    pagemax = fmaxf(pagemax, __shfl_xor(pagemax, 32, QSA_WAVE));
    const float m_new = fmaxf(m, pagemax);
    float alpha = __expf(m - m_new);
    if (m <= -3.0e38f) alpha = 0.f;
    m = m_new;
    // o_acc element (dt, r) belongs to OUTPUT ROW hi*4 + r (the PV
    // C-layout), while alpha lives per score COLUMN (this lane's l&15):
    // fetch each row's own alpha from the lane holding that column —
    // using the lane's own alpha zeroes/mis-scales other rows' history
    // whenever per-row maxima diverge across pages
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float alpha_r = __shfl(alpha, hi * 4 + r, 16);
#pragma unroll
      for (int dt = 0; dt < DTILES; ++dt) o_acc[dt][r] *= alpha_r;
    }
    // P = exp(sc - m) (invalid -> 0), packed bf16x2 per tile quad
    unsigned int ppk[8];   // tile pt -> 2 uints (4 bf16 = quads r0..3)
    float psum = 0.f;
#pragma unroll
    for (int pt = 0; pt < 4; ++pt) {
      float p0f = 0.f, p1f = 0.f, p2f = 0.f, p3f = 0.f;
      if (sc[pt][0] > -1.0e38f) p0f = __expf(sc[pt][0] - m_new);
      if (sc[pt][1] > -1.0e38f) p1f = __expf(sc[pt][1] - m_new);
      if (sc[pt][2] > -1.0e38f) p2f = __expf(sc[pt][2] - m_new);
      if (sc[pt][3] > -1.0e38f) p3f = __expf(sc[pt][3] - m_new);
      psum += p0f + p1f + p2f + p3f;
      ppk[pt * 2] = f32x2_to_bf16x2(p0f, p1f);
      ppk[pt * 2 + 1] = f32x2_to_bf16x2(p2f, p3f);
    }
    psum += __shfl_xor(psum, 16, QSA_WAVE);
    psum += __shfl_xor(psum, 32, QSA_WAVE);
    lsum = lsum * alpha + psum;

    // ---- PV: two 32-pos halves ---------------------------------------
    // A-frag needs lane (head=col, hi) to hold P[head][pos = hi*8 + e]:
    // packed pairs come from source lanes (same col) with hi' = (2*hi)&3
    // and (2*hi+1)&3, tile = half*2 + (hi>>1).
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      // lane (col, hi) needs P[head=col][pos = half*32 + hi*8 + e]:
      // tile T = half*2 + (hi>>1), quads (hi&1)*2 and (hi&1)*2+1 — i.e.
      // source lanes (col, g) with g = (2*hi)&3 and (2*hi+1)&3.  __shfl
      // evaluates the value expression in EACH lane, so the register
      // index must be compile-time: shuffle both candidate tiles'
      // packed regs and select by hi (guide rule 20: runtime-indexed
      // arrays spill to scratch; and a runtime index would read the
      // SOURCE lane's differently-computed tile).
      const int src_a = col + (((2 * hi) & 3) << 4);
      const int src_b = col + (((2 * hi + 1) & 3) << 4);
      const int tA = half * 2;           // tile for hi 0,1
      const int tB = half * 2 + 1;       // tile for hi 2,3
      const unsigned int a0A = __shfl(ppk[tA * 2], src_a, QSA_WAVE);
      const unsigned int a1A = __shfl(ppk[tA * 2 + 1], src_a, QSA_WAVE);
      const unsigned int b0A = __shfl(ppk[tA * 2], src_b, QSA_WAVE);
      const unsigned int b1A = __shfl(ppk[tA * 2 + 1], src_b, QSA_WAVE);
      const unsigned int a0B = __shfl(ppk[tB * 2], src_a, QSA_WAVE);
      const unsigned int a1B = __shfl(ppk[tB * 2 + 1], src_a, QSA_WAVE);
      const unsigned int b0B = __shfl(ppk[tB * 2], src_b, QSA_WAVE);
      const unsigned int b1B = __shfl(ppk[tB * 2 + 1], src_b, QSA_WAVE);
      const bool lo = hi < 2;
      bf16x8_a pa;
      unsigned int* pa_u = reinterpret_cast<unsigned int*>(&pa);
      pa_u[0] = lo ? a0A : a0B;
      pa_u[1] = lo ? a1A : a1B;
      pa_u[2] = lo ? b0A : b0B;
      pa_u[3] = lo ? b1A : b1B;
#pragma unroll
      for (int dt = 0; dt < DTILES; ++dt) {
        // B-frag: lane holds V^T[pos = half*32 + hi*8 + e][d = dt*16+col]
        // = vc[.., d, pos]: 16 B at (d*64 + half*32 + hi*8)
        const bf16x8_a vf = *reinterpret_cast<const bf16x8_a*>(
            vbase + ((long long)(dt * 16 + col) * QSA_PAGE) + half * 32 +
            hi * 8);
        o_acc[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pa, vf,
                                                            o_acc[dt],
                                                            0, 0, 0);
      }
    }
  }

  // ---- store partials: O C-layout row = head = hi*4 + r, col = dim ----
  // lane (hi, col): holds O[head hi*4+r][d = dt*16 + col]
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int head = hi * 4 + r;
    if (head < R) {
      float* po = part_o +
          (((long long)b * QH + kvh * R + head) * NS + split) * D;
#pragma unroll
      for (int dt = 0; dt < DTILES; ++dt)
        po[dt * 16 + col] = o_acc[dt][r];
    }
  }
  if (lane < R)
    *reinterpret_cast<float2*>(pml_base + (long long)lane * NS * 2) =
        make_float2(m, lsum);
}

template <int D>
__global__ void __launch_bounds__(128)
qsa_attn_reduce(const float* __restrict__ part_o,   // [rows, NS, D]
                const float* __restrict__ part_ml,  // [rows, NS, 2]
                unsigned short* __restrict__ out,   // [rows, D]
                int NS) {
  const long long row = blockIdx.x;
  const int d = threadIdx.x;  // D threads
  const float* ml = part_ml + row * NS * 2;
  float M = -3.0e38f;
  for (int s = 0; s < NS; ++s)
    if (ml[2 * s + 1] > 0.f) M = fmaxf(M, ml[2 * s]);
  float L = 0.f, acc = 0.f;
  for (int s = 0; s < NS; ++s) {
    const float ls = ml[2 * s + 1];
    if (ls <= 0.f) continue;
    const float w = __expf(ml[2 * s] - M);
    L += w * ls;
    acc += w * part_o[(row * NS + s) * D + d];
  }
  const float v = (L > 0.f) ? acc / L : 0.f;
  out[row * D + d] = f32_to_bf16(v);
}

extern "C" void qsa_paged_attn_mfma_launch(
    const unsigned short* q, const unsigned short* kc,
    const unsigned short* vc, const int* block_table, const int* seq_lens,
    float* part_o, float* part_ml, unsigned short* out, float scale, int B,
    int QH, int KVH, int max_pages, int D, long long qstride, int NS,
    hipStream_t stream) {
  const int nsb = (NS + 3) / 4;
  dim3 grid(B * KVH * nsb);
  dim3 block(256);
  if (D == 128) {
    hipLaunchKernelGGL((qsa_paged_attn_mfma<128>), grid, block, 0, stream,
                       q, kc, vc, block_table, seq_lens, part_o, part_ml,
                       scale, B, QH, KVH, max_pages, qstride, NS);
    hipLaunchKernelGGL((qsa_attn_reduce<128>), dim3(B * QH), dim3(128), 0,
                       stream, part_o, part_ml, out, NS);
  } else if (D == 64) {
    hipLaunchKernelGGL((qsa_paged_attn_mfma<64>), grid, block, 0, stream,
                       q, kc, vc, block_table, seq_lens, part_o, part_ml,
                       scale, B, QH, KVH, max_pages, qstride, NS);
    hipLaunchKernelGGL((qsa_attn_reduce<64>), dim3(B * QH), dim3(64), 0,
                       stream, part_o, part_ml, out, NS);
  }
}

__device__ __forceinline__ float qsa_bperm_f(int byte_addr, float v) {
  return __builtin_bit_cast(
      float, __builtin_amdgcn_ds_bpermute(byte_addr, __builtin_bit_cast(int, v)));
}
__device__ __forceinline__ unsigned int qsa_bperm_u(int byte_addr,
                                                   unsigned int v) {
  return (unsigned int)__builtin_amdgcn_ds_bpermute(byte_addr, (int)v);
}

// One page of the fused decode loop.  PREFETCH is compile-time so that each
// instantiation is straight-line code: with a runtime "is there a next
// page" branch around the K loads the compiler's wait-count bookkeeping
// merges both paths and makes PV wait for the prefetched K as well.
template <int D, bool PREFETCH>
__device__ __forceinline__ void qsa_decode_page(
    const unsigned short* kc, const unsigned short* vc, const int* btab,
    int pi, int p1, int seqlen, int KVH, int kvh, int koff, int voff,
    int col, int hi, float scale, int& page, int& page_n,
    const bf16x8_a (&qf)[D / 32], bf16x8_a (&kfr)[4][D / 32],
    bf16x8_a (&vfr)[2][D / 16], f32x4_a (&o_acc)[D / 16], float& m,
    float& lsum) {
  constexpr int KSTEPS = D / 32;
  constexpr int DTILES = D / 16;
  // lane shuffles as bare ds_bpermute on byte addresses (lane * 4): the
  // same data movement as __shfl/__shfl_xor without their per-call range
  // check, which costs VALU work and registers in this loop
  const int lane4 = (hi * 16 + col) * 4;
  const int x16 = lane4 ^ 64, x32 = lane4 ^ 128;
  const int arow = hi * (16 + 4) * 4;              // lane hi*16 + hi*4 (+ r)
  const int asrc_a = (col + (((2 * hi) & 3) << 4)) * 4;
  const int asrc_b = (col + (((2 * hi + 1) & 3) << 4)) * 4;
  // ---- this page's V: in flight under the score MFMAs -----------------
  {
    // wave-uniform 64-bit base + 32-bit lane offset: one address VGPR
    const char* vbase = reinterpret_cast<const char*>(
        vc + (((long long)page * KVH + kvh) * D) * QSA_PAGE);
#pragma unroll
    for (int half = 0; half < 2; ++half)
#pragma unroll
      for (int dt = 0; dt < DTILES; ++dt)
        vfr[half][dt] = *reinterpret_cast<const bf16x8_a*>(
            vbase + (unsigned)(voff + (dt * 16 * QSA_PAGE + half * 32) * 2));
  }
  // keep the V loads ahead of the wait for K: left alone, the scheduler
  // sinks them below the first score MFMAs, i.e. behind K's latency
  __builtin_amdgcn_sched_barrier(0);
  const int nvalid = min(seqlen - pi * QSA_PAGE, QSA_PAGE);

  // ---- scores: 4 pos-tiles x KSTEPS MFMAs -----------------------------
  f32x4_a sc[4];
#pragma unroll
  for (int pt = 0; pt < 4; ++pt) {
    f32x4_a acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < KSTEPS; ++ks)
      acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kfr[pt][ks], qf[ks],
                                                    acc, 0, 0, 0);
    sc[pt] = acc;
  }

  // ---- next page's K: in flight under softmax + PV --------------------
  if (PREFETCH) {
    page = page_n;
    page_n = btab[min(pi + 2, p1 - 1)];
    const char* kbase = reinterpret_cast<const char*>(
        kc + ((((long long)page * KVH + kvh) * (D / 8)) * QSA_PAGE) * 8);
#pragma unroll
    for (int pt = 0; pt < 4; ++pt)
#pragma unroll
      for (int ks = 0; ks < KSTEPS; ++ks)
        kfr[pt][ks] = *reinterpret_cast<const bf16x8_a*>(
            kbase + (unsigned)(koff + (ks * 4 * QSA_PAGE + pt * 16) * 16));
  }

  // ---- online softmax (qsa_paged_attn_mfma's, verbatim) ---------------
  float pagemax = -3.0e38f;
#pragma unroll
  for (int pt = 0; pt < 4; ++pt) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int kpos = pt * 16 + hi * 4 + r;
      float v = (kpos < nvalid) ? sc[pt][r] * scale : -3.0e38f;
      sc[pt][r] = v;
      pagemax = fmaxf(pagemax, v);
    }
  }
  pagemax = fmaxf(pagemax, qsa_bperm_f(x16, pagemax));
  pagemax = fmaxf(pagemax, qsa_bperm_f(x32, pagemax));
  const float m_new = fmaxf(m, pagemax);
  float alpha = __expf(m - m_new);
  if (m <= -3.0e38f) alpha = 0.f;
  m = m_new;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const float alpha_r = qsa_bperm_f(arow + r * 4, alpha);
#pragma unroll
    for (int dt = 0; dt < DTILES; ++dt) o_acc[dt][r] *= alpha_r;
  }
  unsigned int ppk[8];
  float psum = 0.f;
#pragma unroll
  for (int pt = 0; pt < 4; ++pt) {
    float p0f = 0.f, p1f = 0.f, p2f = 0.f, p3f = 0.f;
    if (sc[pt][0] > -1.0e38f) p0f = __expf(sc[pt][0] - m_new);
    if (sc[pt][1] > -1.0e38f) p1f = __expf(sc[pt][1] - m_new);
    if (sc[pt][2] > -1.0e38f) p2f = __expf(sc[pt][2] - m_new);
    if (sc[pt][3] > -1.0e38f) p3f = __expf(sc[pt][3] - m_new);
    psum += p0f + p1f + p2f + p3f;
    ppk[pt * 2] = f32x2_to_bf16x2(p0f, p1f);
    ppk[pt * 2 + 1] = f32x2_to_bf16x2(p2f, p3f);
  }
  psum += qsa_bperm_f(x16, psum);
  psum += qsa_bperm_f(x32, psum);
  lsum = lsum * alpha + psum;

  // ---- PV: two 32-pos halves (P repack as qsa_paged_attn_mfma) --------
#pragma unroll
  for (int half = 0; half < 2; ++half) {
    const int tA = half * 2;
    const int tB = half * 2 + 1;
    const unsigned int a0A = qsa_bperm_u(asrc_a, ppk[tA * 2]);
    const unsigned int a1A = qsa_bperm_u(asrc_a, ppk[tA * 2 + 1]);
    const unsigned int b0A = qsa_bperm_u(asrc_b, ppk[tA * 2]);
    const unsigned int b1A = qsa_bperm_u(asrc_b, ppk[tA * 2 + 1]);
    const unsigned int a0B = qsa_bperm_u(asrc_a, ppk[tB * 2]);
    const unsigned int a1B = qsa_bperm_u(asrc_a, ppk[tB * 2 + 1]);
    const unsigned int b0B = qsa_bperm_u(asrc_b, ppk[tB * 2]);
    const unsigned int b1B = qsa_bperm_u(asrc_b, ppk[tB * 2 + 1]);
    const bool lo = hi < 2;
    const u32x4_a pu = {lo ? a0A : a0B, lo ? a1A : a1B,
                        lo ? b0A : b0B, lo ? b1A : b1B};
    const bf16x8_a pa = __builtin_bit_cast(bf16x8_a, pu);
#pragma unroll
    for (int dt = 0; dt < DTILES; ++dt)
      o_acc[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
          pa, vfr[half][dt], o_acc[dt], 0, 0, 0);
  }
}

// ---------------------------------------------------------------------------
// FUSED decode step: RoPE + KV append + pipelined flash-decode + split merge
// in ONE launch (what LlamaModel.forward_decode runs).  Bit-identical to
// qsa_rope_kv_append -> qsa_paged_attn_mfma -> qsa_attn_reduce: the same
// wave/split/page decomposition, MFMA order, online softmax and P repack;
// only WHEN loads are issued and WHERE the partials meet changes.
//
//   RoPE     q arrives un-rotated.  A lane's Q fragments hold
//            k = ks*32 + hi*8 + e, whose rotation partner k +- D/2 is
//            fragment ks ^ (KSTEPS/2) of the SAME lane: rotated in registers
//            with qsa_rope_kv_append's expressions, never written back.
//   append   the one wave whose split owns page (seq_len-1)/64 rotates the
//            new k row, stores it and v into the cache, and makes the
//            stores visible (workgroup fence) BEFORE it issues any K/V load
//            of that page; no other wave of the grid reads that page.
//   loop     a page's 16 K fragments load back to back into kfr[][], its 16
//            V fragments into vfr[][] at the top of the iteration, and the
//            NEXT page's K loads issue right after the score MFMAs, so
//            softmax + PV run under 16 KiB of K in flight and the scores run
//            under 16 KiB of V.  Block-table entries are scalar loads
//            issued one page before the address that needs them, so no
//            address waits on a table load and the vector-memory counter
//            only ever counts K/V fragments.  Prefetch never goes through
//            an entry past p1-1.
//   merge    NS <= 4: all splits of (b, kvh) are waves of this workgroup.
//            (m, l, o) meet in LDS and every thread evaluates
//            qsa_attn_reduce's formula in its order; bf16 out is written
//            directly.  NS > 4: fp32 partials + qsa_attn_reduce as before.
// WPE = waves per SIMD the register budget is held to (1: <= 512 unified
// registers, 2: <= 256).
// ---------------------------------------------------------------------------
template <int D, int WPE>
__global__ void __launch_bounds__(256, WPE)
qsa_paged_attn_mfma_fused(
    const unsigned short* __restrict__ q,     // [B, QH, D] strided, UN-rotated
    const unsigned short* __restrict__ knew,  // [B, KVH, D] strided
    const unsigned short* __restrict__ vnew,  // [B, KVH, D] strided
    unsigned short* kc,                       // [P, KVH, D/8, 64, 8]
    unsigned short* vc,                       // [P, KVH, D, 64]
    const float* __restrict__ cos_t, const float* __restrict__ sin_t,
    const int* __restrict__ block_table,      // [B, max_pages]
    const int* __restrict__ seq_lens,         // [B]
    float* __restrict__ part_o,               // [B, QH, NS, D]   (NS > 4)
    float* __restrict__ part_ml,              // [B, QH, NS, 2]   (NS > 4)
    unsigned short* __restrict__ out,         // [B, QH, D]       (NS <= 4)
    float scale, int B, int QH, int KVH, int max_pages, long long qstride,
    long long kvstride, int NS) {
  constexpr int KSTEPS = D / 32;
  constexpr int DTILES = D / 16;
  constexpr int HALF = D / 2;
  constexpr int KH = KSTEPS / 2;      // fragment distance of a RoPE partner
  constexpr int OP = D + 4;           // LDS pitch of one head's o row (floats)
  // [4 splits][16 heads][OP] o, then [4][16][2] (m, l)
  __shared__ float4 lds4[(4 * 16 * OP + 4 * 16 * 2) / 4];
  float* lds_o = reinterpret_cast<float*>(lds4);
  float* lds_ml = lds_o + 4 * 16 * OP;

  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int nsb = (NS + 3) / 4;
  const int bk = blockIdx.x / nsb;
  const int split = (blockIdx.x % nsb) * 4 + wave;
  const int b = bk / KVH;
  const int kvh = bk % KVH;
  const int R = QH / KVH;
  const bool merge = NS <= 4;

  const int seqlen = seq_lens[b];
  const int npages = (seqlen + QSA_PAGE - 1) / QSA_PAGE;
  const int chunk = (npages + NS - 1) / NS;
  const int p0 = split * chunk;
  const int p1 = min(npages, p0 + chunk);
  const int col = lane & 15;
  const int hi = lane >> 4;
  const bool live = split < NS && seqlen > 0 && p0 < npages;

  float m = -3.0e38f, lsum = 0.f;
  f32x4_a o_acc[DTILES];
#pragma unroll
  for (int dt = 0; dt < DTILES; ++dt)
    o_acc[dt] = (f32x4_a){0.f, 0.f, 0.f, 0.f};

  if (live) {
    const int* btab = block_table + (long long)b * max_pages;
    const int pos = seqlen - 1;
    const float* cosr = cos_t + (long long)pos * HALF;
    const float* sinr = sin_t + (long long)pos * HALF;

    // ---- append: only the split that owns the last page -----------------
    if (p1 == npages) {
      const int page = btab[npages - 1];
      const int pin = pos % QSA_PAGE;
      if (lane < D / 16) {
        // 8 dims j*8.. and their +D/2 partners, as qsa_rope_kv_scatter
        const int j = lane;
        const unsigned short* base =
            knew + (long long)b * kvstride + (long long)kvh * D + j * 8;
        float c[8], s[8];
        *reinterpret_cast<float4*>(c) = *reinterpret_cast<const float4*>(cosr + j * 8);
        *reinterpret_cast<float4*>(c + 4) = *reinterpret_cast<const float4*>(cosr + j * 8 + 4);
        *reinterpret_cast<float4*>(s) = *reinterpret_cast<const float4*>(sinr + j * 8);
        *reinterpret_cast<float4*>(s + 4) = *reinterpret_cast<const float4*>(sinr + j * 8 + 4);
        uint4 a4 = *reinterpret_cast<const uint4*>(base);
        uint4 b4 = *reinterpret_cast<const uint4*>(base + HALF);
        unsigned int* au = reinterpret_cast<unsigned int*>(&a4);
        unsigned int* bu = reinterpret_cast<unsigned int*>(&b4);
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
        unsigned short* kdst = kc +
            (((((long long)page * KVH + kvh) * (D / 8) + j) * QSA_PAGE) + pin) * 8;
        *reinterpret_cast<uint4*>(kdst) = a4;
        *reinterpret_cast<uint4*>(kdst + (long long)(HALF / 8) * QSA_PAGE * 8) = b4;
      }
      const unsigned short* vrow =
          vnew + (long long)b * kvstride + (long long)kvh * D;
      unsigned short* vdst =
          vc + (((long long)page * KVH + kvh) * D) * QSA_PAGE + pin;
#pragma unroll
      for (int d = lane; d < D; d += QSA_WAVE)
        vdst[(long long)d * QSA_PAGE] = vrow[d];
      // the other lanes of this wave load these rows below
      __threadfence_block();
    }

    // ---- Q B-fragments, rotated in registers ------------------------------
    const int qh_l = kvh * R + min(col, R - 1);   // clamp: pad heads compute
    const unsigned short* qrow = q + (long long)b * qstride + (long long)qh_l * D;
    bf16x8_a qf[KSTEPS];
#pragma unroll
    for (int ks = 0; ks < KSTEPS; ++ks)
      qf[ks] = *reinterpret_cast<const bf16x8_a*>(qrow + ks * 32 + hi * 8);
#pragma unroll
    for (int ks = 0; ks < KH; ++ks) {
      float c[8], s[8];
      const int o = ks * 32 + hi * 8;
      *reinterpret_cast<float4*>(c) = *reinterpret_cast<const float4*>(cosr + o);
      *reinterpret_cast<float4*>(c + 4) = *reinterpret_cast<const float4*>(cosr + o + 4);
      *reinterpret_cast<float4*>(s) = *reinterpret_cast<const float4*>(sinr + o);
      *reinterpret_cast<float4*>(s + 4) = *reinterpret_cast<const float4*>(sinr + o + 4);
      u32x4_a au = __builtin_bit_cast(u32x4_a, qf[ks]);
      u32x4_a bu = __builtin_bit_cast(u32x4_a, qf[ks + KH]);
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
      qf[ks] = __builtin_bit_cast(bf16x8_a, au);
      qf[ks + KH] = __builtin_bit_cast(bf16x8_a, bu);
    }

    // ---- block-table entries: wave-uniform scalar loads, read one page
    // ahead of their use and never past entry p1-1 --------------------------
    int page = btab[p0];
    int page_n = btab[min(p0 + 1, p1 - 1)];

    // lane's fragment offsets inside a (page, kv head) block, in bytes
    const int koff = (hi * QSA_PAGE + col) * 16;      // + (ks*4*64 + pt*16)*16
    const int voff = (col * QSA_PAGE + hi * 8) * 2;   // + (dt*16*64 + half*32)*2
    bf16x8_a kfr[4][KSTEPS];
    bf16x8_a vfr[2][DTILES];
    {
      const char* kbase = reinterpret_cast<const char*>(
          kc + ((((long long)page * KVH + kvh) * (D / 8)) * QSA_PAGE) * 8);
#pragma unroll
      for (int pt = 0; pt < 4; ++pt)
#pragma unroll
        for (int ks = 0; ks < KSTEPS; ++ks)
          kfr[pt][ks] = *reinterpret_cast<const bf16x8_a*>(
              kbase + (unsigned)(koff + (ks * 4 * QSA_PAGE + pt * 16) * 16));
    }

    // all pages but the last prefetch their successor's K
    for (int pi = p0; pi < p1 - 1; ++pi)
      qsa_decode_page<D, true>(kc, vc, btab, pi, p1, seqlen, KVH, kvh, koff,
                               voff, col, hi, scale, page, page_n, qf, kfr,
                               vfr, o_acc, m, lsum);
    qsa_decode_page<D, false>(kc, vc, btab, p1 - 1, p1, seqlen, KVH, kvh,
                              koff, voff, col, hi, scale, page, page_n, qf,
                              kfr, vfr, o_acc, m, lsum);
  }

  if (!merge) {
    // ---- NS > 4: fp32 partials for qsa_attn_reduce -------------------------
    if (split >= NS) return;
    float* pml_base =
        part_ml + (((long long)b * QH + kvh * R) * NS + split) * 2;
    if (live) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int head = hi * 4 + r;
        if (head < R) {
          float* po = part_o +
              (((long long)b * QH + kvh * R + head) * NS + split) * D;
#pragma unroll
          for (int dt = 0; dt < DTILES; ++dt)
            po[dt * 16 + col] = o_acc[dt][r];
        }
      }
    }
    if (lane < R)
      *reinterpret_cast<float2*>(pml_base + (long long)lane * NS * 2) =
          make_float2(m, lsum);
    return;
  }

  // ---- NS <= 4: the splits are this workgroup's waves; merge through LDS --
  if (split < NS) {
    if (live) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int head = hi * 4 + r;
        if (head < R) {
          float* po = lds_o + (wave * 16 + head) * OP;
#pragma unroll
          for (int dt = 0; dt < DTILES; ++dt)
            po[dt * 16 + col] = o_acc[dt][r];
        }
      }
    }
    if (lane < R)
      *reinterpret_cast<float2*>(lds_ml + (wave * 16 + lane) * 2) =
          make_float2(m, lsum);
  }
  __syncthreads();
  // qsa_attn_reduce's formula, in its order, per (head, d)
  for (int idx = threadIdx.x; idx < R * D; idx += 256) {
    const int head = idx / D;
    const int d = idx % D;
    float M = -3.0e38f;
    for (int s = 0; s < NS; ++s)
      if (lds_ml[(s * 16 + head) * 2 + 1] > 0.f)
        M = fmaxf(M, lds_ml[(s * 16 + head) * 2]);
    float L = 0.f, acc = 0.f;
    for (int s = 0; s < NS; ++s) {
      const float ls = lds_ml[(s * 16 + head) * 2 + 1];
      if (ls <= 0.f) continue;
      const float w = __expf(lds_ml[(s * 16 + head) * 2] - M);
      L += w * ls;
      acc += w * lds_o[(s * 16 + head) * OP + d];
    }
    const float v = (L > 0.f) ? acc / L : 0.f;
    out[((long long)b * QH + kvh * R + head) * D + d] = f32_to_bf16(v);
  }
}

// variant: waves per SIMD the kernel is compiled for (1 or 2)
extern "C" void qsa_paged_attn_mfma_fused_launch(
    const unsigned short* q, const unsigned short* knew,
    const unsigned short* vnew, unsigned short* kc, unsigned short* vc,
    const float* cos_t, const float* sin_t, const int* block_table,
    const int* seq_lens, float* part_o, float* part_ml, unsigned short* out,
    float scale, int B, int QH, int KVH, int max_pages, int D,
    long long qstride, long long kvstride, int NS, int variant,
    hipStream_t stream) {
  const int nsb = (NS + 3) / 4;
  dim3 grid(B * KVH * nsb);
  dim3 block(256);
#define QSA_FUSED_CASE(DD, WW)                                              \
  if (D == DD && variant == WW) {                                           \
    hipLaunchKernelGGL((qsa_paged_attn_mfma_fused<DD, WW>), grid, block, 0, \
                       stream, q, knew, vnew, kc, vc, cos_t, sin_t,         \
                       block_table, seq_lens, part_o, part_ml, out, scale,  \
                       B, QH, KVH, max_pages, qstride, kvstride, NS);       \
    if (NS > 4)                                                             \
      hipLaunchKernelGGL((qsa_attn_reduce<DD>), dim3(B * QH), dim3(DD), 0,  \
                         stream, part_o, part_ml, out, NS);                 \
    return;                                                                 \
  }
  QSA_FUSED_CASE(128, 1) QSA_FUSED_CASE(128, 2)
  QSA_FUSED_CASE(64, 1) QSA_FUSED_CASE(64, 2)
#undef QSA_FUSED_CASE
}

// ---------------------------------------------------------------------------
// KV-cache writers.  K layout [page, kvh, D/8, 64, 8]; V layout
// [page, kvh, D, 64] (transposed for the PV B-fragment stream).
// ---------------------------------------------------------------------------

// Fused decode-step RoPE + KV append: rotates q in place, rotates k and
// writes it (and v) STRAIGHT into the paged cache.
__global__ void
qsa_rope_kv_append(unsigned short* __restrict__ q,        // [B, QH, D]
                   const unsigned short* __restrict__ k,  // [B, KVH, D]
                   const unsigned short* __restrict__ v,  // [B, KVH, D]
                   unsigned short* __restrict__ kc, unsigned short* __restrict__ vc,
                   const float* __restrict__ cos_t, const float* __restrict__ sin_t,
                   const int* __restrict__ block_table,
                   const int* __restrict__ seq_lens,
                   int B, int QH, int KVH, int D, int max_pages,
                   long long qstride, long long kvstride) {
  const int nheads = QH + KVH;
  const int b = blockIdx.x / nheads;
  const int h = blockIdx.x % nheads;
  const int half = D / 2;
  const int d = threadIdx.x;
  const int pos = seq_lens[b] - 1;
  if (pos < 0) return;
  const long long toff = (long long)pos * half + (d % half);
  const float c = cos_t[toff], s = sin_t[toff];
  if (h < QH) {
    if (d >= half) return;
    unsigned short* base = q + (long long)b * qstride + (long long)h * D;
    const float x0 = bf16_to_f32(base[d]);
    const float x1 = bf16_to_f32(base[d + half]);
    base[d] = f32_to_bf16(x0 * c - x1 * s);
    base[d + half] = f32_to_bf16(x0 * s + x1 * c);
    return;
  }
  if (d >= D) return;
  const int kvh = h - QH;
  const int page = block_table[(long long)b * max_pages + pos / QSA_PAGE];
  const int pin = pos % QSA_PAGE;
  const unsigned short* kbase =
      k + (long long)b * kvstride + (long long)kvh * D;
  const int dl = d % half;
  const float x0 = bf16_to_f32(kbase[dl]);
  const float x1 = bf16_to_f32(kbase[dl + half]);
  const float kr = (d < half) ? (x0 * c - x1 * s) : (x0 * s + x1 * c);
  kc[((((long long)page * KVH + kvh) * (D / 8) + d / 8) * QSA_PAGE + pin) * 8 +
     d % 8] = f32_to_bf16(kr);
  vc[(((long long)page * KVH + kvh) * D + d) * QSA_PAGE + pin] =
      v[(long long)b * kvstride + (long long)kvh * D + d];
}

extern "C" void qsa_rope_kv_append_launch(
    unsigned short* q, const unsigned short* k, const unsigned short* v,
    unsigned short* kc, unsigned short* vc, const float* cos_t,
    const float* sin_t, const int* block_table, const int* seq_lens, int B,
    int QH, int KVH, int D, int max_pages, long long qstride,
    long long kvstride, hipStream_t stream) {
  hipLaunchKernelGGL(qsa_rope_kv_append, dim3(B * (QH + KVH)), dim3(D), 0,
                     stream, q, k, v, kc, vc, cos_t, sin_t, block_table,
                     seq_lens, B, QH, KVH, D, max_pages, qstride, kvstride);
}

// Un-fused single-step append (numerics tests / CPU-parity surface).
__global__ void
qsa_kv_append(const unsigned short* __restrict__ knew,  // [B, KVH, D]
              const unsigned short* __restrict__ vnew,
              unsigned short* __restrict__ kc, unsigned short* __restrict__ vc,
              const int* __restrict__ block_table, const int* __restrict__ seq_lens,
              int B, int KVH, int D, int max_pages, long long kvstride) {
  const int b = blockIdx.x / KVH;
  const int kvh = blockIdx.x % KVH;
  const int d = threadIdx.x;
  if (d >= D) return;
  const int pos = seq_lens[b] - 1;
  if (pos < 0) return;
  const int page = block_table[(long long)b * max_pages + pos / QSA_PAGE];
  const int pin = pos % QSA_PAGE;
  const unsigned short kv = knew[(long long)b * kvstride + (long long)kvh * D + d];
  const unsigned short vv = vnew[(long long)b * kvstride + (long long)kvh * D + d];
  kc[((((long long)page * KVH + kvh) * (D / 8) + d / 8) * QSA_PAGE + pin) * 8 +
     d % 8] = kv;
  vc[(((long long)page * KVH + kvh) * D + d) * QSA_PAGE + pin] = vv;
}

// Prefill bulk scatter: T tokens' k/v by precomputed slot ids
// (slot = page*64 + offset).  The V^T write is a 2-byte-per-thread scatter;
// consecutive tokens of a page share cache lines per d, so L2 absorbs it.
__global__ void
qsa_kv_scatter(const unsigned short* __restrict__ knew,  // [T, KVH, D] (row stride kvstride)
               const unsigned short* __restrict__ vnew,
               unsigned short* __restrict__ kc, unsigned short* __restrict__ vc,
               const int* __restrict__ slots,  // [T]
               int T, int KVH, int D, long long kvstride) {
  const long long t = blockIdx.x / KVH;
  const int kvh = blockIdx.x % KVH;
  const int d = threadIdx.x;
  if (t >= T || d >= D) return;
  const int slot = slots[t];
  const long long page = slot / QSA_PAGE;
  const int pin = slot % QSA_PAGE;
  const unsigned short kv = knew[t * kvstride + (long long)kvh * D + d];
  const unsigned short vv = vnew[t * kvstride + (long long)kvh * D + d];
  kc[(((page * KVH + kvh) * (D / 8) + d / 8) * QSA_PAGE + pin) * 8 + d % 8] = kv;
  vc[((page * KVH + kvh) * D + d) * QSA_PAGE + pin] = vv;
}

extern "C" void qsa_kv_append_launch(const unsigned short* knew,
                                     const unsigned short* vnew,
                                     unsigned short* kc, unsigned short* vc,
                                     const int* block_table,
                                     const int* seq_lens, int B, int KVH,
                                     int D, int max_pages, long long kvstride,
                                     hipStream_t stream) {
  hipLaunchKernelGGL(qsa_kv_append, dim3(B * KVH), dim3(D), 0, stream, knew,
                     vnew, kc, vc, block_table, seq_lens, B, KVH, D, max_pages,
                     kvstride);
}

extern "C" void qsa_kv_scatter_launch(const unsigned short* knew,
                                      const unsigned short* vnew,
                                      unsigned short* kc, unsigned short* vc,
                                      const int* slots, int T, int KVH, int D,
                                      long long kvstride, hipStream_t stream) {
  hipLaunchKernelGGL(qsa_kv_scatter, dim3((long long)T * KVH), dim3(D), 0,
                     stream, knew, vnew, kc, vc, slots, T, KVH, D, kvstride);
}

// ---------------------------------------------------------------------------
// Varlen flash PREFILL attention over the paged cache (K4 prefill path).
//
// One WAVE per (16-row q-block, q head): streams the sequence's K/V pages
// directly from the paged cache (K [P,KVH,D/8,64,8], V^T [P,KVH,D,64] —
// the same coalesced MFMA fragment reads as the decode kernel), online
// softmax per q-row column, causal masking against the row's absolute
// position (cached prefix start + row).  No K/V gather, no padding, no
// materialized score matrix: each KV byte is read once per wave and the
// bmm+softmax+bmm chain collapses into one kernel per layer.
//
// Host passes per-q-block maps (item id, first q position) plus per-item
// row offset / cached start / new length and the padded page table.
//
// CAUSAL=false is the ENCODER path (K1, models/encoder.py): bidirectional
// attention over the full item — every row attends to every valid key —
// with the same varlen layout and paged K/V fragment reads.
// ---------------------------------------------------------------------------
template <int D, bool CAUSAL>
__global__ void __launch_bounds__(256)
qsa_paged_attn_prefill(const unsigned short* __restrict__ q,   // [T, QH, D] strided
                       const unsigned short* __restrict__ kc,
                       const unsigned short* __restrict__ vc,
                       const int* __restrict__ block_table,    // [nb, npmax]
                       const int* __restrict__ qb_item,        // [QB]
                       const int* __restrict__ qb_pos0,        // [QB]
                       const int* __restrict__ item_off,       // [nb] row offset
                       const int* __restrict__ item_start,     // [nb] cached
                       const int* __restrict__ item_len,       // [nb] new rows
                       unsigned short* __restrict__ out,       // [T, QH*D]
                       float scale, int QB, int QH, int KVH, int npmax,
                       long long qstride) {
  constexpr int KSTEPS = D / 32;
  constexpr int DTILES = D / 16;
  const int lane = threadIdx.x & 63;
  const int gw = blockIdx.x * 4 + (threadIdx.x >> 6);  // global wave id
  // the 4 waves of a workgroup are 4 consecutive heads of the SAME
  // q-block (and, at R>=4, the same kv head): they stream identical
  // K/V pages, so keeping them in lockstep (per-page barrier below)
  // turns 3 of the 4 streams into L1 hits
  const bool live = gw < QB * QH;
  const int gws = live ? gw : QB * QH - 1;   // dead waves shadow the last
  const int qb = gws / QH;
  const int qh = gws % QH;
  const int R = QH / KVH;
  const int kvh = qh / R;
  const int item = qb_item[qb];
  const int pos0 = qb_pos0[qb];          // first new-row index in the item
  const int n_i = item_len[item];
  const int start = item_start[item];
  const int off = item_off[item];
  const int col = lane & 15;             // q-row column in the score tiles
  const int hi = lane >> 4;

  // ---- Q B-fragments: lane holds Q[row pos0+col][k = ks*32 + hi*8+e] --
  const int qrow_l = min(pos0 + col, n_i - 1);   // clamp pad rows
  const unsigned short* qrow =
      q + (long long)(off + qrow_l) * qstride + (long long)qh * D;
  bf16x8_a qf[KSTEPS];
#pragma unroll
  for (int ks = 0; ks < KSTEPS; ++ks)
    qf[ks] = *reinterpret_cast<const bf16x8_a*>(qrow + ks * 32 + hi * 8);

  float m = -3.0e38f, lsum = 0.f;
  f32x4_a o_acc[DTILES];
#pragma unroll
  for (int dt = 0; dt < DTILES; ++dt)
    o_acc[dt] = (f32x4_a){0.f, 0.f, 0.f, 0.f};

  // attention horizon: causal -> the block's LAST row's position;
  // bidirectional -> the whole item
  const int max_abs = CAUSAL ? start + min(pos0 + 15, n_i - 1)
                             : start + n_i - 1;
  const int npages = (max_abs + QSA_PAGE) / QSA_PAGE;  // ceil(max_abs+1/64)
  const int* btab = block_table + (long long)item * npmax;

  for (int pi = 0; pi < npages; ++pi) {
    __syncthreads();   // lockstep the 4 head-waves on the shared page
    const int page = btab[pi];
    const unsigned short* kbase =
        kc + ((((long long)page * KVH + kvh) * (D / 8)) * QSA_PAGE) * 8;
    const unsigned short* vbase =
        vc + (((long long)page * KVH + kvh) * D) * QSA_PAGE;
    const int nvalid = min(max_abs + 1 - pi * QSA_PAGE, QSA_PAGE);

    f32x4_a sc[4];
#pragma unroll
    for (int pt = 0; pt < 4; ++pt) {
      f32x4_a acc = {0.f, 0.f, 0.f, 0.f};
      const int pos = pt * 16 + col;
#pragma unroll
      for (int ks = 0; ks < KSTEPS; ++ks) {
        const bf16x8_a kf = *reinterpret_cast<const bf16x8_a*>(
            kbase + (((long long)(ks * 4 + hi) * QSA_PAGE) + pos) * 8);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[ks], acc,
                                                      0, 0, 0);
      }
      sc[pt] = acc;
    }
    // mask: kpos (abs) must be <= start + qrow (abs) and < nvalid bound;
    // C layout row kpos = pt*16 + hi*4 + r, col = q-row
    const int qabs = start + pos0 + col;          // this column's row
    float pagemax = -3.0e38f;
#pragma unroll
    for (int pt = 0; pt < 4; ++pt) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int kpos = pt * 16 + hi * 4 + r;
        const int kabs = pi * QSA_PAGE + kpos;
        const bool ok = (kpos < nvalid) && (!CAUSAL || kabs <= qabs) &&
                        (pos0 + col < n_i);
        float v = ok ? sc[pt][r] * scale : -3.0e38f;
        sc[pt][r] = v;
        pagemax = fmaxf(pagemax, v);
      }
    }
    pagemax = fmaxf(pagemax, __shfl_xor(pagemax, 16, QSA_WAVE));
    pagemax = fmaxf(pagemax, __shfl_xor(pagemax, 32, QSA_WAVE));
    // skip only when EVERY column is masked: the skip must be
    // wave-uniform — MFMA reads all 64 lanes' source registers
    // regardless of EXEC, so divergence around the PV MFMAs corrupts
    // active lanes' products
    if (__all(pagemax <= -3.0e38f)) continue;
    const float m_new = fmaxf(m, pagemax);
    float alpha = __expf(m - m_new);
    if (m <= -3.0e38f) alpha = 0.f;
    m = m_new;
    // o_acc element (dt, r) belongs to OUTPUT ROW hi*4 + r (the PV
    // C-layout), while alpha lives per score COLUMN (this lane's l&15):
    // fetch each row's own alpha from the lane holding that column —
    // using the lane's own alpha zeroes/mis-scales other rows' history
    // whenever per-row maxima diverge across pages
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float alpha_r = __shfl(alpha, hi * 4 + r, 16);
#pragma unroll
      for (int dt = 0; dt < DTILES; ++dt) o_acc[dt][r] *= alpha_r;
    }
    unsigned int ppk[8];
    float psum = 0.f;
#pragma unroll
    for (int pt = 0; pt < 4; ++pt) {
      float p0f = 0.f, p1f = 0.f, p2f = 0.f, p3f = 0.f;
      if (sc[pt][0] > -1.0e38f) p0f = __expf(sc[pt][0] - m_new);
      if (sc[pt][1] > -1.0e38f) p1f = __expf(sc[pt][1] - m_new);
      if (sc[pt][2] > -1.0e38f) p2f = __expf(sc[pt][2] - m_new);
      if (sc[pt][3] > -1.0e38f) p3f = __expf(sc[pt][3] - m_new);
      psum += p0f + p1f + p2f + p3f;
      ppk[pt * 2] = f32x2_to_bf16x2(p0f, p1f);
      ppk[pt * 2 + 1] = f32x2_to_bf16x2(p2f, p3f);
    }
    psum += __shfl_xor(psum, 16, QSA_WAVE);
    psum += __shfl_xor(psum, 32, QSA_WAVE);
    lsum = lsum * alpha + psum;

#pragma unroll
    for (int half = 0; half < 2; ++half) {
      const int src_a = col + (((2 * hi) & 3) << 4);
      const int src_b = col + (((2 * hi + 1) & 3) << 4);
      const int tA = half * 2;
      const int tB = half * 2 + 1;
      const unsigned int a0A = __shfl(ppk[tA * 2], src_a, QSA_WAVE);
      const unsigned int a1A = __shfl(ppk[tA * 2 + 1], src_a, QSA_WAVE);
      const unsigned int b0A = __shfl(ppk[tA * 2], src_b, QSA_WAVE);
      const unsigned int b1A = __shfl(ppk[tA * 2 + 1], src_b, QSA_WAVE);
      const unsigned int a0B = __shfl(ppk[tB * 2], src_a, QSA_WAVE);
      const unsigned int a1B = __shfl(ppk[tB * 2 + 1], src_a, QSA_WAVE);
      const unsigned int b0B = __shfl(ppk[tB * 2], src_b, QSA_WAVE);
      const unsigned int b1B = __shfl(ppk[tB * 2 + 1], src_b, QSA_WAVE);
      const bool lo = hi < 2;
      bf16x8_a pa;
      unsigned int* pa_u = reinterpret_cast<unsigned int*>(&pa);
      pa_u[0] = lo ? a0A : a0B;
      pa_u[1] = lo ? a1A : a1B;
      pa_u[2] = lo ? b0A : b0B;
      pa_u[3] = lo ? b1A : b1B;
#pragma unroll
      for (int dt = 0; dt < DTILES; ++dt) {
        const bf16x8_a vf = *reinterpret_cast<const bf16x8_a*>(
            vbase + ((long long)(dt * 16 + col) * QSA_PAGE) + half * 32 +
            hi * 8);
        o_acc[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pa, vf,
                                                            o_acc[dt],
                                                            0, 0, 0);
      }
    }
  }

  // ---- epilogue: O C-layout row = q-row = hi*4 + r, col = dim ----------
  // per-row 1/l lives in the lanes of its COLUMN; fetch via shfl
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int qr = hi * 4 + r;               // q-row this lane holds
    const float lr = __shfl(lsum, qr, 16);   // lanes 0-15 hold cols 0-15
    const float inv = (lr > 0.f) ? 1.f / lr : 0.f;
    if (pos0 + qr < n_i) {
      unsigned short* orow =
          out + (long long)(off + pos0 + qr) * (QH * D) + (long long)qh * D;
#pragma unroll
      for (int dt = 0; dt < DTILES; ++dt)
        orow[dt * 16 + col] = f32_to_bf16(o_acc[dt][r] * inv);
    }
  }
}

extern "C" void qsa_paged_attn_prefill_launch(
    const unsigned short* q, const unsigned short* kc,
    const unsigned short* vc, const int* block_table, const int* qb_item,
    const int* qb_pos0, const int* item_off, const int* item_start,
    const int* item_len, unsigned short* out, float scale, int QB, int QH,
    int KVH, int npmax, int D, long long qstride, int causal,
    hipStream_t stream) {
  const long long waves = (long long)QB * QH;
  dim3 grid((unsigned)((waves + 3) / 4));
#define QSA_PREFILL_CASE(DD, CC)                                          \
  if (D == DD && causal == (int)CC) {                                     \
    hipLaunchKernelGGL((qsa_paged_attn_prefill<DD, CC>), grid, dim3(256), \
                       0, stream, q, kc, vc, block_table, qb_item,        \
                       qb_pos0, item_off, item_start, item_len, out,      \
                       scale, QB, QH, KVH, npmax, qstride);               \
    return;                                                               \
  }
  QSA_PREFILL_CASE(128, true) QSA_PREFILL_CASE(128, false)
  QSA_PREFILL_CASE(64, true) QSA_PREFILL_CASE(64, false)
#undef QSA_PREFILL_CASE
}

// ---------------------------------------------------------------------------
// TILED varlen flash prefill: the same arithmetic as qsa_paged_attn_prefill,
// row for row and bit for bit, with each K/V page fetched from global memory
// ONCE per workgroup and shared through LDS.
//
// Workgroup = 256 threads = one tile of ROWS q rows of one item x 4
// consecutive q heads (wave = head; at R % 4 == 0 all four share one kv
// head).  Each wave owns S = ROWS/16 sub-tiles of 16 rows: a K or V
// fragment is read from LDS once and feeds the MFMAs of all S sub-tiles,
// so the per-page fragment traffic drops from 4 x 32 KiB of global loads
// to one 32 KiB cooperative copy plus S-fold reuse of every ds_read_b128.
//
// Pipeline: the (page, kv head) K block and V^T block are each D*128 bytes
// contiguous in the cache.  All 256 threads copy page i+1 into registers
// (16 B per lane and load) before computing page i out of LDS buffer i&1,
// then write the registers into buffer (i+1)&1; ONE barrier per page
// separates "everyone finished reading buffer i&1 and writing the other"
// from the next iteration.  2 buffers x (K + V) = D*512 bytes: 64 KiB at
// D=128, two workgroups per CU.
//
// LDS images, in 16-byte slots (bank = slot mod 16 for ds_read_b128, lanes
// conflict only inside the instruction's four 16-lane groups, each of
// which holds 8 lanes of one hi value and 8 of the next, covering all 16
// col values exactly once):
//   K: copied LINEAR.  The A-fragment read takes slot (ks*4+hi)*64 +
//      pt*16 + col, i.e. slot mod 16 == col: the 16 lanes of a group hit 16
//      different slots -> conflict-free as stored, no padding needed.
//   V^T: row d holds 8 slots (128 B pitch); the B-fragment read takes slot
//      s = half*4 + hi of row d = dt*16 + col, so linear storage gives
//      slot mod 16 = (col&1)*8 + half*4 + hi: 4 distinct values per group,
//      a 4-way conflict.  Stored XOR-swizzled, slot s of row d lives at
//      d*8 + (s ^ ((d>>1)&7)).  Inside a group hi takes two adjacent values
//      {2g, 2g+1} on col sets whose (col>>1) values are {0,1,6,7} and
//      {2,3,4,5}; XOR with s maps them onto disjoint halves of 0..7, and
//      (col&1) picks the upper or lower 8 slots -> 16 distinct slots,
//      conflict-free.
//
// Bit-exactness against the one-wave-per-block kernel: a sub-tile keeps its
// own horizon (max_abs), processes exactly the pages the old kernel would
// (pi < its own page count, and the same wave-uniform "whole page masked"
// skip), and every accumulator sees the same MFMA/VALU sequence: the same
// ks order, mask, scale, __expf, alpha, psum order, P packing shuffles, PV
// order (half, then dt) and epilogue.
// ---------------------------------------------------------------------------
template <int D, bool CAUSAL, int ROWS>
__global__ void __launch_bounds__(256, ROWS == 32 ? 2 : 1)
qsa_paged_attn_prefill_tiled(
    const unsigned short* __restrict__ q,   // [T, QH, D] strided
    const unsigned short* __restrict__ kc,
    const unsigned short* __restrict__ vc,
    const int* __restrict__ block_table,    // [nb, npmax]
    const int* __restrict__ tile_item,      // [NT]
    const int* __restrict__ tile_pos0,      // [NT] first new-row of the tile
    const int* __restrict__ item_off,       // [nb] row offset
    const int* __restrict__ item_start,     // [nb] cached
    const int* __restrict__ item_len,       // [nb] new rows
    unsigned short* __restrict__ out,       // [T, QH*D]
    float scale, int NT, int QH, int KVH, int npmax, long long qstride) {
  constexpr int S = ROWS / 16;            // sub-tiles per wave
  constexpr int KSTEPS = D / 32;
  constexpr int DTILES = D / 16;
  constexpr int SLOTS = D * 8;            // 16-B slots per K (or V) page
  constexpr int LD = SLOTS / 256;         // slots per thread and image
  __shared__ u32x4_a lds[2][2][SLOTS];      // [buffer][K, V][slot]

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int HG = QH >> 2;                 // 4-head groups
  const int tile = blockIdx.x / HG;
  const int hg = blockIdx.x % HG;
  const int qh = hg * 4 + wave;
  const int R = QH / KVH;
  const int kvh = (hg * 4) / R;
  const int item = tile_item[tile];
  const int tpos0 = tile_pos0[tile];
  const int n_i = item_len[item];
  const int start = item_start[item];
  const int off = item_off[item];
  const int col = lane & 15;
  const int hi = lane >> 4;

  // ---- per-sub-tile state ------------------------------------------------
  bf16x8_a qf[S][KSTEPS];
  float m[S], lsum[S];
  f32x4_a o_acc[S][DTILES];
  int max_abs[S], npg[S];
#pragma unroll
  for (int s = 0; s < S; ++s) {
    const int pos0 = tpos0 + 16 * s;
    const int qrow_l = max(min(pos0 + col, n_i - 1), 0);   // clamp pad rows
    const unsigned short* qrow =
        q + (long long)(off + qrow_l) * qstride + (long long)qh * D;
#pragma unroll
    for (int ks = 0; ks < KSTEPS; ++ks)
      qf[s][ks] = *reinterpret_cast<const bf16x8_a*>(qrow + ks * 32 + hi * 8);
    m[s] = -3.0e38f;
    lsum[s] = 0.f;
#pragma unroll
    for (int dt = 0; dt < DTILES; ++dt)
      o_acc[s][dt] = (f32x4_a){0.f, 0.f, 0.f, 0.f};
    max_abs[s] = CAUSAL ? start + min(pos0 + 15, n_i - 1) : start + n_i - 1;
    // a sub-tile past the item's end has no rows: it walks no page
    npg[s] = (pos0 < n_i) ? (max_abs[s] + QSA_PAGE) / QSA_PAGE : 0;
  }
  // the workgroup walks pages up to its last live sub-tile's horizon
  const int wg_abs = CAUSAL ? start + min(tpos0 + ROWS - 1, n_i - 1)
                            : start + n_i - 1;
  const int np_wg = (tpos0 < n_i) ? (wg_abs + QSA_PAGE) / QSA_PAGE : 0;
  const int* btab = block_table + (long long)item * npmax;

  // page copy, 16 B per lane and load: global -> registers (QSA_FETCH),
  // registers -> LDS buffer (QSA_STASH; V^T slot swizzled, see above)
  u32x4_a kreg[LD], vreg[LD];
#define QSA_FETCH(PI)                                                      \
  {                                                                        \
    const long long pbase = ((long long)btab[PI] * KVH + kvh) * SLOTS;     \
    const u32x4_a* kp = reinterpret_cast<const u32x4_a*>(kc) + pbase;          \
    const u32x4_a* vp = reinterpret_cast<const u32x4_a*>(vc) + pbase;          \
    _Pragma("unroll") for (int i = 0; i < LD; ++i) {                       \
      kreg[i] = kp[tid + 256 * i];                                         \
      vreg[i] = vp[tid + 256 * i];                                         \
    }                                                                      \
  }
#define QSA_STASH(BUF)                                                     \
  {                                                                        \
    _Pragma("unroll") for (int i = 0; i < LD; ++i) {                       \
      const int g = tid + 256 * i;                                         \
      const int d = g >> 3;                                                \
      lds[BUF][0][g] = kreg[i];                                            \
      lds[BUF][1][d * 8 + ((g & 7) ^ ((d >> 1) & 7))] = vreg[i];           \
    }                                                                      \
  }

  if (np_wg > 0) {
    QSA_FETCH(0)
    QSA_STASH(0)
  }
  __syncthreads();

  const int vsw = (col >> 1) & 7;          // V^T swizzle of this lane's rows
  for (int pi = 0; pi < np_wg; ++pi) {
    const int buf = pi & 1;
    const bool more = pi + 1 < np_wg;
    if (more) QSA_FETCH(pi + 1)
    const u32x4_a* ldsK = lds[buf][0];
    const u32x4_a* ldsV = lds[buf][1];

    bool act[S];
#pragma unroll
    for (int s = 0; s < S; ++s) act[s] = pi < npg[s];

    // ---- scores: one K fragment read feeds all live sub-tiles ----------
    f32x4_a sc[S][4];
#pragma unroll
    for (int pt = 0; pt < 4; ++pt) {
#pragma unroll
      for (int s = 0; s < S; ++s) sc[s][pt] = (f32x4_a){0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < KSTEPS; ++ks) {
        const bf16x8_a kf = __builtin_bit_cast(
            bf16x8_a, ldsK[(ks * 4 + hi) * QSA_PAGE + pt * 16 + col]);
#pragma unroll
        for (int s = 0; s < S; ++s)
          if (act[s])
            sc[s][pt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                kf, qf[s][ks], sc[s][pt], 0, 0, 0);
      }
    }

    // ---- online softmax per sub-tile (lifted from the old kernel) -------
    bool pv[S];
    bf16x8_a pa[S][2];
#pragma unroll
    for (int s = 0; s < S; ++s) {
      pv[s] = false;
      if (!act[s]) continue;
      const int pos0 = tpos0 + 16 * s;
      const int nvalid = min(max_abs[s] + 1 - pi * QSA_PAGE, QSA_PAGE);
      const int qabs = start + pos0 + col;
      float pagemax = -3.0e38f;
#pragma unroll
      for (int pt = 0; pt < 4; ++pt) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int kpos = pt * 16 + hi * 4 + r;
          const int kabs = pi * QSA_PAGE + kpos;
          const bool ok = (kpos < nvalid) && (!CAUSAL || kabs <= qabs) &&
                          (pos0 + col < n_i);
          float v = ok ? sc[s][pt][r] * scale : -3.0e38f;
          sc[s][pt][r] = v;
          pagemax = fmaxf(pagemax, v);
        }
      }
      pagemax = fmaxf(pagemax, __shfl_xor(pagemax, 16, QSA_WAVE));
      pagemax = fmaxf(pagemax, __shfl_xor(pagemax, 32, QSA_WAVE));
      // wave-uniform skip of a page masked for EVERY column, as before
      if (__all(pagemax <= -3.0e38f)) continue;
      pv[s] = true;
      const float m_new = fmaxf(m[s], pagemax);
      float alpha = __expf(m[s] - m_new);
      if (m[s] <= -3.0e38f) alpha = 0.f;
      m[s] = m_new;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float alpha_r = __shfl(alpha, hi * 4 + r, 16);
#pragma unroll
        for (int dt = 0; dt < DTILES; ++dt) o_acc[s][dt][r] *= alpha_r;
      }
      unsigned int ppk[8];
      float psum = 0.f;
#pragma unroll
      for (int pt = 0; pt < 4; ++pt) {
        float p0f = 0.f, p1f = 0.f, p2f = 0.f, p3f = 0.f;
        if (sc[s][pt][0] > -1.0e38f) p0f = __expf(sc[s][pt][0] - m_new);
        if (sc[s][pt][1] > -1.0e38f) p1f = __expf(sc[s][pt][1] - m_new);
        if (sc[s][pt][2] > -1.0e38f) p2f = __expf(sc[s][pt][2] - m_new);
        if (sc[s][pt][3] > -1.0e38f) p3f = __expf(sc[s][pt][3] - m_new);
        psum += p0f + p1f + p2f + p3f;
        ppk[pt * 2] = f32x2_to_bf16x2(p0f, p1f);
        ppk[pt * 2 + 1] = f32x2_to_bf16x2(p2f, p3f);
      }
      psum += __shfl_xor(psum, 16, QSA_WAVE);
      psum += __shfl_xor(psum, 32, QSA_WAVE);
      lsum[s] = lsum[s] * alpha + psum;
#pragma unroll
      for (int half = 0; half < 2; ++half) {
        const int src_a = col + (((2 * hi) & 3) << 4);
        const int src_b = col + (((2 * hi + 1) & 3) << 4);
        const int tA = half * 2;
        const int tB = half * 2 + 1;
        const unsigned int a0A = __shfl(ppk[tA * 2], src_a, QSA_WAVE);
        const unsigned int a1A = __shfl(ppk[tA * 2 + 1], src_a, QSA_WAVE);
        const unsigned int b0A = __shfl(ppk[tA * 2], src_b, QSA_WAVE);
        const unsigned int b1A = __shfl(ppk[tA * 2 + 1], src_b, QSA_WAVE);
        const unsigned int a0B = __shfl(ppk[tB * 2], src_a, QSA_WAVE);
        const unsigned int a1B = __shfl(ppk[tB * 2 + 1], src_a, QSA_WAVE);
        const unsigned int b0B = __shfl(ppk[tB * 2], src_b, QSA_WAVE);
        const unsigned int b1B = __shfl(ppk[tB * 2 + 1], src_b, QSA_WAVE);
        const bool lo = hi < 2;
        const u32x4_a pu = {lo ? a0A : a0B, lo ? a1A : a1B,
                            lo ? b0A : b0B, lo ? b1A : b1B};
        pa[s][half] = __builtin_bit_cast(bf16x8_a, pu);
      }
    }

    // ---- PV: one V^T fragment read feeds all live sub-tiles -------------
#pragma unroll
    for (int half = 0; half < 2; ++half) {
#pragma unroll
      for (int dt = 0; dt < DTILES; ++dt) {
        const bf16x8_a vf = __builtin_bit_cast(
            bf16x8_a, ldsV[(dt * 16 + col) * 8 + ((half * 4 + hi) ^ vsw)]);
#pragma unroll
        for (int s = 0; s < S; ++s)
          if (pv[s])
            o_acc[s][dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                pa[s][half], vf, o_acc[s][dt], 0, 0, 0);
      }
    }

    if (more) QSA_STASH(buf ^ 1)
    __syncthreads();
  }

#undef QSA_FETCH
#undef QSA_STASH

  // ---- epilogue per sub-tile (as the old kernel) --------------------------
#pragma unroll
  for (int s = 0; s < S; ++s) {
    const int pos0 = tpos0 + 16 * s;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int qr = hi * 4 + r;
      const float lr = __shfl(lsum[s], qr, 16);
      const float inv = (lr > 0.f) ? 1.f / lr : 0.f;
      if (pos0 + qr < n_i) {
        unsigned short* orow = out +
            (long long)(off + pos0 + qr) * (QH * D) + (long long)qh * D;
#pragma unroll
        for (int dt = 0; dt < DTILES; ++dt)
          orow[dt * 16 + col] = f32_to_bf16(o_acc[s][dt][r] * inv);
      }
    }
  }
}

// rows: q rows per workgroup tile (32; 64 at D=64 only).  Returns 0 when the
// GQA ratio is not covered (the binding then runs the one-wave-per-block
// kernel).
extern "C" int qsa_paged_attn_prefill_tiled_launch(
    const unsigned short* q, const unsigned short* kc,
    const unsigned short* vc, const int* block_table, const int* tile_item,
    const int* tile_pos0, const int* item_off, const int* item_start,
    const int* item_len, unsigned short* out, float scale, int NT, int QH,
    int KVH, int npmax, int D, long long qstride, int causal, int rows,
    hipStream_t stream) {
  if (KVH <= 0 || QH % KVH != 0 || (QH / KVH) % 4 != 0) return 0;
  if (NT <= 0) return 1;
  dim3 grid((unsigned)((long long)NT * (QH / 4)));
#define QSA_TILED_CASE(DD, CC, RR)                                         \
  if (D == DD && causal == (int)CC && rows == RR) {                        \
    hipLaunchKernelGGL((qsa_paged_attn_prefill_tiled<DD, CC, RR>), grid,   \
                       dim3(256), 0, stream, q, kc, vc, block_table,       \
                       tile_item, tile_pos0, item_off, item_start,         \
                       item_len, out, scale, NT, QH, KVH, npmax, qstride); \
    return 1;                                                              \
  }
  // D=128 with 64 rows needs 4 x 32 accumulator + 64 Q + 64 score
  // registers per lane on top of the 32 staging registers and spills even
  // at one wave per SIMD, so it is not instantiated
  QSA_TILED_CASE(128, true, 32) QSA_TILED_CASE(128, false, 32)
  QSA_TILED_CASE(64, true, 32) QSA_TILED_CASE(64, false, 32)
  QSA_TILED_CASE(64, true, 64) QSA_TILED_CASE(64, false, 64)
#undef QSA_TILED_CASE
  return 0;
}

// ---------------------------------------------------------------------------
// Fused PREFILL RoPE + KV scatter (the prefill twin of qsa_rope_kv_append).
//
// One launch, two kinds of 256-thread block:
//   q blocks   rotate q in place over ALL rows passed (pad rows included).
//              A thread owns 8 consecutive dims and their +D/2 partners:
//              two 16-byte loads, two 16-byte stores, lanes along d.
//   kv blocks  take 64 consecutive tokens of one kv head.  k is rotated and
//              written ONLY to the cache (nothing reads rotated k from the
//              qkv buffer: prefill attention reads the cache).  In the K
//              layout [page, kvh, D/8, 64, 8] a token's 8 consecutive dims
//              are one 16-byte store, and lanes run along the tokens, so
//              consecutive slots give consecutive 16-byte stores.  v is
//              transposed through LDS and stored with lanes along the
//              tokens too: for a run of consecutive slots a wave writes one
//              contiguous run of the V^T row per d, where qsa_kv_scatter
//              wrote 64 different cache lines per wave store.  The stores
//              are per element and each goes through its own slot id, so
//              ANY slot pattern (page crossings, item boundaries,
//              permutations) is correct with no special case; only the
//              coalescing depends on the slots being consecutive.
// Rows >= T (pad rows) never touch the cache.  Rotation expressions are the
// ones of qsa_rope_kernel, so results are bit-identical to rope_inplace
// followed by kv_scatter.
// ---------------------------------------------------------------------------
#define QSA_RKS_TOK 64
template <int D>
__global__ void __launch_bounds__(256)
qsa_rope_kv_scatter(unsigned short* __restrict__ q,        // [Tq, QH, D]
                    const unsigned short* __restrict__ k,  // [>=T, KVH, D]
                    const unsigned short* __restrict__ v,
                    unsigned short* __restrict__ kc,
                    unsigned short* __restrict__ vc,
                    const float* __restrict__ cos_t,
                    const float* __restrict__ sin_t,
                    const int* __restrict__ pos,           // [Tq]
                    const int* __restrict__ slots,         // [T]
                    int Tq, int T, int QH, int KVH, int nqblocks,
                    long long qstride, long long kvstride) {
  constexpr int half = D / 2;
  constexpr int JD = D / 16;                // 8-dim groups per half
  constexpr int VP = D / 2 + 1;             // LDS row pitch in dwords (odd)
  __shared__ unsigned int vt[QSA_RKS_TOK * VP];
  const int tid = threadIdx.x;

  if ((int)blockIdx.x < nqblocks) {
    // ---- q: (token, head, j) units, j fastest ---------------------------
    const long long u = (long long)blockIdx.x * 256 + tid;
    const long long unit = u / JD;
    const int j = (int)(u % JD);
    const long long t = unit / QH;
    const int h = (int)(unit % QH);
    if (t >= Tq) return;
    unsigned short* base = q + t * qstride + (long long)h * D + j * 8;
    const long long toff = (long long)pos[t] * half + j * 8;
    float c[8], s[8];
    *reinterpret_cast<float4*>(c) = *reinterpret_cast<const float4*>(cos_t + toff);
    *reinterpret_cast<float4*>(c + 4) = *reinterpret_cast<const float4*>(cos_t + toff + 4);
    *reinterpret_cast<float4*>(s) = *reinterpret_cast<const float4*>(sin_t + toff);
    *reinterpret_cast<float4*>(s + 4) = *reinterpret_cast<const float4*>(sin_t + toff + 4);
    uint4 a = *reinterpret_cast<const uint4*>(base);
    uint4 b = *reinterpret_cast<const uint4*>(base + half);
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
    *reinterpret_cast<uint4*>(base) = a;
    *reinterpret_cast<uint4*>(base + half) = b;
    return;
  }

  // ---- k/v: 64 tokens of one kv head -------------------------------------
  const int kb = blockIdx.x - nqblocks;
  const int kvh = kb % KVH;
  const long long t0 = (long long)(kb / KVH) * QSA_RKS_TOK;
  const int nt = (int)min((long long)QSA_RKS_TOK, (long long)T - t0);

  // v rows -> LDS, 16-byte global loads with lanes along d
#pragma unroll
  for (int i = 0; i < QSA_RKS_TOK * (D / 8) / 256; ++i) {
    const int item = tid + 256 * i;
    const int tl = item / (D / 8);
    const int dg = item % (D / 8);
    if (tl < nt) {
      const uint4 x = *reinterpret_cast<const uint4*>(
          v + (t0 + tl) * kvstride + (long long)kvh * D + dg * 8);
      unsigned int* dst = vt + tl * VP + dg * 4;
      dst[0] = x.x; dst[1] = x.y; dst[2] = x.z; dst[3] = x.w;
    }
  }

  // k: rotate 8 dims + partners per thread, lanes along the tokens
#pragma unroll
  for (int i = 0; i < QSA_RKS_TOK * JD / 256; ++i) {
    const int item = tid + 256 * i;
    const int tl = item % QSA_RKS_TOK;
    const int j = item / QSA_RKS_TOK;
    if (tl < nt) {
      const long long t = t0 + tl;
      const unsigned short* base = k + t * kvstride + (long long)kvh * D + j * 8;
      const long long toff = (long long)pos[t] * half + j * 8;
      float c[8], s[8];
      *reinterpret_cast<float4*>(c) = *reinterpret_cast<const float4*>(cos_t + toff);
      *reinterpret_cast<float4*>(c + 4) = *reinterpret_cast<const float4*>(cos_t + toff + 4);
      *reinterpret_cast<float4*>(s) = *reinterpret_cast<const float4*>(sin_t + toff);
      *reinterpret_cast<float4*>(s + 4) = *reinterpret_cast<const float4*>(sin_t + toff + 4);
      uint4 a = *reinterpret_cast<const uint4*>(base);
      uint4 b = *reinterpret_cast<const uint4*>(base + half);
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
      const int slot = slots[t];
      const long long page = slot / QSA_PAGE;
      const int pin = slot % QSA_PAGE;
      unsigned short* kdst =
          kc + ((((page * KVH + kvh) * (D / 8) + j) * QSA_PAGE) + pin) * 8;
      *reinterpret_cast<uint4*>(kdst) = a;
      *reinterpret_cast<uint4*>(kdst + (long long)(half / 8) * QSA_PAGE * 8) = b;
    }
  }

  __syncthreads();

  // v: transposed store, lanes along the tokens
  const unsigned short* vt16 = reinterpret_cast<const unsigned short*>(vt);
  const int tl = tid % QSA_RKS_TOK;
  if (tl < nt) {
    const int slot = slots[t0 + tl];
    const long long page = slot / QSA_PAGE;
    const int pin = slot % QSA_PAGE;
    unsigned short* vdst = vc + ((page * KVH + kvh) * D) * QSA_PAGE + pin;
#pragma unroll 8
    for (int d = tid / QSA_RKS_TOK; d < D; d += 256 / QSA_RKS_TOK)
      vdst[(long long)d * QSA_PAGE] = vt16[tl * (VP * 2) + d];
  }
}

extern "C" void qsa_rope_kv_scatter_launch(
    unsigned short* q, const unsigned short* k, const unsigned short* v,
    unsigned short* kc, unsigned short* vc, const float* cos_t,
    const float* sin_t, const int* pos, const int* slots, int Tq, int T,
    int QH, int KVH, int D, long long qstride, long long kvstride,
    hipStream_t stream) {
  const long long qthreads = (long long)Tq * QH * (D / 16);
  const int nqblocks = (int)((qthreads + 255) / 256);
  const int nkvblocks = ((T + QSA_RKS_TOK - 1) / QSA_RKS_TOK) * KVH;
  if (nqblocks + nkvblocks == 0) return;
  dim3 grid(nqblocks + nkvblocks);
  if (D == 128)
    hipLaunchKernelGGL((qsa_rope_kv_scatter<128>), grid, dim3(256), 0, stream,
                       q, k, v, kc, vc, cos_t, sin_t, pos, slots, Tq, T, QH,
                       KVH, nqblocks, qstride, kvstride);
  else if (D == 64)
    hipLaunchKernelGGL((qsa_rope_kv_scatter<64>), grid, dim3(256), 0, stream,
                       q, k, v, kc, vc, cos_t, sin_t, pos, slots, Tq, T, QH,
                       KVH, nqblocks, qstride, kvstride);
}
