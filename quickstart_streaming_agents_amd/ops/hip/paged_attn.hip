// Paged attention for CDNA4 (gfx950) on MFMA — the K4 hot op: decode,
// prefill and the KV-cache writers over a paged KV cache in HBM3E.
//
// Replaces the reference's managed-LLM call (ML_PREDICT 'llm_textgen_model',
// terraform/core/main.tf:461) with on-GPU batched attention.
//
// Cache layouts:
//   K [page, kvh, D/8, 64, 8] (d-major x8): the score A-fragment read
//     (lane = pos x k-slice) is one fully coalesced 1 KiB wave load.
//   V [page, kvh, D, 64] (TRANSPOSED, pos minor): the PV B-fragment read
//     (lane = dim x pos-slice) is also one coalesced 1 KiB wave load.
//
// The arithmetic is written once, in attn_core.h: mask + scale, the column
// reduce, the online-softmax page update with its P repack, the score MFMAs
// over global K fragments, the partials store, the split merge, the prefill
// epilogue and the RoPE rotation.  Scores are mfma_f32_16x16x32_bf16 with
// A = K-tile [16 pos x 32 k] and B = Q [32 k x 16 columns]; PV has
// A = P [16 columns x 32 pos] (packed bf16) and B = V^T [32 pos x 16 dims].
// A score column is a GQA head in decode (all R heads of a kv head compute
// together, padded to 16, so every KV byte is read once per (b, kvh)) and a
// q row in prefill.  The kernels differ only in when loads are issued, where
// the K/V fragments come from and where the partials meet:
//   qsa_paged_attn_mfma  flash-decoding, one WAVE per (batch, kv head, context
//       split), fragments from global memory, fp32 partials merged by
//       qsa_attn_reduce.  With qsa_rope_kv_append, the oracle of the fused
//       kernel (QSA_DECODE_V1=1 runs them).
//   qsa_paged_attn_mfma_fused  what the model runs: the same decomposition
//       with RoPE and the KV append folded in, K/V fragment loads issued one
//       stage ahead of the MFMAs, splits merged in LDS when NS <= 4.
//   qsa_paged_attn_prefill  varlen prefill, one wave per 16 q rows x head,
//       fragments from global memory: the encoder's path, the oracle of the
//       tiled kernel and the path for shapes it does not cover.
//   qsa_paged_attn_prefill_tiled  one workgroup per 32/64 q rows x 4 heads,
//       K/V pages double-buffered in LDS; what LlamaModel prefill runs.
// Also here: the KV-cache writers (decode append, prefill scatter and the
// fused prefill rope + scatter qsa_rope_kv_scatter).
#include "attn_core.h"

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

  const int qh_l = kvh * R + min(col, R - 1);   // clamp: pad heads compute
  bf16x8_a qf[D / 32];
  qsa_load_q<D>(q + (long long)b * qstride + (long long)qh_l * D, hi, qf);

  const qsa_lanes L = qsa_lanes_of(col, hi);
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

    f32x4_a sc[4];
    qsa_scores_global<D>(kbase, qf, col, hi, sc);
    const float pagemax = qsa_col_reduce<true>(
        L, qsa_mask_scale<false>(sc, scale, hi, nvalid, 0, 0, true));
    bf16x8_a pa[2];
    qsa_page_update<DTILES>(L, sc, pagemax, m, lsum, o_acc, pa);

    // ---- PV: two 32-pos halves; B-frag: lane holds
    // V^T[pos = half*32 + hi*8 + e][d = dt*16 + col] = vc[.., d, pos]:
    // 16 B at (d*64 + half*32 + hi*8)
#pragma unroll
    for (int half = 0; half < 2; ++half) {
#pragma unroll
      for (int dt = 0; dt < DTILES; ++dt) {
        const bf16x8_a vf = *reinterpret_cast<const bf16x8_a*>(
            vbase + ((long long)(dt * 16 + col) * QSA_PAGE) + half * 32 +
            hi * 8);
        o_acc[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            pa[half], vf, o_acc[dt], 0, 0, 0);
      }
    }
  }

  qsa_store_partials<DTILES>(
      o_acc, m, lsum, true,
      part_o + (((long long)b * QH + kvh * R) * NS + split) * D, NS * D,
      pml_base, NS * 2, R, lane);
}

template <int D>
__global__ void __launch_bounds__(128)
qsa_attn_reduce(const float* __restrict__ part_o,   // [rows, NS, D]
                const float* __restrict__ part_ml,  // [rows, NS, 2]
                unsigned short* __restrict__ out,   // [rows, D]
                int NS) {
  const long long row = blockIdx.x;
  const int d = threadIdx.x;  // D threads
  const float v = qsa_merge_splits(NS, part_ml + row * NS * 2, 2,
                                   part_o + row * NS * D + d, D);
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

// One page of the fused decode loop.  PREFETCH is compile-time so that each
// instantiation is straight-line code: with a runtime "is there a next
// page" branch around the K loads the compiler's wait-count bookkeeping
// merges both paths and makes PV wait for the prefetched K as well.
template <int D, bool PREFETCH>
__device__ __forceinline__ void qsa_decode_page(
    const unsigned short* kc, const unsigned short* vc, const int* btab,
    int pi, int p1, int seqlen, int KVH, int kvh, int koff, int voff,
    const qsa_lanes& L, int hi, float scale, int& page, int& page_n,
    const bf16x8_a (&qf)[D / 32], bf16x8_a (&kfr)[4][D / 32],
    bf16x8_a (&vfr)[2][D / 16], f32x4_a (&o_acc)[D / 16], float& m,
    float& lsum) {
  constexpr int KSTEPS = D / 32;
  constexpr int DTILES = D / 16;
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

  const float pagemax = qsa_col_reduce<true>(
      L, qsa_mask_scale<false>(sc, scale, hi, nvalid, 0, 0, true));
  bf16x8_a pa[2];
  qsa_page_update<DTILES>(L, sc, pagemax, m, lsum, o_acc, pa);

  // ---- PV: two 32-pos halves ------------------------------------------
#pragma unroll
  for (int half = 0; half < 2; ++half)
#pragma unroll
    for (int dt = 0; dt < DTILES; ++dt)
      o_acc[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
          pa[half], vfr[half][dt], o_acc[dt], 0, 0, 0);
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
//            with qsa_rope8, never written back.
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
//            (m, l, o) meet in LDS and every thread merges one (head, d) with
//            qsa_merge_splits, as qsa_attn_reduce does; bf16 out is written
//            directly.  NS > 4: fp32 partials + qsa_attn_reduce.
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
        // 8 dims j*8.. and their +D/2 partners
        const int j = lane;
        const unsigned short* base =
            knew + (long long)b * kvstride + (long long)kvh * D + j * 8;
        uint4 a4 = *reinterpret_cast<const uint4*>(base);
        uint4 b4 = *reinterpret_cast<const uint4*>(base + HALF);
        qsa_rope8(a4, b4, cosr + j * 8, sinr + j * 8);
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
    bf16x8_a qf[KSTEPS];
    qsa_load_q<D>(q + (long long)b * qstride + (long long)qh_l * D, hi, qf);
#pragma unroll
    for (int ks = 0; ks < KH; ++ks) {
      uint4 a4 = __builtin_bit_cast(uint4, qf[ks]);
      uint4 b4 = __builtin_bit_cast(uint4, qf[ks + KH]);
      qsa_rope8(a4, b4, cosr + ks * 32 + hi * 8, sinr + ks * 32 + hi * 8);
      qf[ks] = __builtin_bit_cast(bf16x8_a, a4);
      qf[ks + KH] = __builtin_bit_cast(bf16x8_a, b4);
    }
    const qsa_lanes L = qsa_lanes_of(col, hi);

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
                               voff, L, hi, scale, page, page_n, qf, kfr,
                               vfr, o_acc, m, lsum);
    qsa_decode_page<D, false>(kc, vc, btab, p1 - 1, p1, seqlen, KVH, kvh,
                              koff, voff, L, hi, scale, page, page_n, qf,
                              kfr, vfr, o_acc, m, lsum);
  }

  // every split slot writes its (m, l), real or empty; o only when live
  if (!merge) {
    // ---- NS > 4: fp32 partials for qsa_attn_reduce -------------------------
    if (split < NS)
      qsa_store_partials<DTILES>(
          o_acc, m, lsum, live,
          part_o + (((long long)b * QH + kvh * R) * NS + split) * D, NS * D,
          part_ml + (((long long)b * QH + kvh * R) * NS + split) * 2, NS * 2,
          R, lane);
    return;
  }

  // ---- NS <= 4: the splits are this workgroup's waves; merge through LDS --
  if (split < NS)
    qsa_store_partials<DTILES>(o_acc, m, lsum, live, lds_o + wave * 16 * OP,
                               OP, lds_ml + wave * 16 * 2, 2, R, lane);
  __syncthreads();
  for (int idx = threadIdx.x; idx < R * D; idx += 256) {
    const int head = idx / D;
    const int d = idx % D;
    const float v = qsa_merge_splits(NS, lds_ml + head * 2, 16 * 2,
                                     lds_o + head * OP + d, 16 * OP);
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

  const int qrow_l = min(pos0 + col, n_i - 1);   // clamp pad rows
  bf16x8_a qf[D / 32];
  qsa_load_q<D>(q + (long long)(off + qrow_l) * qstride + (long long)qh * D,
                hi, qf);

  const qsa_lanes L = qsa_lanes_of(col, hi);

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
    qsa_scores_global<D>(kbase, qf, col, hi, sc);
    const float pagemax = qsa_col_reduce<true>(
        L, qsa_mask_scale<CAUSAL>(sc, scale, hi, nvalid, pi * QSA_PAGE,
                                  start + pos0 + col, pos0 + col < n_i));
    // skip only when EVERY column is masked: the skip must be
    // wave-uniform — MFMA reads all 64 lanes' source registers
    // regardless of EXEC, so divergence around the PV MFMAs corrupts
    // active lanes' products
    if (__all(pagemax <= -3.0e38f)) continue;
    bf16x8_a pa[2];
    qsa_page_update<DTILES>(L, sc, pagemax, m, lsum, o_acc, pa);

#pragma unroll
    for (int half = 0; half < 2; ++half) {
#pragma unroll
      for (int dt = 0; dt < DTILES; ++dt) {
        const bf16x8_a vf = *reinterpret_cast<const bf16x8_a*>(
            vbase + ((long long)(dt * 16 + col) * QSA_PAGE) + half * 32 +
            hi * 8);
        o_acc[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            pa[half], vf, o_acc[dt], 0, 0, 0);
      }
    }
  }

  qsa_prefill_store<DTILES>(
      L, o_acc, lsum,
      out + (long long)(off + pos0) * (QH * D) + (long long)qh * D, QH * D,
      n_i - pos0, col, hi);
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
// own horizon (max_abs), processes exactly the pages that kernel would
// (pi < its own page count, and the same wave-uniform "whole page masked"
// skip), and every accumulator sees the same sequence: the same ks order,
// the shared mask, page update and epilogue, and the same PV order (half,
// then dt).
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
    qsa_load_q<D>(q + (long long)(off + qrow_l) * qstride + (long long)qh * D,
                  hi, qf[s]);
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

  const qsa_lanes L = qsa_lanes_of(col, hi);
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

    // ---- online softmax per sub-tile ------------------------------------
    bool pv[S];
    bf16x8_a pa[S][2];
#pragma unroll
    for (int s = 0; s < S; ++s) {
      pv[s] = false;
      if (!act[s]) continue;
      const int pos0 = tpos0 + 16 * s;
      const int nvalid = min(max_abs[s] + 1 - pi * QSA_PAGE, QSA_PAGE);
      const float pagemax = qsa_col_reduce<true>(
          L, qsa_mask_scale<CAUSAL>(sc[s], scale, hi, nvalid, pi * QSA_PAGE,
                                    start + pos0 + col, pos0 + col < n_i));
      // wave-uniform skip of a page masked for EVERY column
      if (__all(pagemax <= -3.0e38f)) continue;
      pv[s] = true;
      qsa_page_update<DTILES>(L, sc[s], pagemax, m[s], lsum[s], o_acc[s],
                              pa[s]);
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

#pragma unroll
  for (int s = 0; s < S; ++s) {
    const int pos0 = tpos0 + 16 * s;
    qsa_prefill_store<DTILES>(
        L, o_acc[s], lsum[s],
        out + (long long)(off + pos0) * (QH * D) + (long long)qh * D, QH * D,
        n_i - pos0, col, hi);
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
    uint4 a = *reinterpret_cast<const uint4*>(base);
    uint4 b = *reinterpret_cast<const uint4*>(base + half);
    qsa_rope8(a, b, cos_t + toff, sin_t + toff);
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
      uint4 a = *reinterpret_cast<const uint4*>(base);
      uint4 b = *reinterpret_cast<const uint4*>(base + half);
      qsa_rope8(a, b, cos_t + toff, sin_t + toff);
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
