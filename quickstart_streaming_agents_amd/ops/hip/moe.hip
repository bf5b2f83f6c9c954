// Routed mixture-of-experts decode FFN for CDNA4 (gfx950): T <= 64 rows,
// E <= 16 experts, top-k <= 4.  Five launches per layer, no host sync:
//
//   dispatch  h [T,H], top_idx [T,k]      -> counts [E], slot [T,k],
//                                            xg [E,cap,H] (rows by expert)
//   grouped skinny GEMM  xg x wgu[e]      -> gu  [E,cap,2F]
//   swiglu (live rows only)               -> act [E,cap,F]
//   grouped skinny GEMM  act x wdown[e]   -> y   [E,cap,H]
//   combine  sum_k gate * y[e, slot]      -> out [T,H]
//
// cap is the row capacity per expert: 32 at T <= 32, else 64 (a row picks an
// expert at most once, so no expert ever holds more than T rows).  The
// routing stays on the device, so the step is hipGraph-capturable, and a
// grouped-GEMM workgroup of an expert with no rows returns before it reads a
// byte of that expert's weights: the FFN streams only the experts that rows
// chose.
//
// The GEMMs are the skinny body of gemm_core.h with blockIdx.y = expert.
// WAVES is pinned to 8: it alone fixes a row's accumulation order, and 8 is
// what skinny_gemm and every non-lm_head class of skinny_gemm_fp8 run, so a
// live output row has the bits the single-expert kernels give it.
#include "gemm_core.h"

#define QSA_MOE_MAX_K 4
#define QSA_MOE_WAVES 8

// ---------------------------------------------------------------------------
// Dispatch: routing + gather.  One workgroup per row t.  Every wave holds the
// whole routing table with lane = row, so for expert e
//   mask = ballot(row is live and picked e)
//   slot of row t = popcount(mask bits below t), count = popcount(mask):
// slots ascend with the row index by construction, no atomics.  Workgroup t
// recomputes the ballots for its own k picks, copies its row into those
// slots (16-byte accesses) and workgroup 0 also writes counts.  Rows of xg
// at or past counts[e] stay unwritten.  A pick outside [0, E) gets slot -1.
// Precondition (not checked): a row's k experts are distinct.
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
qsa_moe_dispatch_kernel(const unsigned short* __restrict__ h,      // [T,H]
                        const long long* __restrict__ top_idx,     // [T,k]
                        const int* __restrict__ row_live,   // [T] or null
                        int* __restrict__ counts,                  // [E]
                        int* __restrict__ slot,                    // [T,k]
                        unsigned short* __restrict__ xg,    // [E,cap,H]
                        int T, int H, int E, int k, int cap) {
  const int t = blockIdx.x;
  const int lane = threadIdx.x & 63;
  const int row = min(lane, T - 1);
  const bool live =
      lane < T && (row_live == nullptr || row_live[row] != 0);
  long long mine[QSA_MOE_MAX_K];
#pragma unroll
  for (int j = 0; j < QSA_MOE_MAX_K; ++j) {
    const long long v = top_idx[(long long)row * k + min(j, k - 1)];
    mine[j] = (live && j < k) ? v : -1;
  }
  auto mask_of = [&](long long e) -> unsigned long long {
    bool hit = false;
#pragma unroll
    for (int j = 0; j < QSA_MOE_MAX_K; ++j) hit |= (mine[j] == e);
    return __builtin_amdgcn_ballot_w64(hit);
  };
  if (t == 0) {
    for (int e = 0; e < E; ++e) {
      const unsigned long long m = mask_of(e);
      if (threadIdx.x == 0) counts[e] = __popcll(m);
    }
  }
  const bool t_live = row_live == nullptr || row_live[t] != 0;
  const uint4* src = reinterpret_cast<const uint4*>(h + (long long)t * H);
  for (int j = 0; j < k; ++j) {
    const long long e = top_idx[(long long)t * k + j];
    const unsigned long long m = mask_of(e);
    int s = -1;
    if (t_live && e >= 0 && e < E)
      s = __popcll(m & ((1ull << t) - 1ull));   // t <= 63
    if (threadIdx.x == 0) slot[t * k + j] = s;
    if (s >= 0 && s < cap) {
      uint4* dst = reinterpret_cast<uint4*>(
          xg + ((long long)e * cap + s) * H);
      for (int i = threadIdx.x; i < H / 8; i += blockDim.x) dst[i] = src[i];
    }
  }
}

extern "C" void qsa_moe_dispatch_launch(
    const unsigned short* h, const long long* top_idx, const int* row_live,
    int* counts, int* slot, unsigned short* xg, int T, int H, int E, int k,
    int cap, hipStream_t stream) {
  hipLaunchKernelGGL(qsa_moe_dispatch_kernel, dim3(T), dim3(256), 0, stream,
                     h, top_idx, row_live, counts, slot, xg, T, H, E, k, cap);
}

// ---------------------------------------------------------------------------
// Grouped skinny GEMMs: grid (N / (16 * TILES), E), M = counts[e] rows of
// xg[e] against expert e's slice of the stacked stream.  cap = 16 * MT.
// ---------------------------------------------------------------------------
template <int TILES, int MT>
__global__ void __launch_bounds__(QSA_MOE_WAVES * 64)
qsa_moe_skinny_gemm_bf16_t(const unsigned short* __restrict__ xg,  // [E,cap,K]
                           const unsigned short* __restrict__ Wf,  // [E,N*K]
                           unsigned short* __restrict__ out,       // [E,cap,N]
                           const int* __restrict__ counts, int N,
                           long long K) {
  const int e = blockIdx.y;
  const int M = min(counts[e], 16 * MT);
  if (M <= 0) return;   // whole workgroup, before any barrier: no byte read
  qsa_skinny_body<qsa_bf16_stream<0>, QSA_MOE_WAVES, TILES, false, MT>(
      xg + (long long)e * (16 * MT) * K, {Wf + (long long)e * N * K},
      out + (long long)e * (16 * MT) * N, M, N, K, K);
}

template <int TILES, int MT>
__global__ void __launch_bounds__(QSA_MOE_WAVES * 64)
qsa_moe_skinny_gemm_fp8_t(const unsigned short* __restrict__ xg,   // [E,cap,K]
                          const u32x4* __restrict__ Qf,    // [E, N*K bytes]
                          const float* __restrict__ scale,         // [E,N]
                          unsigned short* __restrict__ out,        // [E,cap,N]
                          const int* __restrict__ counts, int N,
                          long long K) {
  const int e = blockIdx.y;
  const int M = min(counts[e], 16 * MT);
  if (M <= 0) return;   // whole workgroup, before any barrier: no byte read
  qsa_skinny_body<qsa_fp8_stream, QSA_MOE_WAVES, TILES, false, MT>(
      xg + (long long)e * (16 * MT) * K,
      {Qf + (long long)e * ((long long)N * K / 16), scale + (long long)e * N},
      out + (long long)e * (16 * MT) * N, M, N, K, K);
}

// cap is 32 or 64 (checked by the binding).
extern "C" void qsa_moe_skinny_gemm_bf16_launch(
    const unsigned short* xg, const unsigned short* Wf, unsigned short* out,
    const int* counts, int E, int cap, int N, long long K,
    hipStream_t stream) {
  const dim3 grid(N / 16, E), block(QSA_MOE_WAVES * 64);
  if (cap == 32)
    hipLaunchKernelGGL((qsa_moe_skinny_gemm_bf16_t<1, 2>), grid, block, 0,
                       stream, xg, Wf, out, counts, N, K);
  else
    hipLaunchKernelGGL((qsa_moe_skinny_gemm_bf16_t<1, 4>), grid, block, 0,
                       stream, xg, Wf, out, counts, N, K);
}

extern "C" const char* qsa_skinny_fp8_class(int, long long);

// TILES follows the single-expert launcher's shape class
// (skinny_gemm_fp8.hip): 4 for wgu, 2 for qkv, else 1.  Returns the tiles
// used, or 0 for the lm_head class: that one runs 2 waves there, so an
// 8-wave grouped kernel would not reproduce its bits.
extern "C" int qsa_moe_skinny_gemm_fp8_launch(
    const unsigned short* xg, const unsigned char* Qf, const float* scale,
    unsigned short* out, const int* counts, int E, int cap, int N,
    long long K, hipStream_t stream) {
  const char* cls = qsa_skinny_fp8_class(N, K);
  if (cls[0] == 'l') return 0;
  const int tiles = (cls[0] == 'w' && cls[1] == 'g') ? 4
                    : cls[0] == 'q'                  ? 2
                                                     : 1;
  const dim3 grid(N / (16 * tiles), E), block(QSA_MOE_WAVES * 64);
  const u32x4* q = reinterpret_cast<const u32x4*>(Qf);
#define QSA_CASE(T, MTV)                                                   \
  if (tiles == T && cap == 16 * MTV) {                                     \
    hipLaunchKernelGGL((qsa_moe_skinny_gemm_fp8_t<T, MTV>), grid, block,   \
                       0, stream, xg, q, scale, out, counts, N, K);        \
    return tiles;                                                          \
  }
  QSA_CASE(1, 2) QSA_CASE(2, 2) QSA_CASE(4, 2)
  QSA_CASE(1, 4) QSA_CASE(2, 4) QSA_CASE(4, 4)
#undef QSA_CASE
  return 0;
}

// ---------------------------------------------------------------------------
// SwiGLU over gu [E,cap,2F] -> act [E,cap,F], rows r < counts[e] only.
// Grid (ceil(F/8/256), cap, E).
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
qsa_moe_swiglu_kernel(const unsigned short* __restrict__ gu,
                      unsigned short* __restrict__ act,
                      const int* __restrict__ counts, int cap, long long F) {
  const int e = blockIdx.z, r = blockIdx.y;
  if (r >= counts[e]) return;
  const long long c = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * 8;
  if (c >= F) return;
  const long long rowi = (long long)e * cap + r;
  const unsigned short* g = gu + rowi * 2 * F + c;
  *reinterpret_cast<uint4*>(act + rowi * F + c) =
      qsa_swiglu8(*reinterpret_cast<const uint4*>(g),
                  *reinterpret_cast<const uint4*>(g + F));
}

extern "C" void qsa_moe_swiglu_launch(const unsigned short* gu,
                                      unsigned short* act, const int* counts,
                                      int E, int cap, long long F,
                                      hipStream_t stream) {
  const dim3 grid((unsigned)((F / 8 + 255) / 256), cap, E);
  hipLaunchKernelGGL(qsa_moe_swiglu_kernel, grid, dim3(256), 0, stream, gu,
                     act, counts, cap, F);
}

// ---------------------------------------------------------------------------
// Combine: out[t,:] = sum over the row's k picks of gate * y[e, slot], in
// ascending EXPERT index, f32 from 0.f, the multiply and the add rounded
// separately (no FMA), one rounding to bf16.  That is the arithmetic of the
// dense masked sum (out += gates[:, e] * y.float(), whose unselected terms
// are exact zeros) and of ExpertDispatch.run, which is what makes the routed
// FFN bit-identical to them.  Dead picks (slot < 0) add nothing; a dead row
// gives zeros.  Grid (ceil(H/8/256), T).
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
qsa_moe_combine_kernel(const unsigned short* __restrict__ y,   // [E,cap,H]
                       const int* __restrict__ slot,           // [T,k]
                       const long long* __restrict__ top_idx,  // [T,k]
                       const float* __restrict__ top_w,        // [T,k]
                       unsigned short* __restrict__ out,       // [T,H]
                       int H, int E, int k, int cap) {
#pragma clang fp contract(off)
  const int t = blockIdx.y;
  const int c = (blockIdx.x * blockDim.x + threadIdx.x) * 8;
  if (c >= H) return;
  long long ex[QSA_MOE_MAX_K];
  int sl[QSA_MOE_MAX_K];
  float gw[QSA_MOE_MAX_K];
#pragma unroll
  for (int j = 0; j < QSA_MOE_MAX_K; ++j) {
    const int jj = t * k + min(j, k - 1);
    const int s = slot[jj];
    ex[j] = top_idx[jj];
    gw[j] = top_w[jj];
    sl[j] = (j < k && s < cap) ? s : -1;
  }
  float acc[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) acc[i] = 0.f;
  for (int e = 0; e < E; ++e) {
#pragma unroll
    for (int j = 0; j < QSA_MOE_MAX_K; ++j) {
      if (ex[j] == e && sl[j] >= 0) {
        const uint4 v = *reinterpret_cast<const uint4*>(
            y + ((long long)e * cap + sl[j]) * H + c);
        const unsigned int p[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float2 f = bf16x2_to_f32x2(p[i]);
          const float m0 = gw[j] * f.x;
          const float m1 = gw[j] * f.y;
          acc[2 * i] = acc[2 * i] + m0;
          acc[2 * i + 1] = acc[2 * i + 1] + m1;
        }
      }
    }
  }
  uint4 o;
  o.x = f32x2_to_bf16x2(acc[0], acc[1]);
  o.y = f32x2_to_bf16x2(acc[2], acc[3]);
  o.z = f32x2_to_bf16x2(acc[4], acc[5]);
  o.w = f32x2_to_bf16x2(acc[6], acc[7]);
  *reinterpret_cast<uint4*>(out + (long long)t * H + c) = o;
}

extern "C" void qsa_moe_combine_launch(
    const unsigned short* y, const int* slot, const long long* top_idx,
    const float* top_w, unsigned short* out, int T, int H, int E, int k,
    int cap, hipStream_t stream) {
  const dim3 grid((H / 8 + 255) / 256, T);
  hipLaunchKernelGGL(qsa_moe_combine_kernel, grid, dim3(256), 0, stream, y,
                     slot, top_idx, top_w, out, H, E, k, cap);
}
