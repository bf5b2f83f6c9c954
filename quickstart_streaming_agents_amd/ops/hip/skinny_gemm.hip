// Skinny-batch decode GEMM for CDNA4 (gfx950): C[M,N] = A[M,K] @ W[N,K]^T,
// M <= 32 (the decode batch), bf16 in / bf16 out.
// Serves the K4 agent-LLM decode projections.
//
// Decode projections are HBM-bandwidth-bound on the WEIGHT stream (the
// activations are KB-sized): speed-of-light is W bytes / 6.3 TB/s.  rocBLAS
// general-GEMM tiles for big M and loses on the latency-critical small
// shapes at M~24.  W is PRE-PACKED once at model init into the bf16
// fragment-major stream of gemm_core.h, and the kernel is that header's
// skinny body with one 16-column n-tile per workgroup and two m-tiles (M
// padded to 32).  Grid = N/16 (wo: 256 WGs, qkv: 384, wgu: 1792, lm_head:
// 8016): every decode shape fills the 256-CU chip.
//
// The VARIANT template parameter exists for ablation probes from
// tools/kernel_bench.py (1 = W stream + MFMA only, 2 = A loads + MFMA
// only); production always runs VARIANT 0.
#include "gemm_core.h"

template <int WAVES, bool NT, int VARIANT>
__global__ void __launch_bounds__(WAVES * 64)
qsa_skinny_gemm_t(const unsigned short* __restrict__ A,   // [M,K] stride lda
                  const unsigned short* __restrict__ Wf,  // [N/16,K/32,16,32]
                  unsigned short* __restrict__ Cbf,       // [M, N]
                  int M, int N, long long K, long long lda) {
  qsa_skinny_body<qsa_bf16_stream<VARIANT>, WAVES, 1, NT, 2>(
      A, {Wf}, Cbf, M, N, K, lda);
}

extern "C" void qsa_skinny_gemm_launch(const unsigned short* A,
                                       const unsigned short* Wf,
                                       unsigned short* Cbf, int M, int N,
                                       long long K, long long lda,
                                       hipStream_t stream) {
  // 8 waves, plain (non-nt) W loads: the measured best full-kernel config
  // (tools/kernel_bench.py sweep; nt helps only the W-isolated stream).
  hipLaunchKernelGGL((qsa_skinny_gemm_t<8, false, 0>), dim3(N / 16),
                     dim3(512), 0, stream, A, Wf, Cbf, M, N, K, lda);
}

// Ablation/tuning probe for tools/kernel_bench.py: returns 0 when
// (waves, nt, variant) is not instantiated.
extern "C" int qsa_skinny_gemm_probe_launch(
    const unsigned short* A, const unsigned short* Wf, unsigned short* Cbf,
    int M, int N, long long K, long long lda, int waves, int nt, int variant,
    hipStream_t stream) {
  dim3 grid(N / 16);
#define QSA_CASE(W, NTB, V)                                            \
  if (waves == W && nt == NTB && variant == V) {                       \
    hipLaunchKernelGGL((qsa_skinny_gemm_t<W, NTB, V>), grid,           \
                       dim3(W * 64), 0, stream, A, Wf, Cbf, M, N, K,   \
                       lda);                                           \
    return 1;                                                          \
  }
  QSA_CASE(4, true, 0) QSA_CASE(4, false, 0) QSA_CASE(4, true, 1)
  QSA_CASE(4, true, 2) QSA_CASE(8, true, 0) QSA_CASE(8, false, 0)
  QSA_CASE(8, true, 1) QSA_CASE(8, true, 2) QSA_CASE(2, true, 0)
  QSA_CASE(1, true, 0)
#undef QSA_CASE
  return 0;
}
