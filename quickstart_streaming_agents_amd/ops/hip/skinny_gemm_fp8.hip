// FP8 (OCP e4m3) weight-streaming decode GEMM for CDNA4 (gfx950):
// C[M,N] = A[M,K] @ (s[N] * Q[N,K])^T, M <= 64, A bf16, Q fp8, C bf16.
// Serves the K4 agent-LLM decode projections.
//
// The bf16 skinny kernel (skinny_gemm.hip) is HBM-bound on the WEIGHT
// stream (PMC: ~3% MFMA util); its ceiling is W bytes / 6.3 TB/s.  FP8
// weights HALVE that stream: per-output-channel symmetric quantization
// (the standard W8A16 weight-only scheme) keeps activations bf16 and
// applies the scale once in the epilogue -- zero inner-loop cost.  The
// kernel is the skinny body of gemm_core.h on that header's fp8 stream,
// dequantised in registers (exactly) to the bf16 MFMA operand.
// Gfx950 also has native fp8 MFMA, but using it would force the
// ACTIVATIONS to fp8 too (non-scaled fp8 MFMA is A8W8); this kernel is
// bandwidth-bound, so bf16 MFMA at half the weight bytes is the same
// speed with better numerics.
#include "gemm_core.h"

// TILES n-tiles (16 cols each) per workgroup: the A (activation) loads --
// L2 traffic that rivals the fp8 W stream at 16 cols/WG -- are loaded once
// per k-step and reused across all TILES MFMA streams.  TILES=4 for the
// big-N projections (wgu/lm_head), 1 for the small ones (grid must still
// exceed 256 CUs).
//
// MT 16-row m-tiles per launch (2 or 4 -> M <= 32, 64; MT = 1 measured no
// faster than 2 at M <= 16 on any shape and is not instantiated).  A row's
// output bits depend on WAVES alone (see the body), so the launcher keeps
// WAVES per shape class the same for every MT.
template <int WAVES, int TILES, bool NT, int MT = 2>
__global__ void __launch_bounds__(WAVES * 64)
qsa_skinny_gemm_fp8_t(const unsigned short* __restrict__ A,  // [M,K] bf16
                      const u32x4* __restrict__ Qf,   // packed fp8 stream
                      const float* __restrict__ scale,     // [N] f32
                      unsigned short* __restrict__ Cbf,    // [M, N]
                      int M, int N, long long K, long long lda) {
  qsa_skinny_body<qsa_fp8_stream, WAVES, TILES, NT, MT>(
      A, {Qf, scale}, Cbf, M, N, K, lda);
}

// Every instantiated (WAVES, TILES, NT, MT): the production launcher's
// choices and the sweeps of tools/fp8_bench.py and tools/fp8_mtile_bench.py.
// (8, 8) at MT = 4 does not fit 256 registers at 8 waves (39 VGPRs spill).
#define QSA_FP8_CONFIGS(X)                                                   \
  X(8, 1, false, 2) X(8, 1, true, 2) X(8, 2, false, 2) X(8, 4, false, 2)    \
  X(8, 4, true, 2) X(8, 8, false, 2) X(16, 1, false, 2) X(16, 2, false, 2)  \
  X(16, 4, false, 2) X(4, 4, false, 2) X(4, 8, false, 2) X(2, 8, false, 2)  \
  X(2, 8, false, 4) X(8, 4, false, 4) X(8, 2, false, 4) X(8, 1, false, 4)

// Launches one configuration (N % (16 * tiles) == 0 and M <= 16 * mt are the
// caller's to check); returns 0 when it is not instantiated.
extern "C" int qsa_skinny_gemm_fp8_config_launch(
    const unsigned short* A, const unsigned char* Qf, const float* scale,
    unsigned short* Cbf, int M, int N, long long K, long long lda,
    int waves, int tiles, int nt, int mt, hipStream_t stream) {
#define QSA_CASE(W, T, NTB, MTV)                                          \
  if (waves == W && tiles == T && nt == (int)NTB && mt == MTV) {          \
    hipLaunchKernelGGL((qsa_skinny_gemm_fp8_t<W, T, NTB, MTV>),           \
                       dim3(N / (16 * T)), dim3(W * 64), 0, stream, A,    \
                       reinterpret_cast<const u32x4*>(Qf), scale, Cbf,    \
                       M, N, K, lda);                                     \
    return 1;                                                             \
  }
  QSA_FP8_CONFIGS(QSA_CASE)
#undef QSA_CASE
  return 0;
}

// The shape class of an [N, K] weight, its last class split by K: the launch
// is the same for wo and wdown, the comparison with rocBLAS at 33..64 rows
// (ops/dispatch.py) is not.  dispatch.skinny_fp8_class is the CPU-only copy;
// tests/test_gpu_gemm_edges.py test_skinny_fp8_class_agrees compares them.
enum qsa_fp8_class { QSA_LM_HEAD, QSA_WGU, QSA_QKV, QSA_WO, QSA_WDOWN };

static qsa_fp8_class qsa_fp8_class_of(int N, long long K) {
  if (N % 128 == 0 && N >= 65536) return QSA_LM_HEAD;
  if (N % 64 == 0 && N >= 16384) return QSA_WGU;
  if (N % 32 == 0 && N >= 6144 && K < 8192) return QSA_QKV;
  return K < 8192 ? QSA_WO : QSA_WDOWN;
}

extern "C" const char* qsa_skinny_fp8_class(int N, long long K) {
  static const char* const names[] = {"lm_head", "wgu", "qkv", "wo", "wdown"};
  return names[qsa_fp8_class_of(N, K)];
}

// Per-shape winners from the measured sweep on MI355X
// (profiles/fp8_decode_gemm.md): huge N wants more tiles + fewer
// waves (lm_head w2t8 = 4.6 TB/s fp8 bytes), mid N wants t4, qkv-size
// t2, small/deep-K t1.  WAVES is a function of the shape class only;
// M <= 32 runs two m-tiles, M <= 64 (checked by the caller) four.
extern "C" void qsa_skinny_gemm_fp8_launch(
    const unsigned short* A, const unsigned char* Qf, const float* scale,
    unsigned short* Cbf, int M, int N, long long K, long long lda,
    hipStream_t stream) {
  int waves = 8, tiles = 1;                  // wo / wdown
  switch (qsa_fp8_class_of(N, K)) {
    case QSA_LM_HEAD: waves = 2; tiles = 8; break;
    case QSA_WGU: tiles = 4; break;
    case QSA_QKV: tiles = 2; break;
    default: break;
  }
  qsa_skinny_gemm_fp8_config_launch(A, Qf, scale, Cbf, M, N, K, lda, waves,
                                    tiles, 0, M <= 32 ? 2 : 4, stream);
}
