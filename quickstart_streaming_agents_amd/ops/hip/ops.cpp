// Torch bindings for the qsa MI355X (gfx950) kernels.  HIP-native: no CUDA
// naming, no compatibility shims — this extension only builds for ROCm.
// Operator inventory these kernels implement: SURVEY.md 2.4 K1-K10
// (embedding, cosine top-k, anomaly scoring, paged-attention LLM decode,
// window aggregation, Avro wire codec).
#include <hip/hip_runtime.h>
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#define CHK(x) TORCH_CHECK(x, #x)
#define CHK_DEV(t) TORCH_CHECK((t).is_cuda(), #t " must be on the GPU")
#define CHK_CONT(t) TORCH_CHECK((t).is_contiguous(), #t " must be contiguous")
#define CHK_BF16(t) TORCH_CHECK((t).scalar_type() == at::kBFloat16, #t " must be bf16")
#define CHK_F32(t) TORCH_CHECK((t).scalar_type() == at::kFloat, #t " must be f32")
#define CHK_I32(t) TORCH_CHECK((t).scalar_type() == at::kInt, #t " must be i32")

static inline const unsigned short* u16(const torch::Tensor& t) {
  return reinterpret_cast<const unsigned short*>(t.data_ptr());
}
static inline unsigned short* u16m(torch::Tensor& t) {
  return reinterpret_cast<unsigned short*>(t.data_ptr());
}
static inline hipStream_t cur_stream() {
  return at::hip::getCurrentHIPStream().stream();
}

// ---- launcher decls (defined in the .hip files) ---------------------------
extern "C" void qsa_rmsnorm_launch(const unsigned short*, const unsigned short*,
                                   unsigned short*, unsigned short*, long long,
                                   int, float, hipStream_t);
extern "C" void qsa_swiglu_launch(const unsigned short*, const unsigned short*,
                                  unsigned short*, long long, long long,
                                  long long, int, hipStream_t);
extern "C" void qsa_rope_launch(unsigned short*, unsigned short*, const float*,
                                const float*, const int*, int, int, int, int,
                                long long, long long, hipStream_t);
extern "C" void qsa_softmax_rows_launch(float*, int, int, int, int, int,
                                        const int*, hipStream_t);
extern "C" void qsa_softmax_rows_bf16_launch(unsigned short*, long long, int,
                                             float, const int*, hipStream_t);
extern "C" void qsa_paged_attn_mfma_launch(
    const unsigned short*, const unsigned short*, const unsigned short*,
    const int*, const int*, float*, float*, unsigned short*, float, int, int,
    int, int, int, long long, int, hipStream_t);
extern "C" void qsa_paged_attn_mfma_fused_launch(
    const unsigned short*, const unsigned short*, const unsigned short*,
    unsigned short*, unsigned short*, const float*, const float*, const int*,
    const int*, float*, float*, unsigned short*, float, int, int, int, int,
    int, long long, long long, int, int, hipStream_t);
extern "C" void qsa_kv_append_launch(const unsigned short*,
                                     const unsigned short*, unsigned short*,
                                     unsigned short*, const int*, const int*,
                                     int, int, int, int, long long,
                                     hipStream_t);
extern "C" void qsa_paged_attn_prefill_launch(
    const unsigned short*, const unsigned short*, const unsigned short*,
    const int*, const int*, const int*, const int*, const int*, const int*,
    unsigned short*, float, int, int, int, int, int, long long, int,
    hipStream_t);
extern "C" int qsa_paged_attn_prefill_tiled_launch(
    const unsigned short*, const unsigned short*, const unsigned short*,
    const int*, const int*, const int*, const int*, const int*, const int*,
    unsigned short*, float, int, int, int, int, int, long long, int, int,
    hipStream_t);
extern "C" void qsa_rope_kv_scatter_launch(
    unsigned short*, const unsigned short*, const unsigned short*,
    unsigned short*, unsigned short*, const float*, const float*, const int*,
    const int*, int, int, int, int, int, long long, long long, hipStream_t);
extern "C" void qsa_rope_kv_append_launch(unsigned short*,
                                          const unsigned short*,
                                          const unsigned short*,
                                          unsigned short*, unsigned short*,
                                          const float*, const float*,
                                          const int*, const int*, int, int,
                                          int, int, int, long long, long long,
                                          hipStream_t);
extern "C" void qsa_kv_scatter_launch(const unsigned short*,
                                      const unsigned short*, unsigned short*,
                                      unsigned short*, const int*, int, int,
                                      int, long long, hipStream_t);
extern "C" void qsa_skinny_gemm_launch(const unsigned short*,
                                       const unsigned short*, unsigned short*,
                                       int, int, long long, long long,
                                       hipStream_t);
extern "C" int qsa_skinny_gemm_probe_launch(
    const unsigned short*, const unsigned short*, unsigned short*, int, int,
    long long, long long, int, int, int, hipStream_t);
extern "C" void qsa_skinny_gemm_fp8_launch(
    const unsigned short*, const unsigned char*, const float*,
    unsigned short*, int, int, long long, long long, hipStream_t);
extern "C" int qsa_skinny_gemm_fp8_config_launch(
    const unsigned short*, const unsigned char*, const float*,
    unsigned short*, int, int, long long, long long, int, int, int, int,
    hipStream_t);
extern "C" const char* qsa_skinny_fp8_class(int, long long);
extern "C" void qsa_moe_dispatch_launch(const unsigned short*,
                                        const long long*, const int*, int*,
                                        int*, unsigned short*, int, int, int,
                                        int, int, hipStream_t);
extern "C" void qsa_moe_skinny_gemm_bf16_launch(
    const unsigned short*, const unsigned short*, unsigned short*, const int*,
    int, int, int, long long, hipStream_t);
extern "C" int qsa_moe_skinny_gemm_fp8_launch(
    const unsigned short*, const unsigned char*, const float*,
    unsigned short*, const int*, int, int, int, long long, hipStream_t);
extern "C" void qsa_moe_swiglu_launch(const unsigned short*, unsigned short*,
                                      const int*, int, int, long long,
                                      hipStream_t);
extern "C" void qsa_moe_combine_launch(const unsigned short*, const int*,
                                       const long long*, const float*,
                                       unsigned short*, int, int, int, int,
                                       int, hipStream_t);
extern "C" void qsa_greedy_sample_launch(
    const unsigned short*, int, long long, int, int, int, const long long*,
    const unsigned char*, int, long long*, long long*, long long, int,
    long long*, unsigned int*, hipStream_t);
extern "C" void qsa_sample_launch(
    const unsigned short*, int, long long, int, int, int, const float*,
    const int*, const int*, const long long*, const int*, const long long*,
    const unsigned char*, int, long long*, long long*, long long, int,
    long long*, unsigned int*, hipStream_t);
extern "C" void qsa_gemm_fp8_batch_launch(const unsigned short*,
                                          const unsigned char*,
                                          const float*, unsigned short*,
                                          float*, int, int, long long,
                                          long long, int, hipStream_t);
extern "C" void qsa_hash_build_launch(const long long*, const long long*,
                                      unsigned long long*,
                                      unsigned long long*, int, unsigned int,
                                      hipStream_t);
extern "C" void qsa_hash_probe_launch(const long long*,
                                      const unsigned long long*,
                                      const unsigned long long*, int*, int,
                                      unsigned int, long long, hipStream_t);
extern "C" void qsa_topk_launch(const float*, const float*, float*, int*,
                                float*, int*, int, int, int, int, int,
                                hipStream_t);
extern "C" void qsa_window_agg_launch(const long long*, const int*,
                                      const float*, int*, float*, long long,
                                      long long, int, long long, int,
                                      hipStream_t);
void register_avro(pybind11::module_&);  // avro_codec.cpp
extern "C" void qsa_anomaly_batch_launch(const float*, const int*, float*,
                                         float*, int*, int, int, int,
                                         hipStream_t);

// ---------------------------------------------------------------------------

torch::Tensor rmsnorm(torch::Tensor x, torch::Tensor w, double eps) {
  CHK_DEV(x); CHK_CONT(x); CHK_BF16(x); CHK_BF16(w); CHK_CONT(w);
  const int H = x.size(-1);
  TORCH_CHECK(H % 8 == 0, "H % 8 == 0");
  const long long rows = x.numel() / H;
  auto y = torch::empty_like(x);
  qsa_rmsnorm_launch(u16(x), u16(w), u16m(y), nullptr, rows, H, (float)eps,
                     cur_stream());
  return y;
}

torch::Tensor rmsnorm_residual(torch::Tensor x, torch::Tensor res,
                               torch::Tensor w, double eps) {
  CHK_DEV(x); CHK_CONT(x); CHK_BF16(x); CHK_BF16(res); CHK_CONT(res);
  CHK_BF16(w); CHK_CONT(w);
  const int H = x.size(-1);
  TORCH_CHECK(H % 8 == 0, "H % 8 == 0");
  TORCH_CHECK(res.sizes() == x.sizes(), "residual shape mismatch");
  const long long rows = x.numel() / H;
  auto y = torch::empty_like(x);
  qsa_rmsnorm_launch(u16(x), u16(w), u16m(y), u16m(res), rows, H, (float)eps,
                     cur_stream());
  return y;
}

torch::Tensor swiglu(torch::Tensor gate, torch::Tensor up) {
  // gate/up: [rows, cols] views with equal row stride (e.g. halves of the
  // fused gate_up GEMM output); cols % 8 == 0, element-contiguous rows.
  CHK_DEV(gate); CHK_BF16(gate); CHK_BF16(up);
  TORCH_CHECK(gate.dim() == 2 && up.dim() == 2, "2-D");
  TORCH_CHECK(gate.sizes() == up.sizes(), "shape mismatch");
  TORCH_CHECK(gate.stride(1) == 1 && up.stride(1) == 1, "rows contiguous");
  TORCH_CHECK(gate.stride(0) == up.stride(0), "row strides must match");
  const long long rows = gate.size(0), cols = gate.size(1);
  TORCH_CHECK(cols % 8 == 0, "cols % 8 == 0");
  // 16-byte loads at row * stride + col
  TORCH_CHECK(gate.stride(0) % 8 == 0 &&
              reinterpret_cast<uintptr_t>(gate.data_ptr()) % 16 == 0 &&
              reinterpret_cast<uintptr_t>(up.data_ptr()) % 16 == 0,
              "swiglu: gate/up rows must be 16-byte aligned");
  auto y = torch::empty({rows, cols}, gate.options());
  const long long n = rows * cols;
  const int blocks = (int)std::min<long long>((n / 8 + 255) / 256, 8192);
  qsa_swiglu_launch(u16(gate), u16(up), u16m(y), rows, cols, gate.stride(0),
                    blocks, cur_stream());
  return y;
}

static inline void chk_hd_strided(const torch::Tensor& t, int D,
                                  const char* name) {
  TORCH_CHECK(t.dim() == 3 && t.stride(2) == 1 && t.stride(1) == D,
              name, " must be a [B, H, D] view with contiguous heads");
}

// ---- argument checks shared by the attention and KV-writer bindings --------
// Everything a kernel dereferences is checked here, ahead of the launch: the
// kernels themselves trust their pointers.

struct named_tensor {
  const char* name;
  const torch::Tensor& t;
};

// Every tensor argument lives on the first one's GPU: a CPU index array
// would hand a host pointer to the kernel.
static void chk_same_gpu(std::initializer_list<named_tensor> ts) {
  const named_tensor& first = *ts.begin();
  for (const named_tensor& a : ts) {
    TORCH_CHECK(a.t.is_cuda(), a.name, " must be on the GPU");
    TORCH_CHECK(a.t.device() == first.t.device(), a.name, " must be on ",
                first.name, "'s device");
  }
}

// bf16 [rows, heads, D] view with contiguous heads, D 64 or 128.
static int chk_heads(const torch::Tensor& t, const char* name) {
  TORCH_CHECK(t.scalar_type() == at::kBFloat16, name, " must be bf16");
  TORCH_CHECK(t.dim() == 3, name, " must be [rows, heads, D]");
  const int D = t.size(2);
  TORCH_CHECK(D == 128 || D == 64, "D must be 64/128");
  chk_hd_strided(t, D, name);
  return D;
}

// 16-byte fragment loads of a [rows, heads, D] view's rows.
static void chk_rows16(const torch::Tensor& t, const char* name) {
  TORCH_CHECK(t.stride(0) % 8 == 0 &&
              reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0,
              name, " rows must be 16-byte aligned");
}

// The paged cache pair for KVH kv heads of width D.
static void chk_kv_cache(const torch::Tensor& kc, const torch::Tensor& vc,
                         int KVH, int D) {
  CHK_BF16(kc); CHK_BF16(vc); CHK_CONT(kc); CHK_CONT(vc);
  TORCH_CHECK(kc.dim() == 5 && kc.size(1) == KVH && kc.size(2) == D / 8 &&
              kc.size(3) == 64 && kc.size(4) == 8,
              "K cache layout [P, KVH, D/8, 64, 8]");
  TORCH_CHECK(vc.dim() == 4 && vc.size(2) == D && vc.size(3) == 64,
              "V cache layout [P, KVH, D, 64] (transposed)");
  TORCH_CHECK(vc.size(1) == KVH && vc.size(0) == kc.size(0),
              "K and V caches must have the same pages and kv heads");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(kc.data_ptr()) % 16 == 0 &&
              reinterpret_cast<uintptr_t>(vc.data_ptr()) % 16 == 0,
              "K/V caches must be 16-byte aligned");
}

// i32 contiguous index array of exactly n entries.
static void chk_index(const torch::Tensor& t, long n, const char* name) {
  TORCH_CHECK(t.scalar_type() == at::kInt, name, " must be i32");
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
  TORCH_CHECK(t.numel() == n, name, " must have ", n, " entries");
}

// i32 contiguous [rows, >= 1 pages] block table.
static void chk_block_table(const torch::Tensor& bt, long rows) {
  CHK_I32(bt); CHK_CONT(bt);
  TORCH_CHECK(bt.dim() == 2 && bt.size(0) == rows && bt.size(1) >= 1,
              "block_table must be [", rows, ", pages >= 1]");
}

// f32 contiguous [positions, D/2] rope tables, 16-byte aligned.
static void chk_rope_tables(const torch::Tensor& cos_t,
                            const torch::Tensor& sin_t, int D) {
  CHK_F32(cos_t); CHK_F32(sin_t); CHK_CONT(cos_t); CHK_CONT(sin_t);
  TORCH_CHECK(cos_t.dim() == 2 && sin_t.dim() == 2 &&
              cos_t.size(1) == D / 2 && sin_t.size(1) == D / 2 &&
              cos_t.size(0) == sin_t.size(0),
              "rope tables must be [positions, D/2]");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(cos_t.data_ptr()) % 16 == 0 &&
              reinterpret_cast<uintptr_t>(sin_t.data_ptr()) % 16 == 0,
              "rope tables must be 16-byte aligned");
}

// New k/v rows of one step: both [rows, KVH, D] views with one row stride.
static void chk_kv_rows(const torch::Tensor& k, const torch::Tensor& v,
                        long rows, int KVH, int D) {
  TORCH_CHECK(chk_heads(k, "k") == D && chk_heads(v, "v") == D &&
              k.size(0) == rows && v.size(0) == rows && k.size(1) == KVH &&
              v.size(1) == KVH, "k/v must be [", rows, ", KVH, D]");
  TORCH_CHECK(k.stride(0) == v.stride(0), "k/v strides must match");
}

// GQA: QH q heads over KVH kv heads, at most 16 per kv head.
static void chk_gqa(int QH, int KVH) {
  TORCH_CHECK(KVH > 0 && QH % KVH == 0, "GQA requires QH % KVH == 0");
  TORCH_CHECK(QH / KVH <= 16, "GQA ratio <= 16");
}

void rope_inplace(torch::Tensor q, torch::Tensor k, torch::Tensor cos_t,
                  torch::Tensor sin_t, torch::Tensor pos) {
  CHK_DEV(q); CHK_BF16(q); CHK_BF16(k);
  CHK_F32(cos_t); CHK_F32(sin_t); CHK_I32(pos);
  const int B = q.size(0), QH = q.size(1), D = q.size(2);
  const int KVH = k.size(1);
  TORCH_CHECK(k.size(0) == B && k.size(2) == D, "k shape");
  chk_hd_strided(q, D, "q"); chk_hd_strided(k, D, "k");
  qsa_rope_launch(u16m(q), u16m(k), cos_t.data_ptr<float>(),
                  sin_t.data_ptr<float>(), pos.data_ptr<int>(), B, QH, KVH, D,
                  q.stride(0), k.stride(0), cur_stream());
}

void softmax_rows_(torch::Tensor scores, long col_offset, bool causal,
                   long row_mod, c10::optional<torch::Tensor> row_limits) {
  CHK_DEV(scores); CHK_CONT(scores); CHK_F32(scores);
  const int rows = scores.size(0), cols = scores.size(1);
  const int* rl = nullptr;
  if (row_limits.has_value()) {
    CHK_I32(row_limits.value());
    rl = row_limits.value().data_ptr<int>();
  }
  qsa_softmax_rows_launch(scores.data_ptr<float>(), rows, cols,
                          (int)col_offset, causal ? 1 : 0, (int)row_mod, rl,
                          cur_stream());
}

void softmax_rows_bf16_(torch::Tensor scores, double scale,
                        torch::Tensor row_limits) {
  CHK_DEV(scores); CHK_CONT(scores); CHK_BF16(scores); CHK_I32(row_limits);
  const long long rows = scores.size(0);
  const int cols = scores.size(1);
  TORCH_CHECK(cols % 8 == 0, "cols % 8 == 0");
  TORCH_CHECK(row_limits.numel() == rows, "one limit per row");
  qsa_softmax_rows_bf16_launch(u16m(scores), rows, cols, (float)scale,
                               row_limits.data_ptr<int>(), cur_stream());
}

// Flash-decoding split count of both decode bindings: it fixes the split
// boundaries and with them the rounding, so the two must never drift apart
// (tests/test_gpu_decode_fused.py compares bits).  Needs B * KVH > 0.
static int decode_num_splits(int B, int KVH, int max_pages) {
  int ns = (int)std::min<long long>(32, std::max<long long>(
      1, (2048 + (long long)B * KVH - 1) / ((long long)B * KVH)));
  if (ns > 1) ns = std::max(ns, 4);   // fill all 4 waves per workgroup
  return std::min(ns, std::max(1, max_pages));
}

torch::Tensor paged_attn_decode(torch::Tensor q, torch::Tensor kc,
                                torch::Tensor vc, torch::Tensor block_table,
                                torch::Tensor seq_lens, double scale) {
  chk_same_gpu({{"q", q}, {"kc", kc}, {"vc", vc},
                {"block_table", block_table}, {"seq_lens", seq_lens}});
  const int D = chk_heads(q, "q");
  const int B = q.size(0), QH = q.size(1);
  chk_rows16(q, "q");
  TORCH_CHECK(kc.dim() == 5, "K cache layout [P, KVH, D/8, 64, 8]");
  const int KVH = kc.size(1);
  chk_gqa(QH, KVH);
  chk_kv_cache(kc, vc, KVH, D);
  chk_block_table(block_table, B);
  chk_index(seq_lens, B, "seq_lens");
  const int max_pages = block_table.size(1);
  auto out = torch::empty({B, QH, D}, q.options());
  if (B == 0) return out;
  // flash-decoding split count: fill the 256-CU chip (one WAVE per
  // (b, kvh, split); 4 splits share a workgroup)
  const int ns = decode_num_splits(B, KVH, max_pages);
  auto opts_f = q.options().dtype(at::kFloat);
  auto part_o = torch::empty({B, QH, ns, D}, opts_f);
  auto part_ml = torch::empty({B, QH, ns, 2}, opts_f);
  qsa_paged_attn_mfma_launch(
      u16(q), u16(kc), u16(vc), block_table.data_ptr<int>(),
      seq_lens.data_ptr<int>(), part_o.data_ptr<float>(),
      part_ml.data_ptr<float>(), u16m(out), (float)scale, B, QH, KVH,
      max_pages, D, q.stride(0), ns, cur_stream());
  return out;
}

// One launch for a decode step's attention: RoPE on q (in registers) and on
// the new k row, k/v append to the paged cache, pipelined flash-decode and
// the split merge.  q/k/v are the UN-rotated strided views of the qkv
// buffer and stay untouched.  Bit-identical to rope_kv_append followed by
// paged_attn_decode.  waves_per_simd picks the register budget the kernel
// was compiled for (1 or 2).
torch::Tensor decode_attn_fused(torch::Tensor q, torch::Tensor k,
                                torch::Tensor v, torch::Tensor kc,
                                torch::Tensor vc, torch::Tensor cos_t,
                                torch::Tensor sin_t,
                                torch::Tensor block_table,
                                torch::Tensor seq_lens, double scale,
                                int64_t waves_per_simd) {
  chk_same_gpu({{"q", q}, {"k", k}, {"v", v}, {"kc", kc}, {"vc", vc},
                {"cos_t", cos_t}, {"sin_t", sin_t},
                {"block_table", block_table}, {"seq_lens", seq_lens}});
  const int D = chk_heads(q, "q");
  const int B = q.size(0), QH = q.size(1);
  TORCH_CHECK(kc.dim() == 5, "K cache layout [P, KVH, D/8, 64, 8]");
  const int KVH = kc.size(1);
  chk_gqa(QH, KVH);
  chk_kv_rows(k, v, B, KVH, D);
  chk_kv_cache(kc, vc, KVH, D);
  chk_rope_tables(cos_t, sin_t, D);
  // 16-byte fragment loads of q rows and of the new k row (v is read by
  // element)
  chk_rows16(q, "q"); chk_rows16(k, "k");
  TORCH_CHECK(waves_per_simd == 1 || waves_per_simd == 2,
              "waves_per_simd must be 1 or 2");
  chk_block_table(block_table, B);
  chk_index(seq_lens, B, "seq_lens");
  const int max_pages = block_table.size(1);
  auto out = torch::empty({B, QH, D}, q.options());
  if (B == 0) return out;
  const int ns = decode_num_splits(B, KVH, max_pages);
  // NS <= 4 merges inside the workgroup: no partial buffers at all
  torch::Tensor part_o, part_ml;
  float* po = nullptr;
  float* pml = nullptr;
  if (ns > 4) {
    auto opts_f = q.options().dtype(at::kFloat);
    part_o = torch::empty({B, QH, ns, D}, opts_f);
    part_ml = torch::empty({B, QH, ns, 2}, opts_f);
    po = part_o.data_ptr<float>();
    pml = part_ml.data_ptr<float>();
  }
  qsa_paged_attn_mfma_fused_launch(
      u16(q), u16(k), u16(v), u16m(kc), u16m(vc), cos_t.data_ptr<float>(),
      sin_t.data_ptr<float>(), block_table.data_ptr<int>(),
      seq_lens.data_ptr<int>(), po, pml, u16m(out), (float)scale, B, QH, KVH,
      max_pages, D, q.stride(0), k.stride(0), ns, (int)waves_per_simd,
      cur_stream());
  return out;
}

void kv_append(torch::Tensor knew, torch::Tensor vnew, torch::Tensor kc,
               torch::Tensor vc, torch::Tensor block_table,
               torch::Tensor seq_lens) {
  chk_same_gpu({{"knew", knew}, {"vnew", vnew}, {"kc", kc}, {"vc", vc},
                {"block_table", block_table}, {"seq_lens", seq_lens}});
  const int D = chk_heads(knew, "knew");
  const int B = knew.size(0), KVH = knew.size(1);
  chk_kv_rows(knew, vnew, B, KVH, D);
  chk_kv_cache(kc, vc, KVH, D);
  chk_block_table(block_table, B);
  chk_index(seq_lens, B, "seq_lens");
  if (B == 0 || KVH == 0) return;
  qsa_kv_append_launch(u16(knew), u16(vnew), u16m(kc), u16m(vc),
                       block_table.data_ptr<int>(), seq_lens.data_ptr<int>(),
                       B, KVH, D, (int)block_table.size(1), knew.stride(0),
                       cur_stream());
}

// Checks common to the two prefill bindings; `map_item` / `map_pos0` are the
// per-block (16 rows) or per-tile (32/64 rows) maps.  Returns D.
static int chk_prefill_args(const torch::Tensor& q, const torch::Tensor& kc,
                            const torch::Tensor& vc,
                            const torch::Tensor& block_table,
                            const torch::Tensor& map_item,
                            const torch::Tensor& map_pos0,
                            const torch::Tensor& item_off,
                            const torch::Tensor& item_start,
                            const torch::Tensor& item_len) {
  chk_same_gpu({{"q", q}, {"kc", kc}, {"vc", vc},
                {"block_table", block_table}, {"item map", map_item},
                {"pos0 map", map_pos0}, {"item_off", item_off},
                {"item_start", item_start}, {"item_len", item_len}});
  const int D = chk_heads(q, "q");
  chk_rows16(q, "q");
  TORCH_CHECK(kc.dim() == 5, "K cache layout [P, KVH, D/8, 64, 8]");
  const int KVH = kc.size(1);
  chk_gqa(q.size(1), KVH);
  chk_kv_cache(kc, vc, KVH, D);
  const long nb = item_len.numel();
  chk_index(item_off, nb, "item_off");
  chk_index(item_start, nb, "item_start");
  chk_index(item_len, nb, "item_len");
  chk_block_table(block_table, nb);
  chk_index(map_item, map_item.numel(), "item map");
  chk_index(map_pos0, map_item.numel(), "pos0 map");
  return D;
}

torch::Tensor paged_attn_prefill(torch::Tensor q, torch::Tensor kc,
                                 torch::Tensor vc, torch::Tensor block_table,
                                 torch::Tensor qb_item, torch::Tensor qb_pos0,
                                 torch::Tensor item_off,
                                 torch::Tensor item_start,
                                 torch::Tensor item_len, double scale,
                                 bool causal) {
  const int QB = qb_item.numel();
  const int D = chk_prefill_args(q, kc, vc, block_table, qb_item, qb_pos0,
                                 item_off, item_start, item_len);
  const int T = q.size(0), QH = q.size(1), KVH = kc.size(1);
  TORCH_CHECK(QH % 4 == 0, "QH % 4 == 0 (4 head-waves per workgroup "
              "lockstep on a shared page stream)");
  const int npmax = block_table.size(1);
  // no block, no launch: rows that no block covers read as zero
  if (QB == 0 || T == 0)
    return torch::zeros({(long long)T, (long long)QH * D}, q.options());
  auto out = torch::empty({(long long)T, (long long)QH * D}, q.options());
  qsa_paged_attn_prefill_launch(
      u16(q), u16(kc), u16(vc), block_table.data_ptr<int>(),
      qb_item.data_ptr<int>(), qb_pos0.data_ptr<int>(),
      item_off.data_ptr<int>(), item_start.data_ptr<int>(),
      item_len.data_ptr<int>(), u16m(out), (float)scale, QB, QH, KVH, npmax,
      D, q.stride(0), causal ? 1 : 0, cur_stream());
  return out;
}

// Tiled prefill attention: tile maps at `rows` (32/64) q-row granularity.
// Shapes the tiled kernel does not cover (GQA ratio not a multiple of 4)
// run the one-wave-per-block kernel on 16-row maps expanded from the tiles;
// a 16-row block that starts past its item's end masks every column and
// stores nothing.
torch::Tensor paged_attn_prefill_tiled(
    torch::Tensor q, torch::Tensor kc, torch::Tensor vc,
    torch::Tensor block_table, torch::Tensor tile_item,
    torch::Tensor tile_pos0, torch::Tensor item_off, torch::Tensor item_start,
    torch::Tensor item_len, double scale, bool causal, long rows) {
  const int NT = tile_item.numel();
  const int D = chk_prefill_args(q, kc, vc, block_table, tile_item, tile_pos0,
                                 item_off, item_start, item_len);
  const int T = q.size(0), QH = q.size(1), KVH = kc.size(1);
  TORCH_CHECK(rows == 32 || (rows == 64 && D == 64),
              "rows must be 32 (or 64 at D == 64)");
  const int npmax = block_table.size(1);
  // no tile, no launch, on the tiled path and on the fallback alike
  if (NT == 0 || T == 0)
    return torch::zeros({(long long)T, (long long)QH * D}, q.options());
  auto out = torch::empty({(long long)T, (long long)QH * D}, q.options());
  const int done = qsa_paged_attn_prefill_tiled_launch(
      u16(q), u16(kc), u16(vc), block_table.data_ptr<int>(),
      tile_item.data_ptr<int>(), tile_pos0.data_ptr<int>(),
      item_off.data_ptr<int>(), item_start.data_ptr<int>(),
      item_len.data_ptr<int>(), u16m(out), (float)scale, NT, QH, KVH, npmax,
      D, q.stride(0), causal ? 1 : 0, (int)rows, cur_stream());
  if (done) return out;
  const long sub = rows / 16;
  auto qb_item = tile_item.repeat_interleave(sub).contiguous();
  auto step = torch::arange(sub, tile_pos0.options()) * 16;
  auto qb_pos0 = (tile_pos0.unsqueeze(1) + step.unsqueeze(0))
                     .reshape({-1}).contiguous();
  return paged_attn_prefill(q, kc, vc, block_table, qb_item, qb_pos0,
                            item_off, item_start, item_len, scale, causal);
}

// Fused prefill rope + KV scatter: q [Tq, QH, D] rotated in place over all
// rows; the first T = slots.numel() rows of k (rotated) and v go straight
// into the paged cache.  k itself is left untouched.
void rope_kv_scatter(torch::Tensor q, torch::Tensor k, torch::Tensor v,
                     torch::Tensor kc, torch::Tensor vc, torch::Tensor cos_t,
                     torch::Tensor sin_t, torch::Tensor pos,
                     torch::Tensor slots) {
  chk_same_gpu({{"q", q}, {"k", k}, {"v", v}, {"kc", kc}, {"vc", vc},
                {"cos_t", cos_t}, {"sin_t", sin_t}, {"pos", pos},
                {"slots", slots}});
  const int D = chk_heads(q, "q");
  const int Tq = q.size(0), QH = q.size(1);
  TORCH_CHECK(k.dim() == 3 && v.dim() == 3 && k.size(0) == v.size(0),
              "k/v must be [rows, KVH, D]");
  const int KVH = k.size(1);
  const int T = slots.numel();
  chk_kv_rows(k, v, k.size(0), KVH, D);
  chk_index(pos, Tq, "pos");
  chk_index(slots, T, "slots");
  TORCH_CHECK(T <= Tq && T <= k.size(0), "slots longer than q/k/v");
  chk_kv_cache(kc, vc, KVH, D);
  chk_rope_tables(cos_t, sin_t, D);
  // 16-byte loads of q, k and v rows
  chk_rows16(q, "q"); chk_rows16(k, "k"); chk_rows16(v, "v");
  if (Tq == 0) return;
  qsa_rope_kv_scatter_launch(u16m(q), u16(k), u16(v), u16m(kc), u16m(vc),
                             cos_t.data_ptr<float>(), sin_t.data_ptr<float>(),
                             pos.data_ptr<int>(), slots.data_ptr<int>(), Tq, T,
                             QH, KVH, D, q.stride(0), k.stride(0),
                             cur_stream());
}

void rope_kv_append(torch::Tensor q, torch::Tensor k, torch::Tensor v,
                    torch::Tensor kc, torch::Tensor vc, torch::Tensor cos_t,
                    torch::Tensor sin_t, torch::Tensor block_table,
                    torch::Tensor seq_lens) {
  chk_same_gpu({{"q", q}, {"k", k}, {"v", v}, {"kc", kc}, {"vc", vc},
                {"cos_t", cos_t}, {"sin_t", sin_t},
                {"block_table", block_table}, {"seq_lens", seq_lens}});
  const int D = chk_heads(q, "q");
  const int B = q.size(0), QH = q.size(1);
  TORCH_CHECK(k.dim() == 3, "k/v must be [rows, KVH, D]");
  const int KVH = k.size(1);
  chk_kv_rows(k, v, B, KVH, D);
  chk_kv_cache(kc, vc, KVH, D);
  chk_rope_tables(cos_t, sin_t, D);
  chk_block_table(block_table, B);
  chk_index(seq_lens, B, "seq_lens");
  if (B == 0 || QH + KVH == 0) return;
  qsa_rope_kv_append_launch(u16m(q), u16(k), u16(v), u16m(kc), u16m(vc),
                            cos_t.data_ptr<float>(), sin_t.data_ptr<float>(),
                            block_table.data_ptr<int>(),
                            seq_lens.data_ptr<int>(), B, QH, KVH, D,
                            (int)block_table.size(1), q.stride(0),
                            k.stride(0), cur_stream());
}

void kv_scatter(torch::Tensor knew, torch::Tensor vnew, torch::Tensor kc,
                torch::Tensor vc, torch::Tensor slots) {
  chk_same_gpu({{"knew", knew}, {"vnew", vnew}, {"kc", kc}, {"vc", vc},
                {"slots", slots}});
  const int D = chk_heads(knew, "knew");
  const int T = knew.size(0), KVH = knew.size(1);
  chk_kv_rows(knew, vnew, T, KVH, D);
  chk_kv_cache(kc, vc, KVH, D);
  chk_index(slots, T, "slots");
  if (T == 0 || KVH == 0) return;
  qsa_kv_scatter_launch(u16(knew), u16(vnew), u16m(kc), u16m(vc),
                        slots.data_ptr<int>(), T, KVH, D, knew.stride(0),
                        cur_stream());
}

torch::Tensor pack_weight_frag(torch::Tensor w) {
  // [N, K] bf16 -> MFMA-fragment-major [N/16, K/32, 16, 32] for the
  // skinny-GEMM weight stream (one wave reads one contiguous 1 KiB block).
  CHK_BF16(w); CHK_CONT(w);
  const long long N = w.size(0), K = w.size(1);
  TORCH_CHECK(N % 16 == 0 && K % 32 == 0, "pack needs N%16==0, K%32==0");
  return w.reshape({N / 16, 16, K / 32, 32})
      .permute({0, 2, 1, 3}).contiguous();
}

// ---- weight-streaming GEMMs: checks shared by the six bindings -------------
// Activations a[M,K] of `op`, M in [1, max_m]; the kernels load 16 B from
// A + row * lda + k (k % 8 == 0).  Returns M.
static int chk_gemm_a(const torch::Tensor& a, long K, long max_m,
                      const char* op) {
  CHK_DEV(a); CHK_BF16(a);
  TORCH_CHECK(a.dim() == 2 && a.stride(1) == 1, "a rows must be contiguous");
  TORCH_CHECK(a.stride(0) % 8 == 0 &&
              reinterpret_cast<uintptr_t>(a.data_ptr()) % 16 == 0,
              op, ": a rows must be 16-byte aligned");
  const long M = a.size(0);
  TORCH_CHECK(M >= 1 && M <= max_m, op, ": M in [1,", max_m, "]");
  TORCH_CHECK(a.size(1) == K, "K mismatch");
  return (int)M;
}

// A skinny launch with `tiles` 16-column n-tiles per workgroup: checks a and
// the shape, returns the [M, N] output.
static torch::Tensor skinny_out(const torch::Tensor& a, long N, long K,
                                long tiles, long max_m, const char* op) {
  const int M = chk_gemm_a(a, K, max_m, op);
  TORCH_CHECK(K % 256 == 0 && N % 16 == 0, "K%256==0, N%16==0");
  TORCH_CHECK(tiles >= 1 && N % (16 * tiles) == 0, "N%(16*tiles)==0");
  return torch::empty({M, (long long)N}, a.options());
}

static void chk_bf16_stream(const torch::Tensor& wf, long N, long K) {
  CHK_DEV(wf); CHK_BF16(wf); CHK_CONT(wf);
  TORCH_CHECK(wf.numel() == (long long)N * K, "wf size");
}

// fp8 e4m3 stream (layout: gemm_core.h) and its per-channel scales.
static void chk_fp8_stream(const torch::Tensor& qf,
                           const torch::Tensor& scale, long N, long K) {
  CHK_DEV(qf); CHK_CONT(qf);
  TORCH_CHECK(qf.scalar_type() == torch::kUInt8, "qf must be uint8 (fp8)");
  TORCH_CHECK(scale.scalar_type() == torch::kFloat32 && scale.is_cuda() &&
                  scale.is_contiguous() && scale.numel() == N,
              "scale must be f32 [N] on device");
  TORCH_CHECK(qf.numel() == (long long)N * K, "qf size");
}

torch::Tensor skinny_gemm(torch::Tensor a, torch::Tensor wf, long N, long K) {
  // C[M,N] = a[M,K] @ W^T with W pre-packed by pack_weight_frag.
  auto out = skinny_out(a, N, K, 1, 32, "skinny_gemm");
  chk_bf16_stream(wf, N, K);
  qsa_skinny_gemm_launch(u16(a), u16(wf), u16m(out), (int)a.size(0), (int)N,
                         K, a.stride(0), cur_stream());
  return out;
}

torch::Tensor skinny_gemm_probe(torch::Tensor a, torch::Tensor wf, long N,
                                long K, long waves, long nt, long variant) {
  auto out = skinny_out(a, N, K, 1, 32, "skinny_gemm_probe");
  chk_bf16_stream(wf, N, K);
  const int ok = qsa_skinny_gemm_probe_launch(
      u16(a), u16(wf), u16m(out), (int)a.size(0), (int)N, K, a.stride(0),
      (int)waves, (int)nt, (int)variant, cur_stream());
  TORCH_CHECK(ok, "skinny_gemm_probe: (waves, nt, variant) not instantiated");
  return out;
}

// C[M,N] = a @ (scale[N] * dequant(Q))^T through one fp8 skinny
// configuration; an error when it is not instantiated.
static torch::Tensor skinny_fp8_config(torch::Tensor a, torch::Tensor qf,
                                       torch::Tensor scale, long N, long K,
                                       long waves, long tiles, long nt,
                                       long mt, const char* op) {
  TORCH_CHECK(mt >= 1 && mt <= 4, op, ": mt in [1,4]");
  auto out = skinny_out(a, N, K, tiles, 16 * mt, op);
  chk_fp8_stream(qf, scale, N, K);
  const int ok = qsa_skinny_gemm_fp8_config_launch(
      u16(a), qf.data_ptr<unsigned char>(), scale.data_ptr<float>(),
      u16m(out), (int)a.size(0), (int)N, K, a.stride(0), (int)waves,
      (int)tiles, (int)nt, (int)mt, cur_stream());
  TORCH_CHECK(ok, op, ": (waves, tiles, nt, mt) not instantiated");
  return out;
}

torch::Tensor skinny_gemm_fp8(torch::Tensor a, torch::Tensor qf,
                              torch::Tensor scale, long N, long K) {
  auto out = skinny_out(a, N, K, 1, 64, "skinny_gemm_fp8");
  chk_fp8_stream(qf, scale, N, K);
  qsa_skinny_gemm_fp8_launch(u16(a), qf.data_ptr<unsigned char>(),
                             scale.data_ptr<float>(), u16m(out),
                             (int)a.size(0), (int)N, K, a.stride(0),
                             cur_stream());
  return out;
}

torch::Tensor skinny_gemm_fp8_probe(torch::Tensor a, torch::Tensor qf,
                                    torch::Tensor scale, long N, long K,
                                    long waves, long tiles, long nt) {
  return skinny_fp8_config(a, qf, scale, N, K, waves, tiles, nt, 2,
                           "skinny_gemm_fp8_probe");
}

torch::Tensor skinny_gemm_fp8_probe_mt(torch::Tensor a, torch::Tensor qf,
                                       torch::Tensor scale, long N, long K,
                                       long waves, long tiles, long mt) {
  return skinny_fp8_config(a, qf, scale, N, K, waves, tiles, 0, mt,
                           "skinny_gemm_fp8_probe_mt");
}

torch::Tensor gemm_fp8_batch(torch::Tensor a, torch::Tensor qf,
                             torch::Tensor scale, long N, long K,
                             long splitk) {
  // C[M,N] = a @ (scale * dequant(Q))^T for decode batches 32 < M <= 256
  const int M = chk_gemm_a(a, K, 256, "gemm_fp8_batch");
  TORCH_CHECK(N % 64 == 0, "N % 64 == 0");
  TORCH_CHECK(splitk == 1 || splitk == 2 || splitk == 4, "splitk 1/2/4");
  TORCH_CHECK(K % (64 * splitk) == 0, "K % (64*splitk) == 0");
  chk_fp8_stream(qf, scale, N, K);
  auto out = torch::empty({(long long)M, (long long)N}, a.options());
  torch::Tensor ws;
  float* wsp = nullptr;
  if (splitk > 1) {
    ws = torch::empty({splitk, (long long)M, (long long)N},
                      a.options().dtype(torch::kFloat32));
    wsp = ws.data_ptr<float>();
  }
  qsa_gemm_fp8_batch_launch(u16(a), qf.data_ptr<unsigned char>(),
                            scale.data_ptr<float>(), u16m(out), wsp, M,
                            (int)N, K, a.stride(0), (int)splitk,
                            cur_stream());
  return out;
}

// ---- routed MoE decode FFN (moe.hip) ----------------------------------------
// Limits: T <= 64 rows, E <= 16 experts, top-k <= 4; cap (rows per expert)
// is 32 at T <= 32, else 64.

static bool aligned16(const torch::Tensor& t) {
  return reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0;
}

// counts [E] i32 on the device; returns E.
static int chk_moe_counts(const torch::Tensor& counts, long E) {
  CHK_DEV(counts); CHK_I32(counts); CHK_CONT(counts);
  TORCH_CHECK(counts.dim() == 1 && counts.numel() == E, "counts must be [E]");
  TORCH_CHECK(E >= 1 && E <= 16, "moe: E in [1,16]");
  return (int)E;
}

// A grouped activation buffer [E, cap, cols] bf16, cap 32 or 64.
static void chk_moe_rows(const torch::Tensor& x, const char* name) {
  CHK_DEV(x); CHK_BF16(x); CHK_CONT(x);
  TORCH_CHECK(x.dim() == 3, name, " must be [E, cap, cols]");
  TORCH_CHECK(x.size(1) == 32 || x.size(1) == 64, name, ": cap must be 32/64");
  TORCH_CHECK(x.size(2) % 8 == 0 && aligned16(x), name,
              " rows must be 16-byte aligned");
}

// top_idx [T,k] i64 (as torch.topk returns it), T <= 64, k <= 4.
static void chk_moe_top_idx(const torch::Tensor& top_idx, long T) {
  CHK_DEV(top_idx); CHK_CONT(top_idx);
  TORCH_CHECK(top_idx.scalar_type() == at::kLong && top_idx.dim() == 2 &&
                  top_idx.size(0) == T, "top_idx must be i64 [T, k]");
  TORCH_CHECK(T >= 1 && T <= 64, "moe: T in [1,64]");
  TORCH_CHECK(top_idx.size(1) >= 1 && top_idx.size(1) <= 4,
              "moe: top-k in [1,4]");
}

// h [T,H] -> (counts [E], slot [T,k], xg [E,cap,H]): slot is the row's slot
// inside its expert, ascending by row index, -1 for a dead row.  Rows of xg
// at or past counts[e] are left unwritten.  A row's k experts must be
// distinct (not checked).
std::vector<torch::Tensor> moe_dispatch(torch::Tensor h, torch::Tensor top_idx,
                                        long n_experts,
                                        c10::optional<torch::Tensor> row_live) {
  CHK_DEV(h); CHK_BF16(h); CHK_CONT(h);
  TORCH_CHECK(h.dim() == 2, "h must be [T, H]");
  const long T = h.size(0), H = h.size(1);
  chk_moe_top_idx(top_idx, T);
  TORCH_CHECK(n_experts >= 1 && n_experts <= 16, "moe: E in [1,16]");
  TORCH_CHECK(H % 8 == 0 && aligned16(h), "h rows must be 16-byte aligned");
  const int k = top_idx.size(1);
  const int* live = nullptr;
  if (row_live.has_value()) {
    const auto& rl = row_live.value();
    CHK_DEV(rl); CHK_I32(rl); CHK_CONT(rl);
    TORCH_CHECK(rl.numel() == T, "row_live must be [T]");
    live = rl.data_ptr<int>();
  }
  const long cap = T <= 32 ? 32 : 64;
  auto opts_i = h.options().dtype(at::kInt);
  auto counts = torch::empty({n_experts}, opts_i);
  auto slot = torch::empty({T, (long)k}, opts_i);
  auto xg = torch::empty({n_experts, cap, H}, h.options());
  qsa_moe_dispatch_launch(
      u16(h), reinterpret_cast<const long long*>(top_idx.data_ptr<int64_t>()),
      live, counts.data_ptr<int>(), slot.data_ptr<int>(), u16m(xg), (int)T,
      (int)H, (int)n_experts, k, (int)cap, cur_stream());
  return {counts, slot, xg};
}

// out[e, :counts[e]] = xg[e, :counts[e]] @ W_e^T on the stacked bf16 fragment
// stream wf [E, ...]; experts with no rows are not read.  Rows at or past
// counts[e] of the [E, cap, N] result are left unwritten.
torch::Tensor moe_skinny_gemm(torch::Tensor xg, torch::Tensor counts,
                              torch::Tensor wf, long N, long K) {
  chk_moe_rows(xg, "xg");
  const int E = chk_moe_counts(counts, xg.size(0));
  TORCH_CHECK(xg.size(2) == K, "K mismatch");
  TORCH_CHECK(K % 256 == 0 && N % 16 == 0, "K%256==0, N%16==0");
  CHK_DEV(wf); CHK_BF16(wf); CHK_CONT(wf);
  TORCH_CHECK(wf.size(0) == E && wf.numel() == (long long)E * N * K,
              "wf must be the [E, ...] stack of N*K streams");
  auto out = torch::empty({(long)E, xg.size(1), N}, xg.options());
  qsa_moe_skinny_gemm_bf16_launch(u16(xg), u16(wf), u16m(out),
                                  counts.data_ptr<int>(), E, (int)xg.size(1),
                                  (int)N, K, cur_stream());
  return out;
}

torch::Tensor moe_skinny_gemm_fp8(torch::Tensor xg, torch::Tensor counts,
                                  torch::Tensor qf, torch::Tensor scale,
                                  long N, long K) {
  chk_moe_rows(xg, "xg");
  const int E = chk_moe_counts(counts, xg.size(0));
  TORCH_CHECK(xg.size(2) == K, "K mismatch");
  TORCH_CHECK(K % 256 == 0 && N % 16 == 0, "K%256==0, N%16==0");
  CHK_DEV(qf); CHK_CONT(qf);
  TORCH_CHECK(qf.scalar_type() == torch::kUInt8, "qf must be uint8 (fp8)");
  TORCH_CHECK(qf.size(0) == E && qf.numel() == (long long)E * N * K,
              "qf must be the [E, ...] stack of N*K streams");
  TORCH_CHECK(scale.scalar_type() == torch::kFloat32 && scale.is_cuda() &&
                  scale.is_contiguous() && scale.dim() == 2 &&
                  scale.size(0) == E && scale.size(1) == N,
              "scale must be f32 [E, N] on device");
  // the launcher's tiles (4 wgu, 2 qkv, else 1) divide N/16 by the class rule
  const std::string cls = qsa_skinny_fp8_class((int)N, K);
  const long tiles = cls == "wgu" ? 4 : cls == "qkv" ? 2 : 1;
  TORCH_CHECK(N % (16 * tiles) == 0, "N%(16*tiles)==0");
  auto out = torch::empty({(long)E, xg.size(1), N}, xg.options());
  const int ok = qsa_moe_skinny_gemm_fp8_launch(
      u16(xg), qf.data_ptr<unsigned char>(), scale.data_ptr<float>(),
      u16m(out), counts.data_ptr<int>(), E, (int)xg.size(1), (int)N, K,
      cur_stream());
  TORCH_CHECK(ok, "moe_skinny_gemm_fp8: the lm_head shape class (N >= 65536) "
              "is not supported");
  return out;
}

// act[e, r, :] = silu(gu[e, r, :F]) * gu[e, r, F:] for r < counts[e].
torch::Tensor moe_swiglu(torch::Tensor gu, torch::Tensor counts) {
  chk_moe_rows(gu, "gu");
  const int E = chk_moe_counts(counts, gu.size(0));
  TORCH_CHECK(gu.size(2) % 16 == 0, "gu cols (2F) % 16 == 0");
  const long F = gu.size(2) / 2;
  auto act = torch::empty({(long)E, gu.size(1), F}, gu.options());
  qsa_moe_swiglu_launch(u16(gu), u16m(act), counts.data_ptr<int>(), E,
                        (int)gu.size(1), F, cur_stream());
  return act;
}

// out[t, :] = sum over row t's picks of top_w * y[top_idx, slot], ascending
// expert index, f32 with separately rounded multiply and add, one rounding
// to bf16.  Dead rows give zeros.
torch::Tensor moe_combine(torch::Tensor y, torch::Tensor slot,
                          torch::Tensor top_idx, torch::Tensor top_w) {
  chk_moe_rows(y, "y");
  const long E = y.size(0), H = y.size(2);
  TORCH_CHECK(E >= 1 && E <= 16, "moe: E in [1,16]");
  const long T = slot.size(0);
  chk_moe_top_idx(top_idx, T);
  CHK_DEV(slot); CHK_I32(slot); CHK_CONT(slot);
  CHK_DEV(top_w); CHK_F32(top_w); CHK_CONT(top_w);
  TORCH_CHECK(slot.sizes() == top_idx.sizes() &&
                  top_w.sizes() == top_idx.sizes(),
              "slot, top_idx and top_w must all be [T, k]");
  TORCH_CHECK(y.size(1) == (T <= 32 ? 32 : 64), "y cap does not match T");
  auto out = torch::empty({T, H}, y.options());
  qsa_moe_combine_launch(
      u16(y), slot.data_ptr<int>(),
      reinterpret_cast<const long long*>(top_idx.data_ptr<int64_t>()),
      top_w.data_ptr<float>(), u16m(out), (int)T, (int)H, (int)E,
      (int)top_idx.size(1), (int)y.size(1), cur_stream());
  return out;
}

std::vector<torch::Tensor> hash_build(torch::Tensor keys,
                                      torch::Tensor ts) {
  // latest-event-time-per-key hash table in HBM (K8 streaming join state)
  CHK_DEV(keys);
  TORCH_CHECK(keys.scalar_type() == torch::kInt64 && keys.is_contiguous(),
              "keys must be contiguous i64");
  TORCH_CHECK(ts.scalar_type() == torch::kInt64 && ts.is_contiguous() &&
                  ts.numel() == keys.numel(), "ts must be i64 like keys");
  const long long n = keys.numel();
  TORCH_CHECK(n < (1 << 24), "hash_build: <= 2^24 rows per batch");
  long long cap = 64;
  while (cap < 2 * n) cap <<= 1;
  auto opts = keys.options();
  auto tkeys = torch::full({cap}, -1, opts);   // all-ones bits == EMPTY
  auto tpay = torch::zeros({cap}, opts);
  qsa_hash_build_launch((const long long*)keys.data_ptr<int64_t>(),
                        (const long long*)ts.data_ptr<int64_t>(),
                        (unsigned long long*)tkeys.data_ptr<int64_t>(),
                        (unsigned long long*)tpay.data_ptr<int64_t>(),
                        (int)n, (unsigned int)(cap - 1), cur_stream());
  return {tkeys, tpay};
}

torch::Tensor hash_probe(torch::Tensor tkeys, torch::Tensor tpay,
                         torch::Tensor keys, long long min_ts) {
  CHK_DEV(keys);
  TORCH_CHECK(keys.scalar_type() == torch::kInt64 && keys.is_contiguous(),
              "keys must be contiguous i64");
  const long long m = keys.numel();
  const long long cap = tkeys.numel();
  TORCH_CHECK((cap & (cap - 1)) == 0, "table capacity must be pow2");
  auto out = torch::empty({m}, keys.options().dtype(torch::kInt32));
  qsa_hash_probe_launch((const long long*)keys.data_ptr<int64_t>(),
                        (const unsigned long long*)tkeys.data_ptr<int64_t>(),
                        (const unsigned long long*)tpay.data_ptr<int64_t>(),
                        out.data_ptr<int>(), (int)m,
                        (unsigned int)(cap - 1), min_ts, cur_stream());
  return out;
}

void greedy_sample_step(torch::Tensor logits, long lo, long hi, long eos,
                        torch::Tensor script, torch::Tensor script_mask,
                        torch::Tensor ctr, torch::Tensor hist,
                        torch::Tensor tokens, torch::Tensor ticket) {
  // One decode step's greedy sampling + bookkeeping in one launch
  // (elementwise.hip): tokens/hist/ctr are updated in place.
  CHK_DEV(logits); CHK_CONT(logits); CHK_BF16(logits);
  CHK_DEV(script); CHK_CONT(script); CHK_DEV(script_mask);
  CHK_CONT(script_mask); CHK_DEV(ctr); CHK_DEV(hist); CHK_DEV(tokens);
  CHK_CONT(tokens); CHK_DEV(ticket);
  TORCH_CHECK(logits.dim() == 2, "logits [B, V]");
  const long long B = logits.size(0), V = logits.size(1);
  TORCH_CHECK(0 <= lo && lo <= hi && hi <= V, "0 <= lo <= hi <= V");
  TORCH_CHECK(eos < V, "eos < V");
  TORCH_CHECK(script.scalar_type() == at::kLong && script.dim() == 2 &&
                  script.size(0) >= B, "script i64 [>=B, max_run]");
  TORCH_CHECK(script_mask.scalar_type() == at::kBool &&
                  script_mask.sizes() == script.sizes(),
              "script_mask bool, same shape as script");
  TORCH_CHECK(script.size(1) >= 1, "max_run >= 1");
  TORCH_CHECK(ctr.scalar_type() == at::kLong && ctr.numel() == 1, "ctr i64 [1]");
  TORCH_CHECK(hist.scalar_type() == at::kLong && hist.dim() == 2 &&
                  hist.size(1) >= B && hist.stride(1) == 1,
              "hist i64 [rows, >=B], unit column stride");
  TORCH_CHECK(tokens.scalar_type() == at::kLong && tokens.numel() >= B,
              "tokens i64 [>=B]");
  TORCH_CHECK(ticket.scalar_type() == at::kInt && ticket.numel() == 1,
              "ticket i32 [1]");
  if (B == 0) return;
  qsa_greedy_sample_launch(
      u16(logits), (int)B, V, (int)lo, (int)hi, eos < 0 ? -1 : (int)eos,
      reinterpret_cast<const long long*>(script.data_ptr<int64_t>()),
      reinterpret_cast<const unsigned char*>(script_mask.data_ptr<bool>()),
      (int)script.size(1),
      reinterpret_cast<long long*>(ctr.data_ptr<int64_t>()),
      reinterpret_cast<long long*>(hist.data_ptr<int64_t>()), hist.stride(0),
      (int)hist.size(0),
      reinterpret_cast<long long*>(tokens.data_ptr<int64_t>()),
      reinterpret_cast<unsigned int*>(ticket.data_ptr<int>()), cur_stream());
}

// Checks shared by sample_step and sample_tokens (sampling.hip): the logits,
// the window and the per-row parameter buffers, each of at least B rows.
static void check_sample_rows(const torch::Tensor& logits, long lo, long hi,
                              long eos, const torch::Tensor& inv_temp,
                              const torch::Tensor& top_k,
                              const torch::Tensor& top_p_q,
                              const torch::Tensor& seed,
                              const torch::Tensor& pos) {
  CHK_DEV(logits); CHK_CONT(logits); CHK_BF16(logits);
  TORCH_CHECK(logits.dim() == 2, "logits [B, V]");
  const long long B = logits.size(0), V = logits.size(1);
  TORCH_CHECK(0 <= lo && lo <= hi && hi <= V, "0 <= lo <= hi <= V");
  TORCH_CHECK(eos < V, "eos < V");
  // the kernel keeps one LDS total per 2048 candidates, 2048 of them (two
  // go to the window's unaligned ends); at 2^40 per candidate the weight
  // totals stay far inside 64 bits
  TORCH_CHECK(V <= 2046LL * 2048, "V <= 2046 * 2048");
  CHK_DEV(inv_temp); CHK_CONT(inv_temp); CHK_F32(inv_temp);
  CHK_DEV(top_k); CHK_CONT(top_k); CHK_I32(top_k);
  CHK_DEV(top_p_q); CHK_CONT(top_p_q); CHK_I32(top_p_q);
  CHK_DEV(seed); CHK_CONT(seed);
  TORCH_CHECK(seed.scalar_type() == at::kLong, "seed must be i64");
  CHK_DEV(pos); CHK_CONT(pos); CHK_I32(pos);
  TORCH_CHECK(inv_temp.dim() == 1 && inv_temp.numel() >= B &&
                  top_k.dim() == 1 && top_k.numel() >= B &&
                  top_p_q.dim() == 1 && top_p_q.numel() >= B &&
                  seed.dim() == 1 && seed.numel() >= B && pos.dim() == 1 &&
                  pos.numel() >= B,
              "inv_temp / top_k / top_p_q / seed / pos: 1-D, >= B rows");
}

void sample_step(torch::Tensor logits, long lo, long hi, long eos,
                 torch::Tensor inv_temp, torch::Tensor top_k,
                 torch::Tensor top_p_q, torch::Tensor seed, torch::Tensor pos,
                 torch::Tensor script, torch::Tensor script_mask,
                 torch::Tensor ctr, torch::Tensor hist, torch::Tensor tokens,
                 torch::Tensor ticket) {
  // One decode step's per-request sampling + bookkeeping in one launch
  // (sampling.hip): tokens/hist/ctr are updated in place.
  check_sample_rows(logits, lo, hi, eos, inv_temp, top_k, top_p_q, seed, pos);
  CHK_DEV(script); CHK_CONT(script); CHK_DEV(script_mask);
  CHK_CONT(script_mask); CHK_DEV(ctr); CHK_DEV(hist); CHK_DEV(tokens);
  CHK_CONT(tokens); CHK_DEV(ticket);
  const long long B = logits.size(0), V = logits.size(1);
  TORCH_CHECK(script.scalar_type() == at::kLong && script.dim() == 2 &&
                  script.size(0) >= B, "script i64 [>=B, max_run]");
  TORCH_CHECK(script_mask.scalar_type() == at::kBool &&
                  script_mask.sizes() == script.sizes(),
              "script_mask bool, same shape as script");
  TORCH_CHECK(script.size(1) >= 1, "max_run >= 1");
  TORCH_CHECK(ctr.scalar_type() == at::kLong && ctr.numel() == 1, "ctr i64 [1]");
  TORCH_CHECK(hist.scalar_type() == at::kLong && hist.dim() == 2 &&
                  hist.size(1) >= B && hist.stride(1) == 1,
              "hist i64 [rows, >=B], unit column stride");
  TORCH_CHECK(tokens.scalar_type() == at::kLong && tokens.numel() >= B,
              "tokens i64 [>=B]");
  TORCH_CHECK(ticket.scalar_type() == at::kInt && ticket.numel() == 1,
              "ticket i32 [1]");
  if (B == 0) return;
  qsa_sample_launch(
      u16(logits), (int)B, V, (int)lo, (int)hi, eos < 0 ? -1 : (int)eos,
      inv_temp.data_ptr<float>(), top_k.data_ptr<int>(),
      top_p_q.data_ptr<int>(),
      reinterpret_cast<const long long*>(seed.data_ptr<int64_t>()),
      pos.data_ptr<int>(),
      reinterpret_cast<const long long*>(script.data_ptr<int64_t>()),
      reinterpret_cast<const unsigned char*>(script_mask.data_ptr<bool>()),
      (int)script.size(1),
      reinterpret_cast<long long*>(ctr.data_ptr<int64_t>()),
      reinterpret_cast<long long*>(hist.data_ptr<int64_t>()), hist.stride(0),
      (int)hist.size(0),
      reinterpret_cast<long long*>(tokens.data_ptr<int64_t>()),
      reinterpret_cast<unsigned int*>(ticket.data_ptr<int>()), cur_stream());
}

torch::Tensor sample_tokens(torch::Tensor logits, long lo, long hi, long eos,
                            torch::Tensor inv_temp, torch::Tensor top_k,
                            torch::Tensor top_p_q, torch::Tensor seed,
                            torch::Tensor pos) {
  // The draw of sample_step alone: no script, history or counter.
  check_sample_rows(logits, lo, hi, eos, inv_temp, top_k, top_p_q, seed, pos);
  const long long B = logits.size(0), V = logits.size(1);
  auto tokens = torch::empty({B}, logits.options().dtype(torch::kInt64));
  if (B == 0) return tokens;
  qsa_sample_launch(
      u16(logits), (int)B, V, (int)lo, (int)hi, eos < 0 ? -1 : (int)eos,
      inv_temp.data_ptr<float>(), top_k.data_ptr<int>(),
      top_p_q.data_ptr<int>(),
      reinterpret_cast<const long long*>(seed.data_ptr<int64_t>()),
      pos.data_ptr<int>(), nullptr, nullptr, 1, nullptr, nullptr, 0, 0,
      reinterpret_cast<long long*>(tokens.data_ptr<int64_t>()), nullptr,
      cur_stream());
  return tokens;
}

std::vector<torch::Tensor> topk_cosine(torch::Tensor queries,
                                       torch::Tensor docs, long k) {
  CHK_DEV(queries); CHK_CONT(queries); CHK_F32(queries); CHK_F32(docs);
  CHK_CONT(docs);
  const int Q = queries.size(0), D = queries.size(1), N = docs.size(0);
  TORCH_CHECK(docs.size(1) == D, "dim mismatch");
  TORCH_CHECK(k >= 1 && k <= 16, "k in [1,16]");
  TORCH_CHECK(k <= N, "topk_cosine: k must not exceed the number of docs");
  const int nblk = std::max(1, (N + 2047) / 2048);
  auto opts_f = queries.options();
  auto opts_i = queries.options().dtype(at::kInt);
  auto cand_s = torch::empty({Q, nblk, k}, opts_f);
  auto cand_i = torch::empty({Q, nblk, k}, opts_i);
  auto out_s = torch::empty({Q, k}, opts_f);
  auto out_i = torch::empty({Q, k}, opts_i);
  qsa_topk_launch(queries.data_ptr<float>(), docs.data_ptr<float>(),
                  cand_s.data_ptr<float>(), cand_i.data_ptr<int>(),
                  out_s.data_ptr<float>(), out_i.data_ptr<int>(), Q, N, D,
                  (int)k, nblk, cur_stream());
  return {out_s, out_i};
}

std::vector<torch::Tensor> window_agg(torch::Tensor ts, torch::Tensor key,
                                      c10::optional<torch::Tensor> value,
                                      long t0, long win_ms, long nwin,
                                      long nkeys) {
  CHK_DEV(ts); CHK_CONT(ts); CHK_I32(key);
  TORCH_CHECK(ts.scalar_type() == at::kLong, "ts must be i64");
  const long long n = ts.numel();
  TORCH_CHECK(win_ms > 0, "window_agg: win_ms > 0");
  TORCH_CHECK(nwin >= 1, "window_agg: nwin >= 1");
  TORCH_CHECK(key.numel() == n, "window_agg: one key per event");
  TORCH_CHECK(!value.has_value() || value.value().numel() == n,
              "window_agg: one value per event");
  auto counts = torch::zeros({nkeys, nwin}, key.options());
  auto sums = torch::zeros({nkeys, nwin}, ts.options().dtype(at::kFloat));
  const float* vptr = nullptr;
  if (value.has_value()) {
    CHK_F32(value.value());
    vptr = value.value().data_ptr<float>();
  }
  const int blocks = (int)std::min<long long>((n + 255) / 256, 4096);
  qsa_window_agg_launch(reinterpret_cast<const long long*>(ts.data_ptr<int64_t>()),
                        key.data_ptr<int>(), vptr,
                        counts.data_ptr<int>(), sums.data_ptr<float>(), t0,
                        win_ms, (int)nwin, n, std::max(blocks, 1),
                        cur_stream());
  return {counts, sums};
}

std::vector<torch::Tensor> anomaly_batch(torch::Tensor series,
                                         torch::Tensor lengths, long order) {
  CHK_DEV(series); CHK_CONT(series); CHK_F32(series); CHK_I32(lengths);
  const int K = series.size(0), Tmax = series.size(1);
  auto fc = torch::empty({K}, series.options());
  auto se = torch::empty({K}, series.options());
  auto dof = torch::empty({K}, series.options().dtype(at::kInt));
  qsa_anomaly_batch_launch(series.data_ptr<float>(), lengths.data_ptr<int>(),
                           fc.data_ptr<float>(), se.data_ptr<float>(),
                           dof.data_ptr<int>(), K, Tmax, (int)order,
                           cur_stream());
  return {fc, se, dof};
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("rmsnorm", &rmsnorm, "fused RMSNorm (bf16)");
  m.def("rmsnorm_residual", &rmsnorm_residual,
        "fused residual-add + RMSNorm (bf16; residual updated in place)");
  m.def("swiglu", &swiglu, "fused silu(gate)*up (bf16)");
  m.def("rope_inplace", &rope_inplace, "rotary embedding in place (bf16)");
  m.def("softmax_rows_bf16_", &softmax_rows_bf16_,
        "bf16 masked row softmax with folded scale (in place)");
  m.def("softmax_rows_", &softmax_rows_, "row softmax in place (f32)",
        py::arg("scores"), py::arg("col_offset") = 0, py::arg("causal") = false,
        py::arg("row_mod") = 0, py::arg("row_limits") = py::none());
  m.def("paged_attn_prefill", &paged_attn_prefill,
        "varlen flash prefill attention over the paged cache");
  m.def("paged_attn_decode", &paged_attn_decode,
        "paged-attention decode (bf16, GQA, page=64)");
  m.def("decode_attn_fused", &decode_attn_fused,
        "fused decode step: rope + kv append + paged attention + split merge",
        py::arg("q"), py::arg("k"), py::arg("v"), py::arg("kc"),
        py::arg("vc"), py::arg("cos_t"), py::arg("sin_t"),
        py::arg("block_table"), py::arg("seq_lens"), py::arg("scale"),
        py::arg("waves_per_simd") = 2);
  m.def("kv_append", &kv_append, "append one step's k/v to the paged cache");
  m.def("paged_attn_prefill_tiled", &paged_attn_prefill_tiled,
        "varlen flash prefill attention, K/V pages shared through LDS");
  m.def("rope_kv_scatter", &rope_kv_scatter,
        "fused prefill rope + paged-cache scatter");
  m.def("rope_kv_append", &rope_kv_append,
        "fused decode rope + paged-cache append");
  m.def("kv_scatter", &kv_scatter, "scatter prefill k/v by slot ids");
  m.def("pack_weight_frag", &pack_weight_frag,
        "repack [N,K] bf16 into MFMA-fragment-major for skinny_gemm");
  m.def("skinny_gemm", &skinny_gemm,
        "decode-batch GEMM (M<=32) on the packed weight stream");
  m.def("skinny_gemm_probe", &skinny_gemm_probe,
        "ablation probe: waves/nt/variant sweep");
  m.def("skinny_gemm_fp8", &skinny_gemm_fp8,
        "fp8-weight decode GEMM (M<=32): half the weight stream");
  m.def("gemm_fp8_batch", &gemm_fp8_batch,
        "batched-M (<=256) fp8 weight-stream GEMM with optional split-K");
  m.def("skinny_gemm_fp8_probe", &skinny_gemm_fp8_probe,
        "fp8 ablation probe: waves/tiles/nt sweep");
  m.def("skinny_gemm_fp8_probe_mt", &skinny_gemm_fp8_probe_mt,
        "fp8 skinny GEMM with explicit (waves, tiles, m-tiles) for sweeps");
  m.def("skinny_fp8_class", [](long n, long k) {
    return std::string(qsa_skinny_fp8_class((int)n, k));
  }, "shape class the fp8 skinny launcher gives an [n, k] weight");
  m.def("moe_dispatch", &moe_dispatch,
        "routed MoE: per-expert counts, row slots and gathered rows",
        py::arg("h"), py::arg("top_idx"), py::arg("n_experts"),
        py::arg("row_live") = py::none());
  m.def("moe_skinny_gemm", &moe_skinny_gemm,
        "grouped skinny GEMM over routed experts (bf16 stream)");
  m.def("moe_skinny_gemm_fp8", &moe_skinny_gemm_fp8,
        "grouped skinny GEMM over routed experts (fp8 stream)");
  m.def("moe_swiglu", &moe_swiglu, "SwiGLU over the live rows of each expert");
  m.def("moe_combine", &moe_combine,
        "gate-weighted sum of a row's expert outputs (f32, no FMA)");
  m.def("greedy_sample_step", &greedy_sample_step,
        "fused greedy sampling step: windowed argmax, script override, "
        "history/token/counter update (in place)");
  m.def("sample_step", &sample_step,
        "fused per-request sampling step: seeded temperature / top-k / "
        "top-p draw, script override, history/token/counter update "
        "(in place)");
  m.def("sample_tokens", &sample_tokens,
        "the draw of sample_step alone -> tokens i64 [B]");
  m.def("topk_cosine", &topk_cosine, "exact cosine top-k over the HBM index");
  m.def("hash_build", &hash_build,
        "build latest-per-key hash table from (keys, event ts)");
  m.def("hash_probe", &hash_probe,
        "probe the hash table with TTL cutoff -> row indices or -1");
  m.def("window_agg", &window_agg, "segmented (key, window) count/sum");
  m.def("anomaly_batch", &anomaly_batch, "batched AR+ridge anomaly scorer");
  register_avro(m);
}
