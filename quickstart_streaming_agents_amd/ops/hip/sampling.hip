// Per-request seeded sampling (temperature, top-k, top-p) in one launch:
// one 256-thread workgroup per row, the bf16 row re-read from L2 per pass.
// The rule is written once, in ops/dispatch.py (sample_step); this file is
// its device form and agrees with the CPU branch there bit for bit:
//   * the weight of a logit is a fixed sequence of separately rounded f32
//     operations (no FMA contraction) ending in a 40-bit fixed-point
//     integer, a function of the bf16 logit, the row maximum and inv_temp
//     alone;
//   * everything after the weight (top-k / top-p thresholds on the 16-bit
//     order-preserving key, totals, the Philox draw, the running sum) is
//     integer arithmetic, so no reduction order can change a bit.
// Passes over the row: max/argmax; for top-k or top-p a radix select on
// the key in two 256-bin levels (LDS histograms of count and mass, both
// filled in the same pass, so top-p reuses top-k's histograms when its
// threshold falls in the same high-byte bin); a blocked final pass that
// sums the kept weights per block of 2048 candidates, which gives the total
// and hence the drawn target, and scans by candidate only the block where
// the running sum passes it.  A row with inv_temp == 0, or whose maximum is
// +inf or -inf, leaves after the max pass with the greedy kernel's token
// (elementwise.hip).  NaN logits are outside the claim, as there.  The bookkeeping
// (script override, hist, tokens, ticketed ctr += 1) is the greedy
// kernel's.
#include "common.h"

namespace {

typedef unsigned long long u64;

// LDS histogram replicas per bin: lanes of one wave that hit the same bin
// spread over this many addresses (adjacent banks).
constexpr int kCopies = 8;

// order-preserving 16-bit key of a bf16 bit pattern
__device__ __forceinline__ unsigned int sample_key(unsigned int bits) {
  return (bits & 0x8000u) ? (~bits & 0xffffu) : (bits | 0x8000u);
}

// 2^((l - m) * inv_temp * log2 e) in 40-bit fixed point (2^40 at l == m)
__device__ __forceinline__ u64 sample_weight(unsigned int bits, float m,
                                             float inv_temp) {
#pragma clang fp contract(off)
  const float d = bf16_to_f32((unsigned short)bits) - m;
  const float x = d * inv_temp;
  const float y = fmaxf(x * 0x1.715476p+0f, -64.0f);
  const float n = floorf(y + 0.5f);
  const float f = y - n;
  float p = 0x1.430912p-13f;
  p = p * f; p = p + 0x1.5d87fep-10f;
  p = p * f; p = p + 0x1.3b2ab6p-7f;
  p = p * f; p = p + 0x1.c6b08ep-5f;
  p = p * f; p = p + 0x1.ebfbe0p-3f;
  p = p * f; p = p + 0x1.62e430p-1f;
  p = p * f; p = p + 1.0f;
  const unsigned int q = (unsigned int)(p * 16777216.0f);
  const int sh = -(int)n;
  return sh <= 40 ? (((u64)q << 16) >> sh) : 0ull;
}

// Philox4x32-10, counter (pos, 0, 0, 0), key (seed lo, seed hi): x0 | x1<<32
__device__ __forceinline__ u64 sample_philox(u64 seed, unsigned int pos) {
  unsigned int c0 = pos, c1 = 0u, c2 = 0u, c3 = 0u;
  unsigned int k0 = (unsigned int)seed, k1 = (unsigned int)(seed >> 32);
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    const u64 p0 = (u64)0xD2511F53u * c0;
    const u64 p1 = (u64)0xCD9E8D57u * c2;
    const unsigned int n0 = (unsigned int)(p1 >> 32) ^ c1 ^ k0;
    const unsigned int n2 = (unsigned int)(p0 >> 32) ^ c3 ^ k1;
    c0 = n0; c1 = (unsigned int)p1; c2 = n2; c3 = (unsigned int)p0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  return (u64)c0 | ((u64)c1 << 32);
}

// f(bits, index) for every candidate, any order: the window as scalar head
// up to a 16-byte boundary, uint4 body, scalar tail; eos by thread 0
template <class F>
__device__ __forceinline__ void sample_for_candidates(
    const unsigned short* __restrict__ r, int lo, int hi, int eos, F f) {
  const int mis = (int)((reinterpret_cast<unsigned long long>(r + lo) >> 1) & 7);
  const int body0 = min(hi, lo + ((8 - mis) & 7));
  const int body1 = body0 + ((hi - body0) & ~7);
  for (int i = lo + threadIdx.x; i < body0; i += blockDim.x) f(r[i], i);
  for (int i = body0 + threadIdx.x * 8; i < body1; i += blockDim.x * 8) {
    const uint4 v4 = *reinterpret_cast<const uint4*>(r + i);
    const unsigned int vv[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      f(vv[j] & 0xffffu, i + 2 * j);
      f(vv[j] >> 16, i + 2 * j + 1);
    }
  }
  for (int i = body1 + threadIdx.x; i < hi; i += blockDim.x) f(r[i], i);
  if (threadIdx.x == 0 && eos >= 0 && (eos < lo || eos >= hi)) f(r[eos], eos);
}

__device__ __forceinline__ u64 wave_reduce_sum_u64(u64 v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, QSA_WAVE);
  return v;
}

// all threads receive the sum; scratch holds 4 values
__device__ __forceinline__ u64 block_reduce_sum_u64(u64 v, u64* scratch) {
  v = wave_reduce_sum_u64(v);
  if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = v;
  __syncthreads();
  const u64 t = scratch[0] + scratch[1] + scratch[2] + scratch[3];
  __syncthreads();
  return t;
}

// exclusive prefix of v over the block's threads; *total = the block's sum;
// scratch holds 4 values
__device__ __forceinline__ u64 block_scan_excl_u64(u64 v, u64* scratch,
                                                   u64* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  u64 incl = v;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const u64 t = __shfl_up(incl, off, QSA_WAVE);
    if (lane >= off) incl += t;
  }
  if (lane == 63) scratch[wave] = incl;
  __syncthreads();
  u64 before = incl - v;
  for (int w = 0; w < wave; ++w) before += scratch[w];
  *total = scratch[0] + scratch[1] + scratch[2] + scratch[3];
  return before;
}

// One histogram pass: count and mass per bin, over every candidate by the
// key's high byte (kLevel2 false) or over the candidates whose high byte is
// `prefix` by the low byte.  Leaves the per-bin sums in out_cnt / out_mass
// and returns the mass of all binned candidates to every thread.
template <bool kLevel2>
__device__ __forceinline__ u64 sample_hist_pass(
    const unsigned short* __restrict__ r, int lo, int hi, int eos, float m,
    float inv_temp, unsigned int prefix, unsigned int* s_cnt, u64* s_mass,
    unsigned int* out_cnt, u64* out_mass, u64* scratch) {
  for (int i = threadIdx.x; i < 256 * kCopies; i += blockDim.x) {
    s_cnt[i] = 0u;
    s_mass[i] = 0ull;
  }
  __syncthreads();
  const int cp = threadIdx.x & (kCopies - 1);
  sample_for_candidates(r, lo, hi, eos, [&](unsigned int bits, int) {
    const unsigned int key = sample_key(bits);
    if (kLevel2 && (key >> 8) != prefix) return;
    const int slot = (int)(kLevel2 ? (key & 255u) : (key >> 8)) * kCopies + cp;
    atomicAdd(&s_cnt[slot], 1u);
    const u64 w = sample_weight(bits, m, inv_temp);
    if (w) atomicAdd(&s_mass[slot], w);
  });
  __syncthreads();
  unsigned int c = 0u;
  u64 mm = 0ull;
#pragma unroll
  for (int j = 0; j < kCopies; ++j) {
    c += s_cnt[threadIdx.x * kCopies + j];
    mm += s_mass[threadIdx.x * kCopies + j];
  }
  out_cnt[threadIdx.x] = c;
  out_mass[threadIdx.x] = mm;
  return block_reduce_sum_u64(mm, scratch);     // its barriers publish out_*
}

// Largest bin b whose suffix sum (bins >= b) of count, or of mass, reaches
// thr (1 <= thr <= the sum of all bins).  sel = {b, count above b, mass
// above b}, valid for every thread on return.  Wave 0 scans the 256 bins in
// descending order, 4 per lane.
__device__ __forceinline__ void sample_select256(const unsigned int* cnt,
                                                 const u64* mass, bool by_mass,
                                                 u64 thr, u64* sel) {
  if (threadIdx.x < 64) {
    const int lane = threadIdx.x;
    u64 c[4], m[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      c[j] = cnt[255 - 4 * lane - j];
      m[j] = mass[255 - 4 * lane - j];
    }
    const u64 cs = c[0] + c[1] + c[2] + c[3];
    const u64 ms = m[0] + m[1] + m[2] + m[3];
    u64 ci = cs, mi = ms;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const u64 tc = __shfl_up(ci, off, QSA_WAVE);
      const u64 tm = __shfl_up(mi, off, QSA_WAVE);
      if (lane >= off) { ci += tc; mi += tm; }
    }
    u64 ca = ci - cs, ma = mi - ms;     // sums over the bins above mine
    if ((by_mass ? ma : ca) < thr && (by_mass ? mi : ci) >= thr) {
      bool found = false;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (!found) {
          if ((by_mass ? ma + m[j] : ca + c[j]) >= thr) {
            found = true;
            sel[0] = (u64)(255 - 4 * lane - j);
            sel[1] = ca;
            sel[2] = ma;
          }
          ca += c[j];
          ma += m[j];
        }
      }
    }
  }
  __syncthreads();
}

}  // namespace

__global__ void __launch_bounds__(256)
qsa_sample_kernel(const unsigned short* __restrict__ logits,     // [B,V]
                  long long V, int lo, int hi, int eos,
                  const float* __restrict__ inv_temp,            // [B]
                  const int* __restrict__ top_k,                 // [B]
                  const int* __restrict__ top_p_q,               // [B]
                  const long long* __restrict__ seed,            // [B]
                  const int* __restrict__ pos,                   // [B]
                  const long long* __restrict__ script,   // [B,max_run] | null
                  const unsigned char* __restrict__ script_mask,
                  int max_run,
                  long long* __restrict__ ctr,                   // [1]
                  long long* __restrict__ hist,  // [hist_rows, stride]
                  long long hist_stride, int hist_rows,
                  long long* __restrict__ tokens,                // [B]
                  unsigned int* __restrict__ ticket) {           // [1], 0
  __shared__ u64 s_mass[256 * kCopies];
  __shared__ unsigned int s_cnt[256 * kCopies];
  __shared__ u64 s_m1[256], s_m2[256];
  __shared__ unsigned int s_c1[256], s_c2[256];
  __shared__ u64 s_scan[2][4];
  __shared__ u64 s_sel[3];
  __shared__ float sv[4];
  __shared__ int si[4];
  __shared__ int s_tok;

  const int row = blockIdx.x;
  const unsigned short* r = logits + (long long)row * V;
  const float ninf = -__builtin_inff();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;

  // ---- pass 1: maximum and its lowest index, to every thread ------------
  float bv = ninf;
  int bi = 0;
  sample_for_candidates(r, lo, hi, eos, [&](unsigned int bits, int i) {
    qsa_argmax_take(bv, bi, bf16_to_f32((unsigned short)bits), i);
  });
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float ov = __shfl_xor(bv, off, QSA_WAVE);
    const int oi = __shfl_xor(bi, off, QSA_WAVE);
    qsa_argmax_take(bv, bi, ov, oi);
  }
  if (lane == 0) { sv[wave] = bv; si[wave] = bi; }
  if (threadIdx.x == 0) s_tok = -1;
  __syncthreads();
  bv = sv[0]; bi = si[0];
  for (int w = 1; w < 4; ++w) qsa_argmax_take(bv, bi, sv[w], si[w]);

  // greedy rows; 0 when every candidate is -inf; the lowest-index +inf
  // when the maximum is +inf (no weight is defined against it)
  int tok = bi;
  const float it = inv_temp[row];
  if (it != 0.f && bv != ninf && bv != -ninf) {     // block-uniform
    const float m = bv;
    const int k = top_k[row];
    const int pq = top_p_q[row];
    const bool eos_out = eos >= 0 && (eos < lo || eos >= hi);
    const int ncand = hi - lo + (eos_out ? 1 : 0);
    const bool use_k = k > 0 && k < ncand;    // top_k >= ncand keeps all
    const bool use_p = pq < 65536;
    unsigned int tau = 0u;                     // kept: key >= tau
    if (use_k || use_p) {
      // sum of the weights top-k keeps
      u64 total_k = sample_hist_pass<false>(r, lo, hi, eos, m, it, 0u, s_cnt,
                                            s_mass, s_c1, s_m1, s_scan[0]);
      unsigned int bk = 256u;                  // top-k's high-byte bin
      if (use_k) {
        sample_select256(s_c1, s_m1, false, (u64)k, s_sel);
        bk = (unsigned int)s_sel[0] & 255u;
        const u64 cnt_above = s_sel[1], mass_above = s_sel[2];
        __syncthreads();                       // s_sel is rewritten below
        sample_hist_pass<true>(r, lo, hi, eos, m, it, bk, s_cnt, s_mass,
                               s_c2, s_m2, s_scan[0]);
        sample_select256(s_c2, s_m2, false, (u64)k - cnt_above, s_sel);
        const unsigned int lk = (unsigned int)s_sel[0] & 255u;
        tau = (bk << 8) | lk;
        total_k = mass_above + s_sel[2] + s_m2[lk];
        __syncthreads();
      }
      if (use_p) {
        // need = max(1, floor(total_k * pq / 2^16)), the product split
        u64 need = (total_k >> 16) * (u64)pq +
                   (((total_k & 0xffffull) * (u64)pq) >> 16);
        if (need < 1ull) need = 1ull;
        sample_select256(s_c1, s_m1, true, need, s_sel);
        const unsigned int bp = (unsigned int)s_sel[0] & 255u;   // >= bk
        const u64 mass_above = s_sel[2];
        __syncthreads();
        if (bp != bk)
          sample_hist_pass<true>(r, lo, hi, eos, m, it, bp, s_cnt, s_mass,
                                 s_c2, s_m2, s_scan[0]);
        sample_select256(s_c2, s_m2, true, need - mass_above, s_sel);
        // in bin bk the low byte found is >= top-k's
        tau = (bp << 8) | ((unsigned int)s_sel[0] & 255u);
      }
    }

    // ---- final pass: the first kept candidate, in ascending index, whose
    // running sum exceeds target.  The candidates form steps in index
    // order: {eos below the window, scalar head}, the uint4 body in chunks
    // of 2048, {scalar tail, eos above the window}; within a step thread t
    // holds up to 8 consecutive candidates.  The kept weight of every step
    // goes to LDS (no barrier in that loop), a scan over the steps gives
    // the total, hence the target, and the step that holds it, and only
    // that step is scanned by candidate.
    const int mis = (int)((reinterpret_cast<unsigned long long>(r + lo) >> 1) & 7);
    const int body0 = min(hi, lo + ((8 - mis) & 7));
    const int body1 = body0 + ((hi - body0) & ~7);
    const int nstep = (body1 - body0 + 2047) / 2048 + 2;     // <= 2048
    const bool eos_lo = eos_out && eos < lo, eos_hi = eos_out && eos >= hi;
    // w[j] = kept weight of candidate i0 + j of this thread; returns i0
    auto step_weights = [&](int step, u64 (&w)[8]) -> int {
#pragma unroll
      for (int j = 0; j < 8; ++j) w[j] = 0ull;
      if (step == 0 || step == nstep - 1) {    // one candidate per thread
        int idx = -1;
        if (step == 0) {
          const int t = (int)threadIdx.x - (eos_lo ? 1 : 0);
          if (eos_lo && threadIdx.x == 0) idx = eos;
          else if (t >= 0 && lo + t < body0) idx = lo + t;
        } else {
          const int t = (int)threadIdx.x;
          if (body1 + t < hi) idx = body1 + t;
          else if (eos_hi && body1 + t == hi) idx = eos;
        }
        if (idx >= 0) {
          const unsigned int bits = r[idx];
          if (sample_key(bits) >= tau) w[0] = sample_weight(bits, m, it);
        }
        return idx;
      }
      const int i0 = body0 + (step - 1) * 2048 + (int)threadIdx.x * 8;
      if (i0 < body1) {
        const uint4 v4 = *reinterpret_cast<const uint4*>(r + i0);
        const unsigned int vv[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const unsigned int b0 = vv[j] & 0xffffu, b1 = vv[j] >> 16;
          if (sample_key(b0) >= tau) w[2 * j] = sample_weight(b0, m, it);
          if (sample_key(b1) >= tau) w[2 * j + 1] = sample_weight(b1, m, it);
        }
      }
      return i0;
    };

    u64* s_step = s_mass;                      // kept weight per step
    for (int i = threadIdx.x; i < nstep; i += blockDim.x) s_step[i] = 0ull;
    __syncthreads();
    if (threadIdx.x == 0) { s_sel[0] = 0ull; s_sel[1] = 0ull; }
    for (int step = 0; step < nstep; ++step) {
      u64 w[8];
      step_weights(step, w);
      u64 s = 0ull;
#pragma unroll
      for (int j = 0; j < 8; ++j) s += w[j];
      s = wave_reduce_sum_u64(s);
      if (lane == 0 && s) atomicAdd(&s_step[step], s);
    }
    __syncthreads();

    // scan over the steps, 8 per thread: the total, the draw, its step
    u64 e[8], s = 0ull;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int idx = (int)threadIdx.x * 8 + j;
      e[j] = idx < nstep ? s_step[idx] : 0ull;
      s += e[j];
    }
    u64 total;                                 // sum of the kept weights
    u64 before = block_scan_excl_u64(s, s_scan[0], &total);
    const u64 target = __umul64hi(
        sample_philox((u64)seed[row], (unsigned int)pos[row]), total);
    if (before <= target && target < before + s) {
      bool found = false;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        if (!found) {
          if (before + e[j] > target) {
            found = true;
            s_sel[0] = (u64)(threadIdx.x * 8 + j);
            s_sel[1] = before;
          }
          before += e[j];
        }
      }
    }
    __syncthreads();

    // scan the step that holds the target by candidate
    const int step = min((int)s_sel[0], nstep - 1);
    u64 w[8];
    const int i0 = step_weights(step, w);
    s = 0ull;
#pragma unroll
    for (int j = 0; j < 8; ++j) s += w[j];
    before = s_sel[1] + block_scan_excl_u64(s, s_scan[1], &total);
    if (before <= target && target < before + s) {
      bool found = false;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        if (!found) {
          before += w[j];
          if (before > target) { found = true; s_tok = i0 + j; }
        }
      }
    }
    __syncthreads();
    if (s_tok >= 0) tok = s_tok;
  }

  if (threadIdx.x == 0) {
    if (script == nullptr) {                   // draw only (sample_tokens)
      tokens[row] = (long long)tok;
      return;
    }
    const long long c = ctr[0];
    const long long j = c < (long long)max_run - 1 ? (c < 0 ? 0 : c)
                                                   : (long long)max_run - 1;
    const long long so = (long long)row * max_run + j;
    const long long t = script_mask[so] ? script[so] : (long long)tok;
    if (c >= 0 && c < hist_rows) hist[c * hist_stride + row] = t;
    tokens[row] = t;
    __threadfence();
    if (atomicAdd(ticket, 1u) == gridDim.x - 1) {
      ctr[0] = c + 1;
      *ticket = 0u;
    }
  }
}

extern "C" void qsa_sample_launch(
    const unsigned short* logits, int B, long long V, int lo, int hi, int eos,
    const float* inv_temp, const int* top_k, const int* top_p_q,
    const long long* seed, const int* pos, const long long* script,
    const unsigned char* script_mask, int max_run, long long* ctr,
    long long* hist, long long hist_stride, int hist_rows, long long* tokens,
    unsigned int* ticket, hipStream_t stream) {
  hipLaunchKernelGGL(qsa_sample_kernel, dim3(B), dim3(256), 0, stream, logits,
                     V, lo, hi, eos, inv_temp, top_k, top_p_q, seed, pos,
                     script, script_mask, max_run, ctr, hist, hist_stride,
                     hist_rows, tokens, ticket);
}
