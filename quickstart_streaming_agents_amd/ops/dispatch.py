"""Device dispatch for the op layer.

Same call surface as the qsa_hip extension (ops/hip/ops.cpp). CUDA tensors
go to the hand-written HIP/CDNA4 kernels — fail-loud if the extension is
missing (ops/__init__.py).  CPU tensors run reference implementations with
IDENTICAL semantics (including in-place mutation contracts), which lets the
engine / model / parallel layers run under multi-process gloo tests in
CPU-only CI.  A CUDA tensor NEVER falls back to the CPU path.
"""

from __future__ import annotations

import torch

from . import ext


def _cuda(t: torch.Tensor) -> bool:
    return t.is_cuda


# ---- elementwise ----------------------------------------------------------

def rmsnorm(x: torch.Tensor, w: torch.Tensor, eps: float) -> torch.Tensor:
    if _cuda(x):
        return ext().rmsnorm(x, w, eps)
    xf = x.float()
    y = xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps) * w.float()
    return y.to(x.dtype)


def rmsnorm_residual(x: torch.Tensor, res: torch.Tensor, w: torch.Tensor,
                     eps: float) -> torch.Tensor:
    """res <- res + x (in place); returns rmsnorm(res) * w."""
    if _cuda(x):
        return ext().rmsnorm_residual(x, res, w, eps)
    res.add_(x)
    rf = res.float()
    y = rf * torch.rsqrt(rf.pow(2).mean(-1, keepdim=True) + eps) * w.float()
    return y.to(x.dtype)


def swiglu(gate: torch.Tensor, up: torch.Tensor) -> torch.Tensor:
    if _cuda(gate):
        return ext().swiglu(gate, up)
    return (torch.nn.functional.silu(gate.float()) * up.float()).to(gate.dtype)


def rope_inplace(q: torch.Tensor, k: torch.Tensor, cos_t: torch.Tensor,
                 sin_t: torch.Tensor, pos: torch.Tensor) -> None:
    if _cuda(q):
        ext().rope_inplace(q, k, cos_t, sin_t, pos)
        return
    for t in (q, k):
        D = t.shape[-1]
        half = D // 2
        c = cos_t[pos.long()].unsqueeze(1)
        s = sin_t[pos.long()].unsqueeze(1)
        tf = t.float()
        x0, x1 = tf[..., :half], tf[..., half:]
        t.copy_(torch.cat([x0 * c - x1 * s, x0 * s + x1 * c],
                          dim=-1).to(t.dtype))


def softmax_rows_(scores: torch.Tensor, col_offset: int = 0,
                  causal: bool = False, row_mod: int = 0,
                  row_limits: torch.Tensor | None = None) -> None:
    if _cuda(scores):
        ext().softmax_rows_(scores, col_offset, causal, row_mod, row_limits)
        return
    rows, cols = scores.shape
    limit = torch.full((rows,), cols, dtype=torch.int64)
    if causal:
        r = torch.arange(rows)
        pos = r % row_mod if row_mod > 0 else r
        limit = torch.minimum(limit, pos + col_offset + 1)
    if row_limits is not None:
        limit = torch.minimum(limit, row_limits.long())
    col = torch.arange(cols).unsqueeze(0)
    masked = scores.masked_fill(col >= limit.unsqueeze(1), float("-inf"))
    out = torch.softmax(masked, dim=-1)
    scores.copy_(torch.nan_to_num(out, nan=0.0))


def softmax_rows_bf16_(scores: torch.Tensor, scale: float,
                       row_limits: torch.Tensor) -> None:
    """In-place bf16 masked softmax with folded scale; beyond-limit
    columns zeroed (prefill padded-batch attention)."""
    if _cuda(scores):
        ext().softmax_rows_bf16_(scores, scale, row_limits)
        return
    rows, cols = scores.shape
    s = scores.float() * scale
    col = torch.arange(cols).unsqueeze(0)
    masked = s.masked_fill(col >= row_limits.long().unsqueeze(1),
                           float("-inf"))
    out = torch.nan_to_num(torch.softmax(masked, dim=-1), nan=0.0)
    scores.copy_(out.to(scores.dtype))


# ---- paged KV -------------------------------------------------------------

def kv_append(knew: torch.Tensor, vnew: torch.Tensor, kc: torch.Tensor,
              vc: torch.Tensor, block_table: torch.Tensor,
              seq_lens: torch.Tensor) -> None:
    """Write row b's k/v at position seq_lens[b]-1 of its paged sequence."""
    if _cuda(knew):
        ext().kv_append(knew, vnew, kc, vc, block_table, seq_lens)
        return
    B, KVH, D = knew.shape
    for b in range(B):
        n = int(seq_lens[b])
        if n <= 0:
            continue
        page = int(block_table[b, (n - 1) // 64])
        off = (n - 1) % 64
        # K layout [P, KVH, D/8, 64, 8]; V layout [P, KVH, D, 64]
        kc[page, :, :, off, :] = knew[b].reshape(KVH, D // 8, 8)
        vc[page, :, :, off] = vnew[b]


def rope_kv_append(q, k, v, kc, vc, cos_t, sin_t, block_table,
                   seq_lens) -> None:
    """Fused decode-step rope(q,k in place semantics) + cache append.
    The fused kernel rotates q in place and writes rotated k (+v) straight
    to the paged cache; CPU reference composes the two reference ops."""
    if _cuda(q):
        ext().rope_kv_append(q, k, v, kc, vc, cos_t, sin_t, block_table,
                             seq_lens)
        return
    # positions = seq_lens - 1 (clamped)
    pos = (seq_lens.long() - 1).clamp(min=0).int()
    rope_inplace(q, k, cos_t, sin_t, pos)
    kv_append(k, v, kc, vc, block_table, seq_lens)


def kv_scatter(knew: torch.Tensor, vnew: torch.Tensor, kc: torch.Tensor,
               vc: torch.Tensor, slots: torch.Tensor) -> None:
    """Write row t at global slot ids (page*64 + offset)."""
    if _cuda(knew):
        ext().kv_scatter(knew, vnew, kc, vc, slots)
        return
    T, KVH, D = knew.shape
    for t in range(T):
        s = int(slots[t])
        page, off = s // 64, s % 64
        kc[page, :, :, off, :] = knew[t].reshape(KVH, D // 8, 8)
        vc[page, :, :, off] = vnew[t]


def rope_kv_scatter(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor,
                    kc: torch.Tensor, vc: torch.Tensor, cos_t: torch.Tensor,
                    sin_t: torch.Tensor, positions: torch.Tensor,
                    slots: torch.Tensor) -> None:
    """Fused prefill rope + cache scatter.  q is rotated in place over all
    its rows; the first T = slots.numel() rows of k (rotated) and v land in
    the paged cache.  The fused kernel leaves k itself untouched (nothing
    reads it afterwards); the CPU reference composes the two reference ops
    and so also rotates k in place."""
    if _cuda(q):
        ext().rope_kv_scatter(q, k, v, kc, vc, cos_t, sin_t, positions,
                              slots)
        return
    T = slots.numel()
    rope_inplace(q, k, cos_t, sin_t, positions)
    kv_scatter(k[:T], v[:T], kc, vc, slots)


def paged_attn_decode(q: torch.Tensor, kc: torch.Tensor, vc: torch.Tensor,
                      block_table: torch.Tensor, seq_lens: torch.Tensor,
                      scale: float) -> torch.Tensor:
    if _cuda(q):
        return ext().paged_attn_decode(q, kc, vc, block_table, seq_lens,
                                       scale)
    from .cpu_ref import paged_attn_ref
    return paged_attn_ref(q, kc, vc, block_table, seq_lens,
                          scale).to(q.dtype)


def decode_attn_fused(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor,
                      kc: torch.Tensor, vc: torch.Tensor,
                      cos_t: torch.Tensor, sin_t: torch.Tensor,
                      block_table: torch.Tensor, seq_lens: torch.Tensor,
                      scale: float) -> torch.Tensor:
    """One decode step's attention in a single launch: rope(q, k) at
    position seq_lens-1, append of the rotated k (+v) to the paged cache,
    paged attention and the split merge.  Bit-identical to rope_kv_append
    followed by paged_attn_decode.  The fused kernel rotates q in
    registers and leaves q/k/v untouched (nothing reads them afterwards);
    the CPU reference composes the two reference ops and so rotates q and
    k in place."""
    if _cuda(q):
        return ext().decode_attn_fused(q, k, v, kc, vc, cos_t, sin_t,
                                       block_table, seq_lens, scale)
    rope_kv_append(q, k, v, kc, vc, cos_t, sin_t, block_table, seq_lens)
    return paged_attn_decode(q, kc, vc, block_table, seq_lens, scale)


# ---- skinny decode GEMM ---------------------------------------------------

def can_pack_weight(n: int, k: int) -> bool:
    return n % 16 == 0 and k % 256 == 0


def pack_weight_frag(w: torch.Tensor) -> torch.Tensor:
    """[N,K] bf16 -> fragment-major stream layout for skinny_linear (GPU)."""
    if w.is_cuda:
        return ext().pack_weight_frag(w)
    n, k = w.shape
    return w.reshape(n // 16, 16, k // 32, 32).permute(0, 2, 1, 3).contiguous()


def skinny_linear(x: torch.Tensor, wf: torch.Tensor, n: int,
                  k: int) -> torch.Tensor:
    """x[M,K] @ W^T via the weight-streaming decode kernel (M <= 32)."""
    if x.is_cuda:
        return ext().skinny_gemm(x, wf, n, k)
    w = wf.reshape(n // 16, k // 32, 16, 32).permute(0, 2, 1, 3) \
        .reshape(n, k)
    return (x.float() @ w.float().T).to(x.dtype)


# ---- fp8 weight-only decode GEMM (W8A16, per-channel scales) -------------

def pack_weight_fp8(w: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """[N,K] bf16 -> (fp8-e4m3 fragment-pair-major stream as uint8,
    per-channel f32 scales).  Layout doc: ops/hip/gemm_core.h."""
    n, k = w.shape
    assert n % 16 == 0 and k % 256 == 0
    wf = w.float()
    s = wf.abs().amax(dim=1).clamp(min=1e-12) / 448.0
    q = (wf / s[:, None]).clamp(-448.0, 448.0).to(torch.float8_e4m3fn)
    qf = q.view(torch.uint8) \
        .reshape(n // 16, 16, k // 64, 2, 4, 8) \
        .permute(0, 2, 1, 4, 3, 5).contiguous()
    return qf, s.float().contiguous()


def unpack_weight_fp8(qf: torch.Tensor, scale: torch.Tensor, n: int,
                      k: int) -> torch.Tensor:
    """Inverse of pack_weight_fp8 -> dequantized f32 [N,K] (reference)."""
    q = qf.reshape(n // 16, k // 64, 16, 4, 2, 8) \
        .permute(0, 2, 1, 4, 3, 5).reshape(n, k)
    return q.view(torch.float8_e4m3fn).float() * scale[:, None].float()


def gemm_fp8_batch(x: torch.Tensor, qf: torch.Tensor,
                   scale: torch.Tensor, n: int, k: int,
                   splitk: int = 1) -> torch.Tensor:
    """Batched-M (<=256) fp8 weight-stream GEMM (decode batches)."""
    if x.is_cuda:
        return ext().gemm_fp8_batch(x, qf, scale, n, k, splitk)
    w = unpack_weight_fp8(qf, scale, n, k)
    return (x.float() @ w.T).to(x.dtype)


def skinny_linear_fp8(x: torch.Tensor, qf: torch.Tensor,
                      scale: torch.Tensor, n: int, k: int) -> torch.Tensor:
    """x[M,K] bf16 @ dequant(Q)^T via the fp8 weight-streaming kernel
    (M <= 64)."""
    if x.is_cuda:
        return ext().skinny_gemm_fp8(x, qf, scale, n, k)
    w = unpack_weight_fp8(qf, scale, n, k)
    return (x.float() @ w.T).to(x.dtype)


# Shape classes that beat rocBLAS bf16 at 33..64 rows on MI355X, measured at
# M = 64 (profiles/fp8_decode_gemm.md): only wo-like weights (small N,
# K < 8192).  Every other class keeps the 32-row limit.
SKINNY_FP8_WIDE_CLASSES: frozenset = frozenset({"wo"})


def skinny_fp8_class(n: int, k: int) -> str:
    """The fp8 skinny launcher's shape class for an [n, k] weight
    (ops/hip/skinny_gemm_fp8.hip), its last class split by K: the launch
    is the same for wo and wdown, the comparison with rocBLAS is not.
    The CPU-only copy of the extension's skinny_fp8_class;
    tests/test_gpu_gemm_edges.py test_skinny_fp8_class_agrees compares
    the two."""
    if n % 128 == 0 and n >= 65536:
        return "lm_head"
    if n % 64 == 0 and n >= 16384:
        return "wgu"
    if n % 32 == 0 and n >= 6144 and k < 8192:
        return "qkv"
    return "wo" if k < 8192 else "wdown"


def skinny_fp8_row_limit(n: int, k: int) -> int:
    """Largest M routed to the fp8 skinny kernel for an [n, k] weight."""
    return 64 if skinny_fp8_class(n, k) in SKINNY_FP8_WIDE_CLASSES else 32


# ---- routed MoE decode FFN (ops/hip/moe.hip) ------------------------------
# T <= 64 rows, E <= 16 experts, top-k <= 4.  cap, the row capacity per
# expert, is 32 at T <= 32, else 64.  The GPU kernels leave rows at or past
# counts[e] of every [E, cap, ...] buffer unwritten; the CPU references
# leave them zero.

MOE_MAX_ROWS = 64


def moe_cap(t: int) -> int:
    return 32 if t <= 32 else 64


def moe_pack_experts(ws: list[torch.Tensor], fp8: bool):
    """Stack the experts' [N, K] weights into one stream per layer:
    fp8 -> (qf [E, ...] uint8, scale [E, N] f32) of pack_weight_fp8,
    else wf [E, ...] bf16 of pack_weight_frag."""
    if fp8:
        packed = [pack_weight_fp8(w) for w in ws]
        return (torch.stack([p[0] for p in packed]).contiguous(),
                torch.stack([p[1] for p in packed]).contiguous())
    return torch.stack([pack_weight_frag(w) for w in ws]).contiguous()


def moe_dispatch(h: torch.Tensor, top_idx: torch.Tensor, n_experts: int,
                 row_live: torch.Tensor | None = None):
    """Routing + gather: h [T, H], top_idx [T, k] i64, row_live [T] i32 or
    None -> (counts [E] i32, slot [T, k] i32, xg [E, cap, H]).

    xg[e, slot[t, j]] = h[t] for every live row t and pick j with
    top_idx[t, j] = e; slots ascend with the row index inside an expert;
    a dead row (row_live == 0), or a pick outside [0, E), has slot -1.
    Precondition: a row's k experts are distinct."""
    if h.is_cuda:
        return tuple(ext().moe_dispatch(h, top_idx, n_experts, row_live))
    T, H = h.shape
    k = top_idx.shape[1]
    assert 1 <= T <= MOE_MAX_ROWS and 1 <= k <= 4 and 1 <= n_experts <= 16
    cap = moe_cap(T)
    counts = torch.zeros(n_experts, dtype=torch.int32)
    slot = torch.full((T, k), -1, dtype=torch.int32)
    xg = torch.zeros(n_experts, cap, H, dtype=h.dtype)
    live = [True] * T if row_live is None else \
        [bool(v) for v in row_live.tolist()]
    idx = top_idx.tolist()
    for t in range(T):
        if not live[t]:
            continue
        for e in sorted(set(idx[t])):
            if not 0 <= e < n_experts:
                continue
            s = int(counts[e])
            for j in range(k):
                if idx[t][j] == e:
                    slot[t, j] = s
            xg[e, s] = h[t]
            counts[e] = s + 1
    return counts, slot, xg


def _moe_grouped(xg, counts, n, fn):
    """out[e, :c] = fn(e, xg[e, :c]) with c = counts[e] clamped to
    [0, cap], as the kernels clamp it: a negative count is an expert
    without rows, a count above cap is cap."""
    cap = xg.shape[1]
    out = torch.zeros(xg.shape[0], cap, n, dtype=xg.dtype, device=xg.device)
    for e, c in enumerate(counts.tolist()):
        c = min(c, cap)
        if c > 0:
            out[e, :c] = fn(e, xg[e, :c])
    return out


def moe_skinny_linear(xg: torch.Tensor, counts: torch.Tensor,
                      wf: torch.Tensor, n: int, k: int) -> torch.Tensor:
    """Grouped skinny_linear: out[e, :counts[e]] = xg[e, :counts[e]] @
    W_e^T on the stacked bf16 stream; experts with no rows are not read.
    Each live row has the bits skinny_linear gives it."""
    if xg.is_cuda:
        return ext().moe_skinny_gemm(xg, counts, wf, n, k)
    return _moe_grouped(xg, counts, n,
                        lambda e, x: skinny_linear(x, wf[e], n, k))


def moe_skinny_linear_fp8(xg: torch.Tensor, counts: torch.Tensor,
                          qf: torch.Tensor, scale: torch.Tensor, n: int,
                          k: int) -> torch.Tensor:
    """Grouped skinny_linear_fp8 on the stacked fp8 stream and [E, N]
    scales; experts with no rows are not read."""
    if xg.is_cuda:
        return ext().moe_skinny_gemm_fp8(xg, counts, qf, scale, n, k)
    return _moe_grouped(
        xg, counts, n,
        lambda e, x: skinny_linear_fp8(x, qf[e], scale[e], n, k))


def moe_swiglu(gu: torch.Tensor, counts: torch.Tensor) -> torch.Tensor:
    """act[e, r] = silu(gu[e, r, :F]) * gu[e, r, F:] for r < counts[e]."""
    if gu.is_cuda:
        return ext().moe_swiglu(gu, counts)
    f = gu.shape[2] // 2
    return _moe_grouped(gu, counts, f,
                        lambda e, g: swiglu(g[:, :f], g[:, f:]))


def moe_combine(y: torch.Tensor, slot: torch.Tensor, top_idx: torch.Tensor,
                top_w: torch.Tensor) -> torch.Tensor:
    """out[t] = sum over row t's picks of top_w[t, j] * y[e, slot[t, j]],
    in ascending expert index, in f32 from zero with the multiply and the
    add rounded separately (no FMA), rounded once to y's dtype: the
    arithmetic of the dense masked sum over all experts.  Dead picks
    (a slot outside [0, cap) or an expert outside [0, E)) add nothing, so
    a dead row gives zeros."""
    if y.is_cuda:
        return ext().moe_combine(y, slot, top_idx, top_w)
    T, k = top_idx.shape
    cap = y.shape[1]
    out = torch.zeros(T, y.shape[2], dtype=torch.float32)
    for e in range(y.shape[0]):
        for j in range(k):
            rows = ((top_idx[:, j] == e) & (slot[:, j] >= 0) &
                    (slot[:, j] < cap)).nonzero(as_tuple=True)[0]
            if rows.numel() == 0:
                continue
            prod = top_w[rows, j].float().unsqueeze(1) * \
                y[e, slot[rows, j].long()].float()
            out[rows] = out[rows] + prod
    return out.to(y.dtype)


# ---- fused greedy sampling step ------------------------------------------

def greedy_sample_step(logits: torch.Tensor, lo: int, hi: int, eos: int,
                       script: torch.Tensor, script_mask: torch.Tensor,
                       ctr: torch.Tensor, hist: torch.Tensor,
                       tokens: torch.Tensor,
                       ticket: torch.Tensor | None = None) -> None:
    """One decode step's greedy sampling and bookkeeping, in place.

    tok[b] = lowest-index argmax of logits[b] over [lo, hi) U {eos}
    (eos < 0: no eos), overridden by script[b, min(ctr, max_run - 1)]
    where script_mask is set; then hist[ctr, b] = tok[b],
    tokens[b] = tok[b], ctr += 1.  Rows beyond logits.shape[0] of script /
    hist / tokens are left alone.  Equals argmax(logits.float() + bias)
    with bias 0 on the set and -inf elsewhere, on NaN-free logits.
    ticket: i32 [1] zero-initialised scratch of the GPU kernel."""
    if logits.is_cuda:
        ext().greedy_sample_step(logits, lo, hi, eos, script, script_mask,
                                 ctr, hist, tokens, ticket)
        return
    B = logits.shape[0]
    if B == 0:
        return
    win = logits[:, lo:hi].float()
    if hi > lo:
        bv, bi = win.max(dim=1)
        # lowest index among ties (max's index choice is unspecified)
        bi = (win == bv[:, None]).int().argmax(dim=1) + lo
    else:
        bv = torch.full((B,), float("-inf"))
        bi = torch.zeros(B, dtype=torch.int64)
    if eos >= 0 and not lo <= eos < hi:
        ev = logits[:, eos].float()
        take = (ev > bv) | ((ev == bv) & (eos < bi))
        bi = torch.where(take, torch.full_like(bi, eos), bi)
        bv = torch.where(take, ev, bv)
    # an all -inf candidate set gives index 0, as torch.argmax does
    bi = torch.where(bv == float("-inf"), torch.zeros_like(bi), bi)
    c = int(ctr[0])
    j = min(max(c, 0), script.shape[1] - 1)
    tok = torch.where(script_mask[:B, j], script[:B, j], bi)
    if 0 <= c < hist.shape[0]:
        hist[c, :B] = tok
    tokens[:B] = tok
    ctr.add_(1)


# ---- per-request seeded sampling -----------------------------------------
#
# The sampling rule (the CPU branch below is the specification; the kernel,
# ops/hip/sampling.hip, agrees with it bit for bit).  Per row: bf16
# logits[V]; the window lo, hi, eos of greedy_sample_step; inv_temp (f32);
# top_k (i32, 0 = off); top_p_q (i32 in [1, 65536], 65536 = off); seed (64
# bits); pos (i32).  A row's token depends on these alone.  inv_temp must be
# finite and >= 0 (SamplingParams guarantees it; the ops cannot check a
# device tensor), and the claim is for NaN-free logits, as for
# greedy_sample_step.
#
# Candidates: the indices in [lo, hi) U {eos}, in ascending index order.
# Greedy rows: inv_temp == 0 gives the greedy_sample_step token, the
#   lowest-index argmax over the candidates (0 if all are -inf); the other
#   parameters are ignored.
# Weight: m = the maximum candidate logit; m == -inf gives token 0 and
#   m == +inf gives the greedy token, the lowest-index +inf candidate (no
#   weight is defined against an infinite maximum).  In f32, every operation
#   rounded on its own (no FMA):
#     d = l - m;  x = d * inv_temp;  y = max(x * LOG2E, -64)
#     n = floor(y + 0.5);  f = y - n
#     p = Horner(f), coefficients c_k = f32(ln2^k / k!), k = 6..0: the
#         degree-6 Taylor polynomial of 2^f on [-0.5, 0.5], remainder at
#         most (ln2/2)^7/7! ~ 1.2e-7
#     q = (u32) trunc(p * 2^24)
#     w = ((u64) q << 16) >> (-n) when -n <= 40, else 0
#   The maximum has w = 2^40, so totals stay below 2^40 times the number of
#   candidates: below 2^58 up to 2^18 candidates, below 2^62 at the largest
#   V the kernel takes (2046 * 2048), inside 64 bits either way.  A token
#   below 2^-40 of the maximum has weight 0 and is never drawn.
# Key: the order-preserving 16-bit key of the bf16 logit.  The weight
#   depends on the logit alone, so thresholds are thresholds on the key.
# top-k: tau_k = the largest key with count(key >= tau_k) >= top_k, the
#   smallest key if there are fewer candidates than top_k.  Ties at the
#   threshold are all kept.
# top-p, on what top-k kept: total_k = sum of w;
#   need = max(1, floor(total_k * top_p_q / 2^16)) (an exact integer);
#   tau_p = the largest key with sum over key >= tau_p of w >= need.  Ties
#   are kept.
# Kept set: key >= max(tau_k, tau_p); total = the sum of w over it.
# Draw: Philox4x32-10 (constants 0xD2511F53, 0xCD9E8D57, 0x9E3779B9,
#   0xBB67AE85), key (seed & 0xffffffff, seed >> 32), counter (pos, 0, 0, 0);
#   r = x0 | x1 << 32; target = (r * total) >> 64; the token is the first
#   kept candidate, in ascending index, whose running sum of w exceeds
#   target.
# Everything after the weight is integer arithmetic, so no reduction order
# can change a bit.

_LOG2E = 1.4426950408889634
_M32 = 0xffffffff


def _exp2_coeffs() -> list[float]:
    import math
    return [float(torch.tensor(math.log(2.0) ** k / math.factorial(k),
                               dtype=torch.float64).float())
            for k in range(7)]


def _mulhi32(a: int, b: torch.Tensor) -> torch.Tensor:
    """High word of a * b, a and b below 2^32, in int64 without overflow."""
    return (a * (b >> 16) + ((a * (b & 0xffff)) >> 16)) >> 16


def philox4x32_10(counter: torch.Tensor, key: torch.Tensor) -> torch.Tensor:
    """Philox4x32-10 on int64 tensors of 32-bit words: counter [N, 4],
    key [N, 2] -> [N, 4]."""
    c0, c1, c2, c3 = (counter[:, i].clone() for i in range(4))
    k0, k1 = key[:, 0].clone(), key[:, 1].clone()
    for _ in range(10):
        hi0, lo0 = _mulhi32(0xD2511F53, c0), (0xD2511F53 * c0) & _M32
        hi1, lo1 = _mulhi32(0xCD9E8D57, c2), (0xCD9E8D57 * c2) & _M32
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0 = (k0 + 0x9E3779B9) & _M32
        k1 = (k1 + 0xBB67AE85) & _M32
    return torch.stack([c0, c1, c2, c3], dim=1)


def sample_key(logits: torch.Tensor) -> torch.Tensor:
    """Order-preserving 16-bit key (int64) of bf16 logits."""
    bits = logits.contiguous().view(torch.int16).to(torch.int64) & 0xffff
    return torch.where((bits & 0x8000) != 0, ~bits & 0xffff, bits | 0x8000)


def sample_weights(logits: torch.Tensor, m: torch.Tensor,
                   inv_temp: torch.Tensor) -> torch.Tensor:
    """The rule's integer weights (int64) of bf16 logits [B, C] against the
    row maxima m [B] (f32, finite) and inv_temp [B] (f32, > 0)."""
    f32 = torch.float32
    c = _exp2_coeffs()
    d = logits.float() - m[:, None]
    x = d * inv_temp[:, None]
    y = torch.maximum(x * torch.tensor(_LOG2E, dtype=f32),
                      torch.tensor(-64.0, dtype=f32))
    n = torch.floor(y + 0.5)
    f = y - n
    p = torch.full_like(f, c[6])
    for k in range(5, -1, -1):
        p = p * f
        p = p + torch.tensor(c[k], dtype=f32)
    q = (p * 16777216.0).to(torch.int64)
    sh = (-n).to(torch.int64)
    return torch.where(sh <= 40, (q << 16) >> sh.clamp(max=40),
                       torch.zeros_like(q))


def _candidates(lo: int, hi: int, eos: int) -> list[int]:
    idx = list(range(lo, hi))
    if 0 <= eos < lo:
        idx.insert(0, eos)
    elif eos >= hi:
        idx.append(eos)
    return idx


def _sample_rows_cpu(logits, lo, hi, eos, inv_temp, top_k, top_p_q, seed,
                     pos) -> torch.Tensor:
    B = logits.shape[0]
    idx = _candidates(lo, hi, eos)
    C = len(idx)
    if B == 0 or C == 0:
        return torch.zeros(B, dtype=torch.int64)
    cand = torch.tensor(idx, dtype=torch.int64)
    L = logits[:, cand]
    lf = L.float()
    m = lf.max(dim=1).values
    dead = m == float("-inf")
    # lowest candidate position among ties; an all -inf set gives token 0
    greedy = cand[(lf == m[:, None]).int().argmax(dim=1)]
    greedy = torch.where(dead, torch.zeros_like(greedy), greedy)
    inv_temp = inv_temp[:B].float()
    # a +inf maximum keeps the greedy token: no weight is defined against it
    sampled = (inv_temp != 0) & ~dead & (m != float("inf"))
    if not bool(sampled.any()):
        return greedy
    rows = sampled.nonzero(as_tuple=True)[0]
    R = rows.numel()
    L = L[rows]
    key = sample_key(L)
    w = sample_weights(L, m[rows], inv_temp[rows])
    k = top_k[:B][rows].to(torch.int64)
    pq = top_p_q[:B][rows].to(torch.int64)
    skey, order = key.sort(dim=1, descending=True, stable=True)
    cum = w.gather(1, order).cumsum(dim=1)
    tau_k = skey.gather(1, (k.clamp(1, C) - 1)[:, None]).squeeze(1)
    tau_k = torch.where(k > 0, tau_k, torch.zeros_like(tau_k))
    nk = (skey >= tau_k[:, None]).sum(dim=1)
    total_k = cum.gather(1, (nk - 1)[:, None]).squeeze(1)
    need = torch.tensor([max(1, (t * q) >> 16)
                         for t, q in zip(total_k.tolist(), pq.tolist())],
                        dtype=torch.int64)
    jp = (cum < need[:, None]).sum(dim=1)
    tau_p = skey.gather(1, jp[:, None]).squeeze(1)
    tau = torch.maximum(tau_k, tau_p)
    run = torch.where(key >= tau[:, None], w, torch.zeros_like(w)) \
        .cumsum(dim=1)
    total = run[:, -1]
    sd = seed[:B][rows].to(torch.int64)
    zero = torch.zeros(R, dtype=torch.int64)
    x = philox4x32_10(
        torch.stack([pos[:B][rows].to(torch.int64) & _M32, zero, zero, zero],
                    dim=1),
        torch.stack([sd & _M32, (sd >> 32) & _M32], dim=1))
    target = torch.tensor(
        [((x0 | (x1 << 32)) * t) >> 64
         for x0, x1, t in zip(x[:, 0].tolist(), x[:, 1].tolist(),
                              total.tolist())], dtype=torch.int64)
    tok = cand[(run <= target[:, None]).sum(dim=1)]
    out = greedy.clone()
    out[rows] = tok
    return out


def sample_tokens(logits: torch.Tensor, lo: int, hi: int, eos: int,
                  inv_temp: torch.Tensor, top_k: torch.Tensor,
                  top_p_q: torch.Tensor, seed: torch.Tensor,
                  pos: torch.Tensor) -> torch.Tensor:
    """The draw of the sampling rule above for each row of bf16 logits
    [B, V], no bookkeeping -> tokens i64 [B].  inv_temp f32, top_k /
    top_p_q / pos i32, seed i64 (the 64 bits, two's complement), each of
    at least B rows."""
    if logits.is_cuda:
        return ext().sample_tokens(logits, lo, hi, eos, inv_temp, top_k,
                                   top_p_q, seed, pos)
    if logits.dtype != torch.bfloat16:
        raise RuntimeError("sample_tokens: logits must be bf16")
    return _sample_rows_cpu(logits, lo, hi, eos, inv_temp, top_k, top_p_q,
                            seed, pos)


def sample_step(logits: torch.Tensor, lo: int, hi: int, eos: int,
                inv_temp: torch.Tensor, top_k: torch.Tensor,
                top_p_q: torch.Tensor, seed: torch.Tensor, pos: torch.Tensor,
                script: torch.Tensor, script_mask: torch.Tensor,
                ctr: torch.Tensor, hist: torch.Tensor, tokens: torch.Tensor,
                ticket: torch.Tensor | None = None) -> None:
    """One decode step's per-request sampling and bookkeeping, in place:
    greedy_sample_step with tok[b] drawn by the sampling rule above (rows
    with inv_temp == 0 draw the greedy token)."""
    if logits.is_cuda:
        ext().sample_step(logits, lo, hi, eos, inv_temp, top_k, top_p_q,
                          seed, pos, script, script_mask, ctr, hist, tokens,
                          ticket)
        return
    B = logits.shape[0]
    if B == 0:
        return
    tok = sample_tokens(logits, lo, hi, eos, inv_temp, top_k, top_p_q, seed,
                        pos)
    c = int(ctr[0])
    j = min(max(c, 0), script.shape[1] - 1)
    tok = torch.where(script_mask[:B, j], script[:B, j], tok)
    if 0 <= c < hist.shape[0]:
        hist[c, :B] = tok
    tokens[:B] = tok
    ctr.add_(1)


# ---- retrieval / streaming ------------------------------------------------

def topk_cosine(queries: torch.Tensor, docs: torch.Tensor, k: int):
    if _cuda(queries):
        return ext().topk_cosine(queries, docs, k)
    from .cpu_ref import topk_cosine_ref
    return topk_cosine_ref(queries, docs, k)


def window_agg(ts: torch.Tensor, key: torch.Tensor,
               value: torch.Tensor | None, t0: int, win_ms: int, nwin: int,
               nkeys: int):
    if _cuda(ts):
        return ext().window_agg(ts, key, value, t0, win_ms, nwin, nkeys)
    from .cpu_ref import window_agg_ref
    return window_agg_ref(ts, key, value, t0, win_ms, nwin, nkeys)


# ---- GPU hash join (K8) ---------------------------------------------------

def hash_build(keys: torch.Tensor, ts: torch.Tensor):
    """(i64 keys, i64 event ts) -> opaque latest-per-key table.
    GPU: (tkeys, tpay) HBM tensors; CPU: a dict of key -> (ts, row).
    Event times clamp to [0, 2^40): the GPU payload packs (ts << 24 |
    row), so negative or far-future timestamps would corrupt ordering —
    clamping keeps CPU/GPU semantics identical."""
    ts = ts.clamp(min=0, max=(1 << 40) - 1)
    if _cuda(keys):
        return tuple(ext().hash_build(keys, ts.contiguous()))
    table: dict = {}
    for i, (k, t) in enumerate(zip(keys.tolist(), ts.tolist())):
        prev = table.get(k)
        if prev is None or (t, i) >= prev:
            table[k] = (t, i)
    return table


def hash_probe(table, keys: torch.Tensor, min_ts: int) -> torch.Tensor:
    """Probe -> i32 row indices (-1 = absent or event ts < min_ts)."""
    if isinstance(table, tuple):
        return ext().hash_probe(table[0], table[1], keys, int(min_ts))
    out = torch.full((keys.numel(),), -1, dtype=torch.int32)
    for i, k in enumerate(keys.tolist()):
        hit = table.get(k)
        if hit is not None and hit[0] >= min_ts:
            out[i] = hit[1]
    return out
