"""Edge cases of the elementwise, top-k, window, AR and hash-join ops.

This module holds the case tables, the input builders (fixed seeds, built on
the CPU) and float64 references written in plain torch/numpy.  Its own tests
run every case through the CPU paths of ops.dispatch (and ar_forecast) and
check them against those references; tests/test_gpu_kernel_edges.py runs the
same cases through the HIP kernels with the same assertions.

bf16 tolerance, derived once: the ops compute in f32 (error before rounding
<= ~1e-5 relative) and round once to bf16 (round-to-nearest, <= 2^-8
relative).  The bound is one full bf16 ulp: |got - ref| <= 2^-7 |ref| + 1e-7.
"""

import functools

import numpy as np
import pytest
import torch

from quickstart_streaming_agents_amd.ops import dispatch as D
from quickstart_streaming_agents_amd.runtime.anomaly import ar_forecast

BF16_RTOL = 2.0 ** -7
BF16_ATOL = 1e-7


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def assert_bf16_close(got, ref64, what="", atol=BF16_ATOL):
    """|got - ref64| <= 2^-7 |ref64| + atol, elementwise; got must be finite."""
    got = got.detach().cpu().double()
    assert got.shape == ref64.shape, f"{what}: shape {tuple(got.shape)}"
    assert torch.isfinite(got).all(), f"{what}: non-finite output"
    err = (got - ref64).abs()
    bound = BF16_RTOL * ref64.abs() + atol
    bad = err > bound
    if bad.any():
        i = int((err / bound).argmax())
        raise AssertionError(
            f"{what}: {int(bad.sum())} of {bad.numel()} outside the bf16 "
            f"tolerance; worst at flat index {i}: got "
            f"{got.flatten()[i].item()!r} ref {ref64.flatten()[i].item()!r}")


# ---------------------------------------------------------------------------
# rmsnorm / rmsnorm_residual
# ---------------------------------------------------------------------------

RMSNORM_ROWS = 3
RMSNORM_EPS = 1e-5
# 8: one thread works; 2040: last thread idle; 8192: last register-cached
# width; 8200: first uncached width; 16384: uncached tail with stride
RMSNORM_H = (8, 2040, 2048, 4096, 8192, 8200, 16384)


@functools.lru_cache(maxsize=None)
def rmsnorm_case(H):
    g = _gen(1000 + H)
    x = torch.randn(RMSNORM_ROWS, H, generator=g).bfloat16()
    res = torch.randn(RMSNORM_ROWS, H, generator=g).bfloat16()
    w = torch.randn(H, generator=g).bfloat16()
    return x, res, w


def rmsnorm_ref64(x, w, eps, res=None):
    """(y in f64, updated residual in bf16 or None).  The residual form
    normalises the bf16-rounded sum, which is what gets stored."""
    r = x if res is None else (x.float() + res.float()).bfloat16()
    r64 = r.double()
    y = r64 * torch.rsqrt(r64.pow(2).mean(-1, keepdim=True) + eps) * w.double()
    return y, (None if res is None else r)


def check_rmsnorm(fn_plain, fn_residual, H, to_dev=lambda t: t):
    x, res, w = rmsnorm_case(H)
    y = fn_plain(to_dev(x), to_dev(w), RMSNORM_EPS)
    ref, _ = rmsnorm_ref64(x, w, RMSNORM_EPS)
    assert_bf16_close(y, ref, f"rmsnorm H={H}")
    res_io = to_dev(res.clone())
    y = fn_residual(to_dev(x), res_io, to_dev(w), RMSNORM_EPS)
    ref, r = rmsnorm_ref64(x, w, RMSNORM_EPS, res)
    # one exact f32 add and one round-to-nearest-even: bit-equal
    assert torch.equal(res_io.cpu().view(torch.int16), r.view(torch.int16)), \
        f"rmsnorm_residual H={H}: updated residual differs"
    assert_bf16_close(y, ref, f"rmsnorm_residual H={H}")


@pytest.mark.parametrize("H", RMSNORM_H)
def test_rmsnorm_cpu(H):
    check_rmsnorm(D.rmsnorm, D.rmsnorm_residual, H)


def test_cpu_ref_rmsnorm_normalises_rounded_residual():
    from quickstart_streaming_agents_amd.ops import cpu_ref
    x, res, w = rmsnorm_case(2040)
    y, r = cpu_ref.rmsnorm_ref(x, w, RMSNORM_EPS, residual=res)
    ref, r_ref = rmsnorm_ref64(x, w, RMSNORM_EPS, res)
    assert torch.equal(r, r_ref.float())
    torch.testing.assert_close(y.double(), ref, atol=1e-6, rtol=1e-5)


# ---------------------------------------------------------------------------
# swiglu
# ---------------------------------------------------------------------------

# outputs are compared with the bf16 relative bound down to 1e-30
SWIGLU_ATOL = 1e-30
SWIGLU_CASES = ("strided_halves", "large_gates", "grid_stride")


@functools.lru_cache(maxsize=None)
def swiglu_case(name):
    """-> (buffer, gate view, up view, f64 reference)."""
    if name == "strided_halves":        # as the models call it
        gu = torch.randn(33, 2 * 1024, generator=_gen(2001)).bfloat16()
        gate, up = gu[:, :1024], gu[:, 1024:]
    elif name == "large_gates":
        g = _gen(2002)
        gu = torch.empty(5, 2 * 1024)
        gu[:, :1024] = (torch.randn(5, 1024, generator=g) * 8).clamp(-30, 30)
        gu[:, 1024:] = torch.randn(5, 1024, generator=g)
        # +-30: silu ~ -3e-12 / ~gate; +-100: exp overflows to inf in f32
        # (x / inf) / underflows to 0 (x / 1)
        gu[:, :8] = torch.tensor([30., -30., 0., -0., 100., -100., 29.875,
                                  -29.875])
        gu[2, 1016:1024] = torch.tensor([-30., 30., -100., 100., 0., 1., -1.,
                                         -88.])
        gu = gu.bfloat16()
        gate, up = gu[:, :1024], gu[:, 1024:]
    elif name == "grid_stride":
        # rows * cols > 8192 blocks * 256 threads * 8: the loop iterates
        rows, cols = 2056, 8192
        assert rows * cols > 8192 * 256 * 8
        gu = torch.randn(rows, 2 * cols, generator=_gen(2003)).bfloat16()
        gate, up = gu[:, :cols], gu[:, cols:]
    else:
        raise KeyError(name)
    g64 = gate.double()
    ref = g64 * torch.sigmoid(g64) * up.double()
    return gu, gate, up, ref


def check_swiglu(fn, name, to_dev=lambda t: t):
    gu, _, _, ref = swiglu_case(name)
    cols = gu.shape[1] // 2
    gu_d = to_dev(gu)
    y = fn(gu_d[:, :cols], gu_d[:, cols:])
    assert y.is_contiguous()
    assert_bf16_close(y, ref, f"swiglu {name}", atol=SWIGLU_ATOL)


@pytest.mark.parametrize("name", SWIGLU_CASES)
def test_swiglu_cpu(name):
    check_swiglu(D.swiglu, name)


# ---------------------------------------------------------------------------
# rope_inplace
# ---------------------------------------------------------------------------

ROPE_D = (64, 128)
ROPE_MAX_POS = 512
ROPE_B, ROPE_QH, ROPE_KVH = 6, 4, 2
ROPE_POS = (0, ROPE_MAX_POS - 1, 1, 17, 255, 0)
# seeds chosen so that no reference output is within 1e-4 of zero (checked
# below): x0*c - x1*s cancels, and its f32 error (<= 2 * 2^-24 * |term|,
# terms < 4) must stay inside the 2^-8 |ref| the tolerance leaves after the
# bf16 rounding
ROPE_SEED = {64: 3000, 128: 3000}


@functools.lru_cache(maxsize=None)
def rope_case(Dh, seed=None):
    """-> (qkv [B, (QH+2KVH)*D] bf16, cos, sin, pos, q ref, k ref)."""
    from quickstart_streaming_agents_amd.ops import cpu_ref
    seed = ROPE_SEED[Dh] if seed is None else seed
    width = (ROPE_QH + 2 * ROPE_KVH) * Dh
    qkv = torch.randn(ROPE_B, width, generator=_gen(seed)).bfloat16()
    cos_t, sin_t = cpu_ref.rope_tables(ROPE_MAX_POS, Dh)
    pos = torch.tensor(ROPE_POS, dtype=torch.int32)
    q, k, _ = rope_views(qkv, Dh)
    return qkv, cos_t, sin_t, pos, rope_ref64(q, pos, cos_t, sin_t), \
        rope_ref64(k, pos, cos_t, sin_t)


def rope_views(qkv, Dh):
    """Strided q / k / v views of the fused qkv buffer."""
    nq, nk = ROPE_QH * Dh, ROPE_KVH * Dh
    B = qkv.shape[0]
    return (qkv[:, :nq].view(B, ROPE_QH, Dh),
            qkv[:, nq:nq + nk].view(B, ROPE_KVH, Dh),
            qkv[:, nq + nk:])


def rope_ref64(x, pos, cos_t, sin_t):
    half = x.shape[-1] // 2
    c = cos_t[pos.long()].double().unsqueeze(1)
    s = sin_t[pos.long()].double().unsqueeze(1)
    x0, x1 = x.double()[..., :half], x.double()[..., half:]
    return torch.cat([x0 * c - x1 * s, x0 * s + x1 * c], dim=-1)


def check_rope(fn, Dh, to_dev=lambda t: t):
    qkv, cos_t, sin_t, pos, q_ref, k_ref = rope_case(Dh)
    buf = to_dev(qkv.clone())
    q, k, v = rope_views(buf, Dh)
    assert not q.is_contiguous() and not k.is_contiguous()
    fn(q, k, to_dev(cos_t), to_dev(sin_t), to_dev(pos))
    got = buf.cpu()
    gq, gk, gv = rope_views(got, Dh)
    q0, k0, v0 = rope_views(qkv, Dh)
    assert_bf16_close(gq, q_ref, f"rope q D={Dh}")
    assert_bf16_close(gk, k_ref, f"rope k D={Dh}")
    for b, p in enumerate(ROPE_POS):
        if p == 0:      # cos 1, sin 0: bit-unchanged
            assert torch.equal(gq[b].view(torch.int16),
                               q0[b].view(torch.int16))
            assert torch.equal(gk[b].view(torch.int16),
                               k0[b].view(torch.int16))
    assert torch.equal(gv.view(torch.int16), v0.view(torch.int16)), \
        "rope touched the v slice"


@pytest.mark.parametrize("Dh", ROPE_D)
def test_rope_cpu(Dh):
    _, _, _, _, q_ref, k_ref = rope_case(Dh)
    assert min(q_ref.abs().min().item(), k_ref.abs().min().item()) > 1e-4
    check_rope(D.rope_inplace, Dh)


# ---------------------------------------------------------------------------
# softmax_rows_ (f32) and softmax_rows_bf16_
# ---------------------------------------------------------------------------

SOFTMAX_ROWS, SOFTMAX_COLS = 40, 1000      # cols: no multiple of 256
SOFTMAX_CASES = {
    # name: (col_offset, causal, row_mod, with row_limits)
    "limits_only": (0, False, 0, True),             # as the encoder calls it
    "causal_row_mod": (3, True, 7, False),
    "causal_and_limits": (5, True, 0, True),
}
# row 7: every in-limit score -inf (all-zero row, not NaN); row 8: some
SOFTMAX_NEG_INF_ROW, SOFTMAX_PART_INF_ROW = 7, 8


def masked_softmax64(s64, limit):
    """Softmax over columns < limit[row]; other columns exactly 0; a row
    with no finite in-limit score is all zeros."""
    cols = s64.shape[1]
    keep = torch.arange(cols).unsqueeze(0) < limit.unsqueeze(1)
    s = s64.masked_fill(~keep, float("-inf"))
    m = s.max(dim=-1, keepdim=True).values
    m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
    e = torch.exp(s - m)
    tot = e.sum(-1, keepdim=True)
    out = torch.where(tot > 0, e / tot.clamp(min=1e-300), torch.zeros_like(e))
    return out, keep


@functools.lru_cache(maxsize=None)
def softmax_case(name):
    """-> (scores f32, row_limits i32 or None, f64 reference, keep mask)."""
    col_offset, causal, row_mod, with_limits = SOFTMAX_CASES[name]
    rows, cols = SOFTMAX_ROWS, SOFTMAX_COLS
    g = _gen(4000 + sorted(SOFTMAX_CASES).index(name))
    scores = torch.randn(rows, cols, generator=g) * 4
    limits = None
    eff = torch.full((rows,), cols, dtype=torch.int64)
    if causal:
        r = torch.arange(rows)
        pos = r % row_mod if row_mod > 0 else r
        eff = torch.minimum(eff, pos + col_offset + 1)
    if with_limits:
        limits = torch.randint(0, cols + 1, (rows,), generator=g,
                               dtype=torch.int32)
        edge = [0, 1, 255, 256, 257, cols, cols + 1]
        limits[:len(edge)] = torch.tensor(edge, dtype=torch.int32)
        limits[SOFTMAX_NEG_INF_ROW] = 300
        limits[SOFTMAX_PART_INF_ROW] = 700
        eff = torch.minimum(eff, limits.long())
        scores[SOFTMAX_NEG_INF_ROW, :300] = float("-inf")
        scores[SOFTMAX_PART_INF_ROW, ::2] = float("-inf")
    ref, keep = masked_softmax64(scores.double(), eff)
    return scores, limits, ref, keep


def check_softmax(fn, name, to_dev=lambda t: t):
    col_offset, causal, row_mod, _ = SOFTMAX_CASES[name]
    scores, limits, ref, keep = softmax_case(name)
    s = to_dev(scores.clone())
    fn(s, col_offset, causal, row_mod,
       None if limits is None else to_dev(limits))
    got = s.cpu()
    assert torch.isfinite(got).all(), f"softmax {name}: non-finite output"
    assert (got[~keep] == 0).all(), f"softmax {name}: masked column not 0"
    torch.testing.assert_close(got.double(), ref, atol=1e-6, rtol=1e-5)
    if limits is not None:
        assert (got[SOFTMAX_NEG_INF_ROW] == 0).all()
        assert (got[0] == 0).all()                       # limit 0


@pytest.mark.parametrize("name", sorted(SOFTMAX_CASES))
def test_softmax_rows_cpu(name):
    check_softmax(D.softmax_rows_, name)


SOFTMAX_BF16_COLS = (8, 256, 2056)
SOFTMAX_BF16_SCALES = (0.125, 1.0)


@functools.lru_cache(maxsize=None)
def softmax_bf16_case(cols, scale):
    """-> (scores bf16, limits i32, f64 reference, keep mask)."""
    lims = list(range(18)) + [cols - 1, cols]
    limits = torch.tensor(lims, dtype=torch.int32)
    g = _gen(5000 + cols)
    scores = (torch.randn(len(lims), cols, generator=g) * 4).bfloat16()
    ref, keep = masked_softmax64(scores.double() * scale,
                                 limits.long().clamp(max=cols))
    return scores, limits, ref, keep


def check_softmax_bf16(fn, cols, scale, to_dev=lambda t: t):
    scores, limits, ref, keep = softmax_bf16_case(cols, scale)
    s = to_dev(scores.clone())
    fn(s, scale, to_dev(limits))
    got = s.cpu()
    what = f"softmax_bf16 cols={cols} scale={scale}"
    assert (got[~keep] == 0).all(), f"{what}: masked column not 0"
    assert (got[0] == 0).all(), f"{what}: limit 0 row not all zero"
    assert_bf16_close(got, ref, what)


@pytest.mark.parametrize("scale", SOFTMAX_BF16_SCALES)
@pytest.mark.parametrize("cols", SOFTMAX_BF16_COLS)
def test_softmax_rows_bf16_cpu(cols, scale):
    check_softmax_bf16(D.softmax_rows_bf16_, cols, scale)


# ---------------------------------------------------------------------------
# top-k cosine
# ---------------------------------------------------------------------------

# (N, D, k, Q, seed).  Seeds chosen so that consecutive distinct reference
# scores among the first k+1 are > 1e-4 apart (checked below): then f32 and
# f64 agree on the order.
TOPK_CASES = (
    (5, 64, 5, 1, 6000),         # N == k
    (2048, 64, 16, 3, 6011),     # exactly one block
    (2049, 100, 16, 3, 6015),    # last block holds one doc; D % 64 != 0
    (4099, 1536, 3, 7, 6002),    # lab shape, three blocks
    (2051, 64, 1, 2, 6000),      # k = 1
)
TOPK_MIN_GAP = 1e-4
# bit-identical rows in four different waves of block 0 and in block 1
TOPK_TIE_IDS = (1, 4, 6, 11, 2050)
TOPK_TIE_N, TOPK_TIE_D = 2060, 64
TOPK_TIE_CASES = (("top", 3), ("top", 5), ("below_best", 3),
                  ("below_best", 5))


def _unit(t):
    return t / t.norm(dim=-1, keepdim=True)


def topk_ref64(queries, docs, k):
    """f64 scores, stable descending sort (equal scores: lower index
    first), first k.  Row-by-row reductions, not a matmul: BLAS sums the
    rows of an edge tile in another order, so bit-identical docs would not
    score bit-equal."""
    d64 = docs.double()
    scores = torch.stack([(d64 * q).sum(-1) for q in queries.double()])
    s, i = torch.sort(scores, dim=-1, descending=True, stable=True)
    return s[:, :k], i[:, :k].int(), s


def topk_min_gap(sorted_scores, k):
    """Smallest gap between consecutive distinct scores among the first
    k+1 of each query."""
    head = sorted_scores[:, :k + 1]
    gaps = head[:, :-1] - head[:, 1:]
    gaps = gaps[gaps > 0]
    return float(gaps.min()) if gaps.numel() else float("inf")


@functools.lru_cache(maxsize=None)
def topk_case(N, Dm, k, Q, seed):
    g = _gen(seed)
    docs = _unit(torch.randn(N, Dm, generator=g))
    queries = _unit(torch.randn(Q, Dm, generator=g))
    return queries, docs, topk_ref64(queries, docs, k)


@functools.lru_cache(maxsize=None)
def topk_negated_case():
    """Every doc is -q: all scores are -1 and must beat the -2 sentinel."""
    q = _unit(torch.randn(1, 64, generator=_gen(6100)))
    docs = (-q).repeat(2050, 1).contiguous()
    return q, docs, topk_ref64(q, docs, 4)


@functools.lru_cache(maxsize=None)
def topk_tie_case(kind, k):
    g = _gen(6200)
    docs = _unit(torch.randn(TOPK_TIE_N, TOPK_TIE_D, generator=g))
    q = _unit(torch.randn(1, TOPK_TIE_D, generator=g))
    if kind == "top":             # the copies are the best match
        row = q[0].clone()
    else:                         # one unique best, the copies next
        row = _unit(q[0] + 0.3 * _unit(torch.randn(TOPK_TIE_D, generator=g)))
        docs[100] = q[0]
    for i in TOPK_TIE_IDS:
        docs[i] = row
    return q, docs, topk_ref64(q, docs, k)


def check_topk(fn, queries, docs, k, ref, what, to_dev=lambda t: t):
    ref_s, ref_i, _ = ref
    s, i = fn(to_dev(queries), to_dev(docs), k)
    s, i = s.cpu(), i.cpu()
    assert i.dtype == torch.int32 and (i >= 0).all(), f"{what}: bad id"
    assert torch.equal(i, ref_i), f"{what}: ids {i.tolist()} != " \
        f"{ref_i.tolist()}"
    torch.testing.assert_close(s.double(), ref_s, atol=1e-5, rtol=0)


def expected_tie_ids(kind, k):
    ids = ([] if kind == "top" else [100]) + list(TOPK_TIE_IDS)
    return ids[:k]


@pytest.mark.parametrize("N,Dm,k,Q,seed", TOPK_CASES)
def test_topk_cpu(N, Dm, k, Q, seed):
    queries, docs, ref = topk_case(N, Dm, k, Q, seed)
    assert topk_min_gap(ref[2], k) > TOPK_MIN_GAP
    check_topk(D.topk_cosine, queries, docs, k, ref, f"topk N={N} k={k}")


def test_topk_all_negated_cpu():
    q, docs, ref = topk_negated_case()
    assert ref[1].tolist() == [[0, 1, 2, 3]]
    check_topk(D.topk_cosine, q, docs, 4, ref, "topk negated")


@pytest.mark.parametrize("kind,k", TOPK_TIE_CASES)
def test_topk_ties_lowest_index_first_cpu(kind, k):
    q, docs, ref = topk_tie_case(kind, k)
    assert ref[1].tolist() == [expected_tie_ids(kind, k)]
    assert topk_min_gap(ref[2], k) > TOPK_MIN_GAP
    check_topk(D.topk_cosine, q, docs, k, ref, f"topk ties {kind} k={k}")


def test_topk_k_above_n_raises_cpu():
    queries, docs, _ = topk_case(*TOPK_CASES[0])
    with pytest.raises(RuntimeError):
        D.topk_cosine(queries, docs, 6)


# ---------------------------------------------------------------------------
# window aggregation
# ---------------------------------------------------------------------------

WINDOW_CASES = {
    # name: (n, nkeys, nwin, win_ms, t0, with value, mixed-sign values)
    "span": (2000, 7, 12, 1000, 5000, True, True),
    "negative_t0": (2000, 5, 9, 1000, -123457, True, False),
    "count_only": (2000, 7, 12, 1000, 5000, False, False),
    "one_slot": (600, 1, 1, 250, -77, True, False),
    # above 4096 blocks * 256 threads: the grid-stride loop iterates
    "grid_stride": (1048576 + 777, 64, 288, 300_000, 1_700_000_000_123, True,
                    False),
}


@functools.lru_cache(maxsize=None)
def window_case(name):
    """-> (ts i64, key i32, value f32 or None, counts i64, sums f64,
    per-slot sum of |value|)."""
    n, nkeys, nwin, win, t0, with_value, mixed = WINDOW_CASES[name]
    rng = np.random.default_rng(7000 + sorted(WINDOW_CASES).index(name))
    ts = rng.integers(t0 - 2 * win, t0 + (nwin + 2) * win, n, dtype=np.int64)
    edge = [t0 - 1, t0, t0 + win - 1, t0 + win, t0 + nwin * win - 1,
            t0 + nwin * win]
    ts[:len(edge)] = edge
    key = rng.integers(0, nkeys, n).astype(np.int32)
    value = None
    if with_value:
        value = (rng.standard_normal(n) * 50 if mixed
                 else rng.random(n) * 100).astype(np.float32)
    w = np.floor_divide(ts - t0, win)
    ok = (w >= 0) & (w < nwin)
    counts = np.zeros((nkeys, nwin), dtype=np.int64)
    sums = np.zeros((nkeys, nwin), dtype=np.float64)
    mags = np.zeros((nkeys, nwin), dtype=np.float64)
    np.add.at(counts, (key[ok], w[ok]), 1)
    if with_value:
        np.add.at(sums, (key[ok], w[ok]), value[ok].astype(np.float64))
        np.add.at(mags, (key[ok], w[ok]), np.abs(value[ok]).astype(np.float64))
    # the pre-t0 events exist and the reference drops them
    assert ((ts < t0) & (ts > t0 - win)).any()
    return (torch.from_numpy(ts), torch.from_numpy(key),
            None if value is None else torch.from_numpy(value),
            torch.from_numpy(counts), torch.from_numpy(sums),
            torch.from_numpy(mags))


def check_window(fn, name, to_dev=lambda t: t):
    _, nkeys, nwin, win, t0, _, _ = WINDOW_CASES[name]
    ts, key, value, ref_c, ref_s, mags = window_case(name)
    counts, sums = fn(to_dev(ts), to_dev(key),
                      None if value is None else to_dev(value), t0, win, nwin,
                      nkeys)
    counts, sums = counts.cpu(), sums.cpu()
    assert counts.shape == (nkeys, nwin) and sums.shape == (nkeys, nwin)
    assert torch.equal(counts.long(), ref_c), f"window {name}: counts differ"
    if value is None:
        assert (sums == 0).all()
    # f32 atomics in varying order: 1e-4 of the sum plus 1e-6 of sum |v|
    err = (sums.double() - ref_s).abs()
    bound = 1e-4 * ref_s.abs() + 1e-6 * mags
    assert (err <= bound).all(), f"window {name}: sums off by " \
        f"{float((err - bound).max())} beyond the bound"


@pytest.mark.parametrize("name", sorted(WINDOW_CASES))
def test_window_agg_cpu(name):
    check_window(D.window_agg, name)


def test_window_agg_rejects_bad_arguments_cpu():
    ts, key, value, *_ = window_case("span")
    for args in ((ts, key, value, 0, 0, 4, 7), (ts, key, value, 0, 1000, 0, 7),
                 (ts, key[:-1], value, 0, 1000, 4, 7),
                 (ts, key, value[:-1], 0, 1000, 4, 7)):
        with pytest.raises(RuntimeError):
            D.window_agg(*args)


# ---------------------------------------------------------------------------
# AR anomaly scorer
# ---------------------------------------------------------------------------

# 1, 2, 5: mean/std fallback; 6, 7, 11: p=1; 12: p=2; 16: p=3; 20: p=4;
# 63, 64, 65: lane wrap; 400: long series
AR_LENGTHS = (1, 2, 5, 6, 7, 11, 12, 16, 20, 63, 64, 65, 400)
AR_ORDERS = (1, 2, 4)
AR_TMAX = 416                 # longer than the longest series
AR_FAMILIES = ("level_100_2", "level_1000_1", "level_20000_5", "constant",
               "ramp", "ramp_noise", "step", "sine")


def ar_series(family, n, rng):
    t = np.arange(n, dtype=np.float64)
    if family.startswith("level_"):
        _, level, noise = family.split("_")
        h = float(level) + rng.normal(0, float(noise), n)
    elif family == "constant":
        h = np.full(n, 1234.5)
    elif family == "ramp":
        h = 500 + 3 * t
    elif family == "ramp_noise":
        h = 500 + 3 * t + rng.normal(0, 2, n)
    elif family == "step":
        h = np.where(t < n // 2, 100.0, 900.0) + rng.normal(0, 1, n)
    elif family == "sine":
        h = 1000 + 50 * np.sin(t / 3) + rng.normal(0, 2, n)
    else:
        raise KeyError(family)
    return h.astype(np.float32)


@functools.lru_cache(maxsize=None)
def ar_case(family):
    """One launch per family: a key per length, ragged in a [K, Tmax]
    matrix whose cells past each length hold NaN, so a read past
    lengths[k] poisons that key's outputs."""
    rng = np.random.default_rng(8000 + AR_FAMILIES.index(family))
    series = np.full((len(AR_LENGTHS), AR_TMAX), np.nan, dtype=np.float32)
    for r, n in enumerate(AR_LENGTHS):
        series[r, :n] = ar_series(family, n, rng)
    lengths = np.asarray(AR_LENGTHS, dtype=np.int32)
    return series, lengths


@functools.lru_cache(maxsize=None)
def ar_reference(family, order):
    series, lengths = ar_case(family)
    return [ar_forecast(series[r, :n].astype(np.float64), order)
            for r, n in enumerate(lengths)]


def check_ar(family, order, fc, se, dof):
    """fc / se / dof: per-key results for ar_case(family) at `order`."""
    ref = ar_reference(family, order)
    bad = []
    for r, n in enumerate(AR_LENGTHS):
        f_ref, se_ref, dof_ref = ref[r]
        what = f"{family} order={order} n={n}"
        if not (np.isfinite(fc[r]) and np.isfinite(se[r])):
            bad.append(f"{what}: non-finite ({fc[r]}, {se[r]})")
            continue
        if int(dof[r]) != dof_ref:
            bad.append(f"{what}: dof {dof[r]} != {dof_ref}")
        if abs(fc[r] - f_ref) > 0.05 * se_ref + 1e-5 * abs(f_ref):
            bad.append(f"{what}: forecast {fc[r]} ref {f_ref} "
                       f"(se_ref {se_ref})")
        if abs(se[r] - se_ref) > max(0.05 * se_ref, 1e-2):
            bad.append(f"{what}: se {se[r]} ref {se_ref}")
    assert not bad, "\n".join(bad)


def fallback_one_pass_f32(h):
    """The mean/std fallback as sum(h^2) - n*mean^2 in f32: the form that
    cancels.  Kept to show that the cases below tell it from two passes."""
    n = np.float32(len(h))
    s = np.float32(0)
    sq = np.float32(0)
    for v in h:
        s = np.float32(s + v)
        sq = np.float32(sq + np.float32(v * v))
    mean = np.float32(s / n)
    var = np.float32(np.float32(sq - np.float32(n * np.float32(mean * mean)))
                     / np.float32(n - 1))
    return float(mean), float(np.sqrt(max(var, np.float32(0))))


def fallback_two_pass_f32(h):
    n = np.float32(len(h))
    s = np.float32(0)
    for v in h:
        s = np.float32(s + v)
    mean = np.float32(s / n)
    sq = np.float32(0)
    for v in h:
        d = np.float32(v - mean)
        sq = np.float32(sq + np.float32(d * d))
    return float(mean), float(np.sqrt(np.float32(sq / np.float32(n - 1))))


@pytest.mark.parametrize("order", AR_ORDERS)
@pytest.mark.parametrize("family", AR_FAMILIES)
def test_ar_reference_on_f32_series(family, order):
    """ar_forecast on the f32 series itself meets the bounds against the
    f64 copy, every reference is finite with se > 0, and no NaN from
    beyond a length leaks in."""
    series, lengths = ar_case(family)
    got = [ar_forecast(series[r, :n], order) for r, n in enumerate(lengths)]
    for f_ref, se_ref, _ in ar_reference(family, order):
        assert np.isfinite(f_ref) and se_ref > 0
    check_ar(family, order, [g[0] for g in got], [g[1] for g in got],
             [g[2] for g in got])


def test_ar_short_series_tell_one_pass_from_two_pass():
    """On the steady families the n = 2 and n = 5 cases reject the
    one-pass f32 variance and accept the two-pass one."""
    one_pass_bad = 0
    for family in ("level_1000_1", "level_20000_5"):
        series, lengths = ar_case(family)
        ref = ar_reference(family, 4)
        for r, n in enumerate(lengths):
            if not 2 <= n < 6:
                continue
            _, se_ref, _ = ref[r]
            _, se2 = fallback_two_pass_f32(series[r, :n])
            assert abs(se2 - se_ref) <= max(0.05 * se_ref, 1e-2)
            _, se1 = fallback_one_pass_f32(series[r, :n])
            one_pass_bad += abs(se1 - se_ref) > max(0.05 * se_ref, 1e-2)
    assert one_pass_bad >= 1


# ---------------------------------------------------------------------------
# hash join
# ---------------------------------------------------------------------------

HASH_TS_MAX = (1 << 40) - 1
# the production call, zero, and past every (clamped) event time
HASH_MIN_TS = (-(1 << 62), 0, 1 << 40)
HASH_CASES = ("single", "n32_cap64", "wraparound", "equal_ts", "clamped_ts",
              "empty_probe")
_M64 = (1 << 64) - 1


def hash_slot(key, mask):
    """The kernel's splitmix64 finalizer, then the table mask."""
    x = (key + 0x9E3779B97F4A7C15) & _M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & _M64
    x ^= x >> 31
    return (x & 0xFFFFFFFF) & mask


@functools.lru_cache(maxsize=None)
def hash_case(name):
    """-> (keys i64, ts i64, probe keys i64)."""
    rng = np.random.default_rng(9000 + HASH_CASES.index(name))
    if name == "single":
        keys, ts, probe = [42], [5], [42, 43, 42]
    elif name == "n32_cap64":             # 2n == 64: the smallest table
        keys = rng.integers(0, 20, 32).tolist()            # duplicates
        ts = rng.integers(0, 1000, 32).tolist()
        probe = list(range(25)) + [(1 << 63) - 1]
    elif name == "wraparound":
        # 8 rows -> capacity 64; every key's home slot is 60..63, so the
        # cluster wraps to slot 0; absent probe keys hash into it too
        home = [k for k in range(1, 4000) if hash_slot(k, 63) >= 60]
        assert len(home) >= 14
        keys, absent = home[:8], home[8:14]
        ts = rng.integers(0, 1000, 8).tolist()
        probe = keys + absent + keys[::-1]
    elif name == "equal_ts":              # same key, equal ts: highest row
        keys = [7, 9, 7, 7, 9, 11, 7]
        ts = [50, 50, 50, 20, 50, 0, 50]
        probe = [7, 9, 11, 13]
    elif name == "clamped_ts":            # -5 -> 0, 2^40+7 -> 2^40-1
        keys = [1, 1, 2, 2, 3, 4]
        ts = [-5, 0, (1 << 40) - 1, (1 << 40) + 7, -5, (1 << 40) + 7]
        probe = [1, 2, 3, 4, 5]
    elif name == "empty_probe":
        keys, ts, probe = [3, 4, 5], [1, 2, 3], []
    else:
        raise KeyError(name)
    assert all(0 <= k < (1 << 63) for k in keys + probe)
    mk = lambda v: torch.tensor(v, dtype=torch.int64)   # noqa: E731
    return mk(keys), mk(ts), mk(probe)


def hash_brute_force(keys, ts, probe, min_ts):
    """Row of the max (clamped ts, row) per probe key, -1 if absent or
    older than min_ts."""
    keys, probe = keys.tolist(), probe.tolist()
    ts = [min(max(t, 0), HASH_TS_MAX) for t in ts.tolist()]
    out = []
    for k in probe:
        cands = [(ts[j], j) for j in range(len(keys)) if keys[j] == k]
        best = max(cands) if cands else None
        out.append(best[1] if best and best[0] >= min_ts else -1)
    return torch.tensor(out, dtype=torch.int32)


def check_hash(name, to_dev=lambda t: t):
    keys, ts, probe = hash_case(name)
    table = D.hash_build(to_dev(keys), to_dev(ts))
    for min_ts in HASH_MIN_TS:
        rows = D.hash_probe(table, to_dev(probe), min_ts).cpu()
        want = hash_brute_force(keys, ts, probe, min_ts)
        assert rows.dtype == torch.int32 and rows.shape == want.shape
        assert torch.equal(rows, want), \
            f"hash {name} min_ts={min_ts}: {rows.tolist()} != {want.tolist()}"
        if min_ts == HASH_MIN_TS[-1]:
            assert (rows == -1).all()
    return table


@pytest.mark.parametrize("name", HASH_CASES)
def test_hash_join_cpu(name):
    check_hash(name)
