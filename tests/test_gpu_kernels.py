"""Numerics: each HIP kernel vs its plain-PyTorch fp32 reference.

All tests are @pytest.mark.gpu (MI355X only).  Tolerances account for
bf16 I/O (rel ~1e-2 on normalized magnitudes).
"""

import numpy as np
import pytest
import torch

from quickstart_streaming_agents_amd.ops import cpu_ref
from test_kernel_edges import assert_bf16_close, rmsnorm_ref64

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ext():
    from quickstart_streaming_agents_amd.ops import ext as get_ext
    return get_ext()


def dev():
    return "cuda:0"


def test_rmsnorm(ext):
    torch.manual_seed(0)
    x = torch.randn(33, 4096, dtype=torch.bfloat16, device=dev())
    w = torch.randn(4096, dtype=torch.bfloat16, device=dev())
    y = ext.rmsnorm(x, w, 1e-5)
    ref, _ = rmsnorm_ref64(x.cpu(), w.cpu(), 1e-5)
    assert_bf16_close(y, ref, "rmsnorm")
    # the f32 reference agrees with the f64 one far inside a bf16 ulp
    torch.testing.assert_close(cpu_ref.rmsnorm_ref(x.cpu(), w.cpu()).double(),
                               ref, atol=1e-6, rtol=1e-5)


def test_rmsnorm_residual(ext):
    torch.manual_seed(1)
    x = torch.randn(17, 4096, dtype=torch.bfloat16, device=dev())
    res = torch.randn(17, 4096, dtype=torch.bfloat16, device=dev())
    w = torch.randn(4096, dtype=torch.bfloat16, device=dev())
    ref_y, ref_res = cpu_ref.rmsnorm_ref(x.cpu(), w.cpu(), residual=res.cpu())
    ref64, r = rmsnorm_ref64(x.cpu(), w.cpu(), 1e-5, res.cpu())
    y = ext.rmsnorm_residual(x, res, w, 1e-5)
    assert_bf16_close(y, ref64, "rmsnorm_residual")
    # updated residual: one exact f32 add, one rounding -> bit-equal
    assert torch.equal(res.cpu(), r)
    assert torch.equal(ref_res, r.float())
    torch.testing.assert_close(ref_y.double(), ref64, atol=1e-6, rtol=1e-5)


def test_swiglu(ext):
    torch.manual_seed(2)
    g = torch.randn(64, 14336, dtype=torch.bfloat16, device=dev())
    u = torch.randn(64, 14336, dtype=torch.bfloat16, device=dev())
    y = ext.swiglu(g, u)
    ref = cpu_ref.swiglu_ref(g.cpu(), u.cpu())
    torch.testing.assert_close(y.float().cpu(), ref, atol=5e-2, rtol=5e-2)


def test_rope(ext):
    torch.manual_seed(3)
    B, QH, KVH, D = 9, 8, 2, 128
    cos_t, sin_t = cpu_ref.rope_tables(512, D)
    q = torch.randn(B, QH, D, dtype=torch.bfloat16, device=dev())
    k = torch.randn(B, KVH, D, dtype=torch.bfloat16, device=dev())
    pos = torch.randint(0, 512, (B,), dtype=torch.int32, device=dev())
    q_ref = cpu_ref.rope_ref(q.cpu(), pos.cpu(), cos_t, sin_t)
    k_ref = cpu_ref.rope_ref(k.cpu(), pos.cpu(), cos_t, sin_t)
    ext.rope_inplace(q, k, cos_t.to(dev()), sin_t.to(dev()), pos)
    torch.testing.assert_close(q.float().cpu(), q_ref, atol=3e-2, rtol=3e-2)
    torch.testing.assert_close(k.float().cpu(), k_ref, atol=3e-2, rtol=3e-2)


def test_softmax_rows(ext):
    torch.manual_seed(4)
    s = torch.randn(32, 1000, dtype=torch.float32, device=dev()) * 4
    ref = cpu_ref.softmax_rows_ref(s.cpu(), col_offset=500, causal=True)
    ext.softmax_rows_(s, 500, True)
    torch.testing.assert_close(s.cpu(), ref, atol=1e-5, rtol=1e-4)


def _make_paged_kv(B, KVH, D, seq_lens, npages_total):
    torch.manual_seed(7)
    kc = torch.randn(npages_total, KVH, D // 8, 64, 8, dtype=torch.bfloat16,
                     device=dev())
    vc = torch.randn(npages_total, KVH, D, 64, dtype=torch.bfloat16, device=dev())
    max_pages = max((s + 63) // 64 for s in seq_lens)
    bt = torch.zeros(B, max_pages, dtype=torch.int32, device=dev())
    nxt = 0
    for b, s in enumerate(seq_lens):
        for p in range((s + 63) // 64):
            bt[b, p] = nxt % npages_total
            nxt += 1
    return kc, vc, bt


def test_paged_attn_decode(ext):
    B, QH, KVH, D = 4, 32, 8, 128
    seq_lens = [1, 64, 129, 500]
    kc, vc, bt = _make_paged_kv(B, KVH, D, seq_lens, 64)
    q = torch.randn(B, QH, D, dtype=torch.bfloat16, device=dev())
    sl = torch.tensor(seq_lens, dtype=torch.int32, device=dev())
    scale = 1.0 / (D ** 0.5)
    out = ext.paged_attn_decode(q, kc, vc, bt, sl, scale)
    ref = cpu_ref.paged_attn_ref(q.cpu(), kc.cpu(), vc.cpu(), bt.cpu(),
                                 sl.cpu(), scale)
    torch.testing.assert_close(out.float().cpu(), ref, atol=2e-2, rtol=2e-2)


def test_kv_append_then_attend(ext):
    B, QH, KVH, D = 2, 8, 2, 128
    seq_lens = [65, 120]
    kc, vc, bt = _make_paged_kv(B, KVH, D, seq_lens, 16)
    knew = torch.randn(B, KVH, D, dtype=torch.bfloat16, device=dev())
    vnew = torch.randn(B, KVH, D, dtype=torch.bfloat16, device=dev())
    sl = torch.tensor(seq_lens, dtype=torch.int32, device=dev())
    ext.kv_append(knew, vnew, kc, vc, bt, sl)
    # verify the append landed where the reference expects
    for b, s in enumerate(seq_lens):
        pos = s - 1
        page = int(bt[b, pos // 64])
        pin = pos % 64
        got_v = vc[page, :, :, pin].float().cpu()
        torch.testing.assert_close(got_v, vnew[b].float().cpu(), atol=1e-3,
                                   rtol=1e-3)
        got_k = kc[page, :, :, pin, :].reshape(KVH, D).float().cpu()
        torch.testing.assert_close(got_k, knew[b].float().cpu(), atol=1e-3,
                                   rtol=1e-3)


def test_kv_scatter(ext):
    KVH, D = 2, 128
    T = 100
    kc = torch.zeros(4, KVH, D // 8, 64, 8, dtype=torch.bfloat16, device=dev())
    vc = torch.zeros(4, KVH, D, 64, dtype=torch.bfloat16, device=dev())
    knew = torch.randn(T, KVH, D, dtype=torch.bfloat16, device=dev())
    vnew = torch.randn(T, KVH, D, dtype=torch.bfloat16, device=dev())
    slots = torch.arange(T, dtype=torch.int32, device=dev()) + 28
    ext.kv_scatter(knew, vnew, kc, vc, slots)
    t = 40
    slot = int(slots[t])
    got = vc[slot // 64, :, :, slot % 64].float().cpu()
    torch.testing.assert_close(got, vnew[t].float().cpu(), atol=1e-3, rtol=1e-3)
    # every token's K and V bit-equal at its slot (slots 28..127 cross the
    # page-0 / page-1 boundary), every other slot of the 4 pages still zero
    kc_h, vc_h = kc.cpu(), vc.cpu()
    knew_h, vnew_h = knew.cpu(), vnew.cpu()
    for t, slot in enumerate(slots.tolist()):
        page, off = slot // 64, slot % 64
        assert torch.equal(kc_h[page, :, :, off, :].reshape(KVH, D),
                           knew_h[t]), f"K of token {t}"
        assert torch.equal(vc_h[page, :, :, off], vnew_h[t]), f"V of token {t}"
        kc_h[page, :, :, off, :] = 0
        vc_h[page, :, :, off] = 0
    assert not kc_h.any() and not vc_h.any()


def test_topk_cosine(ext):
    torch.manual_seed(5)
    Q, N, D, k = 7, 20000, 1536, 3
    docs = torch.randn(N, D, device=dev())
    docs = docs / docs.norm(dim=-1, keepdim=True)
    qs = torch.randn(Q, D, device=dev())
    qs = qs / qs.norm(dim=-1, keepdim=True)
    s, i = ext.topk_cosine(qs, docs, k)
    rs, ri = cpu_ref.topk_cosine_ref(qs.cpu(), docs.cpu(), k)
    torch.testing.assert_close(s.cpu(), rs, atol=1e-4, rtol=1e-4)
    assert torch.equal(i.cpu(), ri)


def test_window_agg(ext):
    torch.manual_seed(6)
    n, nkeys, nwin = 50000, 7, 288
    win = 300_000
    ts = torch.randint(0, nwin * win, (n,), dtype=torch.int64, device=dev())
    key = torch.randint(0, nkeys, (n,), dtype=torch.int32, device=dev())
    val = torch.rand(n, dtype=torch.float32, device=dev()) * 100
    counts, sums = ext.window_agg(ts, key, val, 0, win, nwin, nkeys)
    rc, rs = cpu_ref.window_agg_ref(ts.cpu(), key.cpu(), val.cpu(), 0, win,
                                    nwin, nkeys)
    assert torch.equal(counts.cpu(), rc)
    torch.testing.assert_close(sums.cpu(), rs, atol=1e-1, rtol=1e-4)


def test_anomaly_batch_matches_cpu(ext):
    from quickstart_streaming_agents_amd.runtime.anomaly import ar_forecast
    rng = np.random.default_rng(0)
    K, Tmax = 16, 400
    series = np.zeros((K, Tmax), dtype=np.float32)
    lengths = np.zeros(K, dtype=np.int32)
    for kk in range(K):
        n = int(rng.integers(10, Tmax))
        lengths[kk] = n
        base = rng.uniform(10, 1000)
        series[kk, :n] = base + rng.normal(0, base * 0.02, n).astype(np.float32)
    s_t = torch.from_numpy(series).to(dev())
    l_t = torch.from_numpy(lengths).to(dev())
    fc, se, dof = ext.anomaly_batch(s_t, l_t, 4)
    for kk in range(K):
        f_ref, se_ref, dof_ref = ar_forecast(
            series[kk, :lengths[kk]].astype(np.float64), 4)
        assert dof[kk].item() == dof_ref
        assert abs(fc[kk].item() - f_ref) < max(3e-3 * abs(f_ref), 1e-2)
        assert abs(se[kk].item() - se_ref) < max(0.05 * se_ref, 1e-2)


def test_skinny_gemm_matches_linear():
    """Weight-streaming decode GEMM vs fp32 reference: both split-K (small
    N) and single-pass (large N) paths, ragged M."""
    import torch.nn.functional as F
    from quickstart_streaming_agents_amd.ops import ext
    torch.manual_seed(3)
    for M, N, K in [(24, 4096, 4096), (1, 512, 512), (32, 1024, 256),
                    (17, 28672, 512)]:
        a = torch.randn(M, K, device="cuda:0", dtype=torch.bfloat16) * 0.5
        w = torch.randn(N, K, device="cuda:0", dtype=torch.bfloat16) * 0.02
        wf = ext().pack_weight_frag(w)
        out = ext().skinny_gemm(a, wf, N, K)
        ref = a.float() @ w.float().T
        err = (out.float() - ref).abs().max().item()
        scale = ref.abs().max().item() + 1e-6
        assert err / scale < 2e-2, f"M{M} N{N} K{K}: rel err {err/scale}"


def test_skinny_gemm_strided_rows():
    """Row-strided activations (views into a larger buffer) work."""
    from quickstart_streaming_agents_amd.ops import ext
    torch.manual_seed(4)
    buf = torch.randn(8, 1024, device="cuda:0", dtype=torch.bfloat16)
    a = buf[:, :512]
    w = torch.randn(256, 512, device="cuda:0", dtype=torch.bfloat16) * 0.05
    wf = ext().pack_weight_frag(w)
    assert not a.is_contiguous() and a.stride(0) == 1024
    out = ext().skinny_gemm(a, wf, 256, 512)
    ref = a.float() @ w.float().T
    assert (out.float() - ref).abs().max().item() < 2e-2 * (
        ref.abs().max().item() + 1e-6)


def test_softmax_rows_bf16_matches_ref():
    from quickstart_streaming_agents_amd.ops import dispatch as D
    torch.manual_seed(9)
    rows, cols = 300, 256
    scores = torch.randn(rows, cols, device="cuda:0",
                         dtype=torch.bfloat16) * 4
    limits = torch.randint(0, cols + 1, (rows,), dtype=torch.int32,
                           device="cuda:0")
    ref = scores.clone().cpu()
    lim_cpu = limits.cpu()
    D.softmax_rows_bf16_(ref, 0.125, lim_cpu)          # CPU reference path
    D.softmax_rows_bf16_(scores, 0.125, limits)        # HIP kernel
    got = scores.cpu().float()
    torch.testing.assert_close(got, ref.float(), atol=2e-2, rtol=2e-2)
    # beyond-limit strictly zero; rows sum to ~1 where limit > 0
    for r in (0, 7, 123):
        lim = int(lim_cpu[r])
        assert (got[r, lim:] == 0).all()
        if lim > 0:
            assert abs(got[r, :lim].sum().item() - 1.0) < 2e-2


def test_rope_kv_append_matches_composed(ext):
    """Fused rope+append == rope_inplace followed by kv_append."""
    import copy
    torch.manual_seed(6)
    B, QH, KVH, D = 5, 8, 2, 128
    from quickstart_streaming_agents_amd.ops import cpu_ref
    cos_t, sin_t = cpu_ref.rope_tables(256, D)
    cos_t, sin_t = cos_t.to(dev()), sin_t.to(dev())
    seq_lens = torch.tensor([3, 64, 65, 1, 120], dtype=torch.int32,
                            device=dev())
    npages = 3
    bt = torch.arange(B * npages, dtype=torch.int32,
                      device=dev()).reshape(B, npages)
    q = torch.randn(B, QH, D, dtype=torch.bfloat16, device=dev())
    k = torch.randn(B, KVH, D, dtype=torch.bfloat16, device=dev())
    v = torch.randn(B, KVH, D, dtype=torch.bfloat16, device=dev())
    kc1 = torch.zeros(B * npages, KVH, D // 8, 64, 8, dtype=torch.bfloat16,
                      device=dev())
    vc1 = torch.zeros(B * npages, KVH, D, 64, dtype=torch.bfloat16,
                      device=dev())
    kc2, vc2 = kc1.clone(), vc1.clone()

    # composed reference
    q2, k2 = q.clone(), k.clone()
    pos = (seq_lens - 1).clamp(min=0).int()
    ext.rope_inplace(q2, k2, cos_t, sin_t, pos)
    ext.kv_append(k2, v, kc2, vc2, bt, seq_lens)
    # fused
    q1 = q.clone()
    ext.rope_kv_append(q1, k, v, kc1, vc1, cos_t, sin_t, bt, seq_lens)

    torch.testing.assert_close(q1, q2)
    torch.testing.assert_close(kc1, kc2)
    torch.testing.assert_close(vc1, vc2)


def test_paged_attention_forced_rescale(ext):
    """Force the online-softmax rescale with per-head divergent maxima at
    a LATE page (guide rule: a rare data-dependent branch needs its own
    test) — this catches per-row/column alpha mix-ups the random-data
    test cannot."""
    torch.manual_seed(8)
    B, QH, KVH, D = 2, 8, 2, 128
    seqlen = 3 * 64  # 3 pages
    kc = torch.randn(8, KVH, D // 8, 64, 8, dtype=torch.bfloat16,
                     device=dev()) * 0.3
    vc = torch.randn(8, KVH, D, 64, dtype=torch.bfloat16, device=dev())
    q = torch.randn(B, QH, D, dtype=torch.bfloat16, device=dev())
    # spike K at page 2 position 7 so scores jump there; make q for SOME
    # heads align with the spike direction and others anti-align
    spike = torch.randn(D, device=dev(), dtype=torch.bfloat16) * 3
    kc[2 + 3, :, :, 7, :] = spike.reshape(D // 8, 8).unsqueeze(0) * 2
    kc[2, :, :, 7, :] = spike.reshape(D // 8, 8).unsqueeze(0) * 2
    for h in range(QH):
        sgn = 1.0 if h % 2 == 0 else -1.0
        q[:, h] = sgn * spike + torch.randn(D, device=dev(),
                                            dtype=torch.bfloat16) * 0.2
    bt = torch.tensor([[0, 1, 2], [3, 4, 5]], dtype=torch.int32,
                      device=dev())
    sl = torch.tensor([seqlen, seqlen - 10], dtype=torch.int32,
                      device=dev())
    out = ext.paged_attn_decode(q, kc, vc, bt, sl, 0.088)
    ref = cpu_ref.paged_attn_ref(q.cpu(), kc.cpu(), vc.cpu(), bt.cpu(),
                                 sl.cpu(), 0.088)
    torch.testing.assert_close(out.float().cpu(), ref.float(), atol=4e-2,
                               rtol=4e-2)


def test_skinny_gemm_fp8_matches_dequant_ref():
    """fp8 (e4m3, per-channel W8A16) decode GEMM vs the dequantized fp32
    reference: the in-kernel cvt_pk_f32_fp8 + perm pack is exact, so the
    only tolerance is MFMA accumulation order."""
    from quickstart_streaming_agents_amd.ops import dispatch as D
    from quickstart_streaming_agents_amd.ops import ext
    torch.manual_seed(5)
    for M, N, K in [(24, 4096, 4096), (1, 512, 512), (32, 1024, 256),
                    (17, 28672, 512), (24, 128, 14336)]:
        a = torch.randn(M, K, device="cuda:0", dtype=torch.bfloat16) * 0.5
        w = torch.randn(N, K, device="cuda:0", dtype=torch.bfloat16) * 0.02
        qf, s = D.pack_weight_fp8(w)
        out = ext().skinny_gemm_fp8(a, qf, s, N, K)
        wd = D.unpack_weight_fp8(qf, s, N, K)      # exact dequant (f32)
        ref = a.float() @ wd.T
        err = (out.float() - ref).abs().max().item()
        scale = ref.abs().max().item() + 1e-6
        assert err / scale < 2e-2, f"M{M} N{N} K{K}: rel err {err/scale}"
        # quantization error vs the unquantized weights is bounded (e4m3
        # per-channel: ~0.5-3% on random normal weights)
        ref_bf = a.float() @ w.float().T
        qerr = (out.float() - ref_bf).abs().max().item() / \
            (ref_bf.abs().std().item() + 1e-6)
        assert qerr < 0.5, f"quantization error blew up: {qerr}"


def test_skinny_gemm_fp8_gpu_pack_matches_cpu_pack():
    """CPU and GPU packs agree in VALUE (the f32->e4m3 cast may round
    ties differently across backends; one e4m3 quantum of slack)."""
    from quickstart_streaming_agents_amd.ops import dispatch as D
    torch.manual_seed(6)
    w = torch.randn(64, 512, dtype=torch.bfloat16) * 0.02
    qf_cpu, s_cpu = D.pack_weight_fp8(w)
    qf_gpu, s_gpu = D.pack_weight_fp8(w.cuda())
    assert torch.allclose(s_cpu, s_gpu.cpu())
    wd_cpu = D.unpack_weight_fp8(qf_cpu, s_cpu, 64, 512)
    wd_gpu = D.unpack_weight_fp8(qf_gpu.cpu(), s_gpu.cpu(), 64, 512)
    # quantum = scale * 2^-3 at the value's binade; bound by per-channel
    # scale * max step (values <= 448 * s -> step <= 32 * s)
    step = (s_cpu[:, None] * 32.0)
    assert ((wd_cpu - wd_gpu).abs() <= step + 1e-12).all()
    frac_diff = (qf_cpu != qf_gpu.cpu()).float().mean().item()
    assert frac_diff < 0.02, f"packs differ on {frac_diff:.1%} of bytes"


def test_llama_decode_uses_fp8_path():
    """The flagship decode path must run the fp8 kernel by default (the
    driver's native-code check: no silent bf16/rocBLAS fallback)."""
    from quickstart_streaming_agents_amd.models.llama import (LlamaConfig,
                                                              LlamaModel)
    cfg = LlamaConfig.preset("tiny")
    cfg.hidden = 256
    m = LlamaModel(cfg, device="cuda:0", seed=1)
    assert m.use_fp8
    L = m.layers[0]
    assert "wqkv_f8" in L and "wgu_f8" in L and "wdown_f8" in L
    assert m.lm_head_f8 is not None
    # numerics: one decode-shaped _linear call routes through fp8 and
    # stays close to the bf16 matmul
    x = torch.randn(8, cfg.hidden, device="cuda:0",
                    dtype=torch.bfloat16) * 0.5
    out = m._linear(x, L["wqkv"], None, L["wqkv_f8"])
    ref = x.float() @ L["wqkv"].float().T
    rel = (out.float() - ref).abs().max().item() / \
        (ref.abs().std().item() + 1e-6)
    assert rel < 0.5


def test_varlen_attention_noncausal_matches_torch():
    """Bidirectional (CAUSAL=false) varlen flash attention vs a dense
    torch reference over ragged items — the encoder's K1 attention."""
    from quickstart_streaming_agents_amd.ops import dispatch as D
    from quickstart_streaming_agents_amd.ops import ext
    torch.manual_seed(0)
    dev = "cuda:0"
    QH = KVH = 8
    Dh = 64
    lens = [37, 64, 5, 130, 1]
    n, L = len(lens), max(lens)
    ppi = (L + 63) // 64
    scale = Dh ** -0.5
    T = n * L
    q = torch.randn(T, QH, Dh, device=dev, dtype=torch.bfloat16) * 0.5
    k = torch.randn(T, KVH, Dh, device=dev, dtype=torch.bfloat16) * 0.5
    v = torch.randn(T, KVH, Dh, device=dev, dtype=torch.bfloat16) * 0.5
    kc = torch.zeros(n * ppi, KVH, Dh // 8, 64, 8, device=dev,
                     dtype=torch.bfloat16)
    vc = torch.zeros(n * ppi, KVH, Dh, 64, device=dev,
                     dtype=torch.bfloat16)
    slots = torch.arange(n * ppi * 64, dtype=torch.int32, device=dev) \
        .reshape(n, ppi * 64)[:, :L].reshape(-1).contiguous()
    D.kv_scatter(k, v, kc, vc, slots)
    bt = torch.arange(n * ppi, dtype=torch.int32, device=dev) \
        .reshape(n, ppi).contiguous()
    qb_item, qb_pos0 = [], []
    for i in range(n):
        for p0 in range(0, lens[i], 16):
            qb_item.append(i)
            qb_pos0.append(p0)
    mk = lambda x: torch.tensor(x, dtype=torch.int32, device=dev)
    for causal in (False, True):
        out = ext().paged_attn_prefill(
            q, kc, vc, bt, mk(qb_item), mk(qb_pos0),
            mk([i * L for i in range(n)]), mk([0] * n), mk(lens), scale,
            causal)
        for i in range(n):
            li = lens[i]
            qi = q[i * L:i * L + li].float()
            ki = k[i * L:i * L + li].float()
            vi = v[i * L:i * L + li].float()
            sc = torch.einsum("qhd,khd->hqk", qi, ki) * scale
            if causal:
                m = torch.triu(torch.ones(li, li, device=dev,
                                          dtype=torch.bool), 1)
                sc = sc.masked_fill(m.unsqueeze(0), float("-inf"))
            p = sc.softmax(-1)
            ref = torch.einsum("hqk,khd->qhd", p, vi).reshape(li, QH * Dh)
            got = out[i * L:i * L + li].float()
            rel = (got - ref).abs().max().item() / \
                (ref.abs().max().item() + 1e-9)
            assert rel < 2e-2, f"causal={causal} item {i}: rel {rel}"


def test_hash_join_gpu_matches_cpu_semantics():
    """K8 hash build/probe on GPU vs the CPU dispatch fallback: random
    keys with duplicates, latest-event-time-wins, TTL cutoff."""
    from quickstart_streaming_agents_amd.ops import dispatch as D
    torch.manual_seed(11)
    N, M = 5000, 3000
    keys = torch.randint(0, 1500, (N,), dtype=torch.int64)  # many dups
    ts = torch.randint(0, 1_000_000, (N,), dtype=torch.int64)
    probe = torch.randint(0, 2000, (M,), dtype=torch.int64)  # some misses
    cutoff = 400_000
    cpu_table = D.hash_build(keys, ts)
    cpu_rows = D.hash_probe(cpu_table, probe, cutoff)
    gpu_table = D.hash_build(keys.cuda(), ts.cuda())
    gpu_rows = D.hash_probe(gpu_table, probe.cuda(), cutoff).cpu()
    assert torch.equal(cpu_rows, gpu_rows)
    # spot-check semantics: row returned is the max-(ts, idx) for its key
    for i in range(0, M, 137):
        r = int(cpu_rows[i])
        k = int(probe[i])
        cands = [(int(ts[j]), j) for j in range(N) if int(keys[j]) == k]
        if not cands:
            assert r == -1
            continue
        best_ts, best_j = max(cands)
        if best_ts >= cutoff:
            assert r == best_j
        else:
            assert r == -1


def test_lab1_gpu_join_pipeline_matches_cpu():
    """lab1 enriched_orders through the GPU hash-join kernels == CPU."""
    from quickstart_streaming_agents_amd.labs import datagen, pipelines
    from quickstart_streaming_agents_amd.wire import Broker
    b1, b2 = Broker(), Broker()
    datagen.publish_lab1(b1)
    datagen.publish_lab1(b2)
    cpu = pipelines.lab1_enriched_orders(b1, use_gpu=False)
    gpu = pipelines.lab1_enriched_orders(b2, use_gpu=True)
    assert cpu == gpu and len(cpu) >= 1


def test_gemm_fp8_batch_matches_dequant_ref():
    """Batched-M fp8 weight-stream GEMM (LDS-staged A, optional split-K)
    vs the dequantized fp32 reference, across the llama decode shapes and
    ragged M values."""
    from quickstart_streaming_agents_amd.ops import dispatch as D
    from quickstart_streaming_agents_amd.ops import ext
    torch.manual_seed(7)
    cases = [
        (192, 6144, 4096, 4),    # qkv at bench batch (split-K)
        (192, 4096, 4096, 4),    # wo
        (192, 28672, 4096, 1),   # wgu
        (192, 4096, 14336, 4),   # wdown
        (33, 4096, 4096, 2),     # just past the skinny cutover
        (256, 1024, 1024, 1),    # full M tile
        (100, 2048, 512, 2),     # ragged M, small K
    ]
    for M, N, K, splitk in cases:
        a = torch.randn(M, K, device="cuda:0", dtype=torch.bfloat16) * 0.5
        w = torch.randn(N, K, device="cuda:0", dtype=torch.bfloat16) * 0.02
        qf, s = D.pack_weight_fp8(w)
        out = ext().gemm_fp8_batch(a, qf, s, N, K, splitk)
        wd = D.unpack_weight_fp8(qf, s, N, K)
        ref = a.float() @ wd.T
        err = (out.float() - ref).abs().max().item()
        rel = err / (ref.abs().max().item() + 1e-6)
        assert rel < 2e-2, f"M{M} N{N} K{K} sk{splitk}: rel {rel}"


def test_llama_batched_decode_routes_fp8():
    """_linear at decode-batch M routes through the batched fp8 kernel
    and matches the bf16 matmul within quantization error."""
    from quickstart_streaming_agents_amd.models.llama import (LlamaConfig,
                                                              LlamaModel)
    cfg = LlamaConfig.preset("tiny")
    m = LlamaModel(cfg, device="cuda:0", seed=2)
    L = m.layers[0]
    x = torch.randn(192, cfg.hidden, device="cuda:0",
                    dtype=torch.bfloat16) * 0.5
    out = m._linear(x, L["wgu"], None, L["wgu_f8"])
    ref = x.float() @ L["wgu"].float().T
    rel = (out.float() - ref).abs().max().item() / \
        (ref.abs().std().item() + 1e-6)
    assert rel < 0.5
