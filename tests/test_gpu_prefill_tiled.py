"""Tiled prefill attention and fused prefill rope+scatter: both must be
BIT-identical to the kernels they replace (a one-ulp logit change can flip
a greedy token), and the attention also stays within the existing bound of
an fp32 torch reference so that "identical but both wrong" cannot pass.
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"

# (start, len): single rows, sub-tile and tile remainders, page-boundary
# crossings, unaligned cached prefixes, a delta shorter than one tile over
# a multi-page context, tiles whose sub-tiles have different horizons
ITEMS = [(0, 1), (0, 15), (0, 16), (0, 17), (0, 33), (0, 64), (0, 65),
         (0, 130), (63, 2), (64, 1), (100, 33), (130, 70), (200, 5)]

# every (D, QH, KVH, rows) the tiled kernel claims: R % 4 == 0, D 64/128,
# 32-row tiles (and 64-row tiles at D=64)
TILED_SHAPES = [(128, 8, 2, 32), (64, 8, 2, 32), (64, 8, 2, 64),
                (128, 16, 2, 32), (64, 16, 2, 64)]


def _ext():
    from quickstart_streaming_agents_amd.ops import ext
    return ext()


def _mk(x):
    return torch.tensor(x, dtype=torch.int32, device=DEV)


def _maps(lens, rows):
    item, pos0 = [], []
    for i, n in enumerate(lens):
        for p0 in range(0, n, rows):
            item.append(i)
            pos0.append(p0)
    return _mk(item), _mk(pos0)


_CASES = {}


def _case(Dh, QH, KVH):
    """Random caches + q for ITEMS over shuffled, non-contiguous pages;
    built once per shape and shared (never modified)."""
    key = (Dh, QH, KVH)
    if key in _CASES:
        return _CASES[key]
    g = torch.Generator().manual_seed(1234 + Dh + QH)
    starts = [s for s, _ in ITEMS]
    lens = [n for _, n in ITEMS]
    need = [(s + n + 63) // 64 for s, n in ITEMS]
    npmax = max(need)
    n_pages = 2 * sum(need) + 3
    perm = torch.randperm(n_pages, generator=g).tolist()
    bt = torch.zeros(len(ITEMS), npmax, dtype=torch.int32)
    at = 0
    for i, k in enumerate(need):
        bt[i, :k] = torch.tensor(perm[at:at + k], dtype=torch.int32)
        at += k
    T = sum(lens)
    offs = [sum(lens[:i]) for i in range(len(lens))]
    q = (torch.randn(T, QH, Dh, generator=g) * 0.5).to(torch.bfloat16)
    kc = (torch.randn(n_pages, KVH, Dh // 8, 64, 8, generator=g) * 0.5) \
        .to(torch.bfloat16)
    vc = (torch.randn(n_pages, KVH, Dh, 64, generator=g) * 0.5) \
        .to(torch.bfloat16)
    c = dict(q=q.to(DEV), kc=kc.to(DEV), vc=vc.to(DEV), bt=bt.to(DEV),
             bt_cpu=bt, starts=starts, lens=lens, offs=offs,
             scale=Dh ** -0.5)
    _CASES[key] = c
    return c


def _old(c, causal):
    item, pos0 = _maps(c["lens"], 16)
    return _ext().paged_attn_prefill(
        c["q"], c["kc"], c["vc"], c["bt"], item, pos0, _mk(c["offs"]),
        _mk(c["starts"]), _mk(c["lens"]), c["scale"], causal)


def _tiled(c, causal, rows):
    item, pos0 = _maps(c["lens"], rows)
    return _ext().paged_attn_prefill_tiled(
        c["q"], c["kc"], c["vc"], c["bt"], item, pos0, _mk(c["offs"]),
        _mk(c["starts"]), _mk(c["lens"]), c["scale"], causal, rows)


def _torch_ref(c, causal, Dh, QH, KVH):
    """fp32 reference per item, straight from the cache layouts."""
    R = QH // KVH
    outs = []
    for i, (s, n) in enumerate(ITEMS):
        ctx = s + n
        pages = c["bt_cpu"][i, :(ctx + 63) // 64].long().to(DEV)
        k = c["kc"].index_select(0, pages).float()  # [np,KVH,D/8,64,8]
        k = k.permute(1, 0, 3, 2, 4).reshape(KVH, -1, Dh)[:, :ctx]
        v = c["vc"].index_select(0, pages).float()  # [np,KVH,D,64]
        v = v.permute(1, 0, 3, 2).reshape(KVH, -1, Dh)[:, :ctx]
        qi = c["q"][c["offs"][i]:c["offs"][i] + n].float()  # [n,QH,D]
        k = k.repeat_interleave(R, 0)
        v = v.repeat_interleave(R, 0)
        sc = torch.einsum("qhd,hkd->hqk", qi, k) * c["scale"]
        if causal:
            qa = torch.arange(s, s + n, device=DEV).view(1, n, 1)
            ka = torch.arange(ctx, device=DEV).view(1, 1, ctx)
            sc = sc.masked_fill(ka > qa, float("-inf"))
        p = sc.softmax(-1)
        outs.append(torch.einsum("hqk,hkd->qhd", p, v).reshape(n, QH * Dh))
    return outs


@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("Dh,QH,KVH,rows", TILED_SHAPES)
def test_tiled_attention_bit_identical_to_old(Dh, QH, KVH, rows, causal):
    c = _case(Dh, QH, KVH)
    old = _old(c, causal)
    new = _tiled(c, causal, rows)
    assert new.shape == old.shape and new.dtype == torch.bfloat16
    nbad = (new.view(torch.int16) != old.view(torch.int16)).sum().item()
    print(f"D={Dh} QH={QH} KVH={KVH} rows={rows} causal={causal}: "
          f"{nbad} differing elements of {old.numel()}")
    assert torch.equal(new, old)


@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("Dh,QH,KVH,rows",
                         [(128, 8, 2, 32), (64, 8, 2, 32), (64, 8, 2, 64)])
def test_tiled_attention_matches_fp32_reference(Dh, QH, KVH, rows, causal):
    c = _case(Dh, QH, KVH)
    new = _tiled(c, causal, rows)
    refs = _torch_ref(c, causal, Dh, QH, KVH)
    for i, (s, n) in enumerate(ITEMS):
        got = new[c["offs"][i]:c["offs"][i] + n].float()
        rel = (got - refs[i]).abs().max().item() / \
            (refs[i].abs().max().item() + 1e-9)
        print(f"item {i} (start {s}, len {n}): rel {rel:.3e}")
        assert rel < 2e-2, f"causal={causal} item {i}: rel {rel}"


def test_tiled_binding_falls_back_on_unsupported_gqa_ratio():
    """QH=28 / KVH=4 (R=7) is not covered by the tiled kernel: the binding
    must run the old kernel and return its exact output."""
    g = torch.Generator().manual_seed(7)
    Dh, QH, KVH, n = 128, 28, 4, 21
    q = (torch.randn(n, QH, Dh, generator=g) * 0.5).to(torch.bfloat16).to(DEV)
    kc = (torch.randn(3, KVH, Dh // 8, 64, 8, generator=g) * 0.5) \
        .to(torch.bfloat16).to(DEV)
    vc = (torch.randn(3, KVH, Dh, 64, generator=g) * 0.5) \
        .to(torch.bfloat16).to(DEV)
    bt = _mk([[2]])
    args = (_mk([0]), _mk([0]), _mk([n]))
    i16, p16 = _maps([n], 16)
    i32, p32 = _maps([n], 32)
    old = _ext().paged_attn_prefill(q, kc, vc, bt, i16, p16, *args,
                                    Dh ** -0.5, True)
    new = _ext().paged_attn_prefill_tiled(q, kc, vc, bt, i32, p32, *args,
                                          Dh ** -0.5, True, 32)
    assert torch.equal(new, old)


# ---- fused rope + scatter -------------------------------------------------

def _slot_pattern(name, T, n_pages, g):
    if name == "midpage":          # one contiguous run starting mid-page
        return list(range(2 * 64 + 37, 2 * 64 + 37 + T))
    if name == "two_items":        # two items in non-adjacent pages
        a = T // 2
        s = list(range(5 * 64 + 3, 5 * 64 + 3 + a))
        return s + list(range(1 * 64, 1 * 64 + T - a))
    if name == "permuted":         # deliberately non-consecutive
        return torch.randperm(n_pages * 64, generator=g)[:T].tolist()
    raise ValueError(name)


def _rope_scatter_case(Dh, T, pattern, pad):
    from quickstart_streaming_agents_amd.ops import cpu_ref
    g = torch.Generator().manual_seed(T * 131 + Dh + pad)
    QH, KVH, n_pages = 8, 2, 9
    Tq = T + pad
    width = (QH + 2 * KVH) * Dh
    qkv = (torch.randn(Tq, width, generator=g)).to(torch.bfloat16).to(DEV)
    cos_t, sin_t = cpu_ref.rope_tables(1024, Dh)
    cos_t, sin_t = cos_t.float().to(DEV), sin_t.float().to(DEV)
    pos = torch.randint(0, 1024, (Tq,), generator=g).int().to(DEV)
    slots = _mk(_slot_pattern(pattern, T, n_pages, g))
    sentinel = -7.0

    def views(buf):
        q = buf[:, :QH * Dh].view(Tq, QH, Dh)
        k = buf[:, QH * Dh:(QH + KVH) * Dh].view(Tq, KVH, Dh)
        v = buf[:, (QH + KVH) * Dh:].view(Tq, KVH, Dh)
        return q, k, v

    def caches():
        kc = torch.full((n_pages, KVH, Dh // 8, 64, 8), sentinel,
                        dtype=torch.bfloat16, device=DEV)
        vc = torch.full((n_pages, KVH, Dh, 64), sentinel,
                        dtype=torch.bfloat16, device=DEV)
        return kc, vc

    ext = _ext()
    buf_a = qkv.clone()
    qa, ka, va = views(buf_a)
    kca, vca = caches()
    ext.rope_inplace(qa, ka, cos_t, sin_t, pos)
    ext.kv_scatter(ka[:T], va[:T], kca, vca, slots)

    buf_b = qkv.clone()
    qb, kb, vb = views(buf_b)
    kcb, vcb = caches()
    ext.rope_kv_scatter(qb, kb, vb, kcb, vcb, cos_t, sin_t, pos, slots)

    assert torch.equal(qb, qa), "rotated q differs"
    assert torch.equal(kcb, kca), "K cache differs"
    assert torch.equal(vcb, vca), "V cache differs"
    # v and the un-rotated k in the qkv buffer are inputs only
    assert torch.equal(vb, views(qkv)[2])
    assert torch.equal(kb, views(qkv)[1])


@pytest.mark.parametrize("pattern", ["midpage", "two_items", "permuted"])
@pytest.mark.parametrize("T", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("Dh", [64, 128])
def test_rope_kv_scatter_bit_identical_to_two_step(Dh, T, pattern):
    _rope_scatter_case(Dh, T, pattern, pad=0)


@pytest.mark.parametrize("Dh", [64, 128])
def test_rope_kv_scatter_pad_rows(Dh):
    """q longer than slots: pad rows of q are rotated, no cache slot beyond
    the T scattered ones is touched (whole-cache equality with sentinel)."""
    _rope_scatter_case(Dh, 65, "midpage", pad=31)


# ---- model level ----------------------------------------------------------

def _run_prefill(model, v1):
    from quickstart_streaming_agents_amd.models import llama
    from quickstart_streaming_agents_amd.models.kv_cache import PagedKVCache
    c = model.cfg
    kv = PagedKVCache(c.n_layers, model.n_kv, c.d_head, 16, device=DEV)
    g = torch.Generator().manual_seed(5)
    tok = lambda n: torch.randint(1, c.vocab_size, (n,), generator=g).to(DEV)
    old = llama.PREFILL_V1
    llama.PREFILL_V1 = v1
    try:
        # two sequences get their prefixes (70 and 128 positions) first
        kv.allocate(1, 70)
        kv.allocate(2, 128)
        first = model.forward_prefill_batch(
            [(tok(70), 1, 0), (tok(128), 2, 0)], kv)
        # then one fresh item and the two continuations in ONE batch
        kv.allocate(3, 45)
        kv.extend(1, 70 + 37)
        kv.extend(2, 128 + 5)
        logits = model.forward_prefill_batch(
            [(tok(45), 3, 0), (tok(37), 1, 70), (tok(5), 2, 128)], kv)
    finally:
        llama.PREFILL_V1 = old
    torch.cuda.synchronize()
    return first, logits, kv


@pytest.mark.parametrize("n_q", [8, 4])
def test_model_prefill_v1_and_tiled_paths_identical(n_q):
    """forward_prefill_batch through the fused/tiled path equals the
    three-kernel path bit for bit: logits and every layer's caches.  n_q=8
    over 2 kv heads (R=4, D=64) runs the tiled kernel; the stock tiny
    preset (n_q=4, R=2) runs the fused scatter plus the binding's fallback."""
    from quickstart_streaming_agents_amd.models.llama import (LlamaConfig,
                                                              LlamaModel)
    cfg = LlamaConfig.preset("tiny")
    cfg.n_q_heads = n_q
    model = LlamaModel(cfg, device=DEV, seed=3)
    f_old, l_old, kv_old = _run_prefill(model, True)
    f_new, l_new, kv_new = _run_prefill(model, False)
    assert torch.equal(f_new, f_old)
    assert torch.equal(l_new, l_old)
    for li in range(cfg.n_layers):
        assert torch.equal(kv_new.k[li], kv_old.k[li]), f"layer {li} K"
        assert torch.equal(kv_new.v[li], kv_old.v[li]), f"layer {li} V"
