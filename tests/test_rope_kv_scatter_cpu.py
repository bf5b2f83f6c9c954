"""dispatch.rope_kv_scatter on CPU tensors: the fallback must equal the
two-step reference (rope_inplace, then kv_scatter of the first T rows)."""

import torch

from quickstart_streaming_agents_amd.ops import cpu_ref
from quickstart_streaming_agents_amd.ops import dispatch as D


def test_rope_kv_scatter_cpu_equals_two_step_reference():
    torch.manual_seed(0)
    QH, KVH, Dh, T, pad, n_pages = 4, 2, 64, 70, 3, 4
    Tq = T + pad
    width = (QH + 2 * KVH) * Dh
    qkv = torch.randn(Tq, width).to(torch.bfloat16)
    cos_t, sin_t = cpu_ref.rope_tables(256, Dh)
    cos_t, sin_t = cos_t.float(), sin_t.float()
    pos = torch.randint(0, 256, (Tq,)).int()
    # a run starting mid-page in page 2, continuing in page 0
    slots = torch.tensor(
        [2 * 64 + 37 + i for i in range(27)] + list(range(T - 27)),
        dtype=torch.int32)

    def views(buf):
        q = buf[:, :QH * Dh].view(Tq, QH, Dh)
        k = buf[:, QH * Dh:(QH + KVH) * Dh].view(Tq, KVH, Dh)
        v = buf[:, (QH + KVH) * Dh:].view(Tq, KVH, Dh)
        return q, k, v

    def caches():
        return (torch.full((n_pages, KVH, Dh // 8, 64, 8), -7.0,
                           dtype=torch.bfloat16),
                torch.full((n_pages, KVH, Dh, 64), -7.0,
                           dtype=torch.bfloat16))

    a = qkv.clone()
    qa, ka, va = views(a)
    kca, vca = caches()
    D.rope_inplace(qa, ka, cos_t, sin_t, pos)
    D.kv_scatter(ka[:T], va[:T], kca, vca, slots)

    b = qkv.clone()
    qb, kb, vb = views(b)
    kcb, vcb = caches()
    D.rope_kv_scatter(qb, kb, vb, kcb, vcb, cos_t, sin_t, pos, slots)

    assert torch.equal(qb, qa)
    assert torch.equal(kcb, kca)
    assert torch.equal(vcb, vca)
    # pad rows of q were rotated too, and only T slots were written
    assert not torch.equal(qb[T:], views(qkv)[0][T:])
    assert (vcb[:, 0, 0] != -7.0).sum().item() == T
