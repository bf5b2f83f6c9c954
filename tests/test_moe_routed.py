"""Routed MoE decode FFN, CPU references (ops/dispatch.py): the dispatch
against a brute-force loop, the combine against the dense masked sum over
all experts, and an FFN composed from the references against
ExpertDispatch.run.  test_gpu_moe_routed.py runs the same cases through the
HIP kernels."""

import pytest
import torch

from quickstart_streaming_agents_amd.ops import dispatch as D


def topk_routing(T, E, k, seed):
    """Random top-k routing as the model computes it: distinct experts per
    row, softmax-renormalised f32 gates."""
    g = torch.Generator().manual_seed(seed)
    probs = torch.softmax(torch.randn(T, E, generator=g), dim=-1)
    top_w, top_idx = torch.topk(probs, k, dim=-1)
    return top_idx, top_w / top_w.sum(dim=-1, keepdim=True)


def pair_routing(T, pair):
    return torch.tensor([list(pair)] * T, dtype=torch.int64)


def live_mask(T, dead):
    m = torch.ones(T, dtype=torch.int32)
    for t in dead:
        m[t] = 0
    return m


# (id, T, E, top_idx, row_live)
def dispatch_cases():
    cases = []
    for T in (1, 17, 64):
        for E in (4, 8):
            cases.append((f"random-T{T}-E{E}", T, E,
                          topk_routing(T, E, 2, 100 * T + E)[0], None))
    for T in (32, 64):   # every row on one expert pair: count == T == cap
        cases.append((f"one-pair-T{T}", T, 4, pair_routing(T, (2, 0)), None))
    idx = topk_routing(17, 3, 2, 7)[0]   # experts 0..2 only: expert 3 empty
    cases.append(("empty-expert", 17, 4, idx, None))
    cases.append(("dead-interleaved", 17, 4, topk_routing(17, 4, 2, 9)[0],
                  live_mask(17, range(0, 17, 2))))
    cases.append(("dead-all-but-last", 64, 8, topk_routing(64, 8, 2, 10)[0],
                  live_mask(64, range(63))))
    return cases


DISPATCH_CASES = dispatch_cases()


def brute_force_dispatch(top_idx, E, row_live):
    """Rows of each expert in ascending row order, by plain loops."""
    T, k = top_idx.shape
    rows_of = [[] for _ in range(E)]
    for e in range(E):
        for t in range(T):
            if row_live is not None and int(row_live[t]) == 0:
                continue
            if any(int(top_idx[t, j]) == e for j in range(k)):
                rows_of[e].append(t)
    return rows_of


def check_dispatch(fn, T, E, top_idx, row_live, h, to_dev=lambda t: t):
    """fn is D.moe_dispatch on either device; h [T, H]."""
    k = top_idx.shape[1]
    counts, slot, xg = fn(to_dev(h), to_dev(top_idx), E,
                          None if row_live is None else to_dev(row_live))
    counts, slot, xg = counts.cpu(), slot.cpu(), xg.cpu()
    cap = 32 if T <= 32 else 64
    assert counts.dtype == torch.int32 and slot.dtype == torch.int32
    assert tuple(xg.shape) == (E, cap, h.shape[1]) and xg.dtype == h.dtype
    rows_of = brute_force_dispatch(top_idx, E, row_live)
    assert counts.tolist() == [len(r) for r in rows_of]
    n_live = T if row_live is None else int(row_live.sum())
    assert int(counts.sum()) == k * n_live
    want = torch.full((T, k), -1, dtype=torch.int32)
    for e, rows in enumerate(rows_of):
        for s, t in enumerate(rows):     # slots ascend with the row index
            for j in range(k):
                if int(top_idx[t, j]) == e:
                    want[t, j] = s
            assert torch.equal(xg[e, s], h[t]), (e, s, t)
    assert torch.equal(slot, want)
    return counts, slot, xg


@pytest.mark.parametrize("case", DISPATCH_CASES, ids=lambda c: c[0])
def test_moe_dispatch_matches_brute_force(case):
    _, T, E, top_idx, row_live = case
    h = torch.randn(T, 64, generator=torch.Generator().manual_seed(T + E))
    counts, _, _ = check_dispatch(D.moe_dispatch, T, E, top_idx, row_live,
                                  h.bfloat16())
    if case[0].startswith("one-pair"):
        assert counts.tolist() == [T, 0, T, 0]
    if case[0] == "empty-expert":
        assert counts[3] == 0


def dense_combine(ys, top_idx, top_w):
    """The dense loop's masked sum: every expert's term, zeros included."""
    T, E = ys[0].shape[0], len(ys)
    gates = torch.zeros(T, E, dtype=torch.float32, device=top_w.device)
    gates.scatter_(1, top_idx, top_w)
    out = torch.zeros(ys[0].shape, dtype=torch.float32, device=top_w.device)
    for e in range(E):
        out += gates[:, e:e + 1] * ys[e].float()
    return out.to(ys[0].dtype)


def combine_case(T, E, H, seed):
    """Per-expert dense outputs ys[e] [T, H] bf16 and the routed buffers
    (y [E, cap, H] with NaN in every unused row, slot) that hold the same
    rows."""
    g = torch.Generator().manual_seed(seed)
    top_idx, top_w = topk_routing(T, E, 2, seed)
    ys = [torch.randn(T, H, generator=g).bfloat16() for _ in range(E)]
    counts, slot, _ = D.moe_dispatch(torch.zeros(T, 8).bfloat16(), top_idx, E)
    y = torch.full((E, D.moe_cap(T), H), float("nan")).bfloat16()
    for t in range(T):
        for j in range(2):
            e = int(top_idx[t, j])
            y[e, int(slot[t, j])] = ys[e][t]
    return ys, y, slot, top_idx, top_w


@pytest.mark.parametrize("T,E", [(1, 4), (17, 8), (64, 8)])
def test_moe_combine_equals_dense_sum(T, E):
    ys, y, slot, top_idx, top_w = combine_case(T, E, 64, 31 * T + E)
    got = D.moe_combine(y, slot, top_idx, top_w)
    assert torch.equal(got, dense_combine(ys, top_idx, top_w))


def test_moe_combine_dead_rows_are_zero():
    T, E = 17, 4
    top_idx, top_w = topk_routing(T, E, 2, 3)
    live = live_mask(T, (0, 5, 16))
    h = torch.randn(T, 64, generator=torch.Generator().manual_seed(4)) \
        .bfloat16()
    counts, slot, xg = D.moe_dispatch(h, top_idx, E, live)
    full = D.moe_combine(D.moe_dispatch(h, top_idx, E)[2],
                         D.moe_dispatch(h, top_idx, E)[1], top_idx, top_w)
    got = D.moe_combine(xg, slot, top_idx, top_w)
    for t in range(T):
        if live[t]:
            assert torch.equal(got[t], full[t])
        else:
            assert torch.equal(got[t], torch.zeros(64).bfloat16())


def routed_ffn(h, top_idx, top_w, E, expert_fn, row_live=None):
    """The routed FFN composed from the references, the experts through
    expert_fn(e, rows) on the gathered rows."""
    counts, slot, xg = D.moe_dispatch(h, top_idx, E, row_live)
    y = torch.zeros_like(xg)
    for e, c in enumerate(counts.tolist()):
        if c:
            y[e, :c] = expert_fn(e, xg[e, :c])
    return D.moe_combine(y, slot, top_idx, top_w)


@pytest.mark.parametrize("T", [1, 17, 64])
def test_routed_ffn_equals_expert_dispatch_run(T):
    """tiny-moe in f32 on the CPU: same expert_fn, same gathered row order,
    same combine arithmetic -> same bits."""
    import torch.nn.functional as F
    from quickstart_streaming_agents_amd.models.mixtral import (MixtralConfig,
                                                                MixtralModel)
    cfg = MixtralConfig.preset("tiny-moe")
    model = MixtralModel(cfg, device="cpu", dtype=torch.float32, seed=3)
    L = model.layers[0]
    assert "moe_wgu" not in L      # the streams are a GPU/bf16 matter
    h = torch.randn(T, cfg.hidden, generator=torch.Generator().manual_seed(T))
    probs = torch.softmax(F.linear(h, L["router"]).float(), dim=-1)
    top_w, top_idx = torch.topk(probs, cfg.top_k, dim=-1)
    top_w = top_w / top_w.sum(dim=-1, keepdim=True)

    def expert_fn(e, rows):
        wgu, wdown = L["experts"][e]
        gu = F.linear(rows, wgu)
        return F.linear(D.swiglu(gu[:, :cfg.ffn], gu[:, cfg.ffn:]), wdown)

    want = model._dispatch.run(h, top_idx, top_w, expert_fn)
    got = routed_ffn(h, top_idx, top_w, cfg.n_experts, expert_fn)
    assert torch.equal(got, want)
    assert torch.equal(model._ffn(L, h), want)   # the CPU model path


def test_moe_pack_experts_stacks_the_single_packs():
    g = torch.Generator().manual_seed(0)
    ws = [(torch.randn(32, 256, generator=g) * 0.05).bfloat16()
          for _ in range(3)]
    wf = D.moe_pack_experts(ws, fp8=False)
    qf, sc = D.moe_pack_experts(ws, fp8=True)
    assert wf.shape[0] == 3 and wf.numel() == 3 * 32 * 256
    assert qf.dtype == torch.uint8 and qf.numel() == 3 * 32 * 256
    assert tuple(sc.shape) == (3, 32) and sc.dtype == torch.float32
    for e, w in enumerate(ws):
        assert torch.equal(wf[e], D.pack_weight_frag(w))
        q1, s1 = D.pack_weight_fp8(w)
        assert torch.equal(qf[e], q1) and torch.equal(sc[e], s1)


def test_grouped_references_touch_live_rows_only():
    """The CPU grouped GEMM and SwiGLU equal the single-expert references
    on the live rows and never look at rows past the count or at experts
    without rows (NaN there must not spread)."""
    E, N, K = 4, 32, 256
    g = torch.Generator().manual_seed(5)
    ws = [(torch.randn(N, K, generator=g) * 0.05).bfloat16() for _ in range(E)]
    counts = torch.tensor([0, 1, 17, 32], dtype=torch.int32)
    xg = torch.full((E, 32, K), float("nan")).bfloat16()
    for e, c in enumerate(counts.tolist()):
        xg[e, :c] = torch.randn(c, K, generator=g).bfloat16()
    wf = D.moe_pack_experts(ws, fp8=False)
    qf, sc = D.moe_pack_experts(ws, fp8=True)
    wf[0] = float("nan")
    sc[0] = float("nan")
    out = D.moe_skinny_linear(xg, counts, wf, N, K)
    out8 = D.moe_skinny_linear_fp8(xg, counts, qf, sc, N, K)
    act = D.moe_swiglu(out, counts)
    for e, c in enumerate(counts.tolist()):
        if not c:
            continue
        ref = D.skinny_linear(xg[e, :c], wf[e], N, K)
        assert torch.equal(out[e, :c], ref)
        assert torch.equal(out8[e, :c], D.skinny_linear_fp8(
            xg[e, :c], qf[e], sc[e], N, K))
        assert torch.equal(act[e, :c], D.swiglu(ref[:, :16], ref[:, 16:]))
    assert torch.isfinite(out.float()).all()
    assert torch.isfinite(out8.float()).all()
