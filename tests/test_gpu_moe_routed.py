"""Routed MoE decode FFN on the GPU (ops/hip/moe.hip, models/mixtral.py).
Everything is exact: the oracles are the project's own single-expert kernels
(skinny_linear, skinny_linear_fp8, swiglu), the dense compute-all-experts
loop and the CPU references of test_moe_routed.py, so no tolerance is
involved anywhere."""

import gc

import pytest
import torch
import torch.nn.functional as F

import test_moe_routed as R
from quickstart_streaming_agents_amd.ops import dispatch as D

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
E4 = 4


def to_dev(t):
    return t.to(DEV)


# ---- dispatch and combine against the CPU cases ----------------------------

@pytest.mark.parametrize("case", R.DISPATCH_CASES, ids=lambda c: c[0])
def test_moe_dispatch(case):
    _, T, E, top_idx, row_live = case
    h = torch.randn(T, 264, generator=torch.Generator().manual_seed(T + E))
    R.check_dispatch(D.moe_dispatch, T, E, top_idx, row_live, h.bfloat16(),
                     to_dev)


@pytest.mark.parametrize("T,E", [(1, 4), (17, 8), (32, 16), (64, 8)])
def test_moe_combine_equals_dense_sum(T, E):
    ys, y, slot, top_idx, top_w = R.combine_case(T, E, 264, 31 * T + E)
    got = D.moe_combine(to_dev(y), to_dev(slot), to_dev(top_idx),
                        to_dev(top_w))
    want_gpu = R.dense_combine([to_dev(v) for v in ys], to_dev(top_idx),
                               to_dev(top_w))
    assert torch.equal(got, want_gpu)
    assert torch.equal(got.cpu(), D.moe_combine(y, slot, top_idx, top_w))


def test_bindings_refuse_bad_arguments():
    h = torch.zeros(65, 256, dtype=torch.bfloat16, device=DEV)
    idx = torch.zeros(65, 2, dtype=torch.int64, device=DEV)
    with pytest.raises(RuntimeError):
        D.moe_dispatch(h, idx, 4)                       # T > 64
    with pytest.raises(RuntimeError):
        D.moe_dispatch(h[:4], idx[:4], 17)              # E > 16
    with pytest.raises(RuntimeError):
        D.moe_dispatch(h[:4], idx[:4].repeat(1, 3), 4)  # k > 4
    with pytest.raises(RuntimeError):
        D.moe_dispatch(h[:4], idx[:4].int(), 4)         # i32 indices
    with pytest.raises(RuntimeError):
        D.moe_dispatch(h[:4].float(), idx[:4], 4)       # f32 rows
    counts = torch.zeros(4, dtype=torch.int32, device=DEV)
    xg = torch.zeros(4, 32, 128, dtype=torch.bfloat16, device=DEV)
    wf = torch.zeros(4, 16 * 128, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(RuntimeError):
        D.moe_skinny_linear(xg, counts, wf, 16, 128)    # K % 256
    xg = torch.zeros(4, 48, 256, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(RuntimeError):
        D.moe_swiglu(xg, counts)                        # cap not 32/64


# ---- grouped GEMMs against the single-expert kernels -----------------------

SHAPES = [(16, 256), (64, 2304), (1024, 256), (256, 512)]
COUNTS = {"cap32-a": (32, [0, 1, 16, 17]), "cap32-b": (32, [32, 0, 17, 1]),
          "cap64": (64, [0, 33, 48, 64])}
GEMM_CASES = [(fmt, n, k, cid)
              for fmt in ("bf16", "fp8")
              for (n, k) in SHAPES + ([(16384, 256)] if fmt == "fp8" else [])
              for cid in COUNTS]


def grouped_inputs(n, k, cap, counts, seed):
    """xg [E, cap, k] with NaN in every row at or past the count, and the
    experts' weights."""
    g = torch.Generator().manual_seed(seed)
    ws = [(torch.randn(n, k, generator=g) * 0.05).bfloat16()
          for _ in range(E4)]
    xg = torch.full((E4, cap, k), float("nan")).bfloat16()
    for e, c in enumerate(counts):
        xg[e, :c] = torch.randn(c, k, generator=g).bfloat16()
    return ws, xg


def skinny_pieces(x, wf, n, k):
    """skinny_linear takes <= 32 rows; rows are independent."""
    return torch.cat([D.skinny_linear(x[i:i + 32], wf, n, k)
                      for i in range(0, x.shape[0], 32)])


@pytest.mark.parametrize("fmt,n,k,cid", GEMM_CASES)
def test_grouped_gemm_equals_single_expert_kernel(fmt, n, k, cid):
    cap, counts = COUNTS[cid]
    ws, xg = grouped_inputs(n, k, cap, counts, n + k + cap)
    xg = to_dev(xg)
    cnt = torch.tensor(counts, dtype=torch.int32, device=DEV)
    if fmt == "fp8":
        qf, sc = (to_dev(t) for t in D.moe_pack_experts(ws, fp8=True))
        out = D.moe_skinny_linear_fp8(xg, cnt, qf, sc, n, k)
    else:
        wf = to_dev(D.moe_pack_experts(ws, fp8=False))
        out = D.moe_skinny_linear(xg, cnt, wf, n, k)
    assert tuple(out.shape) == (E4, cap, n)
    for e, c in enumerate(counts):
        if c == 0:
            continue
        rows = xg[e, :c]
        if fmt == "fp8":
            ref = D.skinny_linear_fp8(rows, qf[e], sc[e], n, k)
        else:
            ref = skinny_pieces(rows, wf[e], n, k)
        assert torch.isfinite(out[e, :c].float()).all(), (e, c)
        assert torch.equal(out[e, :c], ref), (e, c)


@pytest.mark.parametrize("cid", sorted(COUNTS))
def test_moe_swiglu_equals_swiglu_on_live_rows(cid):
    cap, counts = COUNTS[cid]
    f = 264
    g = torch.Generator().manual_seed(cap)
    gu = torch.full((E4, cap, 2 * f), float("nan")).bfloat16()
    for e, c in enumerate(counts):
        gu[e, :c] = (torch.randn(c, 2 * f, generator=g) * 3).bfloat16()
    gu = to_dev(gu)
    cnt = torch.tensor(counts, dtype=torch.int32, device=DEV)
    act = D.moe_swiglu(gu, cnt)
    assert tuple(act.shape) == (E4, cap, f)
    for e, c in enumerate(counts):
        if c:
            ref = D.swiglu(gu[e, :c, :f], gu[e, :c, f:])
            assert torch.isfinite(act[e, :c].float()).all(), (e, c)
            assert torch.equal(act[e, :c], ref), (e, c)


# ---- the model's routed _ffn ----------------------------------------------

def build_model(env):
    from quickstart_streaming_agents_amd.models.mixtral import (MixtralConfig,
                                                                MixtralModel)
    with pytest.MonkeyPatch.context() as mp:
        for key in ("QSA_FP8", "QSA_MOE_ROUTED"):
            mp.delenv(key, raising=False)
        for key, val in env.items():
            mp.setenv(key, val)
        return MixtralModel(MixtralConfig.preset("tiny-moe"), device=DEV,
                            seed=5)


@pytest.fixture(scope="module")
def models():
    """Same seed, same weights: the routed path on the bf16 stream, on the
    fp8 stream (the default), and the dense loop (the parent's path)."""
    return {"bf16": build_model({"QSA_FP8": "0"}),
            "fp8": build_model({}),
            "dense": build_model({"QSA_FP8": "0", "QSA_MOE_ROUTED": "0"})}


def test_knobs_are_read_at_init(models):
    assert "moe_wgu" in models["bf16"].layers[0]
    assert isinstance(models["fp8"].layers[0]["moe_wgu"], tuple)
    assert models["fp8"].layers[0]["moe_wgu"][0].dtype == torch.uint8
    assert models["bf16"].layers[0]["moe_wgu"].dtype == torch.bfloat16
    assert "moe_wgu" not in models["dense"].layers[0]
    assert models["dense"].layers[0]["experts_f"]    # the dense loop's packs


def rand_h(T, seed, hidden=256):
    g = torch.Generator().manual_seed(seed)
    return to_dev(torch.randn(T, hidden, generator=g).bfloat16())


def routing_of(model, L, h):
    """The routing exactly as _ffn computes it."""
    probs = torch.softmax(F.linear(h, L["router"]).float(), dim=-1)
    top_w, top_idx = torch.topk(probs, model._moe_cfg.top_k, dim=-1)
    return top_idx, top_w / top_w.sum(dim=-1, keepdim=True)


def composed_ffn(model, L, h, fp8, live=None):
    """The routed FFN out of the single-expert kernels: gathered rows in
    ascending order, skinny GEMM, D.swiglu, skinny GEMM, then the f32
    combine in torch with separate multiply and add, ascending experts."""
    c = model._moe_cfg
    top_idx, top_w = routing_of(model, L, h)
    out = torch.zeros(h.shape, dtype=torch.float32, device=h.device)
    alive = torch.ones(h.shape[0], dtype=torch.bool, device=h.device) \
        if live is None else live.bool()
    for e in range(c.n_experts):
        hit = (top_idx == e) & alive[:, None]
        rows = hit.any(dim=1).nonzero(as_tuple=True)[0]
        if rows.numel() == 0:
            continue
        x = h[rows]
        if fp8:
            gu = D.skinny_linear_fp8(x, L["moe_wgu"][0][e],
                                     L["moe_wgu"][1][e], 2 * c.ffn, c.hidden)
            act = D.swiglu(gu[:, :c.ffn], gu[:, c.ffn:])
            y = D.skinny_linear_fp8(act, L["moe_wdown"][0][e],
                                    L["moe_wdown"][1][e], c.hidden, c.ffn)
        else:
            gu = skinny_pieces(x, L["moe_wgu"][e], 2 * c.ffn, c.hidden)
            act = D.swiglu(gu[:, :c.ffn], gu[:, c.ffn:])
            y = skinny_pieces(act, L["moe_wdown"][e], c.hidden, c.ffn)
        w = (top_w * hit.float()).sum(dim=1)[rows]   # the one hit's gate
        prod = w[:, None] * y.float()
        out[rows] = out[rows] + prod
    return out.to(h.dtype)


@pytest.mark.parametrize("T", [1, 2, 16, 17, 32])
def test_routed_ffn_equals_dense_loop(models, T):
    with torch.no_grad():
        for li in (0, 1):
            h = rand_h(T, 10 * T + li)
            got = models["bf16"]._ffn(models["bf16"].layers[li], h)
            want = models["dense"]._ffn(models["dense"].layers[li], h)
            assert torch.isfinite(got.float()).all()
            assert torch.equal(got, want)


@pytest.mark.parametrize("fmt,T", [("bf16", 33), ("bf16", 64), ("fp8", 1),
                                   ("fp8", 17), ("fp8", 32), ("fp8", 33),
                                   ("fp8", 64)])
def test_routed_ffn_equals_composition(models, fmt, T):
    m = models[fmt]
    with torch.no_grad():
        h = rand_h(T, 77 + T)
        L = m.layers[0]
        got = m._ffn(L, h)
        assert torch.isfinite(got.float()).all()
        assert torch.equal(got, composed_ffn(m, L, h, fmt == "fp8"))


# A router that reads the routing off the first E hidden dims, so that a test
# decides which experts a row picks: h[t, e] = 8 / 6 on its two experts.
def steer(L, n_experts=4, hidden=256):
    L = dict(L)
    router = torch.zeros(n_experts, hidden)
    for e in range(n_experts):
        router[e, e] = 1.0
    L["router"] = to_dev(router.bfloat16())
    return L


def steered_h(pairs, seed):
    h = torch.randn(len(pairs), 256,
                    generator=torch.Generator().manual_seed(seed)) * 0.5
    for t, (a, b) in enumerate(pairs):
        h[t, a], h[t, b] = 8.0, 6.0
    return to_dev(h.bfloat16())


def poison(L, fmt, experts):
    """NaN (0xFF bytes in fp8, NaN scales) over the given experts' streams."""
    L = dict(L)
    for key in ("moe_wgu", "moe_wdown"):
        if fmt == "fp8":
            qf, sc = L[key][0].clone(), L[key][1].clone()
            for e in experts:
                qf[e] = 0xFF
                sc[e] = float("nan")
            L[key] = (qf, sc)
        else:
            wf = L[key].clone()
            for e in experts:
                wf[e] = float("nan")
            L[key] = wf
    return L


@pytest.mark.parametrize("fmt", ["bf16", "fp8"])
def test_skipped_experts_are_not_read(models, fmt):
    m = models[fmt]
    L = steer(m.layers[0])
    h = steered_h([(0, 2), (2, 0), (0, 2)], 1)      # experts 1, 3: no rows
    with torch.no_grad():
        top_idx, _ = routing_of(m, L, h)
        assert sorted(set(top_idx.flatten().tolist())) == [0, 2]
        clean = m._ffn(L, h)
        got = m._ffn(poison(L, fmt, (1, 3)), h)
        assert torch.isfinite(got.float()).all()
        assert torch.equal(got, clean)
        # the poison is real: on a routed expert it shows
        assert torch.isnan(m._ffn(poison(L, fmt, (2,)), h).float()).any()


def test_same_poison_through_the_dense_loop_gives_nan(models):
    m = models["dense"]
    L = steer(m.layers[0])
    nan_packs = dict(L["experts_f"])
    for e in (1, 3):
        nan_packs[e] = tuple(torch.full_like(p, float("nan"))
                             for p in nan_packs[e])
    L["experts_f"] = nan_packs
    h = steered_h([(0, 2), (2, 0), (0, 2)], 1)
    with torch.no_grad():
        assert torch.isnan(m._ffn(L, h).float()).any()


def ffn_with_live(m, L, h, live):
    m._row_live = live
    try:
        return m._ffn(L, h)
    finally:
        m._row_live = None


@pytest.mark.parametrize("fmt", ["bf16", "fp8"])
def test_dead_rows(models, fmt):
    m = models[fmt]
    L = steer(m.layers[0])
    # experts 1 and 3 are chosen by dead rows only
    pairs = [(0, 2), (1, 3), (2, 0), (3, 1), (0, 2), (1, 0), (2, 3)]
    dead = (1, 3, 5, 6)
    h = steered_h(pairs, 2)
    live = to_dev(R.live_mask(len(pairs), dead))
    with torch.no_grad():
        full = m._ffn(L, h)
        got = ffn_with_live(m, L, h, live)
        for t in range(len(pairs)):
            if t in dead:
                assert torch.equal(got[t], torch.zeros_like(got[t])), t
            else:
                assert torch.equal(got[t], full[t]), t
        assert torch.equal(got, composed_ffn(m, L, h, fmt == "fp8", live))
        poisoned = ffn_with_live(m, poison(L, fmt, (1, 3)), h, live)
        assert torch.equal(poisoned, got)
        # a mask of another length is not this call's: ignored
        assert torch.equal(ffn_with_live(m, L, h, live[:3]), full)


@pytest.mark.parametrize("fmt", ["bf16", "fp8"])
def test_graph_capture_follows_the_routing(models, fmt):
    m = models[fmt]
    L = steer(m.layers[1])
    T = 16
    spread = [(t % 4, (t + 1 + t // 4) % 4) for t in range(T)]
    spread = [(a, b if b != a else (a + 1) % 4) for a, b in spread]
    only01 = [(t % 2, 1 - t % 2) for t in range(T)]
    only23 = [(2 + t % 2, 3 - t % 2) for t in range(T)]
    one = [(3, 0)] * T
    inputs = [steered_h(p, 40 + i)
              for i, p in enumerate((spread, only01, only23, one, spread))]
    static_h = inputs[0].clone()
    with torch.no_grad():
        side = torch.cuda.Stream(device=DEV)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            m._ffn(L, static_h)
        torch.cuda.current_stream().wait_stream(side)
        gc.collect()    # no dead Engine's graphs may be freed in the capture
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            static_out = m._ffn(L, static_h)
        used = []
        for h in inputs:
            static_h.copy_(h)
            graph.replay()
            assert torch.equal(static_out, m._ffn(L, h))
            used.append(sorted(set(routing_of(m, L, h)[0].flatten()
                                   .tolist())))
    assert used == [[0, 1, 2, 3], [0, 1], [2, 3], [0, 3], [0, 1, 2, 3]]


def padded_decode(model, monkeypatch=None):
    """One eager decode step of three sequences in a four-row batch whose
    last row is padding (seq_lens == 0), as the engine's graph rungs are.
    Returns the logits and the row_live masks moe_dispatch was given."""
    seen = []
    if monkeypatch is not None:
        real = D.moe_dispatch

        def spy(h, top_idx, n_experts, row_live=None):
            seen.append(None if row_live is None else row_live.tolist())
            return real(h, top_idx, n_experts, row_live)

        monkeypatch.setattr(D, "moe_dispatch", spy)
    kv = model.new_kv_cache(16)
    prompts = [[1, 5, 9, 13, 17], [2, 4, 6], [7, 8]]
    for sid, p in enumerate(prompts):
        kv.allocate(sid, len(p))
        model.forward_prefill(torch.tensor(p, dtype=torch.int64, device=DEV),
                              kv, sid)
        kv.extend(sid, len(p) + 1)
    ids = [0, 1, 2]
    bt = kv.block_table(ids)
    bt = torch.cat([bt, torch.zeros_like(bt[:1])])
    sl = torch.cat([kv.seq_lens_tensor(ids), torch.zeros_like(
        kv.seq_lens_tensor(ids)[:1])])
    tokens = torch.tensor([21, 22, 23, 0], dtype=torch.int64, device=DEV)
    logits = model.forward_decode(tokens, kv, bt, sl, None)
    assert model._row_live is None          # cleared when the step returns
    return logits, seen


def test_forward_decode_marks_padding_rows_dead(models, monkeypatch):
    dense, _ = padded_decode(models["dense"])
    routed, seen = padded_decode(models["bf16"], monkeypatch)
    n_layers = len(models["bf16"].layers)
    # three prefill calls without a mask, then the decode step with one
    assert seen[:-n_layers] == [None] * (3 * n_layers)
    assert seen[-n_layers:] == [[1, 1, 1, 0]] * n_layers
    assert torch.isfinite(routed[:3].float()).all()
    assert torch.equal(routed[:3], dense[:3])


def test_engine_tokens(models):
    """bf16: the routed engine generates the dense engine's tokens (the
    prompts prefill in <= 32 rows, where the dense loop runs skinny_linear
    too).  Defaults (fp8): deterministic across two engines."""
    from quickstart_streaming_agents_amd.models.serve import Engine
    prompts, lens = [[1, 5, 9, 13], [2, 4, 6], [7]], [6, 6, 4]

    def run(model):
        eng = Engine(model, max_batch=4, max_seq_len=256)
        return eng.generate_batch(prompts, lens)

    routed, dense = run(models["bf16"]), run(models["dense"])
    assert [len(o) for o in routed] == lens
    assert routed == dense
    assert run(models["fp8"]) == run(models["fp8"])
