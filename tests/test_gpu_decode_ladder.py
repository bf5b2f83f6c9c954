"""Decode-graph ladder on the GPU: the fused greedy sampler kernel against
the torch ops it replaces, the fp8 skinny GEMM at up to 64 rows and its
row-invariance across m-tile counts, the engine's ladder of decode graphs
against the eager engine, and a captured replay of DecodeGraphs.step against
eager calls of it."""

import pytest
import torch

from test_decode_graph import (LONG_SCRIPT, PROMPTS, RUN, SHORT_SCRIPT,
                               _admit, _graphs)
from test_decode_ladder import (MAX_RUN, SAMPLER_CASES, sampler_case,
                                torch_sequence)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SKINNY_SHAPES = [(512, 512), (1024, 256), (28672, 512), (128, 14336)]


@pytest.fixture(scope="module")
def ext():
    from quickstart_streaming_agents_amd.ops import ext as get_ext
    return get_ext()


# ---- fused sampler ---------------------------------------------------------

def _run_sampler_case(B, V, lo, hi, eos, steps):
    from quickstart_streaming_agents_amd.ops import dispatch as D
    ticket = torch.zeros(1, dtype=torch.int32, device=DEV)
    for step in steps:
        c = sampler_case(B, V, lo, hi, eos, seed=B * 1000 + step, step=step)
        c = {k: (v.to(DEV) if torch.is_tensor(v) else v)
             for k, v in c.items()}
        want_tokens, want_hist, want_ctr = torch_sequence(c)
        tokens, hist, ctr = c["tokens"].clone(), c["hist"].clone(), \
            c["ctr"].clone()
        D.greedy_sample_step(c["logits"], lo, hi,
                             -1 if eos is None else eos, c["script"][:B],
                             c["mask"][:B], ctr, hist[:, :B], tokens, ticket)
        torch.cuda.synchronize()
        assert torch.equal(tokens, want_tokens)
        assert torch.equal(hist, want_hist)
        assert torch.equal(ctr, want_ctr)
        assert int(ticket.item()) == 0      # reset for the next launch


@pytest.mark.parametrize("B,V,lo,hi,eos", SAMPLER_CASES)
def test_sampler_kernel_matches_torch_sequence(B, V, lo, hi, eos):
    _run_sampler_case(B, V, lo, hi, eos, steps=(0, 3, MAX_RUN - 1))


def test_sampler_kernel_full_batch():
    _run_sampler_case(192, 128256, 16, 3335, 2, steps=(1,))


def test_sampler_kernel_unaligned_window_and_whole_vocab():
    # odd lo/hi exercise the scalar head and tail around the vector body;
    # V = 2040 + odd lo puts rows at different 16-byte phases
    _run_sampler_case(7, 2040, 3, 2037, None, steps=(0,))
    _run_sampler_case(7, 2040, 0, 2040, 5, steps=(2,))
    _run_sampler_case(4, 2048, 101, 106, 1, steps=(0,))


# ---- fp8 skinny GEMM up to 64 rows -----------------------------------------

@pytest.fixture(scope="module")
def skinny_data():
    """Per (N, K): 64 activation rows, packed weights and the dequantised
    fp32 reference product, computed once."""
    from quickstart_streaming_agents_amd.ops import dispatch as D
    g = torch.Generator(device=DEV).manual_seed(11)
    out = {}
    for N, K in SKINNY_SHAPES:
        a = (torch.randn(64, K, device=DEV, generator=g) * 0.5) \
            .to(torch.bfloat16)
        w = (torch.randn(N, K, device=DEV, generator=g) * 0.02) \
            .to(torch.bfloat16)
        qf, s = D.pack_weight_fp8(w)
        ref = a.float() @ D.unpack_weight_fp8(qf, s, N, K).T
        out[(N, K)] = (a, qf, s, ref)
    return out


@pytest.mark.parametrize("N,K", SKINNY_SHAPES)
def test_skinny_fp8_rows_up_to_64_match_dequant_ref(ext, skinny_data, N, K):
    a, qf, s, ref = skinny_data[(N, K)]
    for M in (1, 16, 17, 33, 48, 64):
        out = ext.skinny_gemm_fp8(a[:M], qf, s, N, K)
        assert out.shape == (M, N)
        err = (out.float() - ref[:M]).abs().max().item()
        scale = ref[:M].abs().max().item() + 1e-6
        print(f"M{M} N{N} K{K}: rel err {err / scale:.3e}")
        assert err / scale < 2e-2, f"M{M} N{N} K{K}: rel err {err / scale}"


@pytest.mark.parametrize("N,K", SKINNY_SHAPES)
def test_skinny_fp8_row_invariance(ext, skinny_data, N, K):
    """A row's output bits do not depend on the m-tile variant."""
    a, qf, s, _ = skinny_data[(N, K)]
    out64 = ext.skinny_gemm_fp8(a, qf, s, N, K)
    for m in (1, 16, 32):
        outm = ext.skinny_gemm_fp8(a[:m], qf, s, N, K)
        assert torch.equal(out64[:m].view(torch.int16),
                           outm.view(torch.int16)), f"m={m}"


def test_skinny_fp8_rejects_65_rows(ext, skinny_data):
    a, qf, s, _ = skinny_data[(512, 512)]
    a65 = torch.cat([a, a[:1]])
    with pytest.raises(RuntimeError):
        ext.skinny_gemm_fp8(a65, qf, s, 512, 512)


# ---- engine ----------------------------------------------------------------

@pytest.fixture(scope="module")
def tiny_model():
    from quickstart_streaming_agents_amd.models.llama import (LlamaConfig,
                                                              LlamaModel)
    return LlamaModel(LlamaConfig.preset("tiny"), device=DEV)


def _prompts(n):
    g = torch.Generator().manual_seed(3)
    lens = [3 + (67 * i) // max(1, n - 1) for i in range(n)]      # 3..70
    new = [2 + (22 * ((i * 7) % n)) // max(1, n - 1) for i in range(n)]
    prompts = [torch.randint(16, 1000, (L,), generator=g).tolist()
               for L in lens]
    return prompts, new


def _captured(eng):
    """The greedy ladder was captured, every rung of it."""
    return eng.graphs is not None and \
        set(eng.graphs.greedy) == set(eng.graphs.rungs)


def _engine(model, graph):
    from quickstart_streaming_agents_amd.models.serve import Engine
    eng = Engine(model, max_batch=48, max_seq_len=128, eos_id=2,
                 valid_vocab=(16, 1000))
    if not graph:
        eng.use_graph = False
    return eng


@pytest.fixture(scope="module")
def eager_tokens(tiny_model):
    prompts, new = _prompts(20)
    return _engine(tiny_model, graph=False).generate_batch(prompts, new)


def test_engine_ladder_matches_eager(tiny_model, eager_tokens, monkeypatch):
    from quickstart_streaming_agents_amd.models import serve
    monkeypatch.setattr(serve, "DECODE_LADDER", True)
    prompts, new = _prompts(20)
    assert min(new) == 2 and max(new) == 24
    eng = _engine(tiny_model, graph=True)
    out = eng.generate_batch(prompts, new)
    assert _captured(eng), "graph capture failed"
    assert eng.graphs.rungs == serve.ladder_rungs(48)
    assert out == eager_tokens
    by_rung = eng.stats.decode_steps_by_rung
    assert len(by_rung) >= 2, by_rung
    assert sum(by_rung.values()) == eng.stats.decode_steps
    by_live = eng.stats.decode_steps_by_live
    assert sum(by_live.values()) == eng.stats.decode_steps
    assert max(by_live) <= 20


def test_engine_one_prompt_uses_smallest_rung(tiny_model, monkeypatch):
    from quickstart_streaming_agents_amd.models import serve
    monkeypatch.setattr(serve, "DECODE_LADDER", True)
    prompts, new = _prompts(20)
    i = max(range(20), key=lambda r: new[r])
    eng = _engine(tiny_model, graph=True)
    out = eng.generate_batch([prompts[i]], [new[i]])
    assert _captured(eng), "graph capture failed"
    # eager on the same single prompt (the prefill GEMMs are rocBLAS, whose
    # row bits may depend on the other rows of the batch)
    want = _engine(tiny_model, graph=False).generate_batch([prompts[i]],
                                                           [new[i]])
    assert out == want
    assert set(eng.stats.decode_steps_by_rung) == {eng.graphs.rungs[0]}
    assert set(eng.stats.decode_steps_by_live) == {1}


def test_engine_single_graph_switch(tiny_model, eager_tokens, monkeypatch):
    """QSA_DECODE_LADDER=0 semantics: one max_batch graph.  Every tiny
    projection is a wo-class weight, which the fp8 skinny kernel serves up
    to 64 rows, so the 48-row graph still matches eager bit for bit."""
    from quickstart_streaming_agents_amd.models import serve
    from quickstart_streaming_agents_amd.ops import dispatch as D
    monkeypatch.setattr(serve, "DECODE_LADDER", False)
    for L in tiny_model.layers:
        for key in ("wqkv", "wo", "wgu", "wdown"):
            assert D.skinny_fp8_row_limit(*L[key].shape) >= 48
    prompts, new = _prompts(20)
    eng = _engine(tiny_model, graph=True)
    out = eng.generate_batch(prompts, new)
    assert _captured(eng), "graph capture failed"
    assert eng.graphs.rungs == (48,)
    assert out == eager_tokens
    assert set(eng.stats.decode_steps_by_rung) == {48}


def test_captured_replay_matches_eager_steps_and_eager_engine(tiny_model,
                                                              monkeypatch):
    """One batch (three live rows on rung 16: no script, a script shorter
    than the run, one longer) from identical engines: graphs.run, fill +
    eager step calls + read, and the eager engine emit the same tokens."""
    from quickstart_streaming_agents_amd.models import serve
    monkeypatch.setattr(serve, "DECODE_LADDER", True)
    scripts = {1: SHORT_SCRIPT, 2: LONG_SCRIPT}
    engs = [serve.Engine(tiny_model, max_batch=20, max_seq_len=256, eos_id=2,
                         valid_vocab=(16, 1000)) for _ in range(3)]
    batches = [_admit(e, PROMPTS, scripts=scripts) for e in engs]
    first = [s.out_tokens for s in batches[0]]
    assert all([s.out_tokens for s in b] == first for b in batches)
    (e_cap, e_step, e_eager), (b_cap, b_step, b_eager) = engs, batches

    assert e_cap._ensure_graphs(), "graph capture failed"
    assert e_cap.graphs.rungs == (16, 20)
    captured, rung, _ = e_cap.graphs.run(b_cap, RUN, False)
    assert rung == 16

    g = _graphs(e_step)
    g.fill(b_step, RUN, False)
    for _ in range(RUN):
        g.step(16, False)
    stepped = g.read(len(b_step), RUN)
    assert captured == stepped

    e_eager._decode_run_eager(b_eager, RUN)
    want = [s.out_tokens[1:] for s in b_eager]
    # the eager engine stops a row at EOS; a run's later tokens are dropped
    assert [t[:len(w)] for t, w in zip(captured, want)] == want
    assert all(len(w) == RUN or w[-1] == 2 for w in want)
    assert want[1][:3] == SHORT_SCRIPT and want[2] == LONG_SCRIPT[:RUN]
