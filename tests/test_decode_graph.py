"""DecodeGraphs on the CPU: fill / step / read called eagerly (no capture)
against a twin Engine's eager decode runs, token for token; stale buffer
state between runs; idle rows of a padded rung; no reference back to the
Engine; and the KV cache's set_len / pages."""

import gc
import weakref

import pytest
import torch

from quickstart_streaming_agents_amd.models.decode_graph import (DecodeGraphs,
                                                                 pick_rung)
from quickstart_streaming_agents_amd.models.kv_cache import PagedKVCache
from quickstart_streaming_agents_amd.models.llama import (LlamaConfig,
                                                          LlamaModel)
from quickstart_streaming_agents_amd.models.serve import (Engine,
                                                          SamplingParams,
                                                          ladder_rungs)

MAX_BATCH = 20
PROMPTS = [[5, 6, 7, 8, 9], [11, 12, 13], [20] * 70]
RUN = 5
# forced tokens inside the vocabulary window, none of them EOS
SHORT_SCRIPT = [101, 102, 103]                    # shorter than the run
LONG_SCRIPT = [201 + i for i in range(9)]         # longer than the run


@pytest.fixture(scope="module")
def model():
    return LlamaModel(LlamaConfig.preset("tiny"), device="cpu")


def _engine(model):
    return Engine(model, max_batch=MAX_BATCH, max_seq_len=256, eos_id=2,
                  valid_vocab=(16, 1000))


def _graphs(eng):
    """The DecodeGraphs the engine would build, nothing captured."""
    return DecodeGraphs(eng.model, eng.kv, eng.policy, eng.max_batch,
                        eng.max_seq_len, Engine.MAX_RUN,
                        ladder_rungs(eng.max_batch))


def _admit(eng, prompts, sampling=None, scripts=None):
    """Submit and prefill `prompts`; scripts (row -> forced tokens) are set
    after admission, as a grammar branch would be."""
    sampling = sampling or [None] * len(prompts)
    seqs = [eng.submit(p, 64, sampling=sp) for p, sp in zip(prompts, sampling)]
    eng._admit()
    assert not eng.pending
    for i, script in (scripts or {}).items():
        seqs[i].script = list(script)
    return seqs


def _step_run(eng, g, batch, run, sampled, after_fill=None):
    """One run through fill, eager step calls and read, followed by what
    Engine._decode_run_graph does with the tokens.  Returns the rung."""
    g.fill(batch, run, sampled)
    if after_fill is not None:
        after_fill()
    rung = pick_rung(g.rungs, len(batch))
    for _ in range(run):
        g.step(rung, sampled)
    for s, new in zip(batch, g.read(len(batch), run)):
        if eng.eos_id in new:
            new = new[: new.index(eng.eos_id) + 1]
        s.out_tokens.extend(new)
        eng.kv.set_len(s.seq_id, len(s.prompt) + len(s.out_tokens))
        eng._maybe_finish(s)
    return rung


def _retire_all(eng):
    for s in eng.running:
        s.done = True
    eng._retire()
    assert not eng.running


def _twins(model, prompts, run, sampled, sampling=None, scripts=None):
    """The same batch through DecodeGraphs' eager steps and through the
    eager engine -> (engine, graphs, batch, rung), (engine, batch)."""
    eng_g, eng_e = _engine(model), _engine(model)
    batch_g = _admit(eng_g, prompts, sampling, scripts)
    batch_e = _admit(eng_e, prompts, sampling, scripts)
    assert [s.out_tokens for s in batch_g] == [s.out_tokens for s in batch_e]
    g = _graphs(eng_g)
    rung = _step_run(eng_g, g, batch_g, run, sampled)
    eng_e._decode_run_eager(batch_e, run)
    return (eng_g, g, batch_g, rung), (eng_e, batch_e)


def test_rungs():
    assert ladder_rungs(MAX_BATCH) == (16, 20)


def test_greedy_steps_match_eager_engine(model):
    (_, _, batch_g, rung), (_, batch_e) = _twins(
        model, PROMPTS, RUN, sampled=False,
        scripts={1: SHORT_SCRIPT, 2: LONG_SCRIPT})
    assert rung == 16
    assert [s.out_tokens for s in batch_g] == [s.out_tokens for s in batch_e]
    # the scripts were honoured: forced while they last, free afterwards
    assert batch_g[1].out_tokens[1:4] == SHORT_SCRIPT
    assert len(batch_g[1].out_tokens) == 1 + RUN
    assert batch_g[2].out_tokens[1:] == LONG_SCRIPT[:RUN]


def test_sampled_steps_match_eager_engine(model):
    sampling = [None,
                SamplingParams(temperature=0.8, top_k=20, top_p=0.9, seed=7),
                SamplingParams()]
    (_, _, batch_g, rung), (_, batch_e) = _twins(
        model, PROMPTS, RUN, sampled=True, sampling=sampling)
    assert rung == 16
    assert [s.out_tokens for s in batch_g] == [s.out_tokens for s in batch_e]
    assert all(len(s.out_tokens) > 1 for s in batch_g)


def test_stale_state_of_a_larger_run_does_not_leak(model):
    g18 = torch.Generator().manual_seed(5)
    first = [torch.randint(16, 1000, (3 + 4 * i,), generator=g18).tolist()
             for i in range(18)]
    sampling = [SamplingParams(temperature=0.7, top_k=10, seed=i)
                if i % 3 == 0 else None for i in range(18)]
    scripts = {i: [300 + i + j for j in range(2 + i)] for i in (1, 4, 17)}
    (eng_g, g, _, rung), (eng_e, _) = _twins(
        model, first, 7, sampled=True, sampling=sampling, scripts=scripts)
    assert rung == 20
    _retire_all(eng_g)
    _retire_all(eng_e)

    fresh = [[31, 32, 33, 34], [41, 42]]
    batch_g, batch_e = _admit(eng_g, fresh), _admit(eng_e, fresh)

    def after_fill():
        assert not g.script_mask.any()
        assert torch.equal(g.active[2:], torch.zeros_like(g.active[2:]))
        assert torch.equal(g.seq_lens[2:], torch.zeros_like(g.seq_lens[2:]))

    assert _step_run(eng_g, g, batch_g, RUN, False, after_fill) == 16
    eng_e._decode_run_eager(batch_e, RUN)
    assert [s.out_tokens for s in batch_g] == [s.out_tokens for s in batch_e]


def _positions(kv, layer, seq_id, n):
    """K and V of positions [0, n) of a sequence -> [KVH, n, D] each."""
    pages = torch.tensor(kv.pages(seq_id), dtype=torch.int64)
    k = kv.k[layer][pages].permute(1, 0, 3, 2, 4)     # [KVH, np, 64, D/8, 8]
    v = kv.v[layer][pages].permute(1, 0, 3, 2)        # [KVH, np, 64, D]
    return (k.reshape(kv.kvh, -1, kv.d_head)[:, :n],
            v.reshape(kv.kvh, -1, kv.d_head)[:, :n])


def test_idle_rows_write_nothing(model):
    eng_g, eng_e = _engine(model), _engine(model)
    scripts = {1: SHORT_SCRIPT, 2: LONG_SCRIPT}
    batch_g = _admit(eng_g, PROMPTS, scripts=scripts)
    batch_e = _admit(eng_e, PROMPTS, scripts=scripts)
    g = _graphs(eng_g)
    kv = eng_g.kv
    before_k = [k.clone() for k in kv.k]
    before_v = [v.clone() for v in kv.v]
    assert _step_run(eng_g, g, batch_g, RUN, False) == 16
    eng_e._decode_run_eager(batch_e, RUN)

    assert torch.equal(g.seq_lens[3:], torch.zeros_like(g.seq_lens[3:]))
    owned = {p for s in batch_g for p in kv.pages(s.seq_id)}
    other = torch.tensor([p for p in range(kv.n_pages) if p not in owned])
    assert len(other) > 0
    for layer in range(kv.n_layers):
        assert torch.equal(kv.k[layer][other], before_k[layer][other])
        assert torch.equal(kv.v[layer][other], before_v[layer][other])
        for sg, se in zip(batch_g, batch_e):
            # positions whose k/v is written: all but the last token's,
            # which the next step appends (the eager engine's length; a
            # graph run's counts that token already)
            n = len(sg.prompt) + len(sg.out_tokens) - 1
            assert n == len(sg.prompt) + RUN
            assert eng_e.kv.seq_len(se.seq_id) == n
            assert kv.seq_len(sg.seq_id) == n + 1
            kg, vg = _positions(kv, layer, sg.seq_id, n)
            ke, ve = _positions(eng_e.kv, layer, se.seq_id, n)
            assert torch.equal(kg, ke)
            assert torch.equal(vg, ve)
            assert kg[:, -RUN:].abs().sum(dim=(0, 2)).min() > 0


def test_decode_graphs_do_not_refer_to_the_engine(model):
    gc.collect()
    was_enabled = gc.isenabled()
    gc.disable()
    try:
        eng = _engine(model)
        eng.graphs = graphs = _graphs(eng)
        ref = weakref.ref(eng)
        del eng
        assert ref() is None
        assert graphs.kv is not None
    finally:
        if was_enabled:
            gc.enable()


def test_kv_set_len_and_pages():
    kv = PagedKVCache(1, 1, 8, n_pages=4, device="cpu")
    kv.allocate(7, 65)
    assert kv.pages(7) == [0, 1]
    kv.set_len(7, 128)
    assert kv.seq_len(7) == 128
    kv.set_len(7, 3)
    assert kv.seq_len(7) == 3
    with pytest.raises(AssertionError):
        kv.set_len(7, 129)
    assert kv.seq_len(7) == 3
    kv.extend(7, 129)
    assert kv.pages(7) == [0, 1, 2]
    kv.set_len(7, 129)
