"""Per-request seeded sampling, CPU side: the rule of ops/dispatch.py
(sample_step / sample_tokens) against known answers, a float64 softmax, an
independent recomputation of the kept set and binomial frequency bounds;
then SamplingParams through the engine on the CPU tiny model and through
/v1/completions."""

import math

import pytest
import torch

from quickstart_streaming_agents_amd.models.serve import (Engine,
                                                          SamplingParams)
from quickstart_streaming_agents_amd.ops import dispatch as D
from test_decode_ladder import MAX_RUN, SAMPLER_CASES, sampler_case

OFF = 65536


def params(B, inv_temp=1.0, top_k=0, top_p_q=OFF, seed=1234, pos=0):
    """Per-row parameter tensors from scalars or per-row lists."""
    def col(v, dtype):
        v = v if isinstance(v, (list, tuple, range)) else [v] * B
        return torch.tensor(list(v), dtype=dtype)
    return (col(inv_temp, torch.float32), col(top_k, torch.int32),
            col(top_p_q, torch.int32), col(seed, torch.int64),
            col(pos, torch.int32))


def kept_set(row, lo, hi, eos, inv_temp, top_k, top_p_q):
    """The rule's kept set, recomputed with plain loops: candidate
    indices, their weights, and the threshold key."""
    cand = D._candidates(lo, hi, eos)
    L = row[cand].unsqueeze(0)
    keys = D.sample_key(L)[0].tolist()
    m = L.float().max(dim=1).values
    ws = D.sample_weights(L, m, torch.tensor([inv_temp]))[0].tolist()
    distinct = sorted(set(keys), reverse=True)
    tau_k = distinct[-1]
    if top_k > 0:
        for t in distinct:
            if sum(1 for k in keys if k >= t) >= top_k:
                tau_k = t
                break
    total_k = sum(w for k, w in zip(keys, ws) if k >= tau_k)
    need = max(1, (total_k * top_p_q) // 65536)
    tau_p = None
    for t in distinct:
        if sum(w for k, w in zip(keys, ws) if k >= t) >= need \
                and t >= tau_k:
            tau_p = t
            break
    tau = max(tau_k, tau_p)
    return cand, keys, ws, tau


# ---- Philox ----------------------------------------------------------------

@pytest.mark.parametrize("ctr,key,want", [
    ((0, 0, 0, 0), (0, 0),
     (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2,
     (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344),
     (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
])
def test_philox_known_answers(ctr, key, want):
    out = D.philox4x32_10(torch.tensor([ctr], dtype=torch.int64),
                          torch.tensor([key], dtype=torch.int64))
    assert tuple(out[0].tolist()) == want


# ---- weights ---------------------------------------------------------------

@pytest.mark.parametrize("T", [0.3, 1.0, 4.0])
def test_weights_match_float64_softmax(T):
    """Bound 2e-5 relative on tokens of probability >= 1e-6: three f32
    roundings on |y| <= 40 (3 * 40 * 2^-24 * ln2 ~ 5e-6 in the exponent),
    the polynomial remainder (1.2e-7) and its f32 evaluation (~4e-7), and
    truncation of weights >= 1e6 to integers (1e-6), on both a weight and
    the total."""
    g = torch.Generator().manual_seed(17)
    logits = (torch.randn(2, 4096, generator=g) * 3).to(torch.bfloat16)
    inv = torch.tensor([1.0 / T] * 2, dtype=torch.float32)
    m = logits.float().max(dim=1).values
    w = D.sample_weights(logits, m, inv)
    assert w.dtype == torch.int64
    for b in range(2):
        assert int(w[b, logits[b].float().argmax()]) == 2 ** 40
    got = w.double() / w.double().sum(dim=1, keepdim=True)
    ref = torch.softmax(logits.double() * float(inv[0].double()), dim=1)
    big = ref >= 1e-6
    rel = ((got - ref).abs() / ref)[big].max().item()
    print(f"T={T}: worst relative error {rel:.3e} over {int(big.sum())}")
    assert rel <= 2e-5


def test_weights_monotone_in_key():
    bits = torch.arange(0, 65536, dtype=torch.int32).to(torch.int16)
    logits = bits.view(torch.bfloat16)
    logits = logits[logits.float().abs() <= 16.0].unsqueeze(0)   # drops NaN
    key = D.sample_key(logits)[0]
    for T in (0.3, 1.0, 4.0):
        w = D.sample_weights(logits, logits.float().max(dim=1).values,
                             torch.tensor([1.0 / T]))[0]
        by_key = w[key.argsort()]
        assert bool((by_key[1:] >= by_key[:-1]).all())


# ---- greedy rows -----------------------------------------------------------

@pytest.mark.parametrize("B,V,lo,hi,eos", SAMPLER_CASES)
def test_all_greedy_rows_equal_greedy_sample_step(B, V, lo, hi, eos):
    e = -1 if eos is None else eos
    for step in (0, 3, MAX_RUN - 1):
        c = sampler_case(B, V, lo, hi, eos, seed=B * 1000 + step, step=step)
        want = [c[k].clone() for k in ("tokens", "hist", "ctr")]
        D.greedy_sample_step(c["logits"], lo, hi, e, c["script"][:B],
                             c["mask"][:B], want[2], want[1][:, :B], want[0])
        got = [c[k].clone() for k in ("tokens", "hist", "ctr")]
        # every other parameter is ignored on a greedy row
        D.sample_step(c["logits"], lo, hi, e,
                      *params(B, inv_temp=0.0, top_k=3, top_p_q=100,
                              seed=-5, pos=step),
                      c["script"][:B], c["mask"][:B], got[2], got[1][:, :B],
                      got[0])
        for a, b in zip(got, want):
            assert torch.equal(a, b)


def test_all_neg_inf_candidates_give_token_zero():
    logits = torch.full((2, 64), float("-inf"), dtype=torch.bfloat16)
    logits[:, :4] = 1.0
    tok = D.sample_tokens(logits, 8, 32, 40, *params(2, inv_temp=[0.0, 1.0]))
    assert tok.tolist() == [0, 0]


# ---- the kept set ----------------------------------------------------------

def test_drawn_tokens_are_in_the_kept_set():
    V, lo, hi, eos = 64, 8, 40, 50
    g = torch.Generator().manual_seed(23)
    table = [(1.0, 0, OFF), (0.5, 3, OFF), (2.0, 0, 40000), (1.0, 5, 20000),
             (1.0, 1, OFF), (1.0, 0, 1), (4.0, 100, 60000), (0.1, 0, 65535)]
    logits = (torch.randn(len(table), V, generator=g) * 2).to(torch.bfloat16)
    logits[3, 10:20] = logits[3, 10]            # ties at a threshold
    for pos in range(48):
        tok = D.sample_tokens(
            logits, lo, hi, eos,
            *params(len(table), inv_temp=[1.0 / t[0] for t in table],
                    top_k=[t[1] for t in table],
                    top_p_q=[t[2] for t in table], seed=99, pos=pos))
        for b, (T, k, pq) in enumerate(table):
            cand, keys, ws, tau = kept_set(
                logits[b], lo, hi, eos,
                float(torch.tensor(1.0 / T, dtype=torch.float32)), k, pq)
            t = int(tok[b])
            assert t in cand
            assert keys[cand.index(t)] >= tau and ws[cand.index(t)] > 0


def test_top_k_1_and_top_p_min_equal_greedy_on_distinct_logits():
    g = torch.Generator().manual_seed(4)
    vals = (torch.arange(64, dtype=torch.float32) * 0.125 - 3.0) \
        .to(torch.bfloat16)
    logits = torch.stack([vals[torch.randperm(64, generator=g)]
                          for _ in range(6)])
    greedy = D.sample_tokens(logits, 4, 60, 63, *params(6, inv_temp=0.0))
    for pos in range(16):
        k1 = D.sample_tokens(logits, 4, 60, 63,
                             *params(6, inv_temp=0.5, top_k=1, pos=pos))
        p1 = D.sample_tokens(logits, 4, 60, 63,
                             *params(6, inv_temp=0.5, top_p_q=1, pos=pos))
        assert torch.equal(k1, greedy) and torch.equal(p1, greedy)


def test_top_k_1_draws_among_tied_maxima():
    c = sampler_case(5, 2048, 16, 1000, 2, seed=1, step=0)
    row = c["logits"][0]
    cand = D._candidates(16, 1000, 2)
    top = row[cand].float().max()
    tied = {i for i in cand if float(row[i]) == float(top)}
    assert len(tied) > 1
    tok = D.sample_tokens(row.expand(64, -1).contiguous(), 16, 1000, 2,
                          *params(64, top_k=1, pos=range(64)))
    assert set(tok.tolist()) <= tied
    assert len(set(tok.tolist())) > 1


@pytest.mark.parametrize("top_k,top_p_q", [(0, OFF), (5, OFF), (0, 32768),
                                           (50, 58982)])
def test_frequencies_within_five_sigma(top_k, top_p_q):
    N, lo, hi, eos = 4096, 8, 40, 50
    g = torch.Generator().manual_seed(5)
    row = (torch.randn(64, generator=g) * 2).to(torch.bfloat16)
    tok = D.sample_tokens(row.expand(N, -1).contiguous(), lo, hi, eos,
                          *params(N, top_k=top_k, top_p_q=top_p_q,
                                  seed=1234, pos=range(N)))
    counts = torch.bincount(tok, minlength=64).tolist()
    cand, keys, ws, tau = kept_set(row, lo, hi, eos, 1.0, top_k, top_p_q)
    total = sum(w for k, w in zip(keys, ws) if k >= tau)
    worst = 0.0
    for i in range(64):
        if i not in cand or keys[cand.index(i)] < tau:
            assert counts[i] == 0, i
            continue
        p = ws[cand.index(i)] / total
        sigma = math.sqrt(N * p * (1 - p))
        dev = abs(counts[i] - N * p)
        if sigma > 0:
            worst = max(worst, dev / sigma)
        assert dev <= 5 * sigma + 1e-9, (i, counts[i], N * p, sigma)
    print(f"top_k={top_k} top_p_q={top_p_q}: worst {worst:.2f} sigma")


# ---- row independence ------------------------------------------------------

def test_rows_are_independent():
    B, V, lo, hi, eos = 7, 512, 3, 500, 1
    g = torch.Generator().manual_seed(8)
    logits = (torch.randn(B, V, generator=g) * 3).to(torch.bfloat16)
    p = params(B, inv_temp=[1.0, 0.0, 0.7, 2.0, 1.0, 1.5, 1.0],
               top_k=[0, 0, 5, 0, 50, 0, 1],
               top_p_q=[OFF, OFF, OFF, 32768, 58982, 1, OFF],
               seed=[11, 12, -13, 14, 2 ** 62, 16, 17],
               pos=[0, 5, 9, 2 ** 31 - 1, 77, 3, 4])
    tok = D.sample_tokens(logits, lo, hi, eos, *p)
    perm = torch.randperm(B, generator=g)
    tok_p = D.sample_tokens(logits[perm], lo, hi, eos, *(t[perm] for t in p))
    assert torch.equal(tok_p, tok[perm])
    for b in range(B):
        one = D.sample_tokens(logits[b:b + 1], lo, hi, eos,
                              *(t[b:b + 1] for t in p))
        assert int(one[0]) == int(tok[b])


def test_pos_and_seed_change_the_stream():
    g = torch.Generator().manual_seed(9)
    row = (torch.randn(512, generator=g) * 3).to(torch.bfloat16)
    rows = row.expand(32, -1).contiguous()

    def stream(seed, pos0):
        return D.sample_tokens(rows, 0, 512, -1,
                               *params(32, seed=seed,
                                       pos=range(pos0, pos0 + 32))).tolist()
    base = stream(1, 0)
    assert stream(1, 0) == base
    assert stream(2, 0) != base
    assert stream(1, 1000) != base
    assert stream(1, 1)[:-1] == base[1:]      # the counter is the position


# ---- SamplingParams --------------------------------------------------------

def test_sampling_params_validation_and_quantisation():
    p = SamplingParams()
    assert (p.temperature, p.top_k, p.top_p, p.seed) == (0.0, 0, 1.0, None)
    assert p.inv_temp == 0.0 and p.top_p_q == 65536
    q = SamplingParams(temperature=0.7, top_k=50, top_p=0.9, seed=2 ** 64 - 1)
    assert q.inv_temp == float(torch.tensor(1 / 0.7, dtype=torch.float32))
    assert q.top_p_q == 58982
    assert SamplingParams(top_p=1e-9).top_p_q == 1
    for bad in (dict(temperature=-0.1), dict(temperature=float("inf")),
                dict(temperature=float("nan")), dict(top_k=-1),
                dict(top_p=0.0), dict(top_p=1.01), dict(seed=-1),
                dict(seed=2 ** 64)):
        with pytest.raises(ValueError):
            SamplingParams(**bad)


# ---- engine, CPU tiny model ------------------------------------------------

@pytest.fixture(scope="module")
def tiny_model():
    from quickstart_streaming_agents_amd.models.llama import (LlamaConfig,
                                                              LlamaModel)
    return LlamaModel(LlamaConfig.preset("tiny"), device="cpu",
                      dtype=torch.float32, seed=3)


PROMPTS = [[1, 5, 9], [1, 17, 23, 99, 40], [7, 7, 7, 7], [300, 2, 11]]
NEW = [12, 9, 12, 7]


def _engine(model, **kw):
    return Engine(model, max_batch=4, max_seq_len=128, eos_id=2,
                  valid_vocab=(16, 1000), **kw)


def test_engine_seeded_sampling_is_reproducible(tiny_model):
    sp = SamplingParams(temperature=1.5, seed=7)
    a = _engine(tiny_model).generate_batch(PROMPTS, NEW, sampling=sp)
    b = _engine(tiny_model).generate_batch(PROMPTS, NEW, sampling=sp)
    assert a == b
    other = _engine(tiny_model).generate_batch(
        PROMPTS, NEW, sampling=SamplingParams(temperature=1.5, seed=8))
    assert other != a
    greedy = _engine(tiny_model).generate_batch(PROMPTS, NEW)
    assert a != greedy
    # alone in the batch: the same tokens as among batch mates
    solo = _engine(tiny_model).generate_batch(PROMPTS[1:2], NEW[1:2],
                                              sampling=sp)
    assert solo[0] == a[1]


def test_engine_chunked_runs_draw_the_same_tokens(tiny_model):
    sp = SamplingParams(temperature=1.5, top_k=40, top_p=0.95, seed=7)
    want = _engine(tiny_model).generate_batch(PROMPTS, NEW, sampling=sp)
    eng = _engine(tiny_model)
    seqs = [eng.submit(p, m, sampling=sp) for p, m in zip(PROMPTS, NEW)]
    while eng.run_chunk(max_run=3):
        pass
    assert [s.out_tokens for s in seqs] == want
    assert all(s.seed == 7 for s in seqs)


def test_engine_mixed_batch_keeps_greedy_rows(tiny_model):
    greedy = _engine(tiny_model).generate_batch(PROMPTS, NEW)
    sp = SamplingParams(temperature=1.5)          # seed from the engine
    eng = _engine(tiny_model, seed=5)
    mixed = eng.generate_batch(PROMPTS, NEW, sampling=[sp, None, sp, None])
    assert mixed[1] == greedy[1] and mixed[3] == greedy[3]
    assert mixed[0] != greedy[0] and mixed[2] != greedy[2]
    by = eng.stats.decode_steps_by_sampler
    assert by["sampled"] > 0
    assert by["greedy"] + by["sampled"] == eng.stats.decode_steps
    # engine-drawn seeds: a function of Engine(seed=...) and arrival order
    again = _engine(tiny_model, seed=5).generate_batch(
        PROMPTS, NEW, sampling=[sp, None, sp, None])
    assert again == mixed
    third = _engine(tiny_model, seed=6).generate_batch(
        PROMPTS, NEW, sampling=[sp, None, sp, None])
    assert third != mixed
    plain = _engine(tiny_model)
    plain.generate_batch(PROMPTS, NEW)
    assert plain.stats.decode_steps_by_sampler == {
        "greedy": plain.stats.decode_steps, "sampled": 0}


# ---- HTTP ------------------------------------------------------------------

fastapi = pytest.importorskip("fastapi")


def _client(llm):
    from fastapi.testclient import TestClient

    from quickstart_streaming_agents_amd.serve_api import create_app
    return TestClient(create_app(llm))


def test_http_default_requests_reach_a_two_argument_llm():
    calls = []

    def llm(prompts, max_tokens):
        calls.append((prompts, max_tokens))
        return ["ok"] * len(prompts)

    with _client(llm) as c:
        r = c.post("/v1/completions", json={"prompt": ["a", "b"],
                                            "max_tokens": 5})
        assert r.status_code == 200 and len(r.json()["choices"]) == 2
        r = c.post("/v1/completions", json={
            "prompt": "a", "temperature": 0, "top_p": 1, "top_k": 0})
        assert r.status_code == 200
        assert calls == [(["a", "b"], [5, 5]), (["a"], [64])]
        # such a callable has nowhere to take sampling parameters
        r = c.post("/v1/completions", json={"prompt": "a",
                                            "temperature": 0.5})
        assert r.status_code == 501


def test_http_sampling_fields_reach_the_llm():
    calls = []

    def llm(prompts, max_tokens, sampling=None):
        calls.append(sampling)
        return ["ok"] * len(prompts)

    with _client(llm) as c:
        r = c.post("/v1/completions", json={
            "prompt": ["a", "b", "c"], "temperature": 0.7, "top_p": 0.9,
            "top_k": 50, "seed": 41})
        assert r.status_code == 200
        r = c.post("/v1/completions", json={"prompt": "a", "top_k": 3})
        assert r.status_code == 200
        r = c.post("/v1/completions", json={"prompt": "a"})
        assert r.status_code == 200
    assert calls[0] == [SamplingParams(0.7, 50, 0.9, 41 + i)
                        for i in range(3)]
    assert calls[1] == [SamplingParams(0.0, 3, 1.0, None)]
    assert calls[2] is None


@pytest.mark.parametrize("field,value", [
    ("temperature", -0.1), ("temperature", 2.5), ("top_p", 0), ("top_p", 1.5),
    ("top_k", -1), ("seed", -1), ("seed", 2 ** 63)])
def test_http_bad_sampling_values_are_422(field, value):
    with _client(lambda p, m, sampling=None: ["ok"] * len(p)) as c:
        r = c.post("/v1/completions", json={"prompt": "x", field: value})
        assert r.status_code == 422
