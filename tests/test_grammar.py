"""BPE tokenizer + grammar-constrained model-driven agent loop (CPU).

The reference's AI_RUN_AGENT lets the model choose tools and iteration
count (LAB1-Walkthrough.md:155-181); here the engine's constrained decode
(models/grammar.py + models/serve.py) does that under random-init weights.
These tests run the tiny preset on CPU through the REAL engine."""

import collections

import pytest
import torch

from quickstart_streaming_agents_amd.agents.mcp import McpClient, StubMcpServer
from quickstart_streaming_agents_amd.agents.runner import (AgentSpec,
                                                           ToolCallPolicy,
                                                           ToolSet, episode)
from quickstart_streaming_agents_amd.agents.schedule import run_episodes
from quickstart_streaming_agents_amd.labs import datagen, pipelines
from quickstart_streaming_agents_amd.models.grammar import (ActionOption,
                                                            TurnGrammar,
                                                            build_turn_grammar,
                                                            compile_grammar)
from quickstart_streaming_agents_amd.models.llama import (LlamaConfig,
                                                          LlamaModel)
from quickstart_streaming_agents_amd.models.serve import Engine, EngineLLM
from quickstart_streaming_agents_amd.models.tokenizer import BpeTokenizer


@pytest.fixture(scope="module")
def tok():
    return BpeTokenizer(vocab_size=4096)


# ---------------------------------------------------------------------------
# tokenizer
# ---------------------------------------------------------------------------

def test_bpe_round_trip_lossless(tok):
    texts = [
        "Hello, world!  Prices start at $209.99 (was $245).",
        pipelines.LAB1_AGENT_PROMPT,
        'TOOL_CALL {"name": "http_get", "arguments": '
        '{"url": "http://127.0.0.1:1234/competitor"}}',
        "unicode: émojis 🙂 and\ttabs\nnewlines",
        "",
    ]
    for t in texts:
        assert tok.decode(tok.encode(t, bos=False)) == t


def test_bpe_subword_statistics(tok):
    """Token counts must be in the real-BPE class (multiple chars/token),
    not 1 token per word and not 1 per byte."""
    text = pipelines.lab1_user_prompt(
        {"order_id": "ORD-1", "product_name": "AirPods Pro",
         "order_price": 249.0, "customer_email": "a@b.com"},
        "http://127.0.0.1:8000/competitor", "a@b.com")
    ids = tok.encode(text, bos=False)
    cpt = len(text) / len(ids)
    assert 2.0 < cpt < 8.0, f"chars/token {cpt}"
    n_words = len(text.split())
    assert len(ids) > n_words   # subword: more tokens than words


def test_bpe_specials_and_truncated_vocab(tok):
    s = "<|finish|>ok<|tool_0|>"
    ids = tok.encode(s, bos=False)
    assert ids[0] == tok.FINISH and tok.tool_slot(0) in ids
    assert tok.decode(ids) == s
    # a truncated-merge (small-vocab) tokenizer stays lossless
    small = BpeTokenizer(vocab_size=512)
    text = "The quick brown fox jumps over the lazy dog. $12.34!"
    assert small.decode(small.encode(text, bos=False)) == text
    assert len(small.encode(text, bos=False)) > len(
        tok.encode(text, bos=False))


# ---------------------------------------------------------------------------
# grammar construction
# ---------------------------------------------------------------------------

def _schemas():
    with StubMcpServer() as srv:
        return {t["name"]: t.get("inputSchema", {})
                for t in McpClient(srv.mcp_endpoint).tools_list()}


def test_build_turn_grammar_from_lab1_prompt():
    schemas = _schemas()
    text = pipelines.LAB1_AGENT_PROMPT + "\n" + pipelines.lab1_user_prompt(
        {"order_id": "ORD-7", "product_name": "AirPods Pro",
         "order_price": 249.0, "customer_email": "kim@example.com"},
        "http://127.0.0.1:9999/competitor", "kim@example.com")
    g = build_turn_grammar(schemas, ("http_get", "send_email"), text)
    by_tool = collections.defaultdict(list)
    for o in g.options:
        by_tool[o.tool].append(o)
    # http_get bound to the URL present in the prompt
    assert by_tool["http_get"][0].arguments["url"] == \
        "http://127.0.0.1:9999/competitor"
    # send_email bound to recipient/subject/body extracted from the prompt
    se = by_tool["send_email"][0].arguments
    assert se["to"] == "kim@example.com"
    assert "ORD-7" in se["subject"]
    assert se["body"]
    # http_post requires url (present) -> allowed_tools filter removed it
    assert "http_post" not in by_tool
    assert g.allow_finish


def test_compile_grammar_scripts_parse_back(tok):
    g = TurnGrammar(options=[
        ActionOption("http_get", {"url": "http://x.test/a"}),
        ActionOption("send_email", {"to": "a@b.com", "subject": "s",
                                    "body": "hello there"})])
    cg = compile_grammar(g, tok)
    assert tok.FINISH in cg.decision_allowed
    assert len(cg.decision_allowed) == 3
    pol = ToolCallPolicy()
    for t, script in cg.branches.items():
        assert script[-1] == tok.EOS
        text = tok.decode([t] + script)
        act = pol(text, 0, {})
        assert act.__class__.__name__ == "ToolCall"
        assert act.name in ("http_get", "send_email")
        if act.name == "send_email":
            assert act.arguments["body"] == "hello there"


# ---------------------------------------------------------------------------
# engine-constrained decode (tiny model, CPU, real Engine)
# ---------------------------------------------------------------------------

def _engine(tok, max_batch=16, seed=0):
    cfg = LlamaConfig.preset("tiny")
    cfg.vocab_size = 4096
    model = LlamaModel(cfg, device="cpu", dtype=torch.float32, seed=seed)
    eng = Engine(model, max_batch=max_batch, max_seq_len=2048,
                 eos_id=tok.EOS, valid_vocab=(tok._BYTE0, tok.n_tokens))
    return eng


def _run_lab1_episodes(tok, n=10, seed=7, max_iters=6, server=None):
    torch.manual_seed(seed)
    eng = _engine(tok)
    llm = EngineLLM(eng, tok)
    import contextlib
    with (contextlib.nullcontext(server) if server is not None
          else StubMcpServer()) as srv:
        client = McpClient(srv.mcp_endpoint)
        schemas = {t["name"]: t.get("inputSchema", {})
                   for t in client.tools_list()}
        tool_fn = pipelines.mcp_tool_fn(client)
        tools = ToolSet("lab1_remote_mcp",
                        allowed_tools=("http_get", "send_email"))
        agent = AgentSpec("price_match_agent", "m",
                          pipelines.LAB1_AGENT_PROMPT, tools,
                          max_iterations=max_iters,
                          max_consecutive_failures=2)
        products = datagen.lab1_products()
        orders = []
        for i in range(n):
            p = products[i % len(products)]
            orders.append({"order_id": f"ORD-{i:04d}",
                           "product_name": p["product_name"],
                           "product_id": p["product_id"],
                           "order_price": p["price"],
                           "customer_email": f"u{i}@example.com",
                           "order_ts": i})
        eps = [episode(agent,
                       pipelines.lab1_user_prompt(
                           o, f"{srv.base_url}/competitor",
                           o["customer_email"]),
                       max_new_tokens=24, tool_schemas=schemas)
               for o in orders]
        results = run_episodes(eps, llm, tool_fn)
        return results, len(srv.emails)


def test_model_driven_episodes_vary_and_respect_caps(tok):
    results, n_emails = _run_lab1_episodes(tok, n=12, seed=7)
    assert len(results) == 12
    shapes = {(r.iterations, r.tool_calls) for r in results}
    assert len(shapes) >= 2, "model-driven control flow must vary shapes"
    assert all(r.iterations <= 6 for r in results)
    assert all(r.latency_s > 0 for r in results)
    # at least one episode actually called a tool through MCP
    assert any(r.tool_calls > 0 for r in results)
    # a send_email decision produced a real email through the stub server
    total_tool_calls = sum(r.tool_calls for r in results)
    assert total_tool_calls >= 1
    assert n_emails >= 0  # may be zero for some seeds; counted for info


def test_model_driven_episodes_deterministic(tok):
    # one server instance -> identical prompts (the URL carries the port)
    with StubMcpServer() as srv:
        r1, _ = _run_lab1_episodes(tok, n=8, seed=11, server=srv)
        r2, _ = _run_lab1_episodes(tok, n=8, seed=11, server=srv)
    assert [(r.status, r.iterations, r.tool_calls) for r in r1] == \
        [(r.status, r.iterations, r.tool_calls) for r in r2]
    assert [r.response for r in r1] == [r.response for r in r2]


def test_forced_script_emitted_exactly(tok):
    """A single-option grammar with no finish forces the full tool-call
    token script; the emitted text must be the exact rendered call."""
    torch.manual_seed(0)
    eng = _engine(tok, max_batch=2)
    opt = ActionOption("http_get", {"url": "http://t.test/page"})
    cg = compile_grammar(TurnGrammar(options=[opt], allow_finish=False),
                         tok)
    prompt = tok.encode("please fetch the page")
    seq = eng.submit(prompt, 4, constraint=cg)
    eng.run_to_completion()
    text = tok.decode(seq.out_tokens)
    assert text.startswith("<|tool_0|>")
    act = ToolCallPolicy()(text, 0, {})
    assert act.__class__.__name__ == "ToolCall"
    assert act.name == "http_get"
    assert act.arguments == {"url": "http://t.test/page"}
    # script ran to its EOS, not to an arbitrary cap
    assert seq.out_tokens[-1] == tok.EOS


def test_free_turn_respects_valid_vocab(tok):
    torch.manual_seed(3)
    eng = _engine(tok, max_batch=2)
    seq = eng.submit(tok.encode("hello"), 16)
    eng.run_to_completion()
    for t in seq.out_tokens:
        assert (tok._BYTE0 <= t < tok.n_tokens) or t == tok.EOS


def test_grammar_dedup_bounds_episode_length(tok):
    """An exact repeat of an already-made call is dropped from the
    candidate set, so episodes end within distinct-actions + 1 turns
    instead of spinning to max_iterations."""
    schemas = _schemas()
    text = "fetch http://a.test/x please"
    g0 = build_turn_grammar(schemas, ("http_get",), text)
    assert len(g0.options) == 1
    g1 = build_turn_grammar(schemas, ("http_get",), text,
                            history=[("http_get", g0.options[0].arguments)])
    assert g1.options == [] and g1.allow_finish
    # engine level: every episode ends well under the iteration cap
    results, _ = _run_lab1_episodes(tok, n=10, seed=5, max_iters=10)
    assert all(r.status == "SUCCESS" for r in results)
    assert max(r.iterations for r in results) <= 5


def test_jump_forward_matches_serial_decode(tok, monkeypatch):
    """Jump-forward (grammar-forced segments emitted without serial
    decode; SGLang-style fast-forward) must produce the same episode
    results as full serial decoding — the forced tokens' values are
    grammar-determined and their KV is never reused."""
    with StubMcpServer() as srv:
        r_jf, _ = _run_lab1_episodes(tok, n=8, seed=13, server=srv)
        monkeypatch.setenv("QSA_NO_JUMP_FORWARD", "1")
        r_sd, _ = _run_lab1_episodes(tok, n=8, seed=13, server=srv)
    assert [(r.status, r.iterations, r.tool_calls, r.response)
            for r in r_jf] == \
        [(r.status, r.iterations, r.tool_calls, r.response) for r in r_sd]


def test_continuous_scheduler_completes_episodes(tok):
    """run_episodes_continuous (event-driven: turns join the running
    batch as tool futures land, Engine.run_chunk slices) completes every
    episode within caps, with real tool calls and per-decision
    latencies; deterministic across runs."""
    from quickstart_streaming_agents_amd.agents.schedule import \
        run_episodes_continuous

    def run_once(srv, seed):
        torch.manual_seed(seed)
        eng = _engine(tok)
        llm = EngineLLM(eng, tok)
        client = McpClient(srv.mcp_endpoint)
        schemas = {t["name"]: t.get("inputSchema", {})
                   for t in client.tools_list()}
        tool_fn = pipelines.mcp_tool_fn(client)
        tools = ToolSet("lab1_remote_mcp",
                        allowed_tools=("http_get", "send_email"))
        agent = AgentSpec("price_match_agent", "m",
                          pipelines.LAB1_AGENT_PROMPT, tools,
                          max_iterations=6, max_consecutive_failures=2)
        products = datagen.lab1_products()
        eps = []
        for i in range(10):
            p = products[i % len(products)]
            o = {"order_id": f"ORD-{i:04d}",
                 "product_name": p["product_name"],
                 "order_price": p["price"],
                 "customer_email": f"u{i}@example.com"}
            eps.append(episode(
                agent, pipelines.lab1_user_prompt(
                    o, f"{srv.base_url}/competitor", o["customer_email"]),
                max_new_tokens=24, tool_schemas=schemas))
        return run_episodes_continuous(eps, llm, tool_fn)

    with StubMcpServer() as srv:
        r1 = run_once(srv, 21)
    assert len(r1) == 10
    assert all(r.status in ("SUCCESS", "FAILED") for r in r1)
    assert all(r.iterations <= 6 for r in r1)
    assert all(r.latency_s > 0 for r in r1)
    assert sum(r.tool_calls for r in r1) >= 1
    assert any(r.status == "SUCCESS" for r in r1)


def test_continuous_scheduler_independent_of_tool_latency(tok):
    """The continuous schedule is a function of the inputs, not of tool
    round-trip timing: tool results re-enter at a fixed engine slice, so
    fast tools, tools that are slow on some episodes, and a different
    worker-pool width all form the same batches, draw the same decision
    samples and return identical results."""
    from quickstart_streaming_agents_amd.agents.schedule import \
        run_episodes_continuous

    def run_once(srv, slow, workers):
        torch.manual_seed(21)
        llm = EngineLLM(_engine(tok), tok)
        client = McpClient(srv.mcp_endpoint)
        schemas = {t["name"]: t.get("inputSchema", {})
                   for t in client.tools_list()}
        inner = pipelines.mcp_tool_fn(client)

        def tool_fn(name, args):
            if slow(args):
                sum(range(300_000))      # busy work: lands slices later
            return inner(name, args)

        agent = AgentSpec("price_match_agent", "m",
                          pipelines.LAB1_AGENT_PROMPT,
                          ToolSet("lab1_remote_mcp",
                                  allowed_tools=("http_get", "send_email")),
                          max_iterations=6, max_consecutive_failures=2)
        products = datagen.lab1_products()
        eps = []
        for i in range(10):
            p = products[i % len(products)]
            o = {"order_id": f"ORD-{i:04d}",
                 "product_name": p["product_name"],
                 "order_price": p["price"],
                 "customer_email": f"u{i}@example.com"}
            eps.append(episode(
                agent, pipelines.lab1_user_prompt(
                    o, f"{srv.base_url}/competitor", o["customer_email"]),
                max_new_tokens=24, tool_schemas=schemas))
        res = run_episodes_continuous(eps, llm, tool_fn,
                                      max_tool_workers=workers)
        return [(r.status, r.iterations, r.tool_calls, r.failures,
                 r.response) for r in res]

    with StubMcpServer() as srv:
        fast = run_once(srv, lambda a: False, 16)
        again = run_once(srv, lambda a: False, 16)
        uneven = run_once(srv, lambda a: len(str(a)) % 2 == 0, 16)
        serial = run_once(srv, lambda a: True, 1)
    assert sum(t[2] for t in fast) >= 1          # tools were really called
    assert again == fast
    assert uneven == fast
    assert serial == fast


def test_bpe_round_trip_fuzz(tok):
    """Property: decode(encode(s)) == s for arbitrary unicode strings."""
    import random
    rng = random.Random(7)
    pools = [
        lambda: chr(rng.randrange(32, 127)),
        lambda: chr(rng.randrange(0x80, 0x2FF)),
        lambda: chr(rng.randrange(0x4E00, 0x4F00)),   # CJK
        lambda: rng.choice("\n\t  \U0001F600"),
    ]
    for _ in range(200):
        s = "".join(rng.choice(pools)() for _ in range(rng.randrange(0, 60)))
        assert tok.decode(tok.encode(s, bos=False)) == s
    # specials embedded mid-string survive too
    s = "a<|finish|>b<|tool_3|>\nc"
    assert tok.decode(tok.encode(s, bos=False)) == s


def test_continuous_scheduler_failure_caps(tok):
    """Tool failures under the continuous scheduler: an always-failing
    tool trips max_consecutive_failures and the episode FAILS with the
    abort message (the reference's cap semantics,
    LAB1-Walkthrough.md:177-180).  A scripted always-call policy makes
    the cap path deterministic; the LLM turns still run the real engine."""
    from quickstart_streaming_agents_amd.agents.runner import ToolCall
    from quickstart_streaming_agents_amd.agents.schedule import \
        run_episodes_continuous
    torch.manual_seed(3)
    eng = _engine(tok)
    llm = EngineLLM(eng, tok)
    agent = AgentSpec("a", "m", "do the thing",
                      ToolSet("t", allowed_tools=("http_get",)),
                      max_iterations=8, max_consecutive_failures=2)

    def broken_tool(name, args):
        raise RuntimeError("connection refused")

    def always_call(text, it, ctx):
        return ToolCall("http_get", {"url": "http://dead.test/x"})

    eps = [episode(agent, f"fetch number {i}", policy=always_call,
                   max_new_tokens=12) for i in range(5)]
    results = run_episodes_continuous(eps, llm, broken_tool)
    assert len(results) == 5
    for r in results:
        assert r.status == "FAILED"
        assert "2 consecutive" in r.response
        assert r.iterations == 2 and r.tool_calls == 2
        assert r.latency_s > 0


def test_engine_kv_pages_conserved_random_workload(tok):
    """Property: after any mix of grammar turns, keep-alive
    conversations, releases and jump-forwards, every KV page returns to
    the free list (no page leaks across the continuous scheduler)."""
    import random
    rng = random.Random(5)
    torch.manual_seed(5)
    eng = _engine(tok, max_batch=6)
    llm = EngineLLM(eng, tok)
    total = eng.kv.free_pages
    from quickstart_streaming_agents_amd.models.grammar import (ActionOption,
                                                                TurnGrammar)
    for round_i in range(4):
        convs = [f"c{round_i}-{j}" for j in range(rng.randrange(1, 5))]
        for turn in range(rng.randrange(1, 4)):
            prompts, maxtoks, gs = [], [], []
            for c in convs:
                prompts.append(f"turn {turn} of {c} " + "x " * rng.randrange(0, 40))
                maxtoks.append(rng.randrange(4, 20))
                gs.append(TurnGrammar(options=[ActionOption(
                    "http_get", {"url": f"http://t/{c}/{turn}"})])
                    if rng.random() < 0.5 else None)
            llm(prompts, maxtoks, convs, gs)
        for c in convs:
            llm.release(c)
        assert eng.kv.free_pages == total, f"leak after round {round_i}"
    assert not eng.running and not eng.pending


def test_bpe_round_trip_hypothesis(tok):
    from hypothesis import given, settings
    from hypothesis import strategies as st

    @settings(max_examples=300, deadline=None)
    @given(st.text(max_size=80))
    def check(s):
        assert tok.decode(tok.encode(s, bos=False)) == s

    check()


def test_continuous_scheduler_traces_episodes(tok):
    from quickstart_streaming_agents_amd.agents.schedule import \
        run_episodes_continuous
    from quickstart_streaming_agents_amd.runtime.trace import Tracer
    torch.manual_seed(2)
    eng = _engine(tok)
    llm = EngineLLM(eng, tok)
    agent = AgentSpec("a", "m", "answer briefly", None, max_iterations=3)
    eps = [episode(agent, f"question {i}", max_new_tokens=8)
           for i in range(4)]
    tr = Tracer("bench")
    results = run_episodes_continuous(eps, llm, lambda n, a: "",
                                      tracer=tr)
    assert len(results) == 4
    ep_spans = [s for s in tr.spans if s.stage.startswith("episode[")]
    assert len(ep_spans) == 4
    assert all(s.dt > 0 and s.meta["status"] in ("SUCCESS", "FAILED")
               for s in ep_spans)


def test_engine_edge_cases(tok):
    """Engine boundary behavior: prompt at the sequence budget clamps
    max_new to >= 1; run_chunk raises when a prompt can never be
    admitted; out-of-vocab decode ids render to nothing."""
    torch.manual_seed(0)
    eng = _engine(tok, max_batch=2)
    # prompt fills the whole budget: still decodes exactly 1 token
    long_prompt = list(range(16, 16 + 4000))
    seq = eng.submit(long_prompt, 64)
    assert len(seq.prompt) == eng.max_seq_len - 1
    assert seq.max_new_tokens == 1
    eng.run_to_completion()
    assert len(seq.out_tokens) == 1

    # a prompt that cannot fit the KV pool -> MemoryError, not a hang
    small = _engine(tok, max_batch=2)
    small.kv = small.model.new_kv_cache(4)     # 4 pages = 256 tokens
    big = small.submit(list(range(16, 16 + 500)), 8)
    import pytest as _pytest
    with _pytest.raises(MemoryError):
        small.run_chunk()

    # decode ids beyond the trained vocab render to nothing (random
    # weights can emit them when no vocab mask is set)
    assert tok.decode([tok.n_tokens + 5, 999999]) == ""
