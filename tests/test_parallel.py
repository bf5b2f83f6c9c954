"""Multi-process (gloo, world_size=2) tests of the parallel layer.

Each test spawns real processes over torch.distributed gloo on 127.0.0.1 —
the same code paths the GPU box runs over RCCL — and checks the parallel
result against the single-rank reference:
  * TP=2 Llama forward == TP=1 forward (deterministic sharded init)
  * sharded vector search == unsharded exact top-k
  * stream-partition sharding covers every record exactly once
"""

from __future__ import annotations

import multiprocessing as mp
import os
import pickle
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run_worker(fn, rank, world, port, q, args):
    os.environ.update({
        "RANK": str(rank), "WORLD_SIZE": str(world),
        "LOCAL_RANK": str(rank), "MASTER_ADDR": "127.0.0.1",
        "MASTER_PORT": str(port),
    })
    sys.path.insert(0, ROOT)
    try:
        out = fn(rank, world, *args)
        q.put((rank, "ok", pickle.dumps(out)))
    except Exception as e:  # pragma: no cover
        import traceback
        q.put((rank, "err", f"{e}\n{traceback.format_exc()}"))


_PORT_SEQ = [0]


def spawn_world(fn, world=2, args=(), timeout=240):
    """Run fn(rank, world, *args) in `world` processes; returns rank->result."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    # fresh port per call: a previous rendezvous socket in TIME_WAIT on
    # the same port can fail the TCP store bind
    _PORT_SEQ[0] += 1
    port = 29600 + (os.getpid() + _PORT_SEQ[0] * 7) % 500
    procs = [ctx.Process(target=_run_worker, args=(fn, r, world, port, q, args))
             for r in range(world)]
    for p in procs:
        p.start()
    results = {}
    try:
        for _ in range(world):
            rank, status, payload = q.get(timeout=timeout)
            assert status == "ok", f"rank {rank} failed:\n{payload}"
            results[rank] = pickle.loads(payload)
    finally:
        for p in procs:
            p.join(timeout=30)
            if p.is_alive():
                p.terminate()
    return results


# ---- worker fns (module-level for spawn pickling) -------------------------

def _tp_llama_worker(rank, world):
    import torch.distributed as dist
    from quickstart_streaming_agents_amd.models.llama import (LlamaConfig,
                                                              LlamaModel)
    from quickstart_streaming_agents_amd.models.serve import Engine
    dist.init_process_group("gloo")
    cfg = LlamaConfig.preset("tiny")
    model = LlamaModel(cfg, device="cpu", dtype=torch.float32, seed=3,
                       tp_rank=rank, tp_size=world, tp_group=None)
    eng = Engine(model, max_batch=4, max_seq_len=256)
    outs = eng.generate_batch([[1, 5, 9, 13], [2, 4, 6]], [6, 6])
    dist.destroy_process_group()
    return outs


def _shard_index_worker(rank, world, docs, queries):
    import torch.distributed as dist
    from quickstart_streaming_agents_amd.parallel.shard_index import \
        ShardedVectorIndex
    from quickstart_streaming_agents_amd.vector.index import HashingEmbedder
    dist.init_process_group("gloo")
    emb = HashingEmbedder()
    idx = ShardedVectorIndex(world_size=world, rank=rank)
    idx.add_documents(docs, emb)
    hits = idx.search_batch(np.stack([emb.embed(q) for q in queries]), k=3)
    dist.destroy_process_group()
    return [[(h.document_id, round(h.score, 5)) for h in hs] for hs in hits]


def _dp_metric_worker(rank, world):
    from quickstart_streaming_agents_amd.parallel.dist import (
        DistContext, init_distributed, max_over_ranks, sum_over_ranks)
    if torch.cuda.is_available() and torch.cuda.device_count() < world:
        # fewer GPUs than ranks (e.g. a 1-GPU host): one rank per GPU is
        # impossible, so run the same context + reductions over gloo/CPU
        # as on a host without GPUs
        ctx = init_distributed(backend="gloo", device="cpu")
    else:
        ctx = init_distributed()
    assert ctx.world_size == world and ctx.rank == rank
    s = sum_over_ranks(ctx, float(rank + 1))
    m = max_over_ranks(ctx, float(rank + 1))
    import torch.distributed as dist
    dist.destroy_process_group()
    return (s, m)


# ---- tests ----------------------------------------------------------------

@pytest.mark.timeout(300)
def test_tp2_matches_tp1():
    from quickstart_streaming_agents_amd.models.llama import (LlamaConfig,
                                                              LlamaModel)
    from quickstart_streaming_agents_amd.models.serve import Engine
    model = LlamaModel(LlamaConfig.preset("tiny"), device="cpu",
                       dtype=torch.float32, seed=3)
    eng = Engine(model, max_batch=4, max_seq_len=256)
    ref = eng.generate_batch([[1, 5, 9, 13], [2, 4, 6]], [6, 6])

    results = spawn_world(_tp_llama_worker, world=2)
    assert results[0] == ref, f"TP2 {results[0]} != TP1 {ref}"
    assert results[1] == ref


@pytest.mark.timeout(300)
def test_sharded_index_matches_exact():
    from quickstart_streaming_agents_amd.vector.index import (HashingEmbedder,
                                                              VectorIndex)
    rng = np.random.default_rng(7)
    docs = [{"document_id": f"d{i:03d}",
             "chunk": f"flink streaming doc {i} " + " ".join(
                 rng.choice(["window", "join", "agent", "table", "sql",
                             "kafka", "state", "watermark"],
                            size=6).tolist())}
            for i in range(40)]
    queries = ["how do windows work in flink sql",
               "agent state table", "kafka watermark join"]
    emb = HashingEmbedder()
    ref_idx = VectorIndex()
    ref_idx.add_documents(docs, emb)
    ref = [[(h.document_id, round(h.score, 5)) for h in
            ref_idx.search(emb.embed(q), 3)] for q in queries]

    results = spawn_world(_shard_index_worker, world=2, args=(docs, queries))
    assert results[0] == ref
    assert results[1] == ref


@pytest.mark.timeout(300)
def test_dist_context_and_reductions():
    results = spawn_world(_dp_metric_worker, world=2)
    assert results[0] == (3.0, 2.0) and results[1] == (3.0, 2.0)


def test_partition_assignment_covers_all():
    from quickstart_streaming_agents_amd.parallel.stream_shard import (
        PartitionAssignment, partition_for_key)
    records = [{"key": f"cust-{i}"} for i in range(100)]
    world = 4
    shards = [PartitionAssignment(8, world, r) for r in range(world)]
    owned = [a.filter_records(records, "key") for a in shards]
    total = sum(len(o) for o in owned)
    assert total == len(records)
    seen = {r["key"] for o in owned for r in o}
    assert len(seen) == 100
    # murmur2 vector: kafka's partitioner is stable across runs
    assert partition_for_key("cust-1", 8) == partition_for_key("cust-1", 8)
    allp = {p for p in range(8)}
    assert {a.owner(p) for p in allp for a in shards[:1]} <= set(range(world))


def _dp_sql_worker(rank, world):
    """Each rank runs the generic anomaly CTAS on ITS key-shard of the
    ride stream (murmur2 partition ownership, 8 partitions like the
    reference topics); rank 0 gathers and compares with unsharded."""
    import torch.distributed as dist

    from quickstart_streaming_agents_amd.labs.deploy import Deployment
    from quickstart_streaming_agents_amd.parallel.stream_shard import \
        PartitionAssignment
    dist.init_process_group("gloo")

    from quickstart_streaming_agents_amd.labs import schemas
    from quickstart_streaming_agents_amd.wire.topics import AvroConsumer
    dep = Deployment(labs=(3,), device="cpu")
    dep.datagen(3)
    topic = dep.broker.topics["ride_requests"]
    # shard on the AGGREGATION key (pickup_zone): keyed window/anomaly
    # state must live with its shard, so the zone decides ownership
    decoded = [v for _, v in AvroConsumer(dep.broker, "ride_requests",
                                          schemas.RIDE_REQUESTS).poll()]
    recs = topic.read_all()
    pa = PartitionAssignment(n_partitions=8, world_size=world, rank=rank)
    topic.purge()
    kept = 0
    for r, v in zip(recs, decoded):
        if pa.owns_key(v["pickup_zone"]):
            topic.append(r.value, key=r.key, timestamp_ms=r.timestamp_ms,
                         partition=0)
            kept += 1
    mine = dep.sql_executor(3).run_table("anomalies_per_zone")
    gathered = [None] * world
    dist.all_gather_object(gathered, (kept, mine))
    dist.destroy_process_group()
    if rank != 0:
        return None
    # unsharded reference
    ref_dep = Deployment(labs=(3,), device="cpu")
    ref_dep.datagen(3)
    ref = ref_dep.sql_executor(3).run_table("anomalies_per_zone")
    total_kept = sum(k for k, _ in gathered)
    merged = sorted((row for _, rows in gathered for row in rows),
                    key=lambda r: (r["window_time"], r["pickup_zone"]))
    ref_sorted = sorted(ref, key=lambda r: (r["window_time"],
                                            r["pickup_zone"]))
    return {"total_kept": total_kept, "n_records": len(decoded),
            "merged": [(r["pickup_zone"], r["window_time"],
                        r["request_count"]) for r in merged],
            "ref": [(r["pickup_zone"], r["window_time"],
                     r["request_count"]) for r in ref_sorted]}


@pytest.mark.timeout(300)
def test_dp_sharded_sql_anomalies_match_unsharded():
    """Keyed DP sharding (per-key state lives with its
    shard, no cross-talk for K3/K7): the union of per-rank generic-SQL
    anomaly outputs equals the single-rank run, and every record is
    owned by exactly one rank."""
    res = spawn_world(_dp_sql_worker, world=2)[0]
    assert res["total_kept"] == res["n_records"]      # exact cover
    assert res["merged"] == res["ref"]
    assert len(res["ref"]) >= 1                       # the FQ anomaly


def _tp_qwen_worker(rank, world):
    import torch.distributed as dist

    from quickstart_streaming_agents_amd.models.llama import (LlamaConfig,
                                                              LlamaModel)
    from quickstart_streaming_agents_amd.models.serve import Engine
    dist.init_process_group("gloo")
    cfg = LlamaConfig.preset("tiny-qwen")
    model = LlamaModel(cfg, device="cpu", dtype=torch.float32, seed=11,
                       tp_rank=rank, tp_size=world, tp_group=None)
    eng = Engine(model, max_batch=4, max_seq_len=256)
    outs = eng.generate_batch([[3, 7, 11], [2, 9, 4, 6]], [5, 5])
    dist.destroy_process_group()
    return outs


@pytest.mark.timeout(300)
def test_tp2_qwen_bias_matches_tp1():
    """Qwen2-family (qkv biases): TP=2 == TP=1 — the bias shards with the
    column-parallel rows."""
    from quickstart_streaming_agents_amd.models.llama import (LlamaConfig,
                                                              LlamaModel)
    from quickstart_streaming_agents_amd.models.serve import Engine
    ref = Engine(LlamaModel(LlamaConfig.preset("tiny-qwen"), device="cpu",
                            dtype=torch.float32, seed=11),
                 max_batch=4, max_seq_len=256)
    want = ref.generate_batch([[3, 7, 11], [2, 9, 4, 6]], [5, 5])
    got = spawn_world(_tp_qwen_worker, world=2)
    assert got[0] == want and got[1] == want


def test_qwen_preset_geometry_and_bias_changes_output():
    from quickstart_streaming_agents_amd.models.llama import (LlamaConfig,
                                                              LlamaModel)
    from quickstart_streaming_agents_amd.models.serve import Engine
    cfg = LlamaConfig.preset("qwen2-7b")
    assert (cfg.n_q_heads, cfg.n_kv_heads, cfg.hidden, cfg.ffn) == \
        (28, 4, 3584, 18_944)
    assert cfg.attn_bias and cfg.rope_theta == 1_000_000.0
    # bias actually participates: zeroing it changes the decode output
    m = LlamaModel(LlamaConfig.preset("tiny-qwen"), device="cpu",
                   dtype=torch.float32, seed=5)
    out1 = Engine(m, max_batch=2, max_seq_len=128).generate_batch(
        [[1, 2, 3]], [4])
    for L in m.layers:
        L["bqkv"].zero_()
    out2 = Engine(m, max_batch=2, max_seq_len=128).generate_batch(
        [[1, 2, 3]], [4])
    assert out1 != out2


def test_murmur2_matches_java_kafka_client():
    """Regression: finalization (h ^= h >>> 13) must
    run unconditionally, including keys whose length % 4 == 0.  Vectors
    are org.apache.kafka.common.utils.UtilsTest#testMurmur2, in
    Utils.toPositive (& 0x7fffffff) form as the partitioner applies."""
    from quickstart_streaming_agents_amd.parallel.stream_shard import murmur2
    java = {  # key -> signed int32 from the Java client
        b"21": -973932308,
        b"foobar": -790332482,
        b"a-little-bit-long-string": -985981536,  # len % 4 == 0
        b"abc": 479470107,
    }
    for k, signed in java.items():
        assert murmur2(k) == (signed & 0x7FFFFFFF), k


def _dp_continuous_worker(rank, world):
    """Per-rank mini flagship step: tiny engine + grammar episodes under
    the CONTINUOUS scheduler, then the bench's MAX-over-ranks reduction
    — the same shape the driver's multi-GPU bench launch runs."""
    import torch
    import torch.distributed as dist
    from quickstart_streaming_agents_amd.agents.mcp import (McpClient,
                                                            StubMcpServer)
    from quickstart_streaming_agents_amd.agents.runner import (AgentSpec,
                                                               ToolSet,
                                                               episode)
    from quickstart_streaming_agents_amd.agents.schedule import \
        run_episodes_continuous
    from quickstart_streaming_agents_amd.labs import datagen, pipelines
    from quickstart_streaming_agents_amd.models.llama import (LlamaConfig,
                                                              LlamaModel)
    from quickstart_streaming_agents_amd.models.serve import Engine, EngineLLM
    from quickstart_streaming_agents_amd.models.tokenizer import BpeTokenizer
    dist.init_process_group("gloo")
    torch.manual_seed(1234 + rank)
    tok = BpeTokenizer(vocab_size=4096)
    cfg = LlamaConfig.preset("tiny")
    cfg.vocab_size = 4096
    model = LlamaModel(cfg, device="cpu", dtype=torch.float32, seed=0)
    eng = Engine(model, max_batch=8, max_seq_len=1024, eos_id=tok.EOS,
                 valid_vocab=(tok._BYTE0, tok.n_tokens))
    llm = EngineLLM(eng, tok)
    with StubMcpServer() as srv:
        client = McpClient(srv.mcp_endpoint)
        schemas = {t["name"]: t.get("inputSchema", {})
                   for t in client.tools_list()}
        tool_fn = pipelines.mcp_tool_fn(client)
        agent = AgentSpec("price_match_agent", "m",
                          pipelines.LAB1_AGENT_PROMPT,
                          ToolSet("t", allowed_tools=("http_get",
                                                      "send_email")),
                          max_iterations=5, max_consecutive_failures=2)
        prods = datagen.lab1_products()
        eps = []
        for i in range(6):
            p = prods[(i + rank) % len(prods)]
            o = {"order_id": f"ORD-{rank}-{i}",
                 "product_name": p["product_name"],
                 "order_price": p["price"],
                 "customer_email": f"u{rank}{i}@example.com"}
            eps.append(episode(agent, pipelines.lab1_user_prompt(
                o, f"{srv.base_url}/competitor", o["customer_email"]),
                max_new_tokens=16, tool_schemas=schemas))
        results = run_episodes_continuous(eps, llm, tool_fn)
    import time
    t = torch.tensor([float(rank) + 1.0], dtype=torch.float64)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)   # bench's MAX-elapsed shape
    dist.destroy_process_group()
    return (len(results), sum(r.status == "SUCCESS" for r in results),
            float(t.item()))


def test_dp_continuous_scheduler_two_ranks():
    results = spawn_world(_dp_continuous_worker, world=2)
    for rank in (0, 1):
        n, ok, mx = results[rank]
        assert n == 6
        assert mx == 2.0                      # reduction saw both ranks


def test_murmur2_hypothesis_vs_reference():
    """Property: the partitioner's murmur2 == a direct transcription of
    org.apache.kafka.common.utils.Utils.murmur2 on arbitrary bytes."""
    from hypothesis import given, settings
    from hypothesis import strategies as st

    from quickstart_streaming_agents_amd.parallel.stream_shard import murmur2

    def ref(data: bytes) -> int:
        length = len(data)
        m, r = 0x5BD1E995, 24
        h = (0x9747B28C ^ length) & 0xFFFFFFFF
        for i in range(length // 4):
            k = int.from_bytes(data[i * 4:i * 4 + 4], "little")
            k = (k * m) & 0xFFFFFFFF
            k ^= k >> r
            k = (k * m) & 0xFFFFFFFF
            h = (h * m) & 0xFFFFFFFF
            h ^= k
        base = length & ~3
        rem = length % 4
        if rem >= 3:
            h ^= data[base + 2] << 16
        if rem >= 2:
            h ^= data[base + 1] << 8
        if rem >= 1:
            h ^= data[base]
            h = (h * m) & 0xFFFFFFFF
        h ^= h >> 13
        h = (h * m) & 0xFFFFFFFF
        h ^= h >> 15
        return h & 0x7FFFFFFF

    @settings(max_examples=300, deadline=None)
    @given(st.binary(max_size=64))
    def check(b):
        assert murmur2(b) == ref(b)

    check()
