#!/usr/bin/env python3
"""Decode-step microbenchmark: N graph-replayed decode steps of the
flagship model at fixed batch/context, no prefill in the timed region.

Usage: python tools/micro_decode.py [--model llama3-8b] [--batch 24]
         [--ctx 512] [--steps 200] [--live N]
--live N runs a --batch engine with only N live rows (the decode-graph
ladder's rung for N; QSA_DECODE_LADDER=0 for the single max_batch graph).
--repeat R prints the median and spread of R timed runs.  --rung R forces
the live rows onto the smallest captured rung >= R, and --candidates
16,32,64,128 captures other rungs than the shipped ones: together they
time one live count on each rung (the pruning table in profiles/README.md).
Prints ms/step, tokens/s, and the HBM-bound floor (weights+KV bytes / 8 TB/s)
for calibration.  Run under rocprofv3 for per-kernel attribution.
"""

import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


def measure(eng, ctx, live, steps, warmup, repeat=1):
    """`repeat` timed graph (or eager) runs of `steps` decode steps with
    `live` rows of context `ctx` on `eng`; returns ms/step per run.  The
    sequences are retired afterwards, so one engine serves several calls."""
    torch.manual_seed(0)
    prompts = [torch.randint(16, 2000, (ctx,)).tolist() for _ in range(live)]
    for pr in prompts:
        eng.submit(pr, warmup + steps * repeat)
    # prefill + warmup decode
    while eng.pending:
        n = len(eng.pending)
        eng._admit()
        if len(eng.pending) == n:
            raise MemoryError("cannot admit")
    batch = [s for s in eng.running]
    if eng.use_graph:
        eng._decode_run_graph(batch, warmup)
    else:
        for _ in range(warmup):
            eng.step()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        if eng.use_graph:
            eng._decode_run_graph(batch, steps)
        else:
            for _ in range(steps):
                eng.step()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) / steps * 1e3)
    eng._retire()
    assert not eng.running, "sequences outlived the measurement"
    eng.finished.clear()
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--model", default="llama3-8b")
    p.add_argument("--batch", type=int, default=24)
    p.add_argument("--ctx", type=int, default=512)
    p.add_argument("--steps", type=int, default=200)
    p.add_argument("--warmup", type=int, default=20)
    p.add_argument("--eager", action="store_true")
    p.add_argument("--live", type=int, default=0,
                   help="live rows (default: --batch)")
    p.add_argument("--repeat", type=int, default=1,
                   help="timed runs; prints their median and max - min")
    p.add_argument("--candidates", default="",
                   help="comma-separated ladder rungs below --batch to "
                        "capture instead of serve.LADDER_CANDIDATES")
    p.add_argument("--rung", type=int, default=0,
                   help="force the smallest captured rung >= RUNG (it must "
                        "hold the live rows): one live count on each rung")
    args = p.parse_args()

    from quickstart_streaming_agents_amd.models import build_model, serve
    from quickstart_streaming_agents_amd.models.serve import Engine

    assert torch.cuda.is_available()
    if args.candidates:
        serve.LADDER_CANDIDATES = tuple(
            sorted(int(c) for c in args.candidates.split(",")))
    model = build_model(args.model, device="cuda:0")
    total = args.ctx + args.steps * args.repeat + args.warmup + 8
    # the vocabulary window bench.py decodes under (tokenizer byte base to
    # trained vocab size): the graph then samples with the fused kernel
    eng = Engine(model, max_batch=args.batch, max_seq_len=total,
                 valid_vocab=(16, 3335))
    if args.eager:
        eng.use_graph = False
    live = args.live or args.batch
    assert 1 <= live <= args.batch
    if args.rung and eng._ensure_graphs():
        g = eng.graphs
        g.rungs = tuple(r for r in g.rungs if r >= args.rung)
        assert g.rungs and g.rungs[0] >= live, \
            f"--rung {args.rung}: no captured rung holds {live} rows"
    runs = measure(eng, args.ctx, live, args.steps, args.warmup, args.repeat)
    ms = statistics.median(runs)

    c = model.cfg
    w_bytes = 2 * (c.vocab_size * c.hidden * 2 +
                   c.n_layers * (model.qkv_dim * c.hidden +
                                 c.hidden * model.n_q * c.d_head +
                                 3 * model.ffn_local * c.hidden))
    kv_bytes = 2 * 2 * c.n_layers * model.n_kv * c.d_head * \
        live * (args.ctx + args.steps / 2)
    floor_ms = (w_bytes + kv_bytes) / 8e12 * 1e3
    print(f"model={args.model} batch={args.batch} live={live} "
          f"ctx={args.ctx} graph={eng.use_graph} "
          f"rungs={dict(eng.stats.decode_steps_by_rung)}")
    print(f"ms_per_step={ms:.3f} tokens_per_s={live / ms * 1e3:.0f} "
          f"hbm_floor_ms={floor_ms:.3f} frac_of_sol={floor_ms / ms:.2%}")
    if args.repeat > 1:
        print(f"runs_ms={[round(r, 3) for r in runs]} "
              f"spread_ms={max(runs) - min(runs):.3f}")


if __name__ == "__main__":
    main()
