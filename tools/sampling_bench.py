#!/usr/bin/env python3
"""Per-request sampler (ops/hip/sampling.hip) against the torch op sequence
it stands beside: TokenPolicy.sample at temperature > 0 (f32 copy + vocab
bias, torch.rand, two logs, argmax) on the same bf16 logits.  B = 192 rows of
V = 128256 (randn * 3), window (16, 3335) + eos and the whole vocabulary,
T = 1, (top_k, top_p) in {(0, 1), (50, 0.9)}.  Results:
profiles/sampling.md.

The cases run in a fixed order, --iters calls each after --warmup, so a
`rocprofv3 --kernel-trace --stats` run of this script attributes its
kernel rows by order; without a profiler the script prints device-event
times (median over the rounds of the per-call mean).  The variants of a
case alternate within a round.

Usage: python tools/sampling_bench.py [--iters 20] [--rounds 5]
"""

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

B, V = 192, 128256
WINDOWS = {"window": (16, 3335, 2), "vocab": (0, V, 2)}
FILTERS = {"plain": (0, 1.0), "k50_p0.9": (50, 0.9)}


def torch_sample(logits, bias, temperature=1.0):
    """TokenPolicy.sample at temperature > 0, verbatim."""
    lg = logits.float() + bias
    u = torch.rand(lg.shape, device=lg.device,
                   dtype=torch.float32).clamp_min_(1e-20)
    gumbel = -torch.log(-torch.log(u).clamp_min_(1e-20))
    return torch.argmax(lg.float() + temperature * gumbel, dim=-1)


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), \
        torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1000.0 / iters          # us per call


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--iters", type=int, default=20)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--rounds", type=int, default=5)
    args = p.parse_args()
    assert torch.cuda.is_available(), "sampling_bench needs a GPU"
    from quickstart_streaming_agents_amd.models.serve import SamplingParams
    from quickstart_streaming_agents_amd.ops import dispatch as D
    dev = "cuda:0"
    g = torch.Generator(device=dev).manual_seed(0)
    logits = (torch.randn(B, V, device=dev, generator=g) * 3) \
        .to(torch.bfloat16)
    seed = torch.arange(B, dtype=torch.int64, device=dev) * 7919 + 1
    pos = torch.arange(B, dtype=torch.int32, device=dev) + 100
    for wname, (lo, hi, eos) in WINDOWS.items():
        bias = torch.full((V,), float("-inf"), device=dev)
        bias[lo:hi] = 0.0
        bias[eos] = 0.0
        variants = {"torch_ops": lambda: torch_sample(logits, bias)}
        for fname, (k, top_p) in FILTERS.items():
            sp = SamplingParams(temperature=1.0, top_k=k, top_p=top_p)
            cols = (torch.full((B,), sp.inv_temp, device=dev),
                    torch.full((B,), sp.top_k, dtype=torch.int32, device=dev),
                    torch.full((B,), sp.top_p_q, dtype=torch.int32,
                               device=dev))
            variants["kernel_" + fname] = (
                lambda cols=cols: D.sample_tokens(logits, lo, hi, eos, *cols,
                                                  seed, pos))
        for fn in variants.values():
            timed(fn, args.warmup)
        rounds = {name: [] for name in variants}
        for _ in range(args.rounds):
            for name, fn in variants.items():
                rounds[name].append(timed(fn, args.iters))
        for name, ts in rounds.items():
            print(json.dumps({
                "case": wname, "variant": name, "B": B, "V": V,
                "candidates": hi - lo + (0 if lo <= eos < hi else 1),
                "us_per_call_median": round(statistics.median(ts), 2),
                "us_per_call_min": round(min(ts), 2),
                "us_per_call_max": round(max(ts), 2),
                "iters": args.iters, "rounds": args.rounds}))


if __name__ == "__main__":
    main()
