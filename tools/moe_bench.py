#!/usr/bin/env python3
"""Mixtral-8x7B decode FFN, one layer (E=8, H=4096, F=14336; about 2.8 GB
of bf16 experts plus 1.4 GB of fp8 stream per layer copy): the dense
compute-all-experts loop against the routed path on the fp8 and on the bf16
stacked streams (models/mixtral.py _ffn), at T rows of random top-2 routing
from a fixed seed.  Results: profiles/moe_routed_decode.md.

Each variant is the model's own _ffn (router included), captured in a
hipGraph per layer copy as the engine's decode step is, and replayed between
device events; the variants of a T alternate in one process and the layer
copies rotate, so that no call finds its weights in the 256 MB last-level
cache.  Prints the median of the round medians and their max - min, the
bytes the routing makes the routed path stream (distinct routed experts x
expert bytes, computed here from the routing) and the rate over those bytes.

Usage: python tools/moe_bench.py [--samples 20] [--rounds 3] [--layers 2]
"""

import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

ROWS = (1, 2, 4, 16, 24, 64)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--samples", type=int, default=20)
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--layers", type=int, default=2,
                   help="layer copies to rotate through")
    args = p.parse_args()
    assert torch.cuda.is_available(), "moe_bench needs a GPU"
    from quickstart_streaming_agents_amd.models.mixtral import (MixtralConfig,
                                                                MixtralModel)
    from quickstart_streaming_agents_amd.ops import dispatch as D
    dev = "cuda:0"
    cfg = MixtralConfig(name="moe-bench", vocab_size=2048,
                        n_layers=args.layers, max_pos=2048)
    os.environ["QSA_MOE_ROUTED"] = "1"
    os.environ["QSA_FP8"] = "1"
    model = MixtralModel(cfg, device=dev, seed=0)
    E, H, Fd = cfg.n_experts, cfg.hidden, cfg.ffn
    # the same layers with the bf16 stacked streams
    bf16_layers = []
    for L in model.layers:
        L2 = dict(L)
        for key, col in (("moe_wgu", 0), ("moe_wdown", 1)):
            L2[key] = D.moe_pack_experts(
                [L["experts"][e][col] for e in range(E)], fp8=False)
        bf16_layers.append(L2)
    torch.cuda.synchronize()
    print(f"resident {torch.cuda.memory_allocated() / 1e9:.1f} GB "
          f"({args.layers} layer copies: bf16 experts, fp8 and bf16 stacks)",
          flush=True)
    # name -> (routed, fp8, layers, bytes per expert)
    per_w = 3 * Fd * H
    variants = {
        "dense": (False, True, model.layers, 2 * per_w),
        "routed-fp8": (True, True, model.layers, per_w + 4 * (2 * Fd + H)),
        "routed-bf16": (True, False, bf16_layers, 2 * per_w),
    }

    def call(name, li, h):
        routed, fp8, layers, _ = variants[name]
        model._moe_routed, model._moe_fp8 = routed, fp8
        return model._ffn(layers[li], h)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), \
            torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3

    g = torch.Generator().manual_seed(0)
    for T in ROWS:
        h = (torch.randn(T, H, generator=g) * 0.5).to(torch.bfloat16).to(dev)
        runs, keep = {}, []
        with torch.no_grad():
            for name in variants:
                fns = []
                for li in range(args.layers):
                    for _ in range(3):                  # warm up
                        call(name, li, h)
                    torch.cuda.synchronize()
                    graph = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(graph):
                        out = call(name, li, h)
                    keep.append(out)                    # the graph's output
                    fns.append(graph.replay)
                runs[name] = fns
            # distinct experts the routing picks, per layer copy
            distinct = []
            for L in model.layers:
                probs = torch.softmax(F.linear(h, L["router"]).float(), -1)
                idx = torch.topk(probs, cfg.top_k, dim=-1)[1]
                distinct.append(len(set(idx.flatten().tolist())))
            for fns in runs.values():
                for fn in fns:
                    fn()
            torch.cuda.synchronize()
            meds = {k: [] for k in runs}
            for _ in range(args.rounds):
                samples = {k: [] for k in runs}
                for i in range(args.samples):
                    for k, fns in runs.items():         # alternate per sample
                        samples[k].append(timed(fns[i % args.layers]))
                for k in runs:
                    meds[k].append(statistics.median(samples[k]))
        nexp = sum(distinct) / len(distinct)
        print(f"T={T:2d}  distinct routed experts {nexp:.1f} of {E}",
              flush=True)
        for k, v in meds.items():
            us = statistics.median(v)
            per_expert = variants[k][3]
            nbytes = (E if k == "dense" else nexp) * per_expert
            print(f"    {k:12s} {us:8.1f} us (spread {max(v) - min(v):5.1f})"
                  f"  streams {nbytes / 1e9:5.2f} GB  "
                  f"{nbytes / us / 1e6:5.2f} TB/s", flush=True)
        del runs, keep
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
