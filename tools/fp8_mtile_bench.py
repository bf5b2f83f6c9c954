#!/usr/bin/env python3
"""fp8 skinny GEMM at 64 rows against rocBLAS bf16 on the flagship decode
projection shapes: the four-m-tile kernel with the class's TILES and with
TILES doubled, against F.linear (rocBLAS bf16) — decides which shape
classes are routed to the skinny kernel at 33..64 rows (ops/dispatch.py
SKINNY_FP8_WIDE_CLASSES).  Results: profiles/fp8_decode_gemm.md.

Device events around single calls, the candidates of a shape alternating in
one process, weights rotated through enough copies to overflow the 256 MB
last-level cache (in a decode step every layer streams its own weights from
HBM).  Prints the median of three round medians and their max - min.

Usage: python tools/fp8_mtile_bench.py [--samples 20] [--rounds 3]
"""

import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

# class, N, K, (waves, tiles) of the shipped two-m-tile launch
SHAPES = [
    ("qkv", 6144, 4096, 8, 2),
    ("wo", 4096, 4096, 8, 1),
    ("wgu", 28672, 4096, 8, 4),
    ("wdown", 4096, 14336, 8, 1),
    ("lm_head", 128256, 4096, 2, 8),
]
PROBED = {(2, 8), (8, 4), (8, 2), (8, 1)}      # instantiated (waves, tiles)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--samples", type=int, default=20)
    p.add_argument("--rounds", type=int, default=3)
    args = p.parse_args()
    from quickstart_streaming_agents_amd.ops import dispatch as D
    from quickstart_streaming_agents_amd.ops import ext
    e = ext()
    dev = "cuda:0"
    torch.manual_seed(0)

    def timed(fn, i):
        a, b = torch.cuda.Event(enable_timing=True), \
            torch.cuda.Event(enable_timing=True)
        a.record()
        fn(i)
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3

    for name, N, K, W, T in SHAPES:
        ncopy = max(2, -(-600_000_000 // (N * K)))
        ws = [(torch.randn(N, K, device=dev) * 0.02).to(torch.bfloat16)
              for _ in range(ncopy)]
        packs = [D.pack_weight_fp8(w) for w in ws]
        for M in (64,):
            x = (torch.randn(M, K, device=dev) * 0.5).to(torch.bfloat16)
            cands = {"rocblas": lambda i: F.linear(x, ws[i % ncopy])}
            tiles = [T] + ([2 * T] if (W, 2 * T) in PROBED else [])
            for t in tiles:
                cands[f"mt4 w{W}t{t}"] = (
                    lambda i, t=t: e.skinny_gemm_fp8_probe_mt(
                        x, *packs[i % ncopy], N, K, W, t, 4))
            for fn in cands.values():          # warm up
                for i in range(3):
                    fn(i)
            torch.cuda.synchronize()
            meds = {k: [] for k in cands}
            for _ in range(args.rounds):
                samples = {k: [] for k in cands}
                for i in range(args.samples):
                    for k, fn in cands.items():   # alternate per sample
                        samples[k].append(timed(fn, i))
                for k in cands:
                    meds[k].append(statistics.median(samples[k]))
            row = "  ".join(
                f"{k}: {statistics.median(v):7.1f} us (spread "
                f"{max(v) - min(v):4.1f})" for k, v in meds.items())
            print(f"{name:8s} N={N:6d} K={K:5d} M={M:2d}  {row}",
                  flush=True)
        del ws, packs
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
