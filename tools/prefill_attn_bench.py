"""Kernel A/B for the prefill path: old vs tiled paged prefill attention and
unfused (rope_inplace + kv_scatter) vs fused rope_kv_scatter, on prefill
batches logged from the flagship bench (Llama-3-8B geometry: 32 q heads,
8 kv heads, d_head 128).

    python tools/prefill_attn_bench.py [--batches FILE.json] [--iters 20]

A batch is a list of (start, len) items: `start` positions already cached,
`len` new rows.  Old and new alternate inside one process; times are
device-event medians.  Attention FLOPs count the causal region only
(4*D per (row, key) pair and head); the roof is the 2.5 PFLOP/s dense bf16
MFMA peak of MI355X, the byte roof 8 TB/s HBM3E.
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from quickstart_streaming_agents_amd.ops import ext  # noqa: E402

QH, KVH, D = 32, 8, 128
MFMA_ROOF = 2.5e15
HBM_ROOF = 8.0e12

# Three of the eight prefill batches logged from one
# `bench.py --steps 1 --warmup 1` run (batch 192): a first-turn batch
# (start = 0) and two continuation batches (cached prefix, ragged deltas).
BATCH_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)),
                          "prefill_batches.json")


def _mk(x, dev):
    return torch.tensor(x, dtype=torch.int32, device=dev)


def _maps(lens, rows, dev):
    item, pos0 = [], []
    for i, n in enumerate(lens):
        for p0 in range(0, n, rows):
            item.append(i)
            pos0.append(p0)
    return _mk(item, dev), _mk(pos0, dev)


def _time(fns, iters):
    """Alternate the callables; per-callable median device time in ms."""
    times = [[] for _ in fns]
    for _ in range(3):
        for f in fns:
            f()
    torch.cuda.synchronize()
    for _ in range(iters):
        for i, f in enumerate(fns):
            a = torch.cuda.Event(enable_timing=True)
            b = torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            b.synchronize()
            times[i].append(a.elapsed_time(b))
    return [statistics.median(t) for t in times]


def run_batch(name, items, iters, dev="cuda:0"):
    g = torch.Generator().manual_seed(0)
    starts = [int(s) for s, _ in items]
    lens = [int(n) for _, n in items]
    T = sum(lens)
    need = [(s + n + 63) // 64 for s, n in zip(starts, lens)]
    npmax, n_pages = max(need), sum(need)
    perm = torch.randperm(n_pages, generator=g).tolist()
    bt = torch.zeros(len(items), npmax, dtype=torch.int32)
    slots, at = [], 0
    for i, k in enumerate(need):
        pages = perm[at:at + k]
        at += k
        bt[i, :k] = torch.tensor(pages, dtype=torch.int32)
        slots += [pages[p // 64] * 64 + p % 64
                  for p in range(starts[i], starts[i] + lens[i])]
    bt = bt.to(dev)
    slots = _mk(slots, dev)
    pos = _mk([p for s, n in zip(starts, lens) for p in range(s, s + n)], dev)
    offs = [sum(lens[:i]) for i in range(len(lens))]
    off_t, start_t, len_t = _mk(offs, dev), _mk(starts, dev), _mk(lens, dev)
    qkv = (torch.randn(T, (QH + 2 * KVH) * D, generator=g) * 0.5) \
        .to(torch.bfloat16).to(dev)
    q = qkv[:, :QH * D].view(T, QH, D)
    k = qkv[:, QH * D:(QH + KVH) * D].view(T, KVH, D)
    v = qkv[:, (QH + KVH) * D:].view(T, KVH, D)
    kc = (torch.randn(n_pages, KVH, D // 8, 64, 8, generator=g) * 0.5) \
        .to(torch.bfloat16).to(dev)
    vc = (torch.randn(n_pages, KVH, D, 64, generator=g) * 0.5) \
        .to(torch.bfloat16).to(dev)
    inv = 1.0 / (500000.0 ** (torch.arange(0, D, 2).float() / D))
    ang = torch.arange(4096).float()[:, None] * inv[None, :]
    cos_t, sin_t = ang.cos().to(dev), ang.sin().to(dev)
    scale = D ** -0.5
    e = ext()

    i16, p16 = _maps(lens, 16, dev)
    old = lambda: e.paged_attn_prefill(q, kc, vc, bt, i16, p16, off_t,
                                       start_t, len_t, scale, True)
    fns, labels = [old], ["old (1 wave / 16 rows x head)"]
    for rows in (32,):
        it, pt = _maps(lens, rows, dev)
        fns.append(lambda it=it, pt=pt, rows=rows: e.paged_attn_prefill_tiled(
            q, kc, vc, bt, it, pt, off_t, start_t, len_t, scale, True, rows))
        labels.append(f"tiled, {rows} rows / workgroup")
    assert torch.equal(fns[0](), fns[1]()), "tiled output differs from old"
    flops = sum(4.0 * D * QH * (n * s + n * (n + 1) / 2)
                for s, n in zip(starts, lens))
    print(f"== {name}: {len(items)} items, {T} new rows, "
          f"{flops / 1e12:.2f} TFLOP causal attention")
    for lab, ms in zip(labels, _time(fns, iters)):
        rate = flops / (ms * 1e-3)
        print(f"  attn  {lab:34s} {ms * 1e3:9.1f} us  "
              f"{rate / 1e12:7.1f} TFLOP/s  {100 * rate / MFMA_ROOF:5.1f}% "
              f"of MFMA roof")

    def unfused():
        e.rope_inplace(q, k, cos_t, sin_t, pos)
        e.kv_scatter(k, v, kc, vc, slots)

    fused = lambda: e.rope_kv_scatter(q, k, v, kc, vc, cos_t, sin_t, pos,
                                      slots)
    # byte floor: q read + write, k and v read once, cache written once
    nbytes = T * D * 2 * (2 * QH + 4 * KVH)
    for lab, ms in zip(["rope_inplace + kv_scatter", "fused rope_kv_scatter"],
                       _time([unfused, fused], iters)):
        rate = nbytes / (ms * 1e-3)
        print(f"  rope  {lab:34s} {ms * 1e3:9.1f} us  "
              f"{rate / 1e12:7.2f} TB/s    {100 * rate / HBM_ROOF:5.1f}% "
              f"of HBM roof (floor {nbytes / HBM_ROOF * 1e6:.1f} us)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", help="JSON: {name: [[start, len], ...]} "
                    "(default: tools/prefill_batches.json)")
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    with open(args.batches or BATCH_FILE) as f:
        batches = json.load(f)
    for name, items in batches.items():
        run_batch(name, items, args.iters)


if __name__ == "__main__":
    main()
