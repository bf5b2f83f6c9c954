"""Kernel A/B for the decode attention step: the three-kernel sequence
(rope_kv_append, paged_attn_decode = attention + split reduce) against the
single fused launch (decode_attn_fused) at both of its register budgets, on
decode batches logged from the flagship bench (Llama-3-8B geometry: 32 q
heads, 8 kv heads, d_head 128, batch 192, block table 32 wide).

    python tools/decode_attn_bench.py [--batches FILE.json] [--iters 20]

A batch is the seq_lens vector of one decode step (new token included, 0 =
inactive row).  Old and new alternate inside one process; a time is the
median of `--iters` device-event samples, taken `--rounds` times, and the
spread of a callable is max - min of its medians.  Every call works on a
different one of several cache copies, as consecutive layers do in the
model, so no call finds its K/V in a cache level from the call before.
KV bytes = pages x 32 KiB x kv heads (K + V); the roof is 6.3 TB/s, what a
streaming read reaches on MI355X.

The fused launch passes when it beats the three old kernels together on
every batch by more than the larger spread; the exit status says so.
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
BT_WIDTH = 32
HBM_ROOF = 6.3e12
COPIES = 5

# Three seq_lens vectors of one `bench.py --steps 1 --warmup 1` run (batch
# 192), as the first replay of a graph run sees them: a full batch, a
# mid-step batch with inactive rows and a tail batch.
BATCH_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)),
                          "decode_batches.json")


def _time(fns, iters, rounds):
    """Alternate the callables; per callable the list of `rounds` medians
    (ms) of `iters` device-event samples."""
    for _ in range(3):
        for f in fns:
            f()
    torch.cuda.synchronize()
    meds = [[] for _ in fns]
    for _ in range(rounds):
        times = [[] for _ in fns]
        for _ in range(iters):
            for i, f in enumerate(fns):
                a = torch.cuda.Event(enable_timing=True)
                b = torch.cuda.Event(enable_timing=True)
                a.record()
                f()
                b.record()
                b.synchronize()
                times[i].append(a.elapsed_time(b))
        for i, t in enumerate(times):
            meds[i].append(statistics.median(t))
    return meds


def run_batch(name, seq_lens, iters, rounds, dev="cuda:0"):
    g = torch.Generator().manual_seed(0)
    B = len(seq_lens)
    need = [(n + 63) // 64 for n in seq_lens]
    n_pages = sum(need) + 1
    perm = torch.randperm(n_pages, generator=g).tolist()
    bt = torch.full((B, BT_WIDTH), perm[-1], dtype=torch.int32)
    at = 0
    for i, k in enumerate(need):
        bt[i, :k] = torch.tensor(perm[at:at + k], dtype=torch.int32)
        at += k
    bt = bt.to(dev)
    sl = torch.tensor(seq_lens, dtype=torch.int32, device=dev)
    qkv = (torch.randn(B, (QH + 2 * KVH) * D, generator=g) * 0.5) \
        .to(torch.bfloat16).to(dev)
    kc0 = (torch.randn(n_pages, KVH, D // 8, 64, 8, generator=g) * 0.5) \
        .to(torch.bfloat16).to(dev)
    vc0 = (torch.randn(n_pages, KVH, D, 64, generator=g) * 0.5) \
        .to(torch.bfloat16).to(dev)
    inv = 1.0 / (500000.0 ** (torch.arange(0, D, 2).float() / D))
    ang = torch.arange(2048).float()[:, None] * inv[None, :]
    cos_t, sin_t = ang.cos().to(dev), ang.sin().to(dev)
    scale = D ** -0.5
    e = ext()

    def views(buf):
        return (buf[:, :QH * D].view(B, QH, D),
                buf[:, QH * D:(QH + KVH) * D].view(B, KVH, D),
                buf[:, (QH + KVH) * D:].view(B, KVH, D))

    # ---- bit equality, on fresh copies --------------------------------------
    b1, k1, v1 = qkv.clone(), kc0.clone(), vc0.clone()
    q, k, v = views(b1)
    e.rope_kv_append(q, k, v, k1, v1, cos_t, sin_t, bt, sl)
    ref = e.paged_attn_decode(q, k1, v1, bt, sl, scale)
    for wps in (1, 2):
        b2, k2, v2 = qkv.clone(), kc0.clone(), vc0.clone()
        q, k, v = views(b2)
        out = e.decode_attn_fused(q, k, v, k2, v2, cos_t, sin_t, bt, sl,
                                  scale, wps)
        assert torch.equal(out, ref), f"fused ({wps}) output differs"
        assert torch.equal(k2, k1) and torch.equal(v2, v1), \
            f"fused ({wps}) cache differs"

    # ---- timing: rotate through cache copies --------------------------------
    sets = [(kc0.clone(), vc0.clone()) for _ in range(COPIES)]
    # the old path rotates q in place: give it a buffer of its own
    bo = qkv.clone()
    qo, ko, vo = views(bo)
    qn, kn, vn = views(qkv)
    turn = [0]

    def nxt():
        turn[0] += 1
        return sets[turn[0] % COPIES]

    def old():
        kc, vc = nxt()
        e.rope_kv_append(qo, ko, vo, kc, vc, cos_t, sin_t, bt, sl)
        return e.paged_attn_decode(qo, kc, vc, bt, sl, scale)

    def old_rope():
        kc, vc = nxt()
        e.rope_kv_append(qo, ko, vo, kc, vc, cos_t, sin_t, bt, sl)

    def old_attn():
        kc, vc = nxt()
        return e.paged_attn_decode(qo, kc, vc, bt, sl, scale)

    def fused(wps):
        def f():
            kc, vc = nxt()
            return e.decode_attn_fused(qn, kn, vn, kc, vc, cos_t, sin_t, bt,
                                       sl, scale, wps)
        return f

    labels = ["old: rope_kv_append + attention + reduce",
              "  old rope_kv_append alone",
              "  old attention + reduce alone",
              "fused, 1 wave/SIMD (<= 512 registers)",
              "fused, 2 waves/SIMD (<= 256 registers)"]
    fns = [old, old_rope, old_attn, fused(1), fused(2)]
    meds = _time(fns, iters, rounds)
    nbytes = sum(need) * 32 * 1024 * KVH
    active = sum(1 for n in seq_lens if n > 0)
    print(f"== {name}: {active}/{B} rows active, {sum(need)} pages, "
          f"{nbytes / 1e6:.0f} MB of K+V, floor "
          f"{nbytes / HBM_ROOF * 1e6:.1f} us")
    for lab, m in zip(labels, meds):
        us = statistics.median(m) * 1e3
        spread = (max(m) - min(m)) * 1e3
        rate = nbytes / (us * 1e-6)
        print(f"  {lab:42s} {us:8.1f} us  (spread {spread:5.1f})  "
              f"{rate / 1e12:5.2f} TB/s  {100 * rate / HBM_ROOF:5.1f}% of roof")
    ok = {}
    for idx, wps in ((3, 1), (4, 2)):
        margin = min(meds[0]) - max(meds[idx])
        spread = max(max(meds[0]) - min(meds[0]),
                     max(meds[idx]) - min(meds[idx]))
        ok[wps] = margin > spread
        print(f"  fused {wps} wave/SIMD vs old: margin {margin * 1e3:7.1f} us, "
              f"spread {spread * 1e3:5.1f} us -> "
              f"{'PASS' if ok[wps] else 'FAIL'}")
    return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", help="JSON: {name: [seq_len, ...]} "
                    "(default: tools/decode_batches.json)")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    with open(args.batches or BATCH_FILE) as f:
        batches = json.load(f)
    results = [run_batch(name, lens, args.iters, args.rounds)
               for name, lens in batches.items()]
    for wps in (1, 2):
        print(f"fused {wps} wave/SIMD beats the old trio on every batch: "
              f"{all(r[wps] for r in results)}")
    # the shipped default is what the binding picks when not told
    sys.exit(0 if any(all(r[w] for r in results) for w in (1, 2)) else 1)


if __name__ == "__main__":
    main()
