"""Decode-graph ladder and fused greedy sampler, CPU side: the rung picker
and the sampler's CPU branch against the torch op sequence it replaces
(Engine._sample plus the bookkeeping of the captured decode step)."""

import pytest
import torch

from quickstart_streaming_agents_amd.models.serve import (ladder_rungs,
                                                          pick_rung)
from quickstart_streaming_agents_amd.ops import dispatch as D

MAX_RUN = 8


def test_pick_rung_full_ladder():
    rungs = ladder_rungs(192)
    assert rungs[-1] == 192 and list(rungs) == sorted(set(rungs))
    assert set(rungs) <= {16, 32, 64, 128, 192}
    full = (16, 32, 64, 128, 192)
    want = {1: 16, 16: 16, 17: 32, 64: 64, 65: 128, 192: 192}
    for n, r in want.items():
        assert pick_rung(full, n) == r
        # whatever rungs survived pruning: smallest rung that holds n
        got = pick_rung(rungs, n)
        assert got >= n and got == min(x for x in rungs if x >= n)
    with pytest.raises(ValueError):
        pick_rung(full, 193)


@pytest.mark.parametrize("max_batch", [2, 48])
def test_rungs_clip_to_max_batch(max_batch):
    rungs = ladder_rungs(max_batch)
    assert rungs[-1] == max_batch
    assert all(r <= max_batch for r in rungs)
    assert list(rungs) == sorted(set(rungs))
    for n in range(1, max_batch + 1):
        assert pick_rung(rungs, n) == min(x for x in rungs if x >= n)
    assert ladder_rungs(max_batch, ladder=False) == (max_batch,)
    if max_batch == 2:
        assert rungs == (2,)


# ---- sampler cases (shared with tests/test_gpu_decode_ladder.py) ----------

def sampler_case(B, V, lo, hi, eos, seed, step):
    """Inputs of one sampling step; logits take 7 distinct bf16 values, so
    ties are everywhere.  Two rows are scripted at `step`."""
    g = torch.Generator().manual_seed(seed)
    vals = torch.tensor([-3.0, -1.5, -0.25, 0.0, 0.5, 1.75, 2.5],
                        dtype=torch.bfloat16)
    logits = vals[torch.randint(0, 7, (B, V), generator=g)]
    Bmax = B + 3          # the buffers are wider than the live rows
    script = torch.randint(0, V, (Bmax, MAX_RUN), generator=g)
    mask = torch.zeros(Bmax, MAX_RUN, dtype=torch.bool)
    mask[0, step] = True
    mask[B - 1, step] = True
    mask[1, (step + 1) % MAX_RUN] = True      # scripted at another step
    hist = torch.full((MAX_RUN, Bmax), -7, dtype=torch.int64)
    tokens = torch.full((Bmax,), -7, dtype=torch.int64)
    ctr = torch.tensor([step], dtype=torch.int64)
    return dict(logits=logits, lo=lo, hi=hi, eos=eos, script=script,
                mask=mask, hist=hist, tokens=tokens, ctr=ctr, B=B)


def torch_sequence(c):
    """The ops of Engine._sample and the captured step, verbatim."""
    logits, B = c["logits"], c["B"]
    dev = logits.device
    V = logits.shape[1]
    bias = torch.full((V,), float("-inf"), device=dev, dtype=torch.float32)
    bias[c["lo"]:c["hi"]] = 0.0
    if c["eos"] is not None:
        bias[c["eos"]] = 0.0
    hist, tokens, ctr = c["hist"].clone(), c["tokens"].clone(), \
        c["ctr"].clone()
    nxt = torch.argmax(logits.float() + bias, dim=-1)
    j = ctr.clamp(max=MAX_RUN - 1)
    forced = c["script"][:B].index_select(1, j).squeeze(1)
    fmask = c["mask"][:B].index_select(1, j).squeeze(1)
    nxt = torch.where(fmask, forced, nxt)
    hist[:, :B].index_copy_(0, ctr, nxt.unsqueeze(0))
    ctr.add_(1)
    tokens[:B].copy_(nxt)
    return tokens, hist, ctr


SAMPLER_CASES = [
    # (B, V, lo, hi, eos): eos outside and inside the window, and none
    (5, 2048, 16, 1000, 2),
    (5, 2048, 16, 1000, 500),
    (5, 2048, 16, 1000, 1500),
    (5, 2048, 16, 1000, None),
    (3, 128256, 16, 3335, 2),
    (3, 128256, 16, 3335, 100),
    (3, 128256, 16, 3335, 128000),
]


@pytest.mark.parametrize("B,V,lo,hi,eos", SAMPLER_CASES)
def test_sampler_cpu_branch_matches_torch_sequence(B, V, lo, hi, eos):
    for step in (0, 3, MAX_RUN - 1):
        c = sampler_case(B, V, lo, hi, eos, seed=B * 1000 + step, step=step)
        want_tokens, want_hist, want_ctr = torch_sequence(c)
        tokens, hist, ctr = c["tokens"].clone(), c["hist"].clone(), \
            c["ctr"].clone()
        D.greedy_sample_step(c["logits"], lo, hi,
                             -1 if eos is None else eos, c["script"][:B],
                             c["mask"][:B], ctr, hist[:, :B], tokens)
        assert torch.equal(tokens, want_tokens)
        assert torch.equal(hist, want_hist)
        assert torch.equal(ctr, want_ctr)
        # the scripted rows took their script, the rest sampled in-window
        assert tokens[0] == c["script"][0, step]
        free = tokens[1:B - 1]
        ok = (free >= lo) & (free < hi)
        if eos is not None:
            ok |= free == eos
        assert bool(ok.all())


def test_sampler_cpu_all_neg_inf_window_gives_index_zero():
    logits = torch.full((2, 64), float("-inf"), dtype=torch.bfloat16)
    logits[:, :4] = 1.0           # outside the window: must not be picked
    c = dict(logits=logits, lo=8, hi=32, eos=40, B=2,
             script=torch.zeros(2, MAX_RUN, dtype=torch.int64),
             mask=torch.zeros(2, MAX_RUN, dtype=torch.bool),
             hist=torch.zeros(MAX_RUN, 2, dtype=torch.int64),
             tokens=torch.zeros(2, dtype=torch.int64),
             ctr=torch.zeros(1, dtype=torch.int64))
    want_tokens, want_hist, want_ctr = torch_sequence(c)
    D.greedy_sample_step(logits, 8, 32, 40, c["script"], c["mask"], c["ctr"],
                         c["hist"], c["tokens"])
    assert torch.equal(c["tokens"], want_tokens)
    assert torch.equal(c["hist"], want_hist)
    assert torch.equal(c["ctr"], want_ctr)
