"""The hipGraph-captured decode step of the serving engine (models/serve.py):
its buffers, the step itself (callable eagerly on any device) and its
captures.  Built from the model, the KV cache and the token policy; the
Engine keeps scheduling and what follows a run (EOS, finishing, stats)."""

from __future__ import annotations

import contextlib
import gc
import os
import time

import torch

from ..ops import dispatch as D

_TIMING = os.environ.get("QSA_TIMING", "") == "1"


@contextlib.contextmanager
def _gc_quiet():
    """Collect dead cycles now and keep the cyclic collector off inside.
    Cyclic garbage that holds CUDAGraphs dies only when the collector runs;
    if that happens while a stream is capturing, the graphs' destructors
    synchronise the device, which a capture does not allow, and the process
    aborts."""
    gc.collect()
    was_enabled = gc.isenabled()
    gc.disable()
    try:
        yield
    finally:
        if was_enabled:
            gc.enable()


def pick_rung(rungs: tuple, n: int) -> int:
    """Smallest rung that holds n live rows (rungs ascending)."""
    for r in rungs:
        if r >= n:
            return r
    raise ValueError(f"{n} live rows exceed the largest rung {rungs[-1]}")


def _seed_i64(seed: int) -> int:
    """The 64 seed bits as the two's-complement value an i64 tensor holds."""
    return seed - (1 << 64) if seed >= 1 << 63 else seed


class TokenPolicy:
    """The engine-wide token policy: temperature, and the free-text
    sampling mask — tokens outside valid_vocab = [lo, hi) (plus EOS) are
    never emitted, which keeps random-init decode inside the tokenizer's
    trained vocab so outputs are real text (models/grammar.py)."""

    def __init__(self, temperature: float,
                 valid_vocab: tuple[int, int] | None, eos_id: int | None,
                 vocab_size: int, device):
        self.temperature = float(temperature)
        self.eos_id = eos_id
        self.valid_vocab = None
        self.vocab_bias: torch.Tensor | None = None
        if valid_vocab is not None:
            lo, hi = valid_vocab
            self.valid_vocab = (int(lo), int(hi))
            bias = torch.full((vocab_size,), float("-inf"), device=device,
                              dtype=torch.float32)
            bias[lo:hi] = 0.0
            if eos_id is not None:
                bias[eos_id] = 0.0
            self.vocab_bias = bias

    def sample(self, logits: torch.Tensor) -> torch.Tensor:
        """Greedy at temperature 0; Gumbel-argmax sampling otherwise."""
        if self.vocab_bias is not None:
            logits = logits.float() + self.vocab_bias
        if self.temperature <= 0.0:
            return torch.argmax(logits, dim=-1)
        u = torch.rand(logits.shape, device=logits.device,
                       dtype=torch.float32).clamp_min_(1e-20)
        gumbel = -torch.log(-torch.log(u).clamp_min_(1e-20))
        return torch.argmax(logits.float() + self.temperature * gumbel,
                            dim=-1)

    def window(self, logits: torch.Tensor) -> tuple[int, int, int]:
        """lo, hi, eos of the samplers: the valid-vocab window, or the
        whole vocabulary without one."""
        lo, hi = self.valid_vocab or (0, logits.shape[-1])
        return lo, hi, -1 if self.eos_id is None else int(self.eos_id)

    def fused(self, logits: torch.Tensor) -> bool:
        """The one-launch greedy sampler (ops/hip/elementwise.hip) applies
        to greedy decoding of GPU bf16 logits under a vocab window."""
        return self.temperature <= 0.0 and self.valid_vocab is not None \
            and logits.is_cuda and logits.dtype == torch.bfloat16


class DecodeGraphs:
    """Buffers, step and captured graphs of the self-feeding decode step.
    Every rung works on the leading rows of the same max_batch buffers and
    all graphs share one memory pool (they never replay concurrently), so a
    small rung costs its kernels, not its own activations."""

    def __init__(self, model, kv, policy: TokenPolicy, max_batch: int,
                 max_seq_len: int, max_run: int, rungs: tuple):
        self.model = model
        self.kv = kv
        self.policy = policy
        self.max_batch = max_batch
        self.max_run = max_run
        self.rungs = rungs
        self.greedy: dict = {}    # rung (rows) -> captured graph
        # the second ladder (per-request sampler), captured on first need
        self.sampled: dict = {}
        self.sampled_failed = False
        self._pool = None
        dev = model.device
        B = max_batch
        cap = (max_seq_len + 63) // 64
        self.tokens = torch.zeros(B, dtype=torch.int64, device=dev)
        self.block_table = torch.zeros(B, cap, dtype=torch.int32, device=dev)
        self.seq_lens = torch.zeros(B, dtype=torch.int32, device=dev)
        self.active = torch.zeros(B, dtype=torch.int32, device=dev)
        self.ctr = torch.zeros(1, dtype=torch.int64, device=dev)
        self.hist = torch.zeros(max_run, B, dtype=torch.int64, device=dev)
        # grammar scripts: forced token at run-step j for each row
        # (script_mask False -> free sample)
        self.script = torch.zeros(B, max_run, dtype=torch.int64, device=dev)
        self.script_mask = torch.zeros(B, max_run, dtype=torch.bool,
                                       device=dev)
        # scratch of the fused sampler kernel
        self.ticket = torch.zeros(1, dtype=torch.int32, device=dev)
        # per-request sampling parameters (inv_temp 0: a greedy row)
        self.inv_temp = torch.zeros(B, dtype=torch.float32, device=dev)
        self.top_k = torch.zeros(B, dtype=torch.int32, device=dev)
        self.top_p_q = torch.full((B,), 65536, dtype=torch.int32, device=dev)
        self.seed = torch.zeros(B, dtype=torch.int64, device=dev)

    def step(self, b: int, sampled: bool = False) -> None:
        """Self-feeding decode step on rows [0, b): advance seq_lens (in
        the graph, when captured), append the step's k/v at seq_lens-1,
        attend, sample, record, feed back.  forward_decode derives positions
        from seq_lens itself; its `positions` argument is unused."""
        tokens, seq_lens = self.tokens[:b], self.seq_lens[:b]
        seq_lens.add_(self.active[:b])
        logits = self.model.forward_decode(
            tokens, self.kv, self.block_table[:b], seq_lens, None)
        if sampled:
            # the second ladder: every row through the per-request sampler,
            # drawn at its absolute position (seq_lens after the add_)
            lo, hi, eos = self.policy.window(logits)
            D.sample_step(
                logits.to(torch.bfloat16), lo, hi, eos,
                self.inv_temp[:b], self.top_k[:b], self.top_p_q[:b],
                self.seed[:b], seq_lens, self.script[:b],
                self.script_mask[:b], self.ctr, self.hist[:, :b], tokens,
                self.ticket)
            return
        if self.policy.fused(logits):
            lo, hi, eos = self.policy.window(logits)
            D.greedy_sample_step(
                logits, lo, hi, eos, self.script[:b], self.script_mask[:b],
                self.ctr, self.hist[:, :b], tokens, self.ticket)
            return
        nxt = self.policy.sample(logits)
        # grammar-forced tokens override the free sample in-graph
        j = self.ctr.clamp(max=self.max_run - 1)
        forced = self.script[:b].index_select(1, j).squeeze(1)
        fmask = self.script_mask[:b].index_select(1, j).squeeze(1)
        nxt = torch.where(fmask, forced, nxt)
        self.hist[:, :b].index_copy_(0, self.ctr, nxt.unsqueeze(0))
        self.ctr.add_(1)
        tokens.copy_(nxt)

    def capture(self, sampled: bool) -> None:
        """One graph of the decode step per rung, into self.greedy or
        self.sampled; both ladders draw on the same memory pool.  A failure
        of the greedy ladder is the caller's to handle; one of the sampled
        ladder is recorded in sampled_failed, and the greedy ladder stays."""
        if sampled:
            # the buffers are idle here (no live row), so the warm-up steps
            # write nothing into the KV cache
            self.active.zero_()
            self.seq_lens.zero_()
        graphs: dict = {}
        try:
            with _gc_quiet():
                # largest first: it sizes the pool
                for b in reversed(self.rungs):
                    # warm up the exact captured ops (allocator + rocBLAS
                    # algo selection)
                    for _ in range(2):
                        self.step(b, sampled)
                    self.ctr.zero_()
                    self.seq_lens.zero_()
                    torch.cuda.synchronize()
                    g = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(g, pool=self._pool):
                        self.step(b, sampled)
                    if self._pool is None:
                        self._pool = g.pool()
                    graphs[b] = g
        except Exception:
            if not sampled:
                raise
            self.sampled_failed = True
            torch.cuda.synchronize()
            return
        if sampled:
            self.sampled = graphs
        else:
            self.greedy = graphs

    def fill(self, batch: list, run: int, sampled: bool = False) -> None:
        """Set the buffers up for `run` steps of `batch` (sequences as the
        engine's: seq_id, prompt, out_tokens, script, sampling, seed)."""
        n = len(batch)
        dev = self.tokens.device
        for s in batch:  # pre-extend pages for the whole run
            self.kv.extend(s.seq_id, len(s.prompt) + len(s.out_tokens) + run)
        bt = self.kv.block_table([s.seq_id for s in batch])
        self.block_table[:n, :bt.shape[1]] = bt
        # seq_lens the steps start from EXCLUDE the token the first step
        # decodes: its add_(active) then yields len(prompt)+len(out) — the
        # same "includes the new token" value the eager path passes
        # (appending at slot len(prompt)+len(out)-1, no zero hole after the
        # prompt)
        self.seq_lens[:n] = torch.tensor(
            [len(s.prompt) + len(s.out_tokens) - 1 for s in batch],
            dtype=torch.int32, device=dev)
        self.tokens[:n] = torch.tensor([s.out_tokens[-1] for s in batch],
                                       dtype=torch.int64, device=dev)
        self.active[:n] = 1
        if n < self.max_batch:
            self.seq_lens[n:] = 0
            self.active[n:] = 0
        # grammar scripts for this run window: run-step j emits
        # out_tokens[d + j] whose script index is d - 1 + j (out_tokens[0]
        # was the prefill-sampled decision token)
        if any(s.script for s in batch):
            sc = torch.zeros(n, run, dtype=torch.int64)
            sm = torch.zeros(n, run, dtype=torch.bool)
            for i, s in enumerate(batch):
                if not s.script:
                    continue
                d = len(s.out_tokens)
                window = s.script[d - 1: d - 1 + run]
                if window:
                    sc[i, :len(window)] = torch.tensor(window,
                                                       dtype=torch.int64)
                    sm[i, :len(window)] = True
            self.script[:n, :run] = sc.to(dev)
            self.script_mask[:n, :run] = sm.to(dev)
            self.script_mask[:n, run:] = False
            if n < self.max_batch:
                self.script_mask[n:] = False
        else:
            self.script_mask.fill_(False)
        self.ctr.zero_()
        if sampled:
            # rows without `sampling` (and the idle rows of the rung) are
            # greedy rows of the per-request sampler
            own = [s.sampling for s in batch]
            self.inv_temp.zero_()
            self.inv_temp[:n] = torch.tensor(
                [p.inv_temp if p else 0.0 for p in own],
                dtype=torch.float32, device=dev)
            self.top_k[:n] = torch.tensor(
                [p.top_k if p else 0 for p in own],
                dtype=torch.int32, device=dev)
            self.top_p_q[:n] = torch.tensor(
                [p.top_p_q if p else 65536 for p in own],
                dtype=torch.int32, device=dev)
            self.seed[:n] = torch.tensor(
                [_seed_i64(s.seed) if s.sampling else 0 for s in batch],
                dtype=torch.int64, device=dev)

    def read(self, n: int, run: int) -> list:
        """Tokens of the last `run` steps, one list per live row (the one
        host sync of a run)."""
        return self.hist[:run, :n].t().tolist()

    def run(self, batch: list, run: int, sampled: bool = False) -> tuple:
        """`run` replays for `batch` with zero host round trips: the graph
        self-feeds, one sync at the end -> (tokens per row, rung, seconds
        between fill and read-back under QSA_TIMING=1, else 0)."""
        self.fill(batch, run, sampled)
        if _TIMING:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
        # the rung depends on len(batch) alone, so the schedule and the
        # results stay a deterministic function of the inputs
        rung = pick_rung(self.rungs, len(batch))
        g = (self.sampled if sampled else self.greedy)[rung]
        for _ in range(run):
            g.replay()
        dt = 0.0
        if _TIMING:
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
        return self.read(len(batch), run), rung, dt
