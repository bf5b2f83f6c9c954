"""Continuous-batching serving engine for the agent LLM — the local
replacement for the managed ML_PREDICT('llm_textgen_model') endpoint
(reference terraform/core/main.tf:461,495 models).

Sequences are admitted into the running decode batch as KV pages free up
(vLLM-style): each step() admits pending prompts via ONE batched prefill
(per-token projections fused across sequences; attention per sequence),
then runs ONE fused decode step for every running sequence through the
paged-attention kernel.  Thousands of agent episodes (agents/schedule.py)
gang their LLM turns into these batches; tool round trips run on host
threads between turns, so the GPU stays busy.

Multi-turn agent episodes reuse their KV prefix: a conversation keeps its
sequence alive between turns, the engine rolls the cache back to the shared
prompt prefix and prefills only the delta (observation text) — turn N of an
episode costs O(new tokens), not O(whole transcript).

The decode step (models/decode_graph.py, DecodeGraphs.step) is
hipGraph-captured at a ladder of row counts (16, 32, 64, max_batch) and
each run replays the smallest rung that holds its live rows,
so a nearly drained batch pays for its own rows, not for max_batch
(QSA_DECODE_LADDER=0: one max_batch graph).

Sampling: free text decodes greedily (deterministic); grammar decision
tokens sample from the model's masked distribution under a fixed seed
(models/grammar.py) — the whole benchmark stays reproducible.  A request
may carry its own SamplingParams (temperature, top-k, top-p, seed): its
tokens are drawn by the seeded rule of ops/dispatch.py (sample_step), a
function of the row's logits, parameters, seed and absolute position alone,
so they do not depend on batch mates, ladder rung, run length or TP rank.
"""

from __future__ import annotations

import math
import os as _os
import random
import time
from dataclasses import dataclass, field

import torch

from .decode_graph import (_TIMING, DecodeGraphs, TokenPolicy,  # noqa: F401
                           _seed_i64, pick_rung)
from .llama import LlamaModel


@dataclass(frozen=True)
class SamplingParams:
    """Per-request sampling.  temperature 0 is greedy; top_k 0 and top_p 1
    are off; seed None draws one from the engine's seed generator."""
    temperature: float = 0.0
    top_k: int = 0
    top_p: float = 1.0
    seed: int | None = None

    def __post_init__(self):
        t = self.temperature
        if not (isinstance(t, (int, float)) and math.isfinite(t) and t >= 0):
            raise ValueError(f"temperature must be finite and >= 0, got {t!r}")
        if not math.isfinite(self.inv_temp):
            raise ValueError(f"temperature {t!r} is too small for f32")
        if not (isinstance(self.top_k, int) and 0 <= self.top_k < 2 ** 31):
            raise ValueError(f"top_k must be an int >= 0, got {self.top_k!r}")
        if not 0.0 < self.top_p <= 1.0:
            raise ValueError(f"top_p must be in (0, 1], got {self.top_p!r}")
        if self.seed is not None and not 0 <= self.seed < 2 ** 64:
            raise ValueError(f"seed must be in [0, 2^64), got {self.seed!r}")

    @property
    def inv_temp(self) -> float:
        """float32(1 / temperature), 0 for greedy."""
        if self.temperature == 0:
            return 0.0
        return float(torch.tensor(1.0 / self.temperature,
                                  dtype=torch.float64).float())

    @property
    def top_p_q(self) -> int:
        """top_p in 16-bit fixed point, 65536 = off."""
        return min(65536, max(1, int(self.top_p * 65536 + 0.5)))


@dataclass
class Sequence:
    seq_id: int
    prompt: list[int]            # full prompt tokens for this turn
    max_new_tokens: int
    cached_len: int = 0          # prefix positions already in the KV cache
    out_tokens: list[int] = field(default_factory=list)
    done: bool = False
    keep_alive: bool = False     # conversation: keep KV after completion
    # grammar-constrained decoding (models/grammar.py): the first generated
    # token is logit-masked to `decision_allowed`; if the sampled decision
    # has an entry in `branches`, the rest of the turn is forced to that
    # token script (ending in EOS), else it decodes free.
    decision_allowed: list[int] | None = None
    branches: dict[int, list[int]] | None = None
    script: list[int] | None = None
    # per-request sampling (None: the engine-wide policy) and the seed its
    # draws actually use
    sampling: SamplingParams | None = None
    seed: int | None = None

    @property
    def sampled(self) -> bool:
        """Draws at a temperature of its own above 0."""
        return self.sampling is not None and self.sampling.temperature > 0


@dataclass
class EngineStats:
    prefill_tokens: int = 0
    cached_prefix_tokens: int = 0
    decode_tokens: int = 0
    decode_steps: int = 0
    jump_forward_tokens: int = 0
    prefills: int = 0
    prefill_batches: int = 0
    wall_s: float = 0.0
    prefill_s: float = 0.0
    decode_s: float = 0.0
    # decode steps bucketed by live rows (len(batch) of the run), and graph
    # replays bucketed by the ladder rung that ran them
    decode_steps_by_live: dict = field(default_factory=dict)
    decode_steps_by_rung: dict = field(default_factory=dict)
    # decode steps by sampler: graph replays by the ladder that ran them,
    # eager steps "sampled" when a live row has a temperature of its own > 0
    decode_steps_by_sampler: dict = field(
        default_factory=lambda: {"greedy": 0, "sampled": 0})


_TUNABLE_DONE = False
# QSA_DECODE_LADDER=0 (read once, here) restores the single max_batch decode
# graph for A/B runs; tests flip the module attribute.
DECODE_LADDER = _os.environ.get("QSA_DECODE_LADDER", "1") != "0"
# row counts of the decode-graph ladder below max_batch, which is always a
# rung.  Each is faster than the next larger rung by far more than the
# run-to-run spread on MI355X; 128 was not (7.27 against 7.16 ms at
# max_batch 192) and is left out (profiles/README.md, "Decode ladder").
LADDER_CANDIDATES = (16, 32, 64)


def ladder_rungs(max_batch: int, ladder: bool = True) -> tuple:
    """Row counts the decode graph is captured at, ascending."""
    if not ladder:
        return (max_batch,)
    return tuple(c for c in LADDER_CANDIDATES if c < max_batch) + (max_batch,)


def _enable_tunableop() -> None:
    """Load the pre-tuned hipBLASLt/rocBLAS GEMM picks for the decode
    and prefill shapes (PyTorch TunableOp results generated on MI355X by
    tools/tune_gemms.py; +5% on the flagship bench measured A/B).
    Tuning itself stays OFF — unknown shapes fall back to the default
    heuristics; any failure falls back silently."""
    global _TUNABLE_DONE
    if _TUNABLE_DONE or _os.environ.get("QSA_NO_TUNABLEOP") == "1":
        return
    _TUNABLE_DONE = True
    try:
        path = _os.path.join(_os.path.dirname(_os.path.abspath(__file__)),
                             "..", "data", "tunableop_mi355x.csv")
        if _os.path.exists(path):
            t = torch.cuda.tunable
            t.enable(True)
            t.tuning_enable(False)
            t.read_file(path)
    except Exception:
        pass


class Engine:
    def __init__(self, model: LlamaModel, kv_pages: int | None = None,
                 max_batch: int = 256, max_seq_len: int = 4096,
                 eos_id: int | None = None, prefill_batch_tokens: int = 65536,
                 temperature: float = 0.0,
                 valid_vocab: tuple[int, int] | None = None,
                 decision_temperature: float = 1.0, seed: int = 0):
        if torch.cuda.is_available():
            _enable_tunableop()   # load the pre-tuned GEMM picks
        self.model = model
        # seeds of requests whose SamplingParams leave the seed open
        self._seed_rng = random.Random(seed)
        # grammar decision tokens are SAMPLED from the model's masked
        # distribution (temperature-1 Gumbel-argmax by default): the
        # model's logits drive tool-vs-finish control flow, as in real
        # tool-choice serving; deterministic under a fixed torch seed.
        # 0 = greedy decisions (degenerate under random-init weights:
        # every episode makes the same choice).
        self.decision_temperature = float(decision_temperature)
        # jump-forward on fully-forced grammar segments (see _admit);
        # QSA_NO_JUMP_FORWARD=1 restores serial decode for comparison
        self.jump_forward = _os.environ.get(
            "QSA_NO_JUMP_FORWARD", "") != "1"
        self.max_batch = max_batch
        self.max_seq_len = max_seq_len
        self.eos_id = eos_id  # None -> run to max_new_tokens (random weights)
        self.prefill_batch_tokens = prefill_batch_tokens
        if kv_pages is None:
            kv_pages = max_batch * ((max_seq_len + 63) // 64) + 64
        self.kv = model.new_kv_cache(kv_pages)
        self._next_id = 0
        self.pending: list[Sequence] = []
        self.running: list[Sequence] = []
        self.finished: list[Sequence] = []   # drained by run_chunk callers
        self.stats = EngineStats()
        # hipGraph-captured decode step (launch-bound otherwise: ~300
        # kernel/GEMM launches per step across 32 layers).  TP ranks
        # capture too — the per-layer RCCL all-reduces are recorded into
        # the graph (validated against eager on hardware,
        # tests/test_gpu_models.py rccl-in-graph test); if capture fails
        # on a given stack the engine falls back to eager decode.
        # TP NOTE: grammar decision sampling draws torch.rand — TP ranks
        # must share a seed so sampled decisions agree across the group.
        # Rows that have `sampling` need no shared torch seed: their draws
        # are a function of the logits, the request's seed and the position.
        # Only a model that lives on the GPU is captured: capturing a CPU
        # model on a GPU host records an empty graph whose replays emit
        # nothing (every decoded token reads back as 0).
        self.use_graph = torch.cuda.is_available() and \
            torch.device(model.device).type == "cuda"
        self.graphs: DecodeGraphs | None = None   # built on first use
        # engine-wide token policy.  temperature 0 = greedy (the
        # deterministic benchmark contract); > 0 samples via the
        # Gumbel-argmax trick, which stays a single argmax and is
        # hipGraph-capture-safe (torch captures RNG state advancement, so
        # replays draw fresh noise)
        self.policy = TokenPolicy(temperature, valid_vocab, eos_id,
                                  model.cfg.vocab_size, model.device)

    def _sample_rows(self, logits: torch.Tensor, seqs: list["Sequence"],
                     pos: list[int]) -> list[int]:
        """Tokens of rows that have `sampling`: the seeded draw of
        ops/dispatch.py at absolute position pos[i] (row i of logits)."""
        from ..ops import dispatch as D
        dev = logits.device

        def col(vals, dtype):
            return torch.tensor(vals, dtype=dtype, device=dev)

        lo, hi, eos = self.policy.window(logits)
        toks = D.sample_tokens(
            logits.to(torch.bfloat16).contiguous(), lo, hi, eos,
            col([s.sampling.inv_temp for s in seqs], torch.float32),
            col([s.sampling.top_k for s in seqs], torch.int32),
            col([s.sampling.top_p_q for s in seqs], torch.int32),
            col([_seed_i64(s.seed) for s in seqs], torch.int64),
            col(pos, torch.int32))
        return [int(t) for t in toks.tolist()]

    def _sample_first(self, logits: torch.Tensor,
                      admitted: list["Sequence"]) -> list[int]:
        """Each admitted sequence's first token.  Rows that have `sampling`
        and no decision mask draw theirs at position len(prompt); the rest
        follow the engine-wide policy, untouched by those rows."""
        out = self._sample_first_policy(logits, admitted)
        own = [i for i, s in enumerate(admitted)
               if s.sampling is not None and not s.decision_allowed]
        if own:
            toks = self._sample_rows(logits[own], [admitted[i] for i in own],
                                     [len(admitted[i].prompt) for i in own])
            for i, t in zip(own, toks):
                out[i] = t
        return out

    def _sample_first_policy(self, logits: torch.Tensor,
                             admitted: list["Sequence"]) -> list[int]:
        """Sample each admitted sequence's first token, honoring per-row
        decision masks (grammar turns) with ONE host sync."""
        free = self.policy.sample(logits)
        rows = [i for i, s in enumerate(admitted) if s.decision_allowed]
        if not rows:
            return [int(t) for t in free.tolist()]
        K = max(len(admitted[i].decision_allowed) for i in rows)
        idx = torch.tensor(
            [admitted[i].decision_allowed
             + [admitted[i].decision_allowed[-1]]
             * (K - len(admitted[i].decision_allowed)) for i in rows],
            dtype=torch.int64, device=logits.device)
        lens = torch.tensor([len(admitted[i].decision_allowed)
                             for i in rows], device=logits.device)
        pad = torch.arange(K, device=logits.device)[None, :] >= lens[:, None]
        sub = logits[rows].float().gather(1, idx)          # [R, K]
        t = self.decision_temperature
        if t > 0.0:
            u = torch.rand(sub.shape, device=sub.device).clamp_min_(1e-20)
            sub = sub / t + (-torch.log(-torch.log(u)))
        sub = sub.masked_fill(pad, float("-inf"))
        pick = idx.gather(1, torch.argmax(sub, 1, keepdim=True)).squeeze(1)
        out = free.tolist()
        for r, t in zip(rows, pick.tolist()):
            out[r] = int(t)
        return [int(t) for t in out]

    # ---- hipGraph decode -------------------------------------------------
    MAX_RUN = 512  # on-device token-history depth per graph run

    def _ensure_graphs(self) -> bool:
        """Build the DecodeGraphs and capture the greedy ladder on first
        use."""
        if self.graphs is not None:
            return True
        if not self.use_graph:
            return False
        try:
            graphs = DecodeGraphs(
                self.model, self.kv, self.policy, self.max_batch,
                self.max_seq_len, self.MAX_RUN,
                ladder_rungs(self.max_batch, DECODE_LADDER))
            graphs.capture(sampled=False)
            self.graphs = graphs
            return True
        except Exception:
            # capture failed (e.g. an op that refuses stream capture on
            # this stack): permanent eager fallback, correctness first
            self.use_graph = False
            self.graphs = None
            torch.cuda.synchronize()
            return False

    def _decode_run_eager(self, batch: list[Sequence], run: int) -> None:
        """Eager fallback for a graph run (capture unavailable)."""
        for _ in range(run):
            live = [s for s in batch if not s.done]
            if not live:
                break
            for s in live:
                self.kv.extend(s.seq_id, len(s.prompt) + len(s.out_tokens))
            self._decode_step_eager(live)

    def _decode_step_eager(self, batch: list[Sequence]) -> None:
        dev = self.model.device
        tokens = torch.tensor([s.out_tokens[-1] for s in batch],
                              dtype=torch.int64, device=dev)
        positions = torch.tensor(
            [len(s.prompt) + len(s.out_tokens) - 1 for s in batch],
            dtype=torch.int32, device=dev)
        seq_ids = [s.seq_id for s in batch]
        bt = self.kv.block_table(seq_ids)
        sl = self.kv.seq_lens_tensor(seq_ids)
        logits = self.model.forward_decode(tokens, self.kv, bt, sl,
                                           positions)
        own = [i for i, s in enumerate(batch) if s.sampling is not None]
        if not own:
            nxt = self.policy.sample(logits).tolist()
        else:
            # rows that have `sampling` draw their own tokens, at the
            # position of the token being drawn; the rest as ever
            nxt = [0] * len(batch)
            rest = [i for i, s in enumerate(batch) if s.sampling is None]
            if rest:
                for i, t in zip(
                        rest, self.policy.sample(logits[rest]).tolist()):
                    nxt[i] = t
            toks = self._sample_rows(
                logits[own], [batch[i] for i in own],
                [len(batch[i].prompt) + len(batch[i].out_tokens)
                 for i in own])
            for i, t in zip(own, toks):
                nxt[i] = t
        for s, tok in zip(batch, nxt):
            if s.script:
                # grammar-forced continuation (script index: out_tokens[0]
                # was the decision token)
                si = len(s.out_tokens) - 1
                if si < len(s.script):
                    tok = s.script[si]
            s.out_tokens.append(int(tok))
            self._maybe_finish(s)
        self._count_decode(
            len(batch), 1,
            "sampled" if any(s.sampled for s in batch) else "greedy")

    def _decode_run_graph(self, batch: list[Sequence], run: int) -> None:
        """Run `run` decode steps for `batch` with zero host round trips:
        pages are pre-extended, the graph self-feeds, one sync at the end.
        A run with a live row at a temperature of its own above 0 replays
        the second ladder; every other run replays the first, whose greedy
        token is also what a row with SamplingParams at temperature 0
        draws.  (Under an engine-wide temperature above 0 the first
        ladder's policy is not greedy, so runs with `sampling` rows go
        eager there.)"""
        if not self._ensure_graphs():
            self._decode_run_eager(batch, run)
            return
        graphs = self.graphs
        sampled = any(s.sampled for s in batch)
        if sampled and not graphs.sampled and not graphs.sampled_failed:
            graphs.capture(sampled=True)
        if (sampled and not graphs.sampled) or (
                self.policy.temperature > 0.0
                and any(s.sampling is not None for s in batch)):
            self._decode_run_eager(batch, run)
            return
        hist, rung, dt = graphs.run(batch, run, sampled)
        self.stats.decode_s += dt
        for s, toks in zip(batch, hist):
            new = [int(t) for t in toks]
            if self.eos_id is not None and self.eos_id in new:
                # honor mid-run EOS: keep tokens up to and including it
                new = new[: new.index(self.eos_id) + 1]
            s.out_tokens.extend(new)
            self.kv.set_len(s.seq_id, len(s.prompt) + len(s.out_tokens))
            self._maybe_finish(s)
        self._count_decode(len(batch), run,
                           "sampled" if sampled else "greedy", rung)

    def _count_decode(self, live: int, steps: int, sampler: str,
                      rung: int | None = None) -> None:
        """Stats of `steps` decode steps with `live` rows (rung: the graph
        rung that ran them, None for eager steps)."""
        st = self.stats
        st.decode_tokens += live * steps
        st.decode_steps += steps
        st.decode_steps_by_live[live] = \
            st.decode_steps_by_live.get(live, 0) + steps
        st.decode_steps_by_sampler[sampler] += steps
        if rung is not None:
            st.decode_steps_by_rung[rung] = \
                st.decode_steps_by_rung.get(rung, 0) + steps

    # ------------------------------------------------------------------
    def submit(self, prompt_tokens: list[int], max_new_tokens: int,
               continue_from: Sequence | None = None,
               keep_alive: bool = False, constraint=None,
               sampling: SamplingParams | None = None) -> Sequence:
        """Queue a prompt.  continue_from: a completed keep-alive sequence
        whose prompt is a prefix of this one — its KV prefix is reused.
        constraint: models.grammar.CompiledGrammar for this turn.
        sampling: this request's own SamplingParams (None: the engine-wide
        policy); an open seed is drawn from the engine's seed generator and
        the seed in use is kept on the sequence."""
        prompt = list(prompt_tokens[: self.max_seq_len - 1])
        seed = None
        if sampling is not None:
            seed = sampling.seed if sampling.seed is not None \
                else self._seed_rng.getrandbits(64)
        decision_allowed = branches = None
        if constraint is not None:
            decision_allowed = list(constraint.decision_allowed)
            branches = dict(constraint.branches)
            # a forced tool-call script must fit in the turn
            max_new_tokens = max(max_new_tokens,
                                 constraint.max_script_len() + 1)
            max_new_tokens = min(max_new_tokens, self.MAX_RUN)
        # prompt + decode must fit the sequence budget (KV pages AND the
        # model's rope table)
        max_new_tokens = max(1, min(max_new_tokens,
                                    self.max_seq_len - len(prompt)))
        if continue_from is not None and not continue_from.keep_alive:
            continue_from = None
        if continue_from is not None:
            # at least one token must prefill (last-position logits)
            shared = min(len(continue_from.prompt), len(prompt) - 1)
            # shared prefix = the previous turn's prompt (its decode-token KV
            # is rolled back); bail to fresh prefill on any mismatch
            if prompt[:shared] != continue_from.prompt[:shared]:
                shared = 0
            if shared > 0:
                seq = Sequence(continue_from.seq_id, prompt, max_new_tokens,
                               cached_len=shared, keep_alive=keep_alive,
                               decision_allowed=decision_allowed,
                               branches=branches, sampling=sampling,
                               seed=seed)
                self.kv.truncate(seq.seq_id, shared)
                self._next_id = max(self._next_id, seq.seq_id + 1)
                self.pending.append(seq)
                return seq
            self.kv.free(continue_from.seq_id)
        seq = Sequence(self._next_id, prompt, max_new_tokens,
                       keep_alive=keep_alive,
                       decision_allowed=decision_allowed, branches=branches,
                       sampling=sampling, seed=seed)
        self._next_id += 1
        self.pending.append(seq)
        return seq

    def release(self, seq: Sequence) -> None:
        """Free a keep-alive conversation's KV."""
        if seq.keep_alive:
            seq.keep_alive = False
            self.kv.free(seq.seq_id)

    # ------------------------------------------------------------------
    def _admit(self) -> None:
        # group like-sized prefills: padded-batch attention pads every
        # admitted sequence to the batch max delta, so sort pending by
        # (has-cached-prefix, delta desc) — fresh long prompts batch with
        # each other, short continuation deltas (large ctx, tiny delta)
        # batch together, minimizing both pad waste and KV-gather width
        self.pending.sort(
            key=lambda s: (s.cached_len > 0,
                           -(len(s.prompt) - s.cached_len)))
        batch_items: list[tuple[torch.Tensor, int, int]] = []
        admitted: list[Sequence] = []
        new_tokens = 0
        while self.pending and len(self.running) + len(admitted) < self.max_batch:
            seq = self.pending[0]
            total = len(seq.prompt) + seq.max_new_tokens
            have = len(self.kv.pages(seq.seq_id)) if seq.cached_len else 0
            need = self.kv.pages_for(total) - have
            if need > self.kv.free_pages:
                break
            delta = len(seq.prompt) - seq.cached_len
            if batch_items and new_tokens + delta > self.prefill_batch_tokens:
                break
            self.pending.pop(0)
            if seq.cached_len:
                self.kv.extend(seq.seq_id, len(seq.prompt))
            else:
                self.kv.allocate(seq.seq_id, len(seq.prompt))
            toks = torch.tensor(seq.prompt[seq.cached_len:],
                                dtype=torch.int64, device=self.model.device)
            batch_items.append((toks, seq.seq_id, seq.cached_len))
            admitted.append(seq)
            new_tokens += delta
            self.stats.prefill_tokens += delta
            self.stats.cached_prefix_tokens += seq.cached_len
            self.stats.prefills += 1
        if not admitted:
            return
        if _TIMING:
            torch.cuda.synchronize()
            _t0 = time.perf_counter()
        logits = self.model.forward_prefill_batch(batch_items, self.kv)
        if _TIMING:
            torch.cuda.synchronize()
            self.stats.prefill_s += time.perf_counter() - _t0
        first = self._sample_first(logits, admitted)
        self.stats.prefill_batches += 1
        for seq, tok in zip(admitted, first):
            seq.out_tokens.append(int(tok))
            if seq.branches is not None:
                seq.script = seq.branches.get(int(tok))
                if seq.script is not None and self.jump_forward:
                    # jump-forward decoding (the SGLang fast-forward on
                    # grammar-forced segments): once the sampled decision
                    # commits to a tool branch, EVERY remaining token of
                    # the turn is grammar-forced — no model choice is
                    # left, and the forced tokens' KV is never reused
                    # (the next turn's prompt carries the OBSERVATION,
                    # not the raw call text, and retire rolls the cache
                    # back to the prompt) — so the engine emits the
                    # script directly instead of serial decode steps.
                    room = seq.max_new_tokens - 1
                    seq.out_tokens.extend(seq.script[:room])
                    self.stats.jump_forward_tokens += min(
                        len(seq.script), room)
            self.running.append(seq)
            self._maybe_finish(seq)

    def _maybe_finish(self, seq: Sequence) -> None:
        if len(seq.out_tokens) >= seq.max_new_tokens or (
                self.eos_id is not None and seq.out_tokens
                and seq.out_tokens[-1] == self.eos_id):
            seq.done = True

    def _retire(self) -> None:
        done = [s for s in self.running if s.done]
        for s in done:
            if not s.keep_alive:
                self.kv.free(s.seq_id)
            else:
                # roll back to the prompt: the next turn extends the prompt,
                # not the decoded tokens
                self.kv.truncate(s.seq_id, len(s.prompt))
        self.finished.extend(done)
        self.running = [s for s in self.running if not s.done]

    def _admit_all(self) -> None:
        """Admit (possibly several prefill batches) until the pending queue
        stops shrinking."""
        while self.pending:
            before = len(self.pending)
            self._admit()
            if len(self.pending) == before:
                break

    def run_chunk(self, max_run: int = 16) -> int:
        """One continuous-batching slice: admit whatever fits, then up
        to `max_run` decode steps (one graph run).  Returns remaining
        work count.  The event-driven scheduler
        (agents/schedule.py run_episodes_continuous) interleaves these
        slices with tool I/O completions, so late turns join the running
        batch instead of waiting for a global round barrier."""
        # NOTE: an overlapped variant (admissions on a side HIP stream
        # while the decode graph replays) was measured to hang
        # NON-deterministically at bench scale — the prefill's H2D /
        # allocator traffic races the replaying graph's memory pool on
        # this stack — so admissions and decode run sequentially.
        self._admit_all()
        batch = [s for s in self.running if not s.done]
        if batch:
            run = min(min(s.max_new_tokens - len(s.out_tokens)
                          for s in batch), max_run, self.MAX_RUN)
            if run > 0:
                if self.use_graph:
                    self._decode_run_graph(batch, run)
                else:
                    self._decode_run_eager(batch, run)
        self._retire()
        if self.pending and not self.running and not batch:
            raise _stalled()
        return len(self.running) + len(self.pending)

    def step(self) -> int:
        """Admit + one decode step; returns remaining work count."""
        self._admit()
        batch = [s for s in self.running if not s.done]
        if not batch:
            self._retire()
            return len(self.running) + len(self.pending)
        for s in batch:
            self.kv.extend(s.seq_id, len(s.prompt) + len(s.out_tokens))
        if self.use_graph:
            # one-step graph run (appends + finishes internally; falls
            # back to eager if capture is unavailable)
            self._decode_run_graph(batch, 1)
        else:
            self._decode_step_eager(batch)
        self._retire()
        return len(self.running) + len(self.pending)

    def run_to_completion(self) -> None:
        self.finished.clear()   # batch callers don't drain it
        t0 = time.perf_counter()
        if self.use_graph:
            while self.pending or self.running:
                before = len(self.pending)
                # drain the whole pending queue (possibly several prefill
                # batches) before decoding: decode runs want the full batch
                self._admit_all()
                batch = [s for s in self.running if not s.done]
                if not batch:
                    self._retire()
                    if self.pending and len(self.pending) == before and \
                            not self.running:
                        raise _stalled()
                    continue
                run = min(min(s.max_new_tokens - len(s.out_tokens)
                              for s in batch), self.MAX_RUN)
                if run > 0:
                    self._decode_run_graph(batch, run)
                self._retire()
        else:
            while self.pending or self.running:
                n_pending = len(self.pending)
                remaining = self.step()
                if remaining and not self.running and \
                        len(self.pending) == n_pending:
                    raise _stalled()
        if torch.cuda.is_available():
            torch.cuda.synchronize()
        self.stats.wall_s += time.perf_counter() - t0

    def generate_batch(self, prompts: list[list[int]],
                       max_new_tokens: list[int],
                       sampling=None) -> list[list[int]]:
        """sampling: one SamplingParams for every prompt, or a list with
        one entry (or None) per prompt."""
        per = _per_prompt(sampling, len(prompts))
        seqs = [self.submit(p, m, sampling=sp)
                for p, m, sp in zip(prompts, max_new_tokens, per)]
        self.run_to_completion()
        return [s.out_tokens for s in seqs]


def _stalled() -> MemoryError:
    return MemoryError("decode stalled: pending prompts cannot be "
                       "admitted (KV pages exhausted?)")


def _per_prompt(sampling, n: int) -> list:
    """One SamplingParams (or None) per prompt from one value or a list."""
    if isinstance(sampling, (list, tuple)):
        if len(sampling) != n:
            raise ValueError(f"{len(sampling)} sampling entries for {n} "
                             "prompts")
        return list(sampling)
    return [sampling] * n


class EngineLLM:
    """llm_batch adapter for the lab pipelines: text in, text out.

    When the scheduler passes conversation ids (agents/schedule.py), each
    conversation keeps its engine sequence alive between turns and only the
    prompt delta is prefassed (KV prefix reuse).  Per-turn TurnGrammar
    specs (models/grammar.py) are compiled against the tokenizer and
    passed into the engine as decision masks + forced scripts."""

    def __init__(self, engine: Engine, tokenizer=None):
        if tokenizer is None:
            from .tokenizer import default_tokenizer
            tokenizer = default_tokenizer(engine.model.cfg.vocab_size)
        self.engine = engine
        self.tokenizer = tokenizer
        self._convs: dict = {}
        self._by_seq: dict = {}

    def __call__(self, prompts: list[str], max_new_tokens: list[int],
                 conv_ids: list | None = None,
                 grammars: list | None = None,
                 sampling=None) -> list[str]:
        """sampling: one SamplingParams for every prompt, or a list with
        one entry (or None) per prompt."""
        from .grammar import compile_grammar
        per = _per_prompt(sampling, len(prompts))
        seqs = []
        for i, (p, m) in enumerate(zip(prompts, max_new_tokens)):
            conv = conv_ids[i] if conv_ids is not None else None
            prev = self._convs.get(conv) if conv is not None else None
            g = grammars[i] if grammars is not None else None
            constraint = compile_grammar(g, self.tokenizer) \
                if g is not None else None
            enc = self.tokenizer.encode(p)
            seq = self.engine.submit(enc, m, continue_from=prev,
                                     keep_alive=conv is not None,
                                     constraint=constraint,
                                     sampling=per[i])
            if conv is not None:
                self._convs[conv] = seq
            seqs.append(seq)
        self.engine.run_to_completion()
        return [self.tokenizer.decode(s.out_tokens) for s in seqs]

    # ---- event-driven (continuous) scheduling interface ----------------
    def submit_turn(self, conv_id, prompt: str, max_new_tokens: int,
                    grammar=None, sampling=None) -> None:
        """Queue one agent turn WITHOUT running the engine — the
        continuous scheduler (agents/schedule.py) interleaves engine
        slices with tool I/O so turns join the running batch as they
        become ready."""
        from .grammar import compile_grammar
        constraint = compile_grammar(grammar, self.tokenizer)             if grammar is not None else None
        prev = self._convs.get(conv_id)
        enc = self.tokenizer.encode(prompt)
        seq = self.engine.submit(enc, max_new_tokens, continue_from=prev,
                                 keep_alive=True, constraint=constraint,
                                 sampling=sampling)
        self._convs[conv_id] = seq
        self._by_seq[id(seq)] = conv_id

    def pop_finished(self) -> list[tuple]:
        """Drain (conv_id, decoded text) for turns completed since the
        last call (engine.finished is filled by retire)."""
        out = []
        for seq in self.engine.finished:
            cid = self._by_seq.pop(id(seq), None)
            if cid is not None:
                out.append((cid, self.tokenizer.decode(seq.out_tokens)))
        self.engine.finished.clear()
        return out

    def release(self, conv_id) -> None:
        seq = self._convs.pop(conv_id, None)
        if seq is not None:
            self._by_seq.pop(id(seq), None)
            self.engine.release(seq)

    def release_all(self) -> None:
        for conv in list(self._convs):
            self.release(conv)
