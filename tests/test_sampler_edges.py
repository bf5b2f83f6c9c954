"""Steered read-out and edge cases of the two sampler kernels
(qsa_greedy_sample_kernel, ops/hip/elementwise.hip, and qsa_sample_kernel,
ops/hip/sampling.hip): case tables, builders, an independent reference, the
expectations and a mutant test.  This file runs everything through the CPU
branches of ops/dispatch.py; test_gpu_sampler_edges.py imports the tables
and makes the same assertions through the kernels.  Every comparison is
exact.

The reference (ref_kept / ref_draw / ref_row) is the sampling rule in plain
Python integers, with numpy.float32 scalars for the weight's f32 sequence,
each operation rounded on its own.  It calls nothing from ops/dispatch.py:
candidates in index order, the key from the bf16 bit pattern, the weight,
top-k and top-p by sorting, need, Philox4x32-10, target = (r * total) >> 64
and the running sum.  It is pinned by the Philox known answers and by
w = 2^40 at the maximum, w == 1 at y = -40 and w == 0 at y = -41.

Steering devices (none needs a tolerance):
  one-hot       one candidate at 0.0, every other candidate -inf: the token
                is that index for any seed and position.
  tie set       n candidates hold one value, the rest are -inf: the token is
                the floor(r * n / 2^64)-th of them in index order, r from the
                reference's Philox.  (total = n * 2^40 and target =
                floor(r * n * 2^40 / 2^64); the running sum (j + 1) * 2^40
                first exceeds it at j = floor(target / 2^40) =
                floor(r * n / 2^64).)  Positions are chosen, by search with
                that Philox, so that a given row draws a given slot.
  exact weights with inv_temp = 0x1.62e430p-1, fl(inv_temp * LOG2E) == 1 and
                a logit m - j has y == -j and weight 2^40 >> j for the
                integers j <= 41 other than 13, 15, 26, 27, 30, 31 (where
                the second product rounds off the integer), so kept sets
                built from j in 0..3 have hand-countable masses.
  unit weights  the maximum first and every other candidate at m - 40
                (weight 1): once target >= 2^40 every integer is a running
                sum, so the token is lo + target - 2^40 + 1 and a `>=` for
                `>` in the running-sum comparison moves it by one.  The
                (seed, pos) pairs that land there (one draw in 2^23) were
                found by search and are checked here.
Every case places traps: logits of +30 at indices outside the candidate
set (below lo, at hi and above, next to an outside eos).  A trap is never a
token.

The slot classes follow the kernels' index arithmetic (layout()): with
mis = the 16-byte phase of the row's first window element, the window is a
scalar head of (8 - mis) & 7 candidates, a uint4 body in chunks of 2048 and
a scalar tail of up to 7; an eos outside the window goes before the head or
after the tail.  The sampled kernel's final pass calls these `steps`: step
0 = {eos below, head}, steps 1.. = the body chunks, the last step = {tail,
eos above}; thread t of its step scan holds steps 8t .. 8t + 7, so steps 8,
512 and 1024 are the first of thread 1, of wave 1 and of wave 2.  The
16.5 K window here has 9 body chunks (nstep 11), so that steps 7, 8 and 9
all exist next to a tail step."""

import functools
import math
import struct
import types

import numpy as np
import pytest
import torch

from quickstart_streaming_agents_amd.ops import dispatch as D

OFF = 65536
NINF = float("-inf")
PINF = float("inf")
TRAP = 30.0
EX = float.fromhex("0x1.62e430p-1")         # the exact-weight inv_temp
SEED = 0x1234ABCD9E3779B9                    # distinct key words
VMAX = 2046 * 2048
M64 = (1 << 64) - 1
M32 = 0xffffffff

F = np.float32
# the j <= 41 at which the exact-weight device holds (y == -j exactly)
EXACT_J = [j for j in range(42) if j not in (13, 15, 26, 27, 30, 31)]


# ---- the independent reference ------------------------------------------------

_LOG2E = F(math.log2(math.e))
_C = [F(math.log(2.0) ** k / math.factorial(k)) for k in range(7)]

LAYOUT_MUTS = ("tail_dropped", "last_chunk_dropped")
MUTANTS = LAYOUT_MUTS + (
    "outside_eos_dropped", "greedy_highest_tie", "topk_gt", "topk_cut_ties",
    "topp_gt", "need_full_total", "running_ge", "key_words_swapped",
    "pos_in_word_1", "target_low_64", "trap_admitted")
GREEDY_MUTANTS = LAYOUT_MUTS + ("outside_eos_dropped", "greedy_highest_tie",
                                "trap_admitted")


def bf16_value(bits):
    return struct.unpack("<f", struct.pack("<I", (bits & 0xffff) << 16))[0]


def ref_key(bits):
    return (~bits & 0xffff) if bits & 0x8000 else (bits | 0x8000)


def ref_weight(bits, m, inv_temp):
    """The rule's 40-bit fixed-point weight; m, inv_temp: python floats
    holding f32 values."""
    with np.errstate(all="ignore"):
        d = F(F(bf16_value(bits)) - F(m))
        x = F(d * F(inv_temp))
        y = F(x * _LOG2E)
        if not y >= F(-64.0):
            y = F(-64.0)
        n = F(np.floor(F(y + F(0.5))))
        f = F(y - n)
        p = _C[6]
        for k in range(5, -1, -1):
            p = F(p * f)
            p = F(p + _C[k])
        q = int(F(p * F(16777216.0)))
    sh = -int(n)
    return ((q << 16) >> sh) if sh <= 40 else 0


def ref_philox(counter, key):
    c0, c1, c2, c3 = counter
    k0, k1 = key
    for _ in range(10):
        p0 = 0xD2511F53 * c0
        p1 = 0xCD9E8D57 * c2
        c0, c1, c2, c3 = ((p1 >> 32) ^ c1 ^ k0, p1 & M32,
                          (p0 >> 32) ^ c3 ^ k1, p0 & M32)
        k0 = (k0 + 0x9E3779B9) & M32
        k1 = (k1 + 0xBB67AE85) & M32
    return c0, c1, c2, c3


def ref_r(seed, pos, mut=None):
    """The 64-bit draw of (seed, pos)."""
    seed &= M64
    key = (seed & M32, seed >> 32)
    if mut == "key_words_swapped":
        key = key[::-1]
    ctr = (pos & M32, 0, 0, 0)
    if mut == "pos_in_word_1":
        ctr = (0, pos & M32, 0, 0)
    x = ref_philox(ctr, key)
    return x[0] | (x[1] << 32)


def layout(base, lo, hi):
    """The kernels' split of the window of a row that starts `base`
    elements after a 16-byte boundary."""
    mis = (base + lo) & 7
    body0 = min(hi, lo + ((8 - mis) & 7))
    body1 = body0 + ((hi - body0) & ~7)
    nchunk = (body1 - body0 + 2047) // 2048
    return types.SimpleNamespace(mis=mis, body0=body0, body1=body1,
                                 nchunk=nchunk, nstep=nchunk + 2,
                                 head=body0 - lo, tail=hi - body1)


def ref_kept(bits, lo, hi, eos, inv_temp, top_k, top_p_q, base=0, mut=None):
    """Everything of the rule before the draw, for one row given as a list
    of bf16 bit patterns."""
    V = len(bits)
    cand = list(range(lo, hi))
    if mut in LAYOUT_MUTS:
        g = layout(base, lo, hi)
        if mut == "tail_dropped":
            cand = list(range(lo, g.body1))
        elif g.nchunk:
            cut = g.body0 + (g.nchunk - 1) * 2048
            cand = list(range(lo, cut)) + list(range(g.body1, hi))
    if mut == "trap_admitted" and hi < V and hi != eos:
        cand.append(hi)
    if eos >= 0 and not lo <= eos < hi and mut != "outside_eos_dropped":
        if eos < lo:
            cand.insert(0, eos)
        else:
            cand.append(eos)
    out = types.SimpleNamespace(cand=cand, greedy=0, sampled=False,
                                kept=set(), total=0, bk=None, bp=None,
                                items=[])
    if not cand:
        return out
    cb = [bits[i] for i in cand]
    val = {b: bf16_value(b) for b in set(cb)}
    m = max(val.values())
    if m == NINF:
        return out
    tied = [i for i, b in zip(cand, cb) if val[b] == m]
    out.greedy = tied[-1] if mut == "greedy_highest_tie" else tied[0]
    if inv_temp == 0 or m == PINF:
        return out
    out.sampled = True
    C = len(cand)
    wt = {b: ref_weight(b, m, inv_temp) for b in val}
    kt = {b: ref_key(b) for b in val}
    keys = [kt[b] for b in cb]
    ws = [wt[b] for b in cb]
    tau_k = 0
    keep = [True] * C
    if top_k > 0:
        tau_k = sorted(keys, reverse=True)[min(top_k, C) - 1]
        if mut == "topk_gt":
            keep = [k > tau_k for k in keys]
        elif mut == "topk_cut_ties":
            order = sorted(range(C), key=lambda j: (-keys[j], j))[:top_k]
            keep = [False] * C
            for j in order:
                keep[j] = True
        else:
            keep = [k >= tau_k for k in keys]
    total_k = sum(w for w, kp in zip(ws, keep) if kp)
    if mut == "need_full_total":
        total_k = sum(ws)
    need = max(1, (total_k * top_p_q) >> 16)
    mass = {}
    for k, w in zip(keys, ws):
        mass[k] = mass.get(k, 0) + w
    tau_p, cum = 0, 0
    for k in sorted(mass, reverse=True):
        cum += mass[k]
        if cum > need or (cum == need and mut != "topp_gt"):
            tau_p = k
            break
    keep = [kp and k >= tau_p for kp, k in zip(keep, keys)]
    out.kept = {i for i, kp, w in zip(cand, keep, ws) if kp and w}
    out.total = sum(w for w, kp in zip(ws, keep) if kp)
    out.bk = tau_k >> 8 if 0 < top_k < C else None
    out.bp = tau_p >> 8 if top_p_q < OFF else None
    # the kept candidates in index order; a weightless one can only matter
    # as the very first
    first = True
    for i, kp, w in zip(cand, keep, ws):
        if kp and (w or first):
            out.items.append((i, w))
        first = first and not kp
    return out


def ref_draw(kp, seed, pos, mut=None):
    if not kp.sampled:
        return kp.greedy
    prod = ref_r(seed, pos, mut) * kp.total
    target = prod & M64 if mut == "target_low_64" else prod >> 64
    run = 0
    for i, w in kp.items:
        run += w
        if run > target or (mut == "running_ge" and run >= target):
            return i
    return kp.greedy


def ref_row(bits, lo, hi, eos, inv_temp, top_k, top_p_q, seed, pos, base=0,
            mut=None):
    """The sampling rule for one row: token, kept set (the candidates of
    non-zero weight that can be drawn), total, and the high-byte bins of
    the two thresholds (None where the threshold is off)."""
    kp = ref_kept(bits, lo, hi, eos, inv_temp, top_k, top_p_q, base, mut)
    return types.SimpleNamespace(token=ref_draw(kp, seed, pos, mut),
                                 kept=kp.kept, total=kp.total, bk=kp.bk,
                                 bp=kp.bp, greedy=kp.greedy)


def pos_for(n, j, seed=SEED, start=0):
    """The first position >= start at which a tie set of n draws slot j."""
    pos = start
    while (ref_r(seed, pos) * n) >> 64 != j:
        pos += 1
    return pos


# ---- cases ----------------------------------------------------------------------

def f32(x):
    return float(F(x))


def new_case(name, V, lo, hi, eos, B, inv_temp=1.0, top_k=0, top_p_q=OFF):
    """B rows of -inf with the traps planted; per-row parameter lists;
    want / want_greedy are filled by the builders (None: from the
    reference)."""
    c = types.SimpleNamespace(
        name=name, V=V, lo=lo, hi=hi, eos=eos, B=B,
        logits=torch.full((B, V), NINF, dtype=torch.bfloat16),
        inv=[f32(inv_temp)] * B, k=[top_k] * B, pq=[top_p_q] * B,
        seed=[SEED] * B, pos=list(range(B)), want=[None] * B,
        want_greedy=[None] * B, cpu_rows=None, shared=False, cls=[None] * B,
        classes=set())
    cands = set(range(lo, hi)) | ({eos} if eos >= 0 else set())
    near = {eos - 1, eos + 1} if eos >= 0 else set()
    c.traps = sorted(i for i in {0, lo - 1, hi, hi + 1, V - 1} | near
                     if 0 <= i < V and i not in cands)
    for i in c.traps:
        c.logits[:, i] = TRAP
    return c


def row_bits(c, b):
    return (c.logits[b].view(torch.int16).to(torch.int32) & 0xffff).tolist()


def set_one_hot(c, b, idx):
    c.logits[b, idx] = 0.0
    c.want[b] = c.want_greedy[b] = idx


def set_ties(c, b, idxs, slot=None, start=0, value=0.0):
    """Plants the tie set; slot: the one this row shall draw (its position
    is then found by search from `start`), else the row keeps its
    position."""
    idxs = sorted(idxs)
    for i in idxs:
        c.logits[b, i] = value
    if slot is not None:
        c.pos[b] = pos_for(len(idxs), slot, c.seed[b], start)
    c.want[b] = idxs[(ref_r(c.seed[b], c.pos[b]) * len(idxs)) >> 64]
    c.want_greedy[b] = idxs[0]


def slot_index(c, b, slot):
    """Index of a slot class in row b, None where the row has no such
    slot.  ("eos",), ("head", p), ("body", offset | "last"),
    ("step", s, offset | "last"), ("tail", p)."""
    g = layout(b * c.V, c.lo, c.hi)
    if slot[0] == "eos":
        return c.eos if c.eos >= 0 else None
    if slot[0] == "head":
        return c.lo + slot[1] if slot[1] < g.head else None
    if slot[0] == "tail":
        return g.body1 + slot[1] if slot[1] < g.tail else None
    start = g.body0 + ((slot[1] - 1) * 2048 if slot[0] == "step" else 0)
    off = slot[-1]
    if off == "last":
        return g.body1 - 1 if g.body1 > start else None
    return start + off if start + off < g.body1 else None


def fill_from_ref(c):
    """want / want_greedy of the rows still open, from the reference."""
    memo = {}
    for b in range(c.B):
        if c.want[b] is not None and c.want_greedy[b] is not None:
            continue
        key = (0 if c.shared else b, c.inv[b], c.k[b], c.pq[b])
        if key not in memo:
            memo[key] = ref_kept(row_bits(c, b), c.lo, c.hi, c.eos, c.inv[b],
                                 c.k[b], c.pq[b])
        kp = memo[key]
        if c.want[b] is None:
            c.want[b] = ref_draw(kp, c.seed[b], c.pos[b])
        if c.want_greedy[b] is None:
            c.want_greedy[b] = kp.greedy
    return c


def ref_drawer(mut, greedy=False):
    """draw(c, rows) by the reference with one change."""
    def draw(c, rows):
        memo, out = {}, []
        for b in rows:
            inv = 0.0 if greedy else c.inv[b]
            phase = (b * c.V) & 7 if mut in LAYOUT_MUTS else 0
            key = (0 if c.shared else b, inv, c.k[b], c.pq[b], phase)
            if key not in memo:
                memo[key] = ref_kept(row_bits(c, b), c.lo, c.hi, c.eos, inv,
                                     c.k[b], c.pq[b], b * c.V, mut)
            out.append(ref_draw(memo[key], c.seed[b], c.pos[b], mut))
        return out
    return draw


# ---- 1. slots -------------------------------------------------------------------

SV, SLO, SHI = 4211, 9, 4099                  # window of 4090: two body chunks
SLOT_EOS = {"below": 3, "inside": 1000, "above": 4205, "absent": -1}
BODY_OFFSETS = (0, 7, 8, 2047, 2048, "last")
SLOT_SPECS = ([("eos",)] + [("head", p) for p in range(7)] +
              [("body", o) for o in BODY_OFFSETS] +
              [("tail", p) for p in range(7)])


@functools.lru_cache(maxsize=None)
def slot_one_hot_case(eos_kind, spec):
    """8 rows, one per 16-byte phase, hot at the slot (at body offset 0
    in a row that has no such slot)."""
    c = new_case(f"slots one-hot eos {eos_kind} {spec}", SV, SLO, SHI,
                 SLOT_EOS[eos_kind], 8)
    for b in range(8):
        idx = slot_index(c, b, spec)
        set_one_hot(c, b, slot_index(c, b, ("body", 0)) if idx is None
                    else idx)
        c.pos[b] = 1000 + b
    return c


@functools.lru_cache(maxsize=None)
def slot_tie_case(eos_kind):
    """64 rows, pos 0..63: ties over one slot of each class."""
    c = new_case(f"slots ties eos {eos_kind}", SV, SLO, SHI,
                 SLOT_EOS[eos_kind], 64)
    for b in range(64):
        g = layout(b * SV, SLO, SHI)
        specs = [("eos",), ("head", (b // 8) % max(g.head, 1)),
                 ("tail", (b // 8) % max(g.tail, 1))] + \
            [("body", o) for o in BODY_OFFSETS]
        where = {slot_index(c, b, s): s[0] + str(s[-1]) * (s[0] == "body")
                 for s in specs if slot_index(c, b, s) is not None}
        set_ties(c, b, list(where))
        c.cls[b] = where[c.want[b]]
        c.classes |= set(where.values())
    return c


@functools.lru_cache(maxsize=None)
def empty_window_case():
    """Rows 0..7: empty window, eos a candidate (the token is eos); the
    twin case without eos is empty_window_no_eos_case."""
    c = new_case("empty window with eos", SV, 100, 100, 50, 8)
    for b in range(8):
        set_one_hot(c, b, 50)
    return c


@functools.lru_cache(maxsize=None)
def empty_window_no_eos_case():
    c = new_case("empty window without eos", SV, 100, 100, -1, 8)
    c.traps = [i for i in c.traps if i != 0]
    c.logits[:, 0] = NINF
    c.want = [0] * 8
    c.want_greedy = [0] * 8
    return c


@functools.lru_cache(maxsize=None)
def all_neg_inf_case():
    """Candidates that are all -inf, eos among them: token 0."""
    c = new_case("all candidates -inf", SV, SLO, SHI, 4205, 8, top_k=3,
                 top_p_q=30000)
    c.traps = [i for i in c.traps if i != 0]
    c.logits[:, 0] = NINF
    c.want = [0] * 8
    c.want_greedy = [0] * 8
    return c


@functools.lru_cache(maxsize=None)
def no_body_case(n, hot):
    """A window of n in 1..7 candidates, so no row has a body; hot: the
    position of a one-hot, None: 64 rows of ties over all n and the eos
    above."""
    if hot is None:
        c = new_case(f"no body n={n} ties", SV, SLO, SLO + n, 4205, 64)
        for b in range(64):
            set_ties(c, b, list(range(SLO, SLO + n)) + [4205])
        return c
    c = new_case(f"no body n={n} hot {hot}", SV, SLO, SLO + n, 4205, 8)
    for b in range(8):
        set_one_hot(c, b, SLO + hot)
    return c


# ---- 2. step scan ---------------------------------------------------------------

def _scan_case(name, V, lo, hi, eos, specs):
    """8 rows of ties over the slots `specs`; the rows draw the slots in
    the order of `specs`, a row without the next one the one after."""
    c = new_case(name, V, lo, hi, eos, 8)
    left = list(specs)
    for b in range(8):
        here = [s for s in specs if slot_index(c, b, s) is not None]
        idxs = sorted(slot_index(c, b, s) for s in here)
        s = ([s for s in left if s in here] + here)[0]
        if s in left:
            left.remove(s)
        set_ties(c, b, idxs, slot=idxs.index(slot_index(c, b, s)))
    return c


def step_of(c, b, t):
    """The final pass's step that holds candidate t of row b."""
    g = layout(b * c.V, c.lo, c.hi)
    if t == c.eos and not c.lo <= t < c.hi:
        return "eos"
    return 0 if t < g.body0 else g.nstep - 1 if t >= g.body1 else \
        1 + (t - g.body0) // 2048


def _step_off(s):
    return (s * 37 + 5) % 90           # inside a partial last chunk too


@functools.lru_cache(maxsize=None)
def scan_16k_case():
    specs = [("step", s, _step_off(s)) for s in (1, 7, 8, 9)] + \
        [("eos",), ("tail", 0), ("head", 0)]
    return _scan_case("step scan 16.5K", 16501, 2, 16490, 16495, specs)


def scan_2m_case():
    specs = [("step", s, _step_off(s)) for s in (1, 511, 513, 512, 1023)] + \
        [("eos",), ("step", 1024, _step_off(1024)), ("tail", 0)]
    c = _scan_case("step scan 2.2M", 2200003, 3, 2199997, 1, specs)
    c.cpu_rows = [3, 6]                # draw in steps 512 and 1024
    return c


def scan_max_case(lo):
    """V = 2046 * 2048 (2048 steps, thread 255).  Rows: ties over steps 1,
    2046 and the tail drawing each in turn (0, 2, 3, 7), all-equal rows
    with top-p off (1) and at 32768 (6): the uniform draw
    cand[floor(r * C / 2^64)] with total about 2^62; one-hots in step 2046
    (4) and in the tail (5)."""
    V, hi, eos = VMAX, VMAX - 3, VMAX - 1
    c = new_case(f"step scan max lo={lo}", V, lo, hi, eos, 8)
    ties = [("step", 1, 11), ("step", 2046, "last"), ("tail", 2)]
    for b, slot in ((0, 1), (2, 2), (3, 0), (7, 1)):
        set_ties(c, b, [slot_index(c, b, s) for s in ties], slot=slot,
                 start=100 * b)
    for b, pq in ((1, OFF), (6, 32768)):
        c.logits[b, lo:hi] = 0.0
        c.logits[b, eos] = 0.0
        c.pq[b] = pq
        C = hi - lo + 1
        j = (ref_r(c.seed[b], c.pos[b]) * C) >> 64
        c.want[b] = lo + j if j < hi - lo else eos
        c.want_greedy[b] = lo
    set_one_hot(c, 4, slot_index(c, 4, ("step", 2046, 1999)))
    set_one_hot(c, 5, slot_index(c, 5, ("tail", 4)))
    g = layout(0, lo, hi)
    assert (g.nstep, g.nchunk, g.tail) == (2048, 2046, 5)
    c.cpu_rows = [0, 1] if lo == 0 else [5, 6]
    return c


# ---- 3, 4. top-k and top-p on exact weights --------------------------------------

KV, KLO, KHI, KEOS = 2219, 7, 2203, 2210      # two body chunks, eos above
NCAND = KHI - KLO + 1
# indices in the head or first octet, both chunks, the chunk seam, the tail
# and the eos
POOL = [7, 9, 15, 16, 500, 2054, 2055, 2063, 2100, 2195, 2200, 2202, 2210]


def _spread(values):
    """values -> {index: value}, the values dealt over POOL so that equal
    ones land far apart."""
    order = [0, 12, 4, 8, 2, 10, 6, 1, 11, 5, 9, 3, 7]
    return {POOL[order[i]]: v for i, v in enumerate(values)}


# m = 9: weights 8, 4, 4, 2, 2, 1, 1, 1 in units of 2^37, total 23; 9 and 8
# are in the high-byte bin of [8, 32), 7 and 6 in that of [2, 8)
LADDER = _spread([9, 8, 8, 7, 7, 6, 6, 6])
NEGS = _spread([-1, -2, -2, -3, -3, -4, -4])  # -1 alone in its bin
LADDER_IDX = {v: {i for i, x in LADDER.items() if x >= v} for v in (9, 8, 7, 6)}


def _kept_table():
    t = []

    def add(name, vals, k=0, pq=OFF, kept=None, it=EX):
        t.append(types.SimpleNamespace(name=name, vals=vals, k=k, pq=pq,
                                       kept=kept, it=it))
    L, at = LADDER, LADDER_IDX
    add("k=2 in the maximum's bin, cuts the ties at 8", L, k=2, kept=at[8])
    add("k=4 in a lower bin, k - above == 1", L, k=4, kept=at[7])
    add("k=8 in a lower bin, k - above == the bin", L, k=8, kept=at[6])
    add("k=7 cuts the ties at 6", L, k=7, kept=at[6])
    add("k=3 all negative", NEGS, k=3,
        kept={i for i, x in NEGS.items() if x >= -2})
    add("k=4 all negative, cuts the ties at -3", NEGS, k=4,
        kept={i for i, x in NEGS.items() if x >= -3})
    for k in (1, NCAND - 1, NCAND, NCAND + 1, 10 ** 6, 2 ** 31 - 1):
        add(f"k={k}", L, k=k, kept=at[9] if k == 1 else at[6])
    add("k=20 above the finite candidates", L, k=20, kept=at[6])
    tied = {16: 9, 2100: 9, 2210: 9, 7: 8, 500: 8, 2195: 8, 2202: 8}
    add("k=1 over tied maxima in three steps", tied, k=1,
        kept={16, 2100, 2210})
    zeros = {9: -0.0, 500: 0.0, 2100: -0.0, 2200: 0.0, 16: -1.0}
    add("k=1 keeps +0.0 and not -0.0", zeros, k=1, kept={500, 2200}, it=1.0)
    add("k=0 weighs +0.0 and -0.0 alike", zeros, kept=set(zeros), it=EX)
    three = {16: 0, 2063: -1, 2210: -1}
    add("p=32768 is the maximum's mass exactly", three, pq=32768, kept={16})
    add("p=32769 needs one more", three, pq=32769, kept=set(three))
    add("p=1", L, pq=1, kept=at[9])
    add("p=65535", L, pq=65535, kept=at[6])
    add("p=65536", L, pq=65536, kept=at[6])
    add("p=60000 in a lower bin, top-k off", L, pq=60000, kept=at[6])
    add("p=52000 stops at 7", L, pq=52000, kept=at[7])
    # top-k keeps 9, 8, 8 (16 units): need 8 is the 9 alone; from the full
    # total (23) it would be 11.5 and keep the 8s
    add("k=3 then p=32768: need from total_k", L, k=3, pq=32768, kept=at[9])
    # top-k keeps down to 7 (20 units), need 10 stops at 8: bp above bk
    add("k=5 then p=32768: bp above bk", L, k=5, pq=32768, kept=at[8])
    add("k=5 then p=65535: top-p in top-k's bin", L, k=5, pq=65535,
        kept=at[7])
    return t


KEPT_TABLE = _kept_table()


@functools.lru_cache(maxsize=None)
def kept_case(i):
    """64 rows of one logits row (V is odd: all eight phases), pos
    0..63."""
    s = KEPT_TABLE[i]
    c = new_case("kept: " + s.name, KV, KLO, KHI, KEOS, 64, inv_temp=s.it,
                 top_k=s.k, top_p_q=s.pq)
    for idx, v in s.vals.items():
        c.logits[:, idx] = v
    c.shared = True
    return fill_from_ref(c)


# ---- 5. weights -----------------------------------------------------------------

WEIGHT_SPECS = [("it=1", 1.0), ("it=exact", EX), ("it=2^-20", 2.0 ** -20),
                ("it=1e30", 1e30)]


@functools.lru_cache(maxsize=None)
def weight_case(i):
    """Logits -j, j = 0..50, the small j four times over; i == 4: a row at
    inv_temp 1 whose non-maximum candidates all have weight 0."""
    if i == 4:
        c = new_case("weights: all but the maxima weigh 0", KV, KLO, KHI,
                     KEOS, 64)
        for idx, v in {16: 0.0, 2100: 0.0, 9: -60.0, 500: -100.0,
                       2195: -28.125, 2210: -61.5}.items():
            c.logits[:, idx] = v
    else:
        name, it = WEIGHT_SPECS[i]
        c = new_case("weights: " + name, KV, KLO, KHI, KEOS, 64, inv_temp=it)
        for j in range(51):
            c.logits[:, 20 + 43 * j] = -float(j)
        for j in range(1, 5):
            for r in range(3):
                c.logits[:, 30 + 43 * j + 700 * r] = -float(j)
    c.shared = True
    return fill_from_ref(c)


# ---- unit weights: every integer a running sum ---------------------------------

UV, ULO, UHI = 131072, 8, 131064
# positions at which SEED's draw r has r * total >> 64 >= 2^40 (about one
# in 2^23), found by search; test_unit_weight_positions checks them
UNIT_POS = (1241553, 2417166)


def unit_weight_case():
    c = new_case("unit weights", UV, ULO, UHI, -1, len(UNIT_POS),
                 inv_temp=EX)
    c.logits[:, ULO:UHI] = -40.0
    c.logits[:, ULO] = 0.0
    c.pos = list(UNIT_POS)
    total = (1 << 40) + UHI - ULO - 1
    for b, pos in enumerate(UNIT_POS):
        target = (ref_r(SEED, pos) * total) >> 64
        c.want[b] = ULO + max(0, target - (1 << 40) + 1)
        c.want_greedy[b] = ULO
    c.shared = True
    c.total = total
    return c


# ---- +inf -----------------------------------------------------------------------

INF_SLOTS = [("head", 0), ("body", 2047), ("tail", 0), ("eos",)]
INF_PARAMS = [(0, OFF), (3, OFF), (0, 30000), (3, 30000)]


@functools.lru_cache(maxsize=None)
def inf_case(si, eos_kind):
    """32 rows: 8 phases x top-k / top-p on and off.  +inf at the slot (at
    body offset 8 in a row without it) and, unless the slot is the eos,
    again at the body's last element; finite logits at lower indices: the
    token is the lowest-index +inf."""
    c = new_case(f"+inf at {INF_SLOTS[si]} eos {eos_kind}", SV, SLO, SHI,
                 SLOT_EOS[eos_kind], 32)
    for b in range(32):
        c.k[b], c.pq[b] = INF_PARAMS[b // 8]
        c.logits[b, SLO] = c.logits[b, 2000] = 3.0
        idx = slot_index(c, b, INF_SLOTS[si])
        hot = [slot_index(c, b, ("body", 8)) if idx is None else idx]
        if INF_SLOTS[si] != ("eos",):
            hot.append(slot_index(c, b, ("body", "last")))
        for i in hot:
            c.logits[b, i] = PINF
        c.want[b] = c.want_greedy[b] = min(hot)
    return c


# ---- running the cases ------------------------------------------------------------

def params(c, rows, dev="cpu", greedy=False):
    inv = [0.0 if greedy else c.inv[b] for b in rows]
    seed = [c.seed[b] - (1 << 64) if c.seed[b] >> 63 else c.seed[b]
            for b in rows]
    return (torch.tensor(inv, dtype=torch.float64).float().to(dev),
            torch.tensor([c.k[b] for b in rows], dtype=torch.int32).to(dev),
            torch.tensor([c.pq[b] for b in rows], dtype=torch.int32).to(dev),
            torch.tensor(seed, dtype=torch.int64).to(dev),
            torch.tensor([c.pos[b] - (1 << 32) if c.pos[b] >> 31
                          else c.pos[b] for b in rows],
                         dtype=torch.int32).to(dev))


def _logits(c, rows, dev):
    """All rows on a device (the phases are the table's); the chosen rows
    on the CPU, whose branch knows no phase."""
    t = c.logits if list(rows) == list(range(c.B)) else \
        c.logits[torch.tensor(rows)]
    t = t.to(dev)
    assert t.data_ptr() % 16 == 0       # layout() counts phases from here
    return t


def _books(n, dev, ctr=0):
    return dict(script=torch.zeros(n, 1, dtype=torch.int64, device=dev),
                mask=torch.zeros(n, 1, dtype=torch.bool, device=dev),
                ctr=torch.tensor([ctr], dtype=torch.int64, device=dev),
                hist=torch.full((1, n), -7, dtype=torch.int64, device=dev),
                tokens=torch.full((n,), -7, dtype=torch.int64, device=dev),
                ticket=None if dev == "cpu" else
                torch.zeros(1, dtype=torch.int32, device=dev))


def _after_step(bk, toks):
    assert bk["hist"][0].tolist() == toks
    assert int(bk["ctr"][0]) == 1
    if bk["ticket"] is not None:
        assert int(bk["ticket"][0]) == 0
    return toks


def draw_tokens(dev, greedy=False):
    def draw(c, rows):
        return D.sample_tokens(_logits(c, rows, dev), c.lo, c.hi, c.eos,
                               *params(c, rows, dev, greedy)).tolist()
    return draw


def draw_step(dev, greedy=False):
    def draw(c, rows):
        bk = _books(len(rows), dev)
        D.sample_step(_logits(c, rows, dev), c.lo, c.hi, c.eos,
                      *params(c, rows, dev, greedy), bk["script"],
                      bk["mask"], bk["ctr"], bk["hist"], bk["tokens"],
                      bk["ticket"])
        return _after_step(bk, bk["tokens"].tolist())
    return draw


def draw_greedy(dev):
    def draw(c, rows):
        bk = _books(len(rows), dev)
        D.greedy_sample_step(_logits(c, rows, dev), c.lo, c.hi, c.eos,
                             bk["script"], bk["mask"], bk["ctr"], bk["hist"],
                             bk["tokens"], bk["ticket"])
        return _after_step(bk, bk["tokens"].tolist())
    return draw


def _check(c, draw, want, rows, what):
    rows = list(range(c.B)) if rows is None else rows
    got = draw(c, rows)
    for b, t in zip(rows, got):
        assert t not in c.traps, f"{c.name}: {what} row {b} returned trap {t}"
        assert t == want[b], \
            f"{c.name}: {what} row {b} (phase {(b * c.V + c.lo) & 7}, " \
            f"pos {c.pos[b]}): token {t}, want {want[b]}"


def check_sampled(c, draw, rows=None):
    _check(c, draw, c.want, rows, "sampled")


def check_greedy(c, draw, rows=None):
    _check(c, draw, c.want_greedy, rows, "greedy")


def check_case(c, dev, all_rows=False):
    """Both kernels' ops on one case: sample_tokens, sample_step, the same
    two at inv_temp 0 and greedy_sample_step."""
    rows = None if all_rows else c.cpu_rows
    check_sampled(c, draw_tokens(dev), rows)
    check_greedy(c, draw_greedy(dev), rows)
    if rows is not None:        # a large case on the CPU: the two ops once
        return
    check_sampled(c, draw_step(dev), rows)
    check_greedy(c, draw_tokens(dev, greedy=True), rows)
    check_greedy(c, draw_step(dev, greedy=True), rows)


EOS_KINDS = tuple(SLOT_EOS)
NO_BODY = [(n, hot) for n in range(1, 8) for hot in [None] + list(range(n))]


def small_cases():
    """Every case of at most 2^17 columns, smallest work first."""
    yield empty_window_case()
    yield empty_window_no_eos_case()
    yield all_neg_inf_case()
    for i in range(len(KEPT_TABLE)):
        yield kept_case(i)
    for i in range(5):
        yield weight_case(i)
    for n, hot in NO_BODY:
        yield no_body_case(n, hot)
    for kind in EOS_KINDS:
        for spec in SLOT_SPECS:
            yield slot_one_hot_case(kind, spec)
        yield slot_tie_case(kind)
        for si in range(len(INF_SLOTS)):
            yield inf_case(si, kind)
    yield scan_16k_case()
    yield unit_weight_case()


# ---- bookkeeping ----------------------------------------------------------------

BK_MAX_RUN, BK_HIST_ROWS, BK_B = 4, 7, 5
BK_CTRS = (-1, 0, BK_MAX_RUN - 1, BK_MAX_RUN, BK_HIST_ROWS - 1, BK_HIST_ROWS,
           BK_HIST_ROWS + 5)


def check_bookkeeping(step, ctr0, dev):
    """step(logits, lo, hi, eos, script, mask, ctr, hist, tokens, ticket)
    on one-hot rows.  hist and tokens are three rows wider than B and
    sentinel-filled, hist a view of a wider buffer; rows 0 and B - 1 are
    scripted at the clamped column, row 1 at another column and a row
    beyond B at the clamped one."""
    B, V, lo, hi, eos = BK_B, 300, 5, 290, 2
    c = new_case("bookkeeping", V, lo, hi, eos, B)
    hot = [2, 5, 150, 289, 17]
    for b in range(B):
        set_one_hot(c, b, hot[b])
    j = min(max(ctr0, 0), BK_MAX_RUN - 1)
    g = torch.Generator().manual_seed(77 + ctr0)
    script = torch.randint(1000, 2000, (B + 3, BK_MAX_RUN), generator=g)
    mask = torch.zeros(B + 3, BK_MAX_RUN, dtype=torch.bool)
    mask[0, j] = mask[B - 1, j] = mask[B + 1, j] = True
    mask[1, (j + 1) % BK_MAX_RUN] = True
    want = list(hot)
    want[0], want[B - 1] = int(script[0, j]), int(script[B - 1, j])
    wide = torch.full((BK_HIST_ROWS, B + 3 + 6), -7, dtype=torch.int64)
    want_wide = wide.clone()
    if 0 <= ctr0 < BK_HIST_ROWS:
        want_wide[ctr0, :B] = torch.tensor(want)
    wide = wide.to(dev)
    hist = wide[:, :B + 3]
    assert hist.stride(0) > hist.shape[1]
    tokens = torch.full((B + 3,), -7, dtype=torch.int64, device=dev)
    ctr = torch.tensor([ctr0], dtype=torch.int64, device=dev)
    ticket = None if dev == "cpu" else \
        torch.zeros(1, dtype=torch.int32, device=dev)
    step(c.logits.to(dev), lo, hi, eos, script.to(dev), mask.to(dev), ctr,
         hist, tokens, ticket)
    assert tokens.tolist() == want + [-7] * 3
    assert torch.equal(wide.cpu(), want_wide)
    assert int(ctr[0]) == ctr0 + 1
    if ticket is not None:
        assert int(ticket[0]) == 0


def sampled_step(dev):
    def step(logits, lo, hi, eos, *rest):
        c = types.SimpleNamespace(inv=[1.0] * BK_B, k=[0, 1, 5, 0, 2],
                                  pq=[OFF, OFF, 40000, 1, OFF],
                                  seed=[SEED] * BK_B, pos=[9] * BK_B)
        D.sample_step(logits, lo, hi, eos, *params(c, range(BK_B), dev),
                      *rest)
    return step


# ---- tests: the reference ---------------------------------------------------------

@pytest.mark.parametrize("ctr,key,want", [
    ((0, 0, 0, 0), (0, 0),
     (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2,
     (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344),
     (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
])
def test_reference_philox_known_answers(ctr, key, want):
    assert ref_philox(ctr, key) == want


def _bits(x):
    return struct.unpack("<I", struct.pack("<f", x))[0] >> 16


def test_reference_weight_pins():
    assert float(F(EX) * _LOG2E) == 1.0
    assert [float(c).hex() for c in _C] == [
        "0x1.0000000000000p+0", "0x1.62e4300000000p-1",
        "0x1.ebfbe00000000p-3", "0x1.c6b08e0000000p-5",
        "0x1.3b2ab60000000p-7", "0x1.5d87fe0000000p-10",
        "0x1.4309120000000p-13"]
    assert float(_LOG2E).hex() == "0x1.7154760000000p+0"
    for m in (0.0, 9.0, -1.0, 30.0):
        for it in (1.0, EX, 2.0 ** -20, 1e30):
            assert ref_weight(_bits(m), m, f32(it)) == 1 << 40
        for j in EXACT_J:
            w = ref_weight(_bits(m - j), m, EX)
            assert w == ((1 << 40) >> j if j <= 40 else 0), (m, j)
    # the second product rounds off the integer at the other j
    assert [j for j in range(42)
            if float(F(F(F(-j) * F(EX)) * _LOG2E)) != -j] == \
        [j for j in range(42) if j not in EXACT_J]
    assert ref_weight(_bits(-40.0), 0.0, EX) == 1
    assert ref_weight(_bits(-41.0), 0.0, EX) == 0
    assert ref_weight(_bits(NINF), 0.0, EX) == 0
    assert ref_weight(_bits(NINF), 0.0, f32(2.0 ** -20)) == 0
    assert ref_weight(_bits(-0.0), 0.0, 1.0) == 1 << 40


def test_reference_key_orders_bf16():
    vals = [NINF, -3.0e38, -4.0, -1.0, -1e-30, -0.0, 0.0, 1e-30, 0.5, 2.0,
            9.0, PINF]
    keys = [ref_key(_bits(v)) for v in vals]
    assert keys == sorted(keys) and len(set(keys)) == len(keys)
    assert (ref_key(_bits(9.0)) >> 8, ref_key(_bits(8.0)) >> 8,
            ref_key(_bits(7.0)) >> 8, ref_key(_bits(2.0)) >> 8,
            ref_key(_bits(1.0)) >> 8) == (0xC1, 0xC1, 0xC0, 0xC0, 0xBF)


def test_weights_match_the_reference_bit_for_bit():
    """D.sample_weights against ref_weight: the weight table's values and
    500 random bit patterns below the maximum, at each inv_temp."""
    g = torch.Generator().manual_seed(3)
    rnd = torch.randint(0, 65536, (500,), generator=g).tolist()
    for m in (0.0, 7.5):
        pats = [_bits(m - j) for j in range(51)] + \
            [b for b in rnd if bf16_value(b) <= m] + [_bits(NINF)]
        L = torch.tensor([p - 65536 if p >> 15 else p for p in pats],
                         dtype=torch.int16).view(torch.bfloat16).unsqueeze(0)
        for _, it in WEIGHT_SPECS:
            it = f32(it)
            got = D.sample_weights(L, torch.tensor([m]),
                                   torch.tensor([it]))[0].tolist()
            assert got == [ref_weight(b, m, it) for b in pats], (m, it)


# ---- tests: the tables ------------------------------------------------------------

def test_slot_table_reaches_every_phase_head_and_tail():
    g = [layout(b * SV, SLO, SHI) for b in range(8)]
    assert {x.mis for x in g} == set(range(8))
    assert {x.head for x in g} == set(range(8))
    assert {x.tail for x in g} == set(range(8))
    assert all(x.nchunk == 2 for x in g)
    for n in range(1, 8):
        assert all(layout(b * SV, SLO, SLO + n).nchunk == 0
                   for b in range(64))
    # every one-hot slot exists in some row, so the fallback never hides one
    c = slot_one_hot_case("above", ("eos",))
    for spec in SLOT_SPECS:
        assert any(slot_index(c, b, spec) is not None for b in range(8)), spec
    g = layout(0, 2, 16490)
    assert (g.nchunk, g.nstep) == (9, 11)
    g = [layout(b * 2200003, 3, 2199997) for b in range(8)]
    assert all(x.nstep == 1077 for x in g)


@pytest.mark.parametrize("kind", EOS_KINDS)
def test_slot_ties_draw_every_class(kind):
    """By the reference alone: over the 64 fixed rows every slot class of
    the tie set is the token at least once."""
    c = slot_tie_case(kind)
    want = {"head", "tail"} | {"body" + str(o) for o in BODY_OFFSETS} | \
        ({"eos"} if kind != "absent" else set())
    assert c.classes == want
    assert set(c.cls) == want
    for b in range(64):             # the formula is the reference's token
        assert ref_row(row_bits(c, b), c.lo, c.hi, c.eos, c.inv[b], 0, OFF,
                       c.seed[b], c.pos[b]).token == c.want[b]


def test_scan_rows_draw_every_slot():
    c = scan_16k_case()
    assert all(layout(b * c.V, c.lo, c.hi).nstep == 11 for b in range(8))
    assert {step_of(c, b, c.want[b]) for b in range(8)} == \
        {0, 1, 7, 8, 9, 10, "eos"}
    c = scan_2m_case()
    steps = [step_of(c, b, c.want[b]) for b in range(8)]
    assert set(steps) == {1, 511, 512, 513, 1023, 1024, 1076, "eos"}
    assert [steps[b] for b in c.cpu_rows] == [512, 1024]
    for lo in (0, 1):
        c = scan_max_case(lo)
        assert [step_of(c, b, c.want[b]) for b in (0, 2, 3, 4, 5, 7)] == \
            [2046, 2047, 1, 2046, 2047, 2046]


def test_kept_table_covers_the_bins():
    """Every kept set is the one written in the table; the table has
    top-p in top-k's bin, above it, and with top-k off."""
    seen = set()
    for i, s in enumerate(KEPT_TABLE):
        c = kept_case(i)
        r = ref_row(row_bits(c, 0), c.lo, c.hi, c.eos, c.inv[0], s.k, s.pq,
                    SEED, 0)
        assert r.kept == s.kept, s.name
        assert set(c.want) <= s.kept, s.name
        if s.pq < OFF:
            seen.add("off" if r.bk is None else
                     "same" if r.bp == r.bk else
                     "above" if r.bp > r.bk else "below")
        if len(s.kept) > 1:
            assert len(set(c.want)) > 1, s.name
    assert seen == {"off", "same", "above"}
    bins = {ref_row(row_bits(kept_case(i), 0), KLO, KHI, KEOS, EX,
                    KEPT_TABLE[i].k, OFF, SEED, 0).bk for i in range(6)}
    assert bins == {0xC1, 0xC0, 0x3F}


def test_unit_weight_positions():
    c = unit_weight_case()
    for b, pos in enumerate(UNIT_POS):
        target = (ref_r(SEED, pos) * c.total) >> 64
        assert target > 1 << 40, pos
    r = ref_row(row_bits(c, 0), c.lo, c.hi, c.eos, c.inv[0], 0, OFF, SEED,
                UNIT_POS[0])
    assert r.total == c.total and r.token == c.want[0]


# ---- tests: the CPU branches -------------------------------------------------------

@pytest.mark.parametrize("kind", EOS_KINDS)
def test_slots_one_hot(kind):
    for spec in SLOT_SPECS:
        check_case(slot_one_hot_case(kind, spec), "cpu")


@pytest.mark.parametrize("kind", EOS_KINDS)
def test_slots_ties(kind):
    check_case(slot_tie_case(kind), "cpu")


def test_empty_windows_and_dead_rows():
    check_case(empty_window_case(), "cpu")
    check_case(empty_window_no_eos_case(), "cpu")
    check_case(all_neg_inf_case(), "cpu")


@pytest.mark.parametrize("n", range(1, 8))
def test_no_body_windows(n):
    for hot in [None] + list(range(n)):
        check_case(no_body_case(n, hot), "cpu")


def test_step_scan_16k():
    check_case(scan_16k_case(), "cpu")


def test_step_scan_2m():
    check_case(scan_2m_case(), "cpu")


@pytest.mark.parametrize("lo", (0, 1))
def test_step_scan_max(lo):
    check_case(scan_max_case(lo), "cpu")


@pytest.mark.parametrize("i", range(len(KEPT_TABLE)),
                         ids=[s.name for s in KEPT_TABLE])
def test_kept_sets(i):
    check_case(kept_case(i), "cpu")


@pytest.mark.parametrize("i", range(5))
def test_weight_rows(i):
    check_case(weight_case(i), "cpu")


def test_unit_weights():
    check_case(unit_weight_case(), "cpu")


@pytest.mark.parametrize("kind", EOS_KINDS)
@pytest.mark.parametrize("si", range(len(INF_SLOTS)))
def test_plus_inf_gives_the_greedy_token(si, kind):
    check_case(inf_case(si, kind), "cpu")


@pytest.mark.parametrize("ctr0", BK_CTRS)
def test_bookkeeping(ctr0):
    check_bookkeeping(D.greedy_sample_step, ctr0, "cpu")
    check_bookkeeping(sampled_step("cpu"), ctr0, "cpu")


# ---- tests: mutants ----------------------------------------------------------------

def test_checks_pass_the_reference():
    for c in small_cases():
        check_sampled(c, ref_drawer(None))
        check_greedy(c, ref_drawer(None, greedy=True))


def test_checks_reject_mutants():
    """The reference with one change each, handed to the checks as a
    sampler: every mutant fails at least one case of the sampled checks,
    and those that change the greedy token one of the greedy checks
    too."""
    for mut in MUTANTS:
        checks = {"sampled": (check_sampled, ref_drawer(mut))}
        if mut in GREEDY_MUTANTS:
            checks["greedy"] = (check_greedy, ref_drawer(mut, greedy=True))
        killed = {}
        for c in small_cases():
            for what, (check, draw) in checks.items():
                if what not in killed:
                    try:
                        check(c, draw)
                    except AssertionError:
                        killed[what] = c.name
            if len(killed) == len(checks):
                break
        for what in checks:
            print(f"mutant {mut}, {what}: rejected by "
                  f"'{killed.get(what)}'")
            assert what in killed, \
                f"mutant {mut} passed every case of the {what} checks"
