"""Exact read-out and edge cases of the paged-attention kernels and the
KV-cache writers (ops/hip/paged_attn.hip, attn_core.h).

This module holds the case tables, the input builders (fixed seeds, built on
the CPU), the expected values and the check_*(fn, case, to_dev) functions,
plus a plain torch model of each op that follows the kernels' decomposition
(pages, splits, online softmax, merge, epilogue).  Its own tests run every
case through the CPU paths of ops.dispatch where one exists and through the
torch models (prefill attention has no CPU dispatch path);
tests/test_gpu_attn_edges.py runs the same cases and assertions through the
HIP kernels.

Three kinds of case:

* exact read-out, compared bit for bit.  scale = 1 and every q and K entry
  is a small integer (bf16-exact), so every score is an integer below 2^24
  and exact in f32 in any order.  K[t] is one-hot in three groups of dims
  (t & 7 -> dims 0-7, (t >> 3) & 7 -> dims 8-15, page t >> 6 -> dims 16-31);
  a q that targets t carries 128 on t's three dims, so the target scores
  384 and every other key <= 256: the keys at the same in-page offset of
  every other page are decoys at 256, which make the running maximum climb
  at the target's page and force a rescale of the history to exactly 0, at
  a different page for every column.  With a lead >= 128, exp(other - max)
  is 0 in f32, P is exactly 1 or 0, alpha exactly 1 or 0 and l the number
  of winners: the output is V of the winner (random bf16, no zeros), or for
  a 2- or 4-way tie over integer V rows their mean, computed in float64 and
  rounded once.  "Ramp" columns carry 128 * 64 on a dim that holds the page
  index and 128 on a dim that holds the in-page index: the score is 128 * t,
  the winner is the LAST permitted key (the row's own position in causal
  prefill, the appended token in fused decode) with key t - 1 the runner-up
  and key t + 1 hotter still, so an off-by-one in either direction changes
  the bits; negated, the winner is key 0.  Every slot a correct kernel must
  mask (stale slots after the context's end, every page named by unused
  block-table entries, pages of inactive rows) is a trap: q carries 2^18 on
  a dim that only traps set, and their V is -7.  A trap that is read shows
  as -7, never as a fault: unused block-table entries name allocated pages.
  No expectation uses attention arithmetic: V rows are picked by index.
* Gaussian data against a float64 softmax, under the per-element bound
      |out - ref| <= 2^-8 |ref| + 2^-8 A,   A = sum p_i |v_i| / sum p_i.
  2^-8 |ref| is the half-ulp of the single bf16 store.  2^-8 A is twice the
  2^-9 relative rounding of P to bf16 ahead of the PV product (l sums the
  unrounded p); the factor 2 covers the f32 score, exp and accumulation
  terms, which are orders of magnitude smaller.  Under this bound a dropped
  key is rejected at contexts <= 65 keys, which is why the contexts are 1,
  2, 17, 63, 64, 65 and 130 keys: single-key errors at longer contexts are
  the exact cases' job.  In fused decode the reference q is the float64
  rotation rounded once to bf16; the kernel's f32 rotation can differ from
  it in the last bit only at a near-tie of the rounding, which moves a
  score by <= 2^-8 |q_d k_d| and stays well inside the P term.
  RoPE itself (rope_kv_append, rope_kv_scatter, the fused append; the real
  rope_tables) is held to
      |out - ref| <= 2^-8 |ref| + 2^-22 (|x0 c| + |x1 s|)
  against a float64 rotation by the same f32 table entries: the bf16 store,
  plus two f32 products and one sum at unit roundoff 2^-24 each, doubled.
* writers on sentinel-filled caches: written slots equal the index-formula
  expectation kc[page, kvh, d // 8, pos % 64, d % 8], vc[page, kvh, d,
  pos % 64] bit for bit (quarter-turn tables, cos = 0 and sin = +-1, keep
  the rotation exact) and every other element still holds the sentinel.
  Row 0 of the quarter-turn tables is the identity, as position 0 of the
  real tables is.

test_checks_reject_mutants hands the checks deliberately wrong models and
expects every one to be rejected.
"""

import functools
import math
import random
import types

import pytest
import torch

from quickstart_streaming_agents_amd.ops import cpu_ref
from quickstart_streaming_agents_amd.ops import dispatch as D

PAGE = 64
TRAP_DIM, PG_DIM, OFF_DIM = 40, 41, 42      # trap flag, page index, in-page index
QW = 128.0                                  # q weight of a code dim
TRAP_W = float(2 ** 18)                     # q weight of the trap dim
TRAP_V = -7.0
NEG = -3.0e38
CODE, RAMP, NEGRAMP = 0, 1, 2

# tests/test_gpu_decode_fused.py::_LENS
LENS = [1, 2, 16, 0, 17, 32, 33, 0, 64, 65, 129, 0, 448, 449, 128, 0,
        192, 200, 300, 0, 440, 570, 800, 0]
# tests/test_gpu_prefill_tiled.py::ITEMS, then: sub-tiles / 16-row blocks
# past the item's end, tile-size neighbours, a 16-row block across a page
# end behind a cached prefix, a page end behind a two-page prefix
ITEMS = [(0, 1), (0, 15), (0, 16), (0, 17), (0, 33), (0, 64), (0, 65),
         (0, 130), (63, 2), (64, 1), (100, 33), (130, 70), (200, 5),
         (0, 5), (0, 31), (0, 32), (0, 63), (60, 16), (127, 2), (128, 64)]
# tests/test_gpu_prefill_tiled.py::TILED_SHAPES
TILED_SHAPES = [(128, 8, 2, 32), (64, 8, 2, 32), (64, 8, 2, 64),
                (128, 16, 2, 32), (64, 16, 2, 64)]
FALLBACK_SHAPE = (128, 28, 4, 32)           # R = 7: the binding's fallback
ONE_WAVE_SHAPES = [(64, 4, 4), (128, 4, 2), (64, 8, 2)]      # R = 1, 2, 4


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _ident(t):
    return t


def bits16(t):
    return t.detach().cpu().contiguous().view(torch.int16)


def assert_bits_equal(got, want, what):
    got = got.detach().cpu()
    assert got.dtype == torch.bfloat16 and got.shape == want.shape, \
        f"{what}: got {got.dtype} {tuple(got.shape)}"
    diff = bits16(got) != bits16(want)
    if diff.any():
        at = tuple(int(v) for v in diff.nonzero()[0])
        raise AssertionError(
            f"{what}: {int(diff.sum())} of {diff.numel()} elements differ; "
            f"first at {at}: got {got[at].item()!r} expected "
            f"{want[at].item()!r}")


def decode_num_splits(B, KVH, width):
    """ops.cpp decode_num_splits."""
    ns = min(32, max(1, -(-2048 // (B * KVH))))
    if ns > 1:
        ns = max(ns, 4)
    return min(ns, max(1, width))


# ---------------------------------------------------------------------------
# paged caches
# ---------------------------------------------------------------------------

def build_cache(Dh, KVH, valid, width, seed, gauss=False):
    """Shuffled pages for sequences of valid[i] keys (every sequence owns at
    least one page), two trap pages for the unused block-table entries.
    Exact mode: code keys, traps in every stale slot.  Gaussian mode: randn
    K and V, NaN K and V = -7 in every stale slot."""
    g = _gen(seed)
    B = len(valid)
    need = [max(1, -(-n // PAGE)) for n in valid]
    assert max(need) <= width and max(need) <= 16
    P = sum(need) + 2
    perm = torch.randperm(P, generator=g)
    bt = perm[-2:][torch.arange(width) % 2].repeat(B, 1).int()
    owner = torch.zeros(P, dtype=torch.long)    # page index inside its sequence
    nval = torch.zeros(P, dtype=torch.long)     # valid slots of the page
    at = 0
    for b, n in enumerate(valid):
        ids = perm[at:at + need[b]]
        at += need[b]
        bt[b, :need[b]] = ids.int()
        j = torch.arange(need[b])
        owner[ids] = j
        nval[ids] = (n - PAGE * j).clamp(0, PAGE)
    o = torch.arange(PAGE)
    stale = (o[None, :] >= nval[:, None])[:, None, :].expand(P, KVH, PAGE)
    if gauss:
        kl = torch.randn(P, KVH, PAGE, Dh, generator=g).bfloat16()
        kl[stale] = float("nan")
        vl = torch.randn(P, KVH, PAGE, Dh, generator=g).bfloat16()
    else:
        code = torch.zeros(P, PAGE, Dh)
        code[:, o, o & 7] = 1
        code[:, o, 8 + (o >> 3)] = 1
        code[torch.arange(P)[:, None], o[None, :], (16 + owner)[:, None]] = 1
        code[:, :, PG_DIM] = owner[:, None].float()
        code[:, :, OFF_DIM] = o[None, :].float()
        kl = torch.randint(-2, 3, (P, KVH, PAGE, Dh), generator=g).float()
        kl[..., :32] = 0
        kl[..., TRAP_DIM:OFF_DIM + 1] = 0
        kl += code[:, None]
        trap = torch.zeros(Dh)
        trap[TRAP_DIM] = 1
        kl[stale] = trap
        kl = kl.bfloat16()
        vl = torch.randn(P, KVH, PAGE, Dh, generator=g).bfloat16()
        vl[vl == 0] = 1
    vl[stale] = TRAP_V
    # logical [P, KVH, pos, d] -> K [P, KVH, D/8, 64, 8], V [P, KVH, D, 64]
    kc = kl.view(P, KVH, PAGE, Dh // 8, 8).permute(0, 1, 3, 2, 4).contiguous()
    vc = vl.permute(0, 1, 3, 2).contiguous()
    return types.SimpleNamespace(D=Dh, KVH=KVH, kc=kc, vc=vc, bt=bt,
                                 valid=list(valid), need=need)


def _page_off(c, seq, t):
    return c.bt.long()[seq, t >> 6], t & 63


def v_rows(c, seq, kvh, t):
    page, off = _page_off(c, seq, t)
    return c.vc[page, kvh, :, off]


def k_rows(c, seq, kvh, t):
    page, off = _page_off(c, seq, t)
    return c.kc[page, kvh, :, off, :].reshape(*page.shape, c.D)


def set_trap(c, seq, t):
    """Make slot t of every kv head of sequences seq a trap."""
    page, off = _page_off(c, seq, t)
    trap = torch.zeros(c.D, dtype=torch.bfloat16)
    trap[TRAP_DIM] = 1
    c.kc[page, :, :, off, :] = trap.view(c.D // 8, 8)
    c.vc[page, :, :, off] = TRAP_V


def make_q(Dh, mode, tg):
    """mode [N]: CODE / RAMP / NEGRAMP; tg [N, 4]: the winners of a CODE
    column (-1 = unused)."""
    N = mode.numel()
    q = torch.zeros(N, Dh)
    q[:, TRAP_DIM] = TRAP_W
    idx = torch.arange(N)
    for j in range(tg.shape[1]):
        sel = (mode == CODE) & (tg[:, j] >= 0)
        i, t = idx[sel], tg[sel, j]
        assert t.numel() == 0 or int(t.max()) < 16 * PAGE
        q[i, t & 7] = QW
        q[i, 8 + ((t >> 3) & 7)] = QW
        q[i, 16 + (t >> 6)] = QW
    q[mode == RAMP, PG_DIM] = QW * PAGE
    q[mode == RAMP, OFF_DIM] = QW
    q[mode == NEGRAMP, PG_DIM] = -QW * PAGE
    q[mode == NEGRAMP, OFF_DIM] = -QW
    return q.bfloat16()


def plant_int_v(c, seq, kvh, tg, seed):
    """Integer V rows in [-64, 64] \\ {0} at the winners of every tie."""
    tie = (tg >= 0).sum(1) > 1
    s = seq[tie][:, None].expand(-1, tg.shape[1])[tg[tie] >= 0]
    k = kvh[tie][:, None].expand(-1, tg.shape[1])[tg[tie] >= 0]
    t = tg[tie][tg[tie] >= 0]
    v = torch.randint(1, 65, (t.numel(), c.D), generator=_gen(seed)).float()
    v *= torch.randint(0, 2, v.shape, generator=_gen(seed + 1)) * 2.0 - 1
    page, off = _page_off(c, s, t)
    c.vc[page, k, :, off] = v.bfloat16()


def expect_rows(c, seq, kvh, tg):
    """V of the winner bit for bit; ties: the float64 mean rounded once."""
    ok = tg >= 0
    n = ok.sum(1)
    rows = v_rows(c, seq[:, None].expand_as(tg), kvh[:, None].expand_as(tg),
                  tg.clamp(min=0))                            # [N, 4, D]
    mean = (rows.double() * ok[..., None]).sum(1) / n.clamp(min=1)[:, None]
    assert torch.equal(mean.float().double(), mean)     # one rounding left
    out = mean.float().bfloat16()
    out[n == 1] = rows[n == 1, 0]
    return out


# ---------------------------------------------------------------------------
# decode cases
# ---------------------------------------------------------------------------

def _stride_for(n):
    return next(s for s in (69, 71, 73, 77, 79, 83, 89) if math.gcd(s, n) == 1)


def decode_targets(lens, QH):
    """Per (row, head) column: mode and winners.  Columns of one length
    class take turns: ramp, negated ramp, 2-way tie (same offset in two
    pages), 4-way tie (two offsets x two pages), then four single targets
    that walk the positions with a stride coprime to the length, so
    neighbouring heads sit in different pages and the class covers
    min(singles, length) distinct positions."""
    N = len(lens) * QH
    mode = torch.zeros(N, dtype=torch.long)
    tg = torch.full((N, 4), -1, dtype=torch.long)
    seen, singles = {}, {}
    for b, n in enumerate(lens):
        if n == 0:
            continue
        npg = -(-n // PAGE)
        last = n - PAGE * (npg - 1)             # valid slots of the last page
        stride = _stride_for(n)
        for h in range(QH):
            i = b * QH + h
            g = seen.get(n, 0)
            seen[n] = g + 1
            kind = g % 8
            if kind == 0:
                mode[i], tg[i, 0] = RAMP, n - 1
            elif kind == 1:
                mode[i], tg[i, 0] = NEGRAMP, 0
            elif kind in (2, 3) and npg > 1:
                pa = PAGE * ((g // 8) % (npg - 1))
                pb = PAGE * (npg - 1)
                if kind == 3 and last >= 2:
                    off = 2 * ((g * 5) % (last // 2))
                    tg[i] = torch.tensor([pa + off, pa + off + 1,
                                          pb + off, pb + off + 1])
                else:
                    off = (g * 5) % last
                    tg[i, :2] = torch.tensor([pa + off, pb + off])
            else:
                s = singles.get(n, 0)
                singles[n] = s + 1
                tg[i, 0] = (s * stride) % n
    return mode, tg, singles


_SHAPES = [(2, 2), (8, 2), (28, 4), (32, 2)]        # R = 1, 4, 7, 16
_PART_LENS = [[800, 0, 449], [570, 1, 64], [65, 440, 2], [300, 129, 33]]
_PATHS = ("one", "wg4", "part2", "part", "narrow")


def _decode_lens(path, KVH, ri):
    if path == "one":           # B * KVH = 2048 -> NS = 1
        pool = [n for n in LENS if n <= 192]
        return [pool[i % len(pool)] for i in range(2048 // KVH)], 32
    if path == "wg4":           # B * KVH = 512 -> NS = 4, merged in LDS
        return [LENS[i % len(LENS)] for i in range(512 // KVH)], 32
    if path == "part2":         # B * KVH = 192 -> NS = 11, two-page splits
        return [LENS[i % len(LENS)] for i in range(192 // KVH)], 32
    if path == "part":          # B = 3 -> NS = 32, one page per split
        return _PART_LENS[ri], 32
    pool = [n for n in LENS if n <= 128]    # 2-wide table caps NS at 2
    return [pool[i % len(pool)] for i in range(512 // KVH)], 2


# every (path, R) and every (path, D), D alternating
DECODE_CASES = [(path, 64 if (pi + ri) % 2 else 128, QH, KVH)
                for pi, path in enumerate(_PATHS)
                for ri, (QH, KVH) in enumerate(_SHAPES)]


def case_id(spec):
    return "-".join(str(v) for v in spec)


@functools.lru_cache(maxsize=2)
def decode_case(path, Dh, QH, KVH):
    ri = _SHAPES.index((QH, KVH))
    lens, width = _decode_lens(path, KVH, ri)
    B, R = len(lens), QH // KVH
    seed = 1000 + 10 * _PATHS.index(path) + ri
    c = build_cache(Dh, KVH, lens, width, seed)
    mode, tg, singles = decode_targets(lens, QH)
    seq = torch.arange(B).repeat_interleave(QH)
    kvh = (torch.arange(QH) // R).repeat(B)
    plant_int_v(c, seq, kvh, tg, seed + 1)
    q = make_q(Dh, mode, tg).view(B, QH, Dh)
    exp = expect_rows(c, seq, kvh, tg).view(B, QH, Dh)
    return types.SimpleNamespace(
        D=Dh, QH=QH, KVH=KVH, lens=lens, cache=c, q=q, expected=exp,
        sl=torch.tensor(lens, dtype=torch.int32), mode=mode, tg=tg,
        singles=singles, ns=decode_num_splits(B, KVH, width))


def check_decode(fn, case, to_dev):
    """fn(q, kc, vc, block_table, seq_lens, scale) -> [B, QH, D] bf16."""
    c = case.cache
    out = fn(to_dev(case.q), to_dev(c.kc), to_dev(c.vc), to_dev(c.bt),
             to_dev(case.sl), 1.0)
    assert_bits_equal(out, case.expected, "decode output")


# ---- fused decode: RoPE + append + attention --------------------------------

def quarter_tables(npos, Dh, seed):
    """cos = 0, sin = +-1 per (position, dim); row 0 is the identity."""
    sin = torch.randint(0, 2, (npos, Dh // 2), generator=_gen(seed)) * 2.0 - 1
    cos = torch.zeros(npos, Dh // 2)
    cos[0], sin[0] = 1, 0
    return cos, sin


def identity_tables(npos, Dh):
    return torch.ones(npos, Dh // 2), torch.zeros(npos, Dh // 2)


def rope64(x, c, s):
    """float64 rotation of x [..., D] by table rows c, s [..., D/2]."""
    half = x.shape[-1] // 2
    x0, x1 = x[..., :half].double(), x[..., half:].double()
    c, s = c.double(), s.double()
    return torch.cat([x0 * c - x1 * s, x0 * s + x1 * c], dim=-1)


def rope_mag(x, c, s):
    """|x0 c| + |x1 s| and |x0 s| + |x1 c|: the products behind each output
    of the rotation."""
    half = x.shape[-1] // 2
    x0, x1 = x[..., :half].double().abs(), x[..., half:].double().abs()
    c, s = c.double().abs(), s.double().abs()
    return torch.cat([x0 * c + x1 * s, x0 * s + x1 * c], dim=-1)


def unrope_exact(y, c, s):
    """The x with rope(x) == y, for identity and quarter-turn rows."""
    half = y.shape[-1] // 2
    y0, y1 = y[..., :half].float(), y[..., half:].float()
    x = torch.cat([y0 * c + y1 * s, y1 * c - y0 * s], dim=-1).bfloat16()
    assert torch.equal(bits16(rope64(x, c, s).float().bfloat16()), bits16(y))
    return x


def qkv_views(buf, QH, KVH, Dh):
    n = buf.shape[0]
    q = buf[:, :QH * Dh].view(n, QH, Dh)
    k = buf[:, QH * Dh:(QH + KVH) * Dh].view(n, KVH, Dh)
    v = buf[:, (QH + KVH) * Dh:].view(n, KVH, Dh)
    return q, k, v


@functools.lru_cache(maxsize=2)
def fused_case(path, Dh, QH, KVH, tables):
    """The decode case with its last token taken out of the caches again:
    that slot is a trap, the token arrives un-rotated in the qkv buffer, q
    arrives un-rotated too.  Expected caches: those of the decode case."""
    base = decode_case(path, Dh, QH, KVH)
    c = base.cache
    B = len(base.lens)
    sl = base.sl.long()
    act = sl > 0
    pos = (sl - 1).clamp(min=0)
    npos = max(base.lens) + 1
    cos, sin = identity_tables(npos, Dh) if tables == "identity" \
        else quarter_tables(npos, Dh, 7 + Dh + QH)
    cr, sr = cos[pos][:, None], sin[pos][:, None]
    rows = torch.arange(B)[:, None].expand(B, KVH)
    heads = torch.arange(KVH)[None, :].expand(B, KVH)
    g = _gen(77 + QH)
    buf = torch.randint(-3, 4, (B, (QH + 2 * KVH) * Dh), generator=g) \
        .float().bfloat16()
    q, k, v = qkv_views(buf, QH, KVH, Dh)
    q.copy_(unrope_exact(base.q, cr, sr))
    k[act] = unrope_exact(k_rows(c, rows, heads, pos[:, None].expand(B, KVH)),
                          cr, sr)[act]
    v[act] = v_rows(c, rows, heads, pos[:, None].expand(B, KVH))[act]
    cin = types.SimpleNamespace(D=Dh, KVH=KVH, kc=c.kc.clone(),
                                vc=c.vc.clone(), bt=c.bt)
    set_trap(cin, torch.arange(B)[act], pos[act])
    return types.SimpleNamespace(
        D=Dh, QH=QH, KVH=KVH, base=base, qkv=buf, kc=cin.kc, vc=cin.vc,
        cos=cos, sin=sin, expected=base.expected)


def check_fused(fn, case, to_dev, keeps_qkv=True):
    """fn(q, k, v, kc, vc, cos, sin, block_table, seq_lens, scale) -> out;
    appends into kc / vc."""
    base = case.base
    buf = to_dev(case.qkv.clone())
    kc, vc = to_dev(case.kc.clone()), to_dev(case.vc.clone())
    q, k, v = qkv_views(buf, case.QH, case.KVH, case.D)
    out = fn(q, k, v, kc, vc, to_dev(case.cos), to_dev(case.sin),
             to_dev(base.cache.bt), to_dev(base.sl), 1.0)
    assert_bits_equal(out, case.expected, "fused decode output")
    assert_bits_equal(kc, base.cache.kc, "K cache after the append")
    assert_bits_equal(vc, base.cache.vc, "V cache after the append")
    if keeps_qkv:
        assert_bits_equal(buf, case.qkv, "qkv buffer")


# ---------------------------------------------------------------------------
# prefill cases
# ---------------------------------------------------------------------------

def tile_maps(lens, rows):
    item, pos0 = [], []
    for i, n in enumerate(lens):
        for p0 in range(0, n, rows):
            item.append(i)
            pos0.append(p0)
    return (torch.tensor(item, dtype=torch.int32),
            torch.tensor(pos0, dtype=torch.int32))


def prefill_targets(QH, causal, seed):
    """Per (row, head) column, by turns: own position (ramp), key 0
    (negated ramp), last key of the previous page, first key of the own
    page, a key inside the cached prefix, a random permitted key, a tie
    over two pages."""
    rnd = random.Random(seed)
    mode, tg, seq = [], [], []
    for i, (start, n) in enumerate(ITEMS):
        for a in range(n):
            qabs = start + a
            limit = qabs if causal else start + n - 1   # last permitted key
            for h in range(QH):
                kind = (a + 3 * h + i) % 7
                md, t = CODE, [rnd.randrange(limit + 1), -1, -1, -1]
                if kind == 0:
                    md, t[0] = RAMP, limit
                elif kind == 1:
                    md, t[0] = NEGRAMP, 0
                elif kind == 2 and qabs >= PAGE:
                    t[0] = PAGE * (qabs >> 6) - 1
                elif kind == 3:
                    t[0] = PAGE * (qabs >> 6)
                elif kind == 4 and start > 0:
                    t[0] = rnd.randrange(start)
                elif kind == 6 and limit >= PAGE:
                    off = rnd.randrange(PAGE)
                    pb = (limit >> 6) if off <= (limit & 63) \
                        else (limit >> 6) - 1
                    if pb >= 1:
                        pa = rnd.randrange(pb)
                        t[:2] = [PAGE * pa + off, PAGE * pb + off]
                mode.append(md)
                tg.append(t)
                seq.append(i)
    return torch.tensor(mode), torch.tensor(tg), torch.tensor(seq)


@functools.lru_cache(maxsize=2)
def prefill_case(Dh, QH, KVH, causal):
    starts = [s for s, _ in ITEMS]
    lens = [n for _, n in ITEMS]
    ctx = [s + n for s, n in ITEMS]
    width = max(-(-x // PAGE) for x in ctx) + 1
    seed = 2000 + Dh + QH + KVH + int(causal)
    c = build_cache(Dh, KVH, ctx, width, seed)
    mode, tg, seq = prefill_targets(QH, causal, seed)
    T = sum(lens)
    kvh = (torch.arange(QH) // (QH // KVH)).repeat(T)
    plant_int_v(c, seq, kvh, tg, seed + 1)
    # q is a strided view, as the model's qkv buffer gives it
    buf = torch.zeros(T, (QH + 2) * Dh, dtype=torch.bfloat16)
    q = buf[:, :QH * Dh].view(T, QH, Dh)
    q.copy_(make_q(Dh, mode, tg).view(T, QH, Dh))
    exp = expect_rows(c, seq, kvh, tg).view(T, QH * Dh)
    offs = [sum(lens[:i]) for i in range(len(lens))]
    mk = lambda x: torch.tensor(x, dtype=torch.int32)
    return types.SimpleNamespace(
        D=Dh, QH=QH, KVH=KVH, causal=causal, cache=c, q=q, expected=exp,
        lens=lens, off=mk(offs), start=mk(starts), len=mk(lens))


def check_prefill(fn, case, rows, to_dev):
    """fn(q, kc, vc, block_table, map_item, map_pos0, item_off, item_start,
    item_len, scale, causal) -> [T, QH * D] bf16, maps at `rows` rows."""
    c = case.cache
    item, pos0 = tile_maps(case.lens, rows)
    out = fn(to_dev(case.q), to_dev(c.kc), to_dev(c.vc), to_dev(c.bt),
             to_dev(item), to_dev(pos0), to_dev(case.off), to_dev(case.start),
             to_dev(case.len), 1.0, case.causal)
    assert_bits_equal(out, case.expected, "prefill output")


# ---------------------------------------------------------------------------
# Gaussian cases and the float64 reference
# ---------------------------------------------------------------------------

def ref64_attn(c, seq, q, nvis, scale):
    """q [S, KVH, C, D]: column (s, kvh, c) sees keys 0 .. nvis[s, c] - 1 of
    sequence seq[s].  -> (softmax(qK) V, softmax(qK) |V|) in float64."""
    S = q.shape[0]
    t = torch.arange(max(int(nvis.max()), 1))
    pg = c.bt.long()[seq[:, None], t >> 6]                  # [S, L]
    K = c.kc[pg, :, :, t & 63, :].reshape(S, t.numel(), c.KVH, c.D).double()
    V = c.vc[pg, :, :, t & 63].double()                     # [S, L, KVH, D]
    s = torch.einsum("skcd,slkd->skcl", q.double(), K) * scale
    vis = t[None, None, None, :] < nvis[:, None, :, None]
    p = torch.nan_to_num(s.masked_fill(~vis, float("-inf")).softmax(-1))
    return (torch.einsum("skcl,slkd->skcd", p, V),
            torch.einsum("skcl,slkd->skcd", p, V.abs()))


def assert_gauss_bound(out, ref, A, what):
    """|out - ref| <= 2^-8 |ref| + 2^-8 A (module docstring); prints and
    returns the worst err / bound."""
    out = out.detach().cpu().double().reshape(ref.shape)
    err = (out - ref).abs()
    bound = 2.0 ** -8 * ref.abs() + 2.0 ** -8 * A
    ratio = torch.where(err > 0, err / bound.clamp(min=1e-300),
                        torch.zeros_like(err))
    worst = float(ratio.max()) if ratio.numel() else 0.0
    print(f"{what}: worst err/bound {worst:.3f}")
    assert not torch.isnan(out).any(), what
    assert worst <= 1.0, f"{what}: err/bound {worst:.3f}"
    return worst


GAUSS_CTX = [1, 2, 17, 63, 64, 65, 130, 0]
# (D, QH, KVH, B): NS = 32, 32, 4, 1
GAUSS_DECODE = [(64, 8, 2, 8), (128, 28, 4, 8), (128, 8, 2, 256),
                (64, 32, 2, 1024)]


@functools.lru_cache(maxsize=2)
def gauss_decode_case(Dh, QH, KVH, B):
    lens = [GAUSS_CTX[i % len(GAUSS_CTX)] for i in range(B)]
    c = build_cache(Dh, KVH, lens, 32, 3000 + Dh + QH + B, gauss=True)
    q = torch.randn(B, QH, Dh, generator=_gen(3001 + B)).bfloat16()
    sl = torch.tensor(lens, dtype=torch.int32)
    scale = Dh ** -0.5
    R = QH // KVH
    ref, A = ref64_attn(c, torch.arange(B), q.view(B, KVH, R, Dh),
                        sl.long()[:, None].expand(B, R), scale)
    return types.SimpleNamespace(
        D=Dh, QH=QH, KVH=KVH, lens=lens, cache=c, q=q, sl=sl, scale=scale,
        ref=ref.reshape(B, QH, Dh), A=A.reshape(B, QH, Dh))


def check_gauss_decode(fn, case, to_dev):
    c = case.cache
    out = fn(to_dev(case.q), to_dev(c.kc), to_dev(c.vc), to_dev(c.bt),
             to_dev(case.sl), case.scale)
    return assert_gauss_bound(out, case.ref, case.A, "decode")


@functools.lru_cache(maxsize=2)
def gauss_fused_case(Dh, QH, KVH, B):
    """The Gaussian decode case behind the real rope tables: the reference
    attends with the float64 rotation of q (rounded once to bf16) over the
    caches with the float64-rotated new k row in place."""
    base = gauss_decode_case(Dh, QH, KVH, B)
    c, sl = base.cache, base.sl.long()
    act = sl > 0
    pos = (sl - 1).clamp(min=0)
    cos, sin = cpu_ref.rope_tables(max(base.lens) + 1, Dh)
    g = _gen(3100 + B)
    buf = torch.randn(B, (QH + 2 * KVH) * Dh, generator=g).bfloat16()
    q, k, v = qkv_views(buf, QH, KVH, Dh)
    cr, sr = cos[pos][:, None], sin[pos][:, None]
    kref = rope64(k, cr, sr)                        # [B, KVH, D] float64
    rows = torch.arange(B)[act]
    page, off = _page_off(c, rows, pos[act])
    want = types.SimpleNamespace(D=Dh, KVH=KVH, kc=c.kc.clone(),
                                 vc=c.vc.clone(), bt=c.bt)
    want.kc[page, :, :, off, :] = kref[act].float().bfloat16() \
        .view(-1, KVH, Dh // 8, 8)
    want.vc[page, :, :, off] = v[act]
    R = QH // KVH
    qr = rope64(q, cr, sr).float().bfloat16()
    ref, A = ref64_attn(want, torch.arange(B), qr.view(B, KVH, R, Dh),
                        sl[:, None].expand(B, R), base.scale)
    cin_k, cin_v = c.kc.clone(), c.vc.clone()
    cin_k[page, :, :, off, :] = float("nan")        # stale slot of the token
    cin_v[page, :, :, off] = TRAP_V
    kmag = rope_mag(k, cr, sr)
    return types.SimpleNamespace(
        D=Dh, QH=QH, KVH=KVH, base=base, qkv=buf, kc=cin_k, vc=cin_v,
        cos=cos, sin=sin, ref=ref.reshape(B, QH, Dh),
        A=A.reshape(B, QH, Dh), kref=kref, kmag=kmag, act=act, page=page,
        off=off, want_v=want.vc)


def assert_rope_bound(out, ref, mag, what):
    """|out - ref| <= 2^-8 |ref| + 2^-22 (|x0 c| + |x1 s|)."""
    err = (out.detach().cpu().double() - ref).abs()
    bound = 2.0 ** -8 * ref.abs() + 2.0 ** -22 * mag
    bad = err > bound
    assert not bad.any(), f"{what}: {int(bad.sum())} elements over the " \
        f"rope bound, worst excess {float((err - bound).max()):.3e}"


def check_gauss_fused(fn, case, to_dev):
    base = case.base
    buf = to_dev(case.qkv.clone())
    kc, vc = to_dev(case.kc.clone()), to_dev(case.vc.clone())
    q, k, v = qkv_views(buf, case.QH, case.KVH, case.D)
    out = fn(q, k, v, kc, vc, to_dev(case.cos), to_dev(case.sin),
             to_dev(base.cache.bt), to_dev(base.sl), base.scale)
    got_k = kc.cpu()[case.page, :, :, case.off, :].reshape(
        -1, case.KVH, case.D)
    assert_rope_bound(got_k, case.kref[case.act], case.kmag[case.act],
                      "appended k row")
    assert_bits_equal(vc, case.want_v, "V cache after the append")
    return assert_gauss_bound(out, case.ref, case.A, "fused decode")


SHORT_ITEMS = [i for i, (s, n) in enumerate(ITEMS) if s + n <= 65]


@functools.lru_cache(maxsize=2)
def gauss_prefill_case(Dh, QH, KVH, causal):
    starts = [s for s, _ in ITEMS]
    lens = [n for _, n in ITEMS]
    ctx = [s + n for s, n in ITEMS]
    width = max(-(-x // PAGE) for x in ctx) + 1
    c = build_cache(Dh, KVH, ctx, width, 4000 + Dh + QH, gauss=True)
    T, R = sum(lens), QH // KVH
    q = torch.randn(T, QH, Dh, generator=_gen(4001 + QH)).bfloat16()
    offs = [sum(lens[:i]) for i in range(len(lens))]
    scale = Dh ** -0.5
    refs = {}
    for i in SHORT_ITEMS:
        s, n = ITEMS[i]
        qi = q[offs[i]:offs[i] + n].view(n, KVH, R, Dh).permute(1, 0, 2, 3) \
            .reshape(1, KVH, n * R, Dh)
        nvis = (s + torch.arange(n) + 1) if causal \
            else torch.full((n,), s + n)
        ref, A = ref64_attn(c, torch.tensor([i]), qi,
                            nvis.repeat_interleave(R)[None], scale)
        back = lambda x: x.view(KVH, n, R, Dh).permute(1, 0, 2, 3) \
            .reshape(n, QH * Dh)
        refs[i] = (back(ref), back(A))
    mk = lambda x: torch.tensor(x, dtype=torch.int32)
    return types.SimpleNamespace(
        D=Dh, QH=QH, KVH=KVH, causal=causal, cache=c, q=q, scale=scale,
        lens=lens, offs=offs, off=mk(offs), start=mk(starts), len=mk(lens),
        refs=refs)


def check_gauss_prefill(fn, case, rows, to_dev):
    c = case.cache
    item, pos0 = tile_maps(case.lens, rows)
    out = fn(to_dev(case.q), to_dev(c.kc), to_dev(c.vc), to_dev(c.bt),
             to_dev(item), to_dev(pos0), to_dev(case.off), to_dev(case.start),
             to_dev(case.len), case.scale, case.causal).cpu()
    worst = 0.0
    for i, (ref, A) in case.refs.items():
        o = case.offs[i]
        worst = max(worst, assert_gauss_bound(
            out[o:o + ref.shape[0]], ref, A, f"prefill item {ITEMS[i]}"))
    return worst


# ---------------------------------------------------------------------------
# writers
# ---------------------------------------------------------------------------

SENTINEL = -7.0
W_QH, W_KVH = 8, 2
# new-token slots 0, 1 and 63 of a page, first and later pages; idle rows
APPEND_LENS = [1, 2, 64, 0, 65, 66, 128, 0, 129, 192]
SCATTER_T = [1, 63, 64, 65]
WRITERS = ("kv_append", "rope_kv_append", "kv_scatter", "rope_kv_scatter")


@functools.lru_cache(maxsize=4)
def writer_case(kind, Dh, T, tables):
    """Inputs of one writer call and what it must leave behind.  Append
    kinds: one row per APPEND_LENS entry (T ignored).  Scatter kinds: T
    tokens to permuted slots of 4 pages; rope_kv_scatter gets 3 pad rows of
    q behind them.  tables: "quarter" (exact) or "real" (Gaussian data)."""
    QH, KVH = W_QH, W_KVH
    append = kind.endswith("append")
    rope = kind.startswith("rope")
    g = _gen(5000 + Dh + T + len(kind))
    n_pages = 32
    if append:
        lens = torch.tensor(APPEND_LENS)
        rows = n = len(APPEND_LENS)
        perm = torch.randperm(n_pages, generator=g)
        bt = perm[:3 * n].view(n, 3).int()
        act = lens > 0
        pos = (lens - 1).clamp(min=0)
        slot = bt.long()[torch.arange(n), pos >> 6] * PAGE + (pos & 63)
        written = torch.arange(n)[act]
        index = dict(bt=bt, sl=lens.int())
    else:
        rows = T + (3 if kind == "rope_kv_scatter" else 0)
        slot = torch.randperm(4 * PAGE, generator=g)[:T] + 5 * PAGE
        pos = torch.randint(1, 300, (rows,), generator=g)
        written = torch.arange(T)
        act = torch.ones(rows, dtype=torch.bool)
        index = dict(pos=pos.int(), slots=slot.int())
    if tables == "quarter":
        cos, sin = quarter_tables(300, Dh, 5001 + Dh)
        buf = torch.randint(-8, 9, (rows, (QH + 2 * KVH) * Dh), generator=g)
    else:
        cos, sin = cpu_ref.rope_tables(300, Dh)
        buf = torch.randn(rows, (QH + 2 * KVH) * Dh, generator=g)
    buf = buf.float().bfloat16()
    q, k, v = qkv_views(buf, QH, KVH, Dh)
    cr, sr = cos[pos][:, None], sin[pos][:, None]
    kref = rope64(k, cr, sr) if rope else k.double()
    qref = rope64(q, cr, sr) if rope else q.double()
    qref[~act] = q[~act].double()           # idle rows are left alone
    mag = lambda x: rope_mag(x, cr, sr)
    # expected caches, element by element from the index formulas
    kc = torch.full((n_pages, KVH, Dh // 8, PAGE, 8), SENTINEL).bfloat16()
    vc = torch.full((n_pages, KVH, Dh, PAGE), SENTINEL).bfloat16()
    d = torch.arange(Dh)
    kwant = kref.float().bfloat16()
    for t in written.tolist():
        page, off = int(slot[t]) // PAGE, int(slot[t]) % PAGE
        for h in range(KVH):
            kc[page, h, d // 8, off, d % 8] = kwant[t, h, d]
            vc[page, h, d, off] = v[t, h, d]
    wmask = torch.zeros(n_pages, PAGE, dtype=torch.bool)
    wmask[slot[written] // PAGE, slot[written] % PAGE] = True
    return types.SimpleNamespace(
        kind=kind, D=Dh, rope=rope, append=append, tables=tables, qkv=buf,
        cos=cos, sin=sin, index=index, kc=kc, vc=vc, wmask=wmask,
        qref=qref, kref=kref, qmag=mag(q), kmag=mag(k), n_pages=n_pages)


def check_writer(fn, case, to_dev, keeps_k=True):
    """fn: the writer with its own signature.  Exact tables: caches (and
    the rotated q) bit for bit.  Real tables: written K and q under the
    rope bound, everything else bit for bit."""
    Dh, KVH = case.D, W_KVH
    buf = to_dev(case.qkv.clone())
    q, k, v = qkv_views(buf, W_QH, KVH, Dh)
    kc = to_dev(torch.full_like(case.kc, SENTINEL))
    vc = to_dev(torch.full_like(case.vc, SENTINEL))
    ix = case.index
    tail = (to_dev(ix["bt"]), to_dev(ix["sl"])) if case.append \
        else ((to_dev(ix["pos"]),) if case.rope else ()) + \
        (to_dev(ix["slots"]),)
    T = ix["slots"].numel() if not case.append else q.shape[0]
    if case.rope:
        fn(q, k, v, kc, vc, to_dev(case.cos), to_dev(case.sin), *tail)
    else:
        fn(k[:T], v[:T], kc, vc, *tail)
    q0, k0, v0 = qkv_views(case.qkv, W_QH, KVH, Dh)
    kc, vc, what = kc.cpu(), vc.cpu(), case.kind
    assert_bits_equal(vc, case.vc, f"{what}: V cache")
    assert_bits_equal(v.cpu(), v0, f"{what}: v rows")
    if keeps_k:
        assert_bits_equal(k.cpu(), k0, f"{what}: k rows")
    if case.tables == "quarter":
        assert_bits_equal(kc, case.kc, f"{what}: K cache")
        assert_bits_equal(q.cpu(), case.qref.float().bfloat16(),
                          f"{what}: q rows")
        return
    # real tables: the untouched slots bit for bit, the written ones bounded
    logical = lambda c: c.permute(0, 3, 1, 2, 4).reshape(
        case.n_pages, PAGE, KVH, Dh)
    got, want = logical(kc), logical(case.kc)
    assert_bits_equal(got[~case.wmask], want[~case.wmask],
                      f"{what}: unwritten K slots")
    slot = ix["slots"].long() if not case.append else None
    if case.append:
        sl = ix["sl"].long()
        rows = torch.arange(sl.numel())[sl > 0]
        pos = sl[rows] - 1
        slot_w = ix["bt"].long()[rows, pos >> 6] * PAGE + (pos & 63)
    else:
        rows, slot_w = torch.arange(slot.numel()), slot
    assert_rope_bound(got[slot_w // PAGE, slot_w % PAGE], case.kref[rows],
                      case.kmag[rows], f"{what}: written K")
    assert_rope_bound(q.cpu(), case.qref, case.qmag, f"{what}: q rows")


# ---------------------------------------------------------------------------
# torch models of the kernels (f32, bf16 P, the kernels' decomposition)
# ---------------------------------------------------------------------------

MUTANTS = ("nvalid_plus_1", "nvalid_minus_1", "causal_lt", "start_ignored",
           "split_last_page_dropped", "alpha_other_row", "merge_unweighted",
           "merge_empty_split", "k_dims_swapped", "v_not_transposed",
           "h_mod_kvh", "bt_next_row", "pad_rows_stored", "append_after_read")


def _online(qc, kc, vc, kvh, pages, live, nvalid, pos0, qabs, row_ok, causal,
            scale, mut):
    """Online softmax of U work units x 16 columns over their page lists:
    qsa_mask_scale, qsa_page_update and the PV product.  -> m, l, o."""
    U, NP = pages.shape
    Dh = qc.shape[-1]
    m = torch.full((U, 16), NEG)
    l = torch.zeros(U, 16)
    o = torch.zeros(U, 16, Dh)
    kpos = torch.arange(PAGE)
    for j in range(NP):
        lv = live[:, j]
        if not lv.any():
            continue
        kraw, vraw = kc[pages[:, j], kvh], vc[pages[:, j], kvh]
        if mut == "k_dims_swapped":
            kp = kraw.reshape(U, 8, PAGE, Dh // 8).permute(0, 2, 3, 1)
        else:
            kp = kraw.permute(0, 2, 1, 3)
        kp = kp.reshape(U, PAGE, Dh).float()
        vp = vraw.reshape(U, PAGE, Dh) if mut == "v_not_transposed" \
            else vraw.transpose(1, 2)
        s = torch.einsum("ucd,upd->ucp", qc, kp) * scale
        ok = (kpos < nvalid[:, j, None, None]) & row_ok[:, :, None] & \
            lv[:, None, None]
        if causal:
            kabs = pos0[:, j, None, None] + kpos
            ok = ok & ((kabs < qabs[:, :, None]) if mut == "causal_lt"
                       else (kabs <= qabs[:, :, None]))
        s = torch.where(ok, s, torch.tensor(NEG))
        pmax = s.amax(-1)
        upd = (lv & (pmax > NEG).any(1))[:, None]   # wave-uniform page skip
        m_new = torch.maximum(m, pmax)
        alpha = torch.where(m <= NEG, torch.zeros(()), torch.exp(m - m_new))
        p = torch.where(s > -1.0e38, torch.exp(s - m_new[..., None]),
                        torch.zeros(()))
        a_o = alpha.roll(1, 1) if mut == "alpha_other_row" else alpha
        l_new = l * alpha + p.sum(-1)
        o_new = o * a_o[..., None] + p.bfloat16().float() @ vp.float()
        m = torch.where(upd, m_new, m)
        l = torch.where(upd, l_new, l)
        o = torch.where(upd[..., None], o_new, o)
    return m, l, o


def model_decode(q, kc, vc, bt, sl, scale, ns=None, mut=None):
    """qsa_paged_attn_mfma + qsa_attn_reduce (and, in arithmetic, the fused
    kernel's loop and merge)."""
    B, QH, Dh = q.shape
    KVH, W = kc.shape[1], bt.shape[1]
    R = QH // KVH
    NS = ns or decode_num_splits(B, KVH, W)
    n = sl.long()
    npages = (n + PAGE - 1) // PAGE
    chunk = (npages + NS - 1) // NS
    b_i, k_i, s_i = (x.reshape(-1) for x in torch.meshgrid(
        torch.arange(B), torch.arange(KVH), torch.arange(NS), indexing="ij"))
    p0 = s_i * chunk[b_i]
    p1 = torch.minimum(npages[b_i], p0 + chunk[b_i])
    alive = (n[b_i] > 0) & (p0 < npages[b_i])
    if mut == "split_last_page_dropped":
        p1 = torch.where(p1 - p0 > 1, p1 - 1, p1)
    pi = p0[:, None] + torch.arange(max(int(chunk.max()), 1))
    live = alive[:, None] & (pi < p1[:, None])
    row = (b_i + 1) % B if mut == "bt_next_row" else b_i
    pages = bt.long()[row[:, None], pi.clamp(max=W - 1)]
    dn = {"nvalid_plus_1": 1, "nvalid_minus_1": -1}.get(mut, 0)
    nvalid = (n[b_i, None] + dn - PAGE * pi).clamp(max=PAGE)
    col = torch.arange(16).clamp(max=R - 1)
    head = (col * KVH + k_i[:, None]) if mut == "h_mod_kvh" \
        else (k_i[:, None] * R + col)
    qc = q.float()[b_i[:, None], head]
    one = torch.ones(b_i.numel(), 16, dtype=torch.bool)
    m, l, o = _online(qc, kc, vc, k_i, pages, live, nvalid, PAGE * pi, None,
                      one, False, scale, mut)
    # a split with no page leaves its o slot unwritten
    o = torch.where(alive[:, None, None], o, torch.tensor(float("nan")))
    m, l = m.view(B, KVH, NS, 16), l.view(B, KVH, NS, 16)
    o = o.view(B, KVH, NS, 16, Dh)
    take = torch.ones_like(l, dtype=torch.bool) \
        if mut == "merge_empty_split" else l > 0
    M = torch.where(take, m, torch.tensor(NEG)).amax(2, keepdim=True)
    w = torch.ones_like(m) if mut == "merge_unweighted" else torch.exp(m - M)
    wo = w[..., None] * o
    if mut != "merge_empty_split":
        w = torch.where(take, w, torch.zeros(()))
        wo = torch.where(take[..., None], wo, torch.zeros(()))
    L = (w * l).sum(2)
    val = torch.where(L[..., None] > 0, wo.sum(2) / L[..., None],
                      torch.zeros(())).bfloat16()           # [B, KVH, 16, D]
    out = torch.zeros(B, QH, Dh, dtype=torch.bfloat16)
    for kv in reversed(range(KVH)):
        if mut == "h_mod_kvh":
            out[:, torch.arange(R) * KVH + kv] = val[:, kv, :R]
            continue
        hi = min(QH, kv * R + (16 if mut == "pad_rows_stored" else R))
        out[:, kv * R:hi] = val[:, kv, :hi - kv * R]
    return out


def model_fused(q, k, v, kc, vc, cos, sin, bt, sl, scale, ns=None, mut=None):
    """qsa_paged_attn_mfma_fused: f32 rotation, append, then the read."""
    B, KVH, Dh = k.shape
    n = sl.long()
    act = n > 0
    pos = (n - 1).clamp(min=0)
    c, s = cos[pos][:, None], sin[pos][:, None]
    half = Dh // 2

    def rot(x):
        x0, x1 = x[..., :half].float(), x[..., half:].float()
        return torch.cat([x0 * c - x1 * s, x0 * s + x1 * c], -1).bfloat16()

    qr = torch.where(act[:, None, None], rot(q), q)
    kr = rot(k)

    def append():
        rows = torch.arange(B)[act]
        page = bt.long()[rows, pos[rows] >> 6]
        off = pos[rows] & 63
        kc[page, :, :, off, :] = kr[rows].view(-1, KVH, Dh // 8, 8)
        vc[page, :, :, off] = v[rows]

    if mut == "append_after_read":
        out = model_decode(qr, kc, vc, bt, sl, scale, ns)
        append()
        return out
    append()
    return model_decode(qr, kc, vc, bt, sl, scale, ns, mut)


def model_prefill(q, kc, vc, bt, map_item, map_pos0, item_off, item_start,
                  item_len, scale, causal, rows=16, mut=None):
    """qsa_paged_attn_prefill on the 16-row blocks of the maps (the tiled
    kernel's sub-tiles are those blocks)."""
    T, QH, Dh = q.shape
    KVH, W = kc.shape[1], bt.shape[1]
    R = QH // KVH
    sub = rows // 16
    item = map_item.long().repeat_interleave(sub)
    pos0 = (map_pos0.long()[:, None] + 16 * torch.arange(sub)).reshape(-1)
    keep = pos0 < item_len.long()[item]     # a block past the end has no rows
    item, pos0 = item[keep], pos0[keep]
    qb_i, h_i = (x.reshape(-1) for x in torch.meshgrid(
        torch.arange(item.numel()), torch.arange(QH), indexing="ij"))
    it, p0 = item[qb_i], pos0[qb_i]
    n_i, off = item_len.long()[it], item_off.long()[it]
    st = torch.zeros_like(n_i) if mut == "start_ignored" \
        else item_start.long()[it]
    r = p0[:, None] + torch.arange(16)
    row_ok = r < n_i[:, None]
    qc = q.float()[off[:, None] + torch.minimum(r, n_i[:, None] - 1),
                   h_i[:, None]]
    max_abs = st + (torch.minimum(p0 + 15, n_i - 1) if causal else n_i - 1)
    npg = max_abs // PAGE + 1
    pi = torch.arange(int(npg.max()))[None, :].expand(qb_i.numel(), -1)
    live = pi < npg[:, None]
    row = (it + 1) % bt.shape[0] if mut == "bt_next_row" else it
    pages = bt.long()[row[:, None], pi.clamp(max=W - 1)]
    dn = {"nvalid_plus_1": 1, "nvalid_minus_1": -1}.get(mut, 0)
    nvalid = (max_abs[:, None] + 1 + dn - PAGE * pi).clamp(max=PAGE)
    kvh = h_i % KVH if mut == "h_mod_kvh" else h_i // R
    m, l, o = _online(qc, kc, vc, kvh, pages, live, nvalid, PAGE * pi,
                      st[:, None] + r, row_ok, causal, scale, mut)
    inv = torch.where(l > 0, 1.0 / l, torch.zeros(()))
    val = (o * inv[..., None]).bfloat16()                   # [U, 16, D]
    out = torch.zeros(T, QH, Dh, dtype=torch.bfloat16)
    dest = off[:, None] + r
    if mut == "pad_rows_stored":
        for u in reversed(range(qb_i.numel())):
            ok = dest[u] < T
            out[dest[u][ok], h_i[u]] = val[u][ok]
    else:
        out[dest[row_ok], h_i[:, None].expand(-1, 16)[row_ok]] = val[row_ok]
    return out.view(T, QH * Dh)


# ---------------------------------------------------------------------------
# CPU tests
# ---------------------------------------------------------------------------

def test_case_tables_match_the_bit_identity_suites():
    import test_gpu_decode_fused as F
    import test_gpu_prefill_tiled as P
    assert LENS == F._LENS
    assert ITEMS[:len(P.ITEMS)] == P.ITEMS
    assert TILED_SHAPES == P.TILED_SHAPES
    for s, n in ((0, 5), (0, 31), (0, 32), (0, 63), (60, 16), (127, 2),
                 (128, 64)):
        assert (s, n) in ITEMS
    assert {(p, QH // KVH) for p, _, QH, KVH in DECODE_CASES} == \
        {(p, r) for p in _PATHS for r in (1, 4, 7, 16)}
    assert {(p, d) for p, d, _, _ in DECODE_CASES} == \
        {(p, d) for p in _PATHS for d in (64, 128)}


def test_cache_layout_is_the_index_formula():
    """build_cache lays K and V out with a permute; element by element that
    is kc[page, kvh, d // 8, pos % 64, d % 8] and vc[page, kvh, d, pos % 64]."""
    c = build_cache(64, 2, [130, 5], 4, 1)
    for seq, t in ((0, 0), (0, 63), (0, 64), (0, 129), (1, 4)):
        page, off = int(c.bt[seq, t >> 6]), t & 63
        for kvh in range(2):
            k = [float(c.kc[page, kvh, d // 8, off, d % 8]) for d in range(64)]
            assert k[t & 7] == 1 and k[8 + ((t >> 3) & 7)] == 1
            assert k[16 + (t >> 6)] == 1 and sum(k[:32]) == 3
            assert (k[TRAP_DIM], k[PG_DIM], k[OFF_DIM]) == (0, t >> 6, off)
            assert torch.equal(k_rows(c, torch.tensor(seq), torch.tensor(kvh),
                                      torch.tensor(t)).float(),
                               torch.tensor(k))
            v = torch.stack([c.vc[page, kvh, d, off] for d in range(64)])
            assert torch.equal(v, v_rows(c, torch.tensor(seq),
                                         torch.tensor(kvh), torch.tensor(t)))
    # stale slots, the idle tail pages and the unused entries are traps
    page = int(c.bt[1, 0])
    assert (c.kc[page, :, TRAP_DIM // 8, 5:, TRAP_DIM % 8] == 1).all()
    assert (c.vc[page, :, :, 5:] == TRAP_V).all()
    for page in c.bt[1, 1:].tolist():
        assert (c.vc[page] == TRAP_V).all()


@pytest.mark.parametrize("spec", DECODE_CASES, ids=case_id)
def test_decode_exact(spec):
    case = decode_case(*spec)
    # the single targets of a length class are distinct positions
    tg, n = case.tg, case.sl.long().repeat_interleave(case.QH)
    one = (case.mode == CODE) & ((tg >= 0).sum(1) == 1)
    for length, count in case.singles.items():
        got = tg[one & (n == length), 0].unique().numel()
        assert got == min(count, length), (length, count, got)
    check_decode(D.paged_attn_decode, case, _ident)
    check_decode(model_decode, case, _ident)


@pytest.mark.parametrize("tables", ("identity", "quarter"))
@pytest.mark.parametrize("spec", DECODE_CASES, ids=case_id)
def test_fused_exact(spec, tables):
    case = fused_case(*spec, tables)
    check_fused(D.decode_attn_fused, case, _ident, keeps_qkv=False)
    check_fused(model_fused, case, _ident)


PREFILL_EXACT = [(d, qh, kvh) for d, qh, kvh, _ in TILED_SHAPES[:2] +
                 TILED_SHAPES[3:]] + [FALLBACK_SHAPE[:3]] + ONE_WAVE_SHAPES


@pytest.mark.parametrize("causal", (True, False))
@pytest.mark.parametrize("shape", sorted(set(PREFILL_EXACT)), ids=case_id)
def test_prefill_exact(shape, causal):
    case = prefill_case(*shape, causal)
    check_prefill(model_prefill, case, 16, _ident)
    tiled = functools.partial(model_prefill, rows=32)
    check_prefill(tiled, case, 32, _ident)


@pytest.mark.parametrize("spec", GAUSS_DECODE, ids=case_id)
def test_decode_gauss(spec):
    check_gauss_decode(D.paged_attn_decode, gauss_decode_case(*spec), _ident)
    check_gauss_decode(model_decode, gauss_decode_case(*spec), _ident)
    check_gauss_fused(model_fused, gauss_fused_case(*spec), _ident)


@pytest.mark.parametrize("causal", (True, False))
@pytest.mark.parametrize("shape", [(128, 8, 2), (64, 8, 2), (128, 28, 4)],
                         ids=case_id)
def test_prefill_gauss(shape, causal):
    check_gauss_prefill(model_prefill, gauss_prefill_case(*shape, causal), 16,
                        _ident)


CPU_WRITER = {"kv_append": D.kv_append, "rope_kv_append": D.rope_kv_append,
              "kv_scatter": D.kv_scatter, "rope_kv_scatter": D.rope_kv_scatter}


def writer_specs():
    for kind in WRITERS:
        for Dh in (64, 128):
            for T in ([0] if kind.endswith("append") else SCATTER_T):
                yield kind, Dh, T


@pytest.mark.parametrize("spec", list(writer_specs()), ids=case_id)
def test_writers_exact(spec):
    # the CPU paths rotate k in place, the kernels leave it alone
    check_writer(CPU_WRITER[spec[0]], writer_case(*spec, "quarter"), _ident,
                 keeps_k=False)


@pytest.mark.parametrize("kind,T", (("rope_kv_append", 0),
                                    ("rope_kv_scatter", 65)))
@pytest.mark.parametrize("Dh", (64, 128))
def test_rope_writers_gauss(kind, Dh, T):
    check_writer(CPU_WRITER[kind], writer_case(kind, Dh, T, "real"), _ident,
                 keeps_k=False)


# ---- mutants -----------------------------------------------------------------

@functools.lru_cache(maxsize=1)
def _mutant_decode_case():
    """All of LENS in one 24-row batch; the model takes NS as an argument."""
    Dh, QH, KVH = 64, 8, 2
    c = build_cache(Dh, KVH, LENS, 32, 6000)
    mode, tg, _ = decode_targets(LENS, QH)
    seq = torch.arange(len(LENS)).repeat_interleave(QH)
    kvh = (torch.arange(QH) // (QH // KVH)).repeat(len(LENS))
    plant_int_v(c, seq, kvh, tg, 6001)
    return types.SimpleNamespace(
        D=Dh, QH=QH, KVH=KVH, lens=LENS, cache=c,
        q=make_q(Dh, mode, tg).view(-1, QH, Dh),
        expected=expect_rows(c, seq, kvh, tg).view(-1, QH, Dh),
        sl=torch.tensor(LENS, dtype=torch.int32))


def _mutant_checks():
    """(name, mutants it can see, check(mut))."""
    dec = ("nvalid_plus_1", "nvalid_minus_1", "split_last_page_dropped",
           "alpha_other_row", "merge_unweighted", "merge_empty_split",
           "k_dims_swapped", "v_not_transposed", "h_mod_kvh", "bt_next_row",
           "pad_rows_stored")
    pre = ("nvalid_plus_1", "nvalid_minus_1", "causal_lt", "start_ignored",
           "alpha_other_row", "k_dims_swapped", "v_not_transposed",
           "h_mod_kvh", "bt_next_row", "pad_rows_stored")
    for ns in (1, 4, 11):
        yield f"decode ns={ns}", dec, lambda mut, ns=ns: check_decode(
            functools.partial(model_decode, ns=ns, mut=mut),
            _mutant_decode_case(), _ident)
    yield "fused", dec + ("append_after_read",), lambda mut: check_fused(
        functools.partial(model_fused, mut=mut),
        fused_case("part", 128, 8, 2, "quarter"), _ident)
    for causal in (True, False):
        yield f"prefill causal={causal}", pre, lambda mut, causal=causal: \
            check_prefill(functools.partial(model_prefill, mut=mut),
                          prefill_case(64, 8, 2, causal), 16, _ident)
    yield "decode gauss", dec, lambda mut: check_gauss_decode(
        functools.partial(model_decode, mut=mut),
        gauss_decode_case(64, 8, 2, 8), _ident)


def test_checks_reject_mutants():
    """Every check passes the correct model; every mutant is rejected by at
    least one exact check."""
    caught = {mut: [] for mut in MUTANTS}
    for name, sees, check in _mutant_checks():
        check(None)
        for mut in sees:
            try:
                check(mut)
            except AssertionError:
                caught[mut].append(name)
    for mut, by in caught.items():
        print(f"mutant {mut}: rejected by {', '.join(by)}")
        assert [b for b in by if "gauss" not in b], mut
