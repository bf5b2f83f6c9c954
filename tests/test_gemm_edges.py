"""Exact-arithmetic and edge cases of the three weight-streaming GEMMs
(ops/hip/skinny_gemm.hip, skinny_gemm_fp8.hip, gemm_fp8_batch.hip).

This module holds the case tables, the input builders (fixed seeds, built on
the CPU), float64 references and the check_*(fn, ..., to_dev) functions.  Its
own tests run every case through the CPU paths of ops.dispatch;
tests/test_gpu_gemm_edges.py runs the same cases and assertions through the
HIP kernels.

Four kinds of case:

* exact integers.  Activations are integers in [-4, 4], weights integers in
  [-8, 8] plus one +-448 per fp8 row, scales powers of two.  Every product
  and every partial sum is an integer below 2^24, so f32 accumulation is
  exact in any order and under any rounding inside an MFMA step; the single
  rounding left is the bf16 store.  Compared bit for bit.
* one-hot read-out.  a[m, k_m] = 1 selects w[n, k_m]: one exact product plus
  zeros.  Pins the packed layout, the lane mapping and the dequantisation of
  every finite e4m3 code.  Compared bit for bit.
* Gaussian data against a float64 product, with the per-element bound
      |out - ref| <= 2^-8 |ref| + K 2^-22 S,   S = |a| |w|^T.
  2^-8 |ref| is the half-ulp of the one bf16 store; K 2^-22 S bounds an f32
  sum of <= 2K terms at unit roundoff 2^-23 (twice the nearest-even figure,
  since the rounding inside an MFMA step is not documented).
* row-strided activations: a view into a wider buffer, bit-equal to the
  contiguous result.

test_checks_reject_mutants hands the checks deliberately wrong CPU
implementations and expects every one to be rejected.
"""

import functools
import os
import re
import types

import pytest
import torch

from quickstart_streaming_agents_amd.ops import dispatch as D


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _ident(t):
    return t


def spec_id(spec):
    return "-".join(str(v) for v in spec if v is not None)


def bits16(t):
    return t.detach().cpu().contiguous().view(torch.int16)


def assert_bits_equal(got, want, what):
    """got == want as bf16 bit patterns; reports the first differing (m, n)."""
    got = got.detach().cpu()
    assert got.dtype == torch.bfloat16 and got.shape == want.shape, \
        f"{what}: got {got.dtype} {tuple(got.shape)}"
    diff = bits16(got) != bits16(want)
    if diff.any():
        m, n = (int(v) for v in diff.nonzero()[0])
        raise AssertionError(
            f"{what}: {int(diff.sum())} of {diff.numel()} outputs differ; "
            f"first at (m={m}, n={n}): got {got[m, n].item()!r} "
            f"(0x{bits16(got)[m, n].item() & 0xffff:04x}) expected "
            f"{want[m, n].item()!r} (0x{bits16(want)[m, n].item() & 0xffff:04x})")


# ---------------------------------------------------------------------------
# weights
# ---------------------------------------------------------------------------

def channel_scales(N):
    """s[n] = 2^((5n mod 8) - 6): neighbouring channels differ by a power of
    two, so an output scaled with a neighbour's s[n] is wrong by >= 2x."""
    e = ((5 * torch.arange(N)) % 8 - 6).int()
    return torch.ldexp(torch.ones(N), e)


def pack_codes(q8):
    """[N, K] e4m3 codes -> the fp8 fragment-pair-major stream of
    ops/hip/gemm_core.h.  Needs only K % 64 == 0, which
    D.pack_weight_fp8 (K % 256 == 0) does not offer; fp8_weight asserts the
    two agree byte for byte wherever both apply."""
    n, k = q8.shape
    return q8.view(torch.uint8).reshape(n // 16, 16, k // 64, 2, 4, 8) \
        .permute(0, 2, 1, 4, 3, 5).contiguous()


def fp8_weight(q, s):
    """q: f32 [N, K] of e4m3 values with +-448 in every row; s: power-of-two
    scales.  -> (packed stream, w = q * s as bf16).  The pack is exact: the
    row maximum is 448 * 2^j, so pack_weight_fp8 must return s and the codes
    of q bit for bit, and unpack_weight_fp8 must return w."""
    N, K = q.shape
    assert (q.abs().amax(dim=1) == 448).all()
    wf = q * s[:, None]
    w = wf.bfloat16()
    assert torch.equal(w.float(), wf), "q * s not exact in bf16"
    q8 = q.to(torch.float8_e4m3fn)
    assert torch.equal(q8.float(), q), "q not exact in e4m3"
    neg0 = (q == 0) & torch.signbit(q)
    assert torch.equal(q8.view(torch.uint8)[neg0],
                       torch.full((int(neg0.sum()),), 0x80, dtype=torch.uint8))
    qf = pack_codes(q8)
    if K % 256 == 0:
        qf_d, s_d = D.pack_weight_fp8(w)
        assert torch.equal(s_d.view(torch.int32), s.view(torch.int32)), \
            "pack_weight_fp8: scale not exact"
        assert torch.equal(qf_d, qf), "pack_weight_fp8: codes differ"
    wd = D.unpack_weight_fp8(qf, s, N, K)
    assert torch.equal(wd, wf) and \
        torch.equal(bits16(wd.bfloat16()), bits16(w)), \
        "unpack_weight_fp8 not exact"
    return qf, w


def unpack_frag(wf, n, k):
    """Inverse of pack_weight_frag."""
    return wf.reshape(n // 16, k // 32, 16, 32).permute(0, 2, 1, 3) \
        .reshape(n, k)


# ---------------------------------------------------------------------------
# 1. exact-integer cases
# ---------------------------------------------------------------------------

# above this many multiply-adds the float64 reference product runs where
# to_dev puts it (integers: any correct float64 matmul gives the same bits)
REF_ON_CPU_MACS = 1 << 30

SKINNY_ROWS = 32
# K = 256: one chunk, only wave 0 works; K = 2304: 9 chunks over 8 waves,
# wave 0 runs twice; N = 6144: many workgroups
SKINNY_SHAPES = ((16, 256), (48, 2304), (6144, 512))
SKINNY_M = (1, 15, 16, 17, 31, 32)
BF16_ALIGNED = 40                       # see int_bf16_case

FP8_ROWS = 64
FP8_M_ALL = (1, 16, 17, 32, 33, 49, 64)   # both sides of every m-tile edge
FP8_M_FEW = (17, 64)                      # one per m-tile variant
# (N, K, launcher class, M)
FP8_SHAPES = (
    (16, 256, "wo", FP8_M_ALL),
    (48, 2304, "wo", FP8_M_ALL),
    (32, 8192, "wdown", FP8_M_FEW),
    (6144, 256, "qkv", FP8_M_FEW),
    (6176, 2304, "qkv", FP8_M_FEW),       # N / 32 odd
    (16384, 256, "wgu", FP8_M_FEW),
    (16448, 768, "wgu", FP8_M_FEW),       # N / 64 odd
    (65536, 768, "lm_head", FP8_M_FEW),   # WAVES = 2: three chunks, two waves
)

FP8_IDS = tuple(f"{n}x{k}-{c}" for n, k, c, _ in FP8_SHAPES)

BATCH_ROWS = 256
# every <M_FRAGS, SPLITK, NT> the batch launcher instantiates
# (test_batch_table_covers_every_instantiation reads the list back from
# gemm_fp8_batch.hip)
BATCH_TRIPLES = tuple((mf, sk, nt) for nt in (2, 1) for sk in (1, 2, 4)
                      for mf in (4, 8, 12, 16) if not (nt == 2 and mf == 16))
# first row count that needs this M_FRAGS (33: first past the skinny
# kernels' 32 rows), and its last
BATCH_M = {4: (33, 64), 8: (65, 128), 12: (129, 192), 16: (193, 256)}
BATCH_EXTRA = ((1, 64, 64, 1), (256, 256, 1024, 4))


def batch_select(M, N):
    """(M_FRAGS, NT) that qsa_gemm_fp8_batch_launch picks."""
    mf = (M + 15) // 16
    nt = 2 if N % 128 == 0 and mf <= 12 else 1
    return min(f for f in (4, 8, 12, 16) if f >= mf), nt


def batch_cases(mf, sk, nt):
    """(M, N, K, splitk) cases of one instantiation: first and last row
    count; one k-block per split (the prologue runs alone) and three (both
    LDS buffers, odd parity at the end)."""
    if nt == 2:
        ns = (128,)
    else:               # N = 128 goes to NT = 1 only at M_FRAGS = 16
        ns = (192, 128) if mf == 16 else (192,)
    return [(M, N, K, sk) for N in ns for M in BATCH_M[mf]
            for K in (64 * sk, 192 * sk)]


def _seed(*key):
    h = 17
    for v in key:
        h = (h * 1000003 + int(v)) % (1 << 31)
    return h


@functools.lru_cache(maxsize=None)
def int_fp8_case(N, K, rows, variant=0):
    """Integer fp8 case: a [rows, K] bf16, packed weights, scales and the
    integer codes.  The exactness of the pack is asserted here.  variant
    > 0: other data of the same recipe (one per expert of a grouped
    case)."""
    g = _gen(_seed(1, N, K) if variant == 0 else _seed(1, N, K, variant))
    a = torch.randint(-4, 5, (rows, K), generator=g).bfloat16()
    q = torch.randint(-8, 9, (N, K), generator=g).to(torch.int16)
    col = torch.randint(0, K, (N,), generator=g)
    sign = torch.randint(0, 2, (N,), generator=g).to(torch.int16) * 2 - 1
    q[torch.arange(N), col] = 448 * sign
    s = channel_scales(N)
    if variant:         # another power-of-two pattern per variant
        s = torch.roll(s, variant % 8) * 2.0 ** -(variant // 8)
    qf, _ = fp8_weight(q.float(), s)
    return types.SimpleNamespace(kind="fp8", N=N, K=K, a=a, qf=qf, s=s, q=q,
                                 refs={})


@functools.lru_cache(maxsize=None)
def int_bf16_case(N, K, rows, variant=0):
    """Integer bf16 case (variant: as in int_fp8_case).
    Uniform integers alone leave most outputs below
    256, where every integer is a bf16 number and the store rounds nothing
    (the fp8 cases have their +-448 for this).  So BF16_ALIGNED seeded
    columns hold a = p[k] * {3, 4} and w = c[n] * p[k] * {6, 7, 8} with
    seeded signs p, c: their products add up to about +-980 per output,
    which needs 10 or 11 bits."""
    g = _gen(_seed(2, N, K) if variant == 0 else _seed(2, N, K, variant))
    a = torch.randint(-4, 5, (rows, K), generator=g).to(torch.int16)
    q = torch.randint(-8, 9, (N, K), generator=g).to(torch.int16)
    cols = torch.randperm(K, generator=g)[:BF16_ALIGNED]
    p = torch.randint(0, 2, (BF16_ALIGNED,), generator=g) * 2 - 1
    c = torch.randint(0, 2, (N, 1), generator=g) * 2 - 1
    a[:, cols] = (p * torch.randint(3, 5, (rows, BF16_ALIGNED),
                                    generator=g)).to(torch.int16)
    q[:, cols] = (c * p * torch.randint(6, 9, (N, BF16_ALIGNED),
                                        generator=g)).to(torch.int16)
    assert a.abs().max() <= 4 and q.abs().max() <= 8
    a = a.bfloat16()
    wf = D.pack_weight_frag(q.bfloat16())
    assert torch.equal(unpack_frag(wf, N, K), q.bfloat16())
    return types.SimpleNamespace(kind="bf16", N=N, K=K, a=a, wf=wf, q=q,
                                 s=torch.ones(N), refs={})


def exact_ref(case, to_dev=_ident):
    """(max |acc|, exact outputs as f32 [rows, N]) of an integer case:
    (a.double() @ q.double().T) * s.double().  acc is an integer below 2^24
    and s a power of two, so the product is exact in f32 as well.  Computed
    once per case."""
    rows = case.a.shape[0]
    on_cpu = rows * case.N * case.K <= REF_ON_CPU_MACS
    put = _ident if on_cpu else to_dev
    key = "cpu" if on_cpu else put(case.s).device.type
    if key not in case.refs:
        acc = put(case.a).double() @ put(case.q).double().T
        v = acc * put(case.s).double()
        v32 = v.float()
        assert torch.equal(v32.double(), v)
        case.refs[key] = (float(acc.abs().max()), v32.cpu())
    return case.refs[key]


def assert_sharp(acc_max, v32, what):
    """The conditions that make an integer case sharp; v32: exact outputs."""
    assert acc_max < 2 ** 24, f"{what}: max |acc| {acc_max}"
    if v32.numel() < 1024:
        return
    low = v32.contiguous().view(torch.int32) & 0xffff
    ties = float((low == 0x8000).float().mean())
    inexact = float((low != 0).float().mean())
    assert ties >= 0.05, f"{what}: only {ties:.1%} round-to-even ties"
    assert inexact >= 0.50, f"{what}: only {inexact:.1%} inexact in bf16"


def activations(a, to_dev=_ident, strided=False):
    """a on the device; strided: as the view buf[:, 32:32+K] of a
    [M, K+64] buffer (16-byte aligned, lda = K + 64) whose margins hold 3."""
    if not strided:
        return to_dev(a.contiguous())
    M, K = a.shape
    buf = torch.full((M, K + 64), 3.0, dtype=torch.bfloat16)
    buf[:, 32:32 + K] = a
    view = to_dev(buf)[:, 32:32 + K]
    assert view.stride(0) == K + 64 and view.data_ptr() % 16 == 0
    return view


def weight_args(case, to_dev=_ident):
    if case.kind == "bf16":
        return (to_dev(case.wf), case.N, case.K)
    return (to_dev(case.qf), to_dev(case.s), case.N, case.K)


def check_exact(fn, case, ms, to_dev=_ident, strided=False, extra=()):
    """fn(a[:M], *weights, *extra) is bit-equal to the exact product rounded
    once to bf16 with round-to-nearest-even, for every M in ms."""
    acc_max, v32 = exact_ref(case, to_dev)
    wargs = weight_args(case, to_dev)
    for M in ms:
        what = f"{case.kind} M={M} N={case.N} K={case.K} extra={extra}" \
            + (" strided" if strided else "")
        assert_sharp(acc_max, v32[:M], what)
        out = fn(activations(case.a[:M], to_dev, strided), *wargs, *extra)
        assert_bits_equal(out, v32[:M].bfloat16(), what)
        if strided:
            cont = fn(activations(case.a[:M], to_dev), *wargs, *extra)
            assert_bits_equal(out, cont.cpu(), what + " vs contiguous")


@pytest.mark.parametrize("N,K", SKINNY_SHAPES)
def test_skinny_gemm_exact_cpu(N, K):
    check_exact(D.skinny_linear, int_bf16_case(N, K, SKINNY_ROWS), SKINNY_M)


@pytest.mark.parametrize("N,K,cls,ms", FP8_SHAPES, ids=FP8_IDS)
def test_skinny_gemm_fp8_exact_cpu(N, K, cls, ms):
    assert D.skinny_fp8_class(N, K) == cls
    check_exact(D.skinny_linear_fp8, int_fp8_case(N, K, FP8_ROWS), ms)


def check_batch_exact(fn, cases, to_dev=_ident, strided=False):
    for M, N, K, sk in cases:
        check_exact(fn, int_fp8_case(N, K, BATCH_ROWS), (M,), to_dev,
                    strided, extra=(sk,))


@pytest.mark.parametrize("mf,sk,nt", BATCH_TRIPLES)
def test_gemm_fp8_batch_exact_cpu(mf, sk, nt):
    check_batch_exact(D.gemm_fp8_batch, batch_cases(mf, sk, nt))


def test_gemm_fp8_batch_exact_extra_cpu():
    check_batch_exact(D.gemm_fp8_batch, BATCH_EXTRA)


def test_batch_table_covers_every_instantiation():
    """The case table reaches each of the launcher's instantiations, under
    its selection rule, and BATCH_TRIPLES is the launcher's own list."""
    src = os.path.join(os.path.dirname(D.__file__), "hip",
                       "gemm_fp8_batch.hip")
    with open(src) as f:
        listed = re.findall(r"QSA_CASE\((\d+), (\d+), (\d+)\)", f.read())
    assert sorted(tuple(int(v) for v in t) for t in listed) == \
        sorted(BATCH_TRIPLES)
    assert len(BATCH_TRIPLES) == 21
    reached = set()
    for mf, sk, nt in BATCH_TRIPLES:
        for M, N, K, splitk in batch_cases(mf, sk, nt):
            assert batch_select(M, N) == (mf, nt), (M, N)
            assert splitk == sk and N % 64 == 0 and K % (64 * sk) == 0
            assert K // sk in (64, 192)
            reached.add(batch_select(M, N)[:1] + (splitk,) +
                        batch_select(M, N)[1:])
    assert reached == set(BATCH_TRIPLES)
    assert batch_select(1, 64) == (4, 1) and batch_select(256, 256) == (16, 1)


# ---------------------------------------------------------------------------
# 4. row-strided activations
# ---------------------------------------------------------------------------

STRIDED_SKINNY = (48, 2304, 17)             # (N, K, M)
STRIDED_FP8 = (48, 2304, 49)
STRIDED_BATCH = ((129, 128, 384, 2), (193, 192, 768, 4))   # with split-K


def check_strided(fn, kind, to_dev=_ident):
    """One integer case per kernel through the view buf[:, 32:32+K]:
    bit-equal to the reference and to the contiguous result."""
    if kind == "bf16":
        N, K, M = STRIDED_SKINNY
        check_exact(fn, int_bf16_case(N, K, SKINNY_ROWS), (M,), to_dev, True)
    elif kind == "fp8":
        N, K, M = STRIDED_FP8
        check_exact(fn, int_fp8_case(N, K, FP8_ROWS), (M,), to_dev, True)
    else:
        check_batch_exact(fn, STRIDED_BATCH, to_dev, True)


CPU_FN = {"bf16": D.skinny_linear, "fp8": D.skinny_linear_fp8,
          "batch": D.gemm_fp8_batch}


@pytest.mark.parametrize("kind", sorted(CPU_FN))
def test_strided_activations_cpu(kind):
    check_strided(CPU_FN[kind], kind)


# ---------------------------------------------------------------------------
# 2. one-hot read-out
# ---------------------------------------------------------------------------

READOUT_K = 256
# (kind, N, M, launches, splitk): M * launches == K, every k is read once
READOUT_FP8 = (("fp8", 32, 64, 4, None), ("fp8", 32, 32, 8, None),
               ("batch", 64, 256, 1, 1), ("batch", 64, 256, 1, 2),
               ("batch", 64, 256, 1, 4))
READOUT_BF16 = ("bf16", 32, 32, 8, None)


def e4m3_finite_codes():
    """The 254 finite e4m3 codes in code order: both zeros, all denormals,
    +-448; 0x7f and 0xff (NaN) left out."""
    c = torch.arange(256, dtype=torch.int32)
    return c[(c & 0x7f) != 0x7f].to(torch.uint8)


@functools.lru_cache(maxsize=None)
def readout_case(kind, N):
    K = READOUT_K
    if kind == "bf16":
        # finite, normal bf16 patterns (exponent field 1..254): how an MFMA
        # treats bf16 denormals is not specified in what we have
        g = _gen(_seed(3, N))
        bits = torch.randint(0, 1 << 16, (N, K), generator=g,
                             dtype=torch.int32)
        exp = torch.randint(1, 255, (N, K), generator=g, dtype=torch.int32)
        bits = (bits & 0x807f) | (exp << 7)
        w = bits.to(torch.int16).view(torch.bfloat16)
        assert torch.isfinite(w.float()).all() and (w.float() != 0).all()
        return types.SimpleNamespace(kind=kind, N=N, K=K, w=w,
                                     wf=D.pack_weight_frag(w))
    codes = e4m3_finite_codes()
    assert codes.numel() == 254
    idx = (37 * torch.arange(N)[:, None] + torch.arange(K)[None, :]) % 254
    q = codes[idx].view(torch.float8_e4m3fn).float()
    for n in range(N):              # every row holds every finite code
        assert torch.unique(idx[n]).numel() == 254
    s = channel_scales(N)
    qf, w = fp8_weight(q, s)
    return types.SimpleNamespace(kind="fp8", N=N, K=K, w=w, qf=qf, s=s)


def check_readout(fn, spec, to_dev=_ident):
    """out[m, n] == w[n, k_m] bit for bit where a[m, k_m] = 1 is the only
    non-zero of row m.  A zero weight reads out as +0: the sum of +0 and -0
    terms is +0 in round-to-nearest (the -0 code itself is pinned by the
    exact pack / unpack assertions of fp8_weight)."""
    kind, N, M, launches, splitk = spec
    case = readout_case("bf16" if kind == "bf16" else "fp8", N)
    K = case.K
    assert M * launches == K
    wargs = weight_args(case, to_dev)
    extra = () if splitk is None else (splitk,)
    for L in range(launches):
        km = L * M + torch.arange(M)
        a = torch.zeros(M, K, dtype=torch.bfloat16)
        a[torch.arange(M), km] = 1.0
        want = case.w[:, km].T.contiguous()
        want = torch.where(want == 0, torch.zeros_like(want), want)
        out = fn(to_dev(a), *wargs, *extra)
        assert_bits_equal(out, want, f"read-out {spec} launch {L}")


@pytest.mark.parametrize("spec", READOUT_FP8 + (READOUT_BF16,), ids=spec_id)
def test_readout_cpu(spec):
    check_readout(CPU_FN[spec[0]], spec)


# ---------------------------------------------------------------------------
# 3. Gaussian cases with the derived bound
# ---------------------------------------------------------------------------

# (kind, M, N, K, splitk).  fp8: one per launcher class; bf16: the three
# shapes; batch: six spanning M_FRAGS, SPLITK and NT.
GAUSS_CASES = (
    ("bf16", 32, 16, 256, None), ("bf16", 32, 48, 2304, None),
    ("bf16", 32, 6144, 512, None),
    ("fp8", 64, 48, 2304, None), ("fp8", 64, 32, 8192, None),
    ("fp8", 64, 6176, 2304, None), ("fp8", 64, 16448, 768, None),
    ("fp8", 17, 65536, 768, None),
    ("batch", 33, 128, 256, 4), ("batch", 65, 192, 768, 1),
    ("batch", 128, 192, 1024, 2), ("batch", 129, 128, 768, 2),
    ("batch", 192, 128, 768, 1), ("batch", 256, 128, 1024, 4),
)


@functools.lru_cache(maxsize=None)
def gauss_case(kind, M, N, K):
    """Today's distributions: a ~ 0.5 N(0,1), w ~ 0.02 N(0,1), bf16."""
    g = _gen(_seed(4, M, N, K))
    a = (torch.randn(M, K, generator=g) * 0.5).bfloat16()
    w = (torch.randn(N, K, generator=g) * 0.02).bfloat16()
    if kind == "bf16":
        return types.SimpleNamespace(kind="bf16", N=N, K=K, a=a, w=w,
                                     wf=D.pack_weight_frag(w), refs={})
    qf, s = D.pack_weight_fp8(w)
    return types.SimpleNamespace(kind="fp8", N=N, K=K, a=a, qf=qf, s=s,
                                 refs={})


def gauss_ref(case, to_dev=_ident):
    """(float64 product with the dequantised weights, S = |a| |w|^T), on
    the CPU, computed once where to_dev puts the operands."""
    key = to_dev(case.a).device.type
    if key not in case.refs:
        if case.kind == "bf16":
            w = to_dev(case.w).double()
        else:
            # q * s in f64: exact
            ones = torch.ones_like(case.s)
            w = to_dev(D.unpack_weight_fp8(case.qf, ones, case.N, case.K)) \
                .double() * to_dev(case.s).double()[:, None]
        a = to_dev(case.a).double()
        case.refs[key] = ((a @ w.T).cpu(), (a.abs() @ w.abs().T).cpu())
    return case.refs[key]


def gauss_ratio(out, ref, S, K):
    """max over the outputs of |out - ref| / (2^-8 |ref| + K 2^-22 S);
    where the bound is 0 (an all-zero row) the output must be exact."""
    out = out.detach().cpu().double()
    err = (out - ref).abs()
    bound = 2.0 ** -8 * ref.abs() + K * 2.0 ** -22 * S
    ratio = torch.where(bound > 0, err / bound.clamp(min=1e-300),
                        torch.where(err == 0, 0.0, float("inf")))
    return float(ratio.max())


def check_gauss(fn, spec, to_dev=_ident):
    kind, M, N, K, splitk = spec
    case = gauss_case("bf16" if kind == "bf16" else "fp8", M, N, K)
    ref, S = gauss_ref(case, to_dev)
    extra = () if splitk is None else (splitk,)
    out = fn(to_dev(case.a), *weight_args(case, to_dev), *extra)
    assert out.shape == (M, N) and out.dtype == torch.bfloat16
    assert torch.isfinite(out.float()).all(), f"gauss {spec}: not finite"
    ratio = gauss_ratio(out, ref, S, K)
    print(f"gauss {spec}: worst err/bound {ratio:.3f}")
    assert ratio <= 1.0, f"gauss {spec}: err/bound {ratio:.3f}"
    return ratio


@pytest.mark.parametrize("spec", GAUSS_CASES, ids=spec_id)
def test_gauss_cpu(spec):
    check_gauss(CPU_FN[spec[0]], spec)


# ---------------------------------------------------------------------------
# 5. a batch row's bits do not depend on the other rows
# ---------------------------------------------------------------------------

BATCH_INVARIANCE = tuple((N, sk) for N in (128, 192) for sk in (1, 4))


def check_batch_row_invariance(fn, N, splitk, to_dev=_ident):
    """The first 33 rows of an M = 64 result against the M = 33 result
    (both M_FRAGS = 4), Gaussian data."""
    case = gauss_case("fp8", 64, N, 768)
    assert batch_select(33, N)[0] == batch_select(64, N)[0] == 4
    wargs = weight_args(case, to_dev)
    out64 = fn(to_dev(case.a), *wargs, splitk)
    out33 = fn(to_dev(case.a[:33].contiguous()), *wargs, splitk)
    assert_bits_equal(out33, out64[:33].cpu(),
                      f"batch rows N={N} splitk={splitk}")


@pytest.mark.parametrize("N,splitk", BATCH_INVARIANCE)
def test_batch_row_invariance_cpu(N, splitk):
    check_batch_row_invariance(D.gemm_fp8_batch, N, splitk)


# ---------------------------------------------------------------------------
# 7. pack edge cases
# ---------------------------------------------------------------------------

PACK_EDGE_N, PACK_EDGE_K, PACK_EDGE_M = 64, 256, 33
PACK_ZERO_ROW, PACK_NEG_ROW = 5, 22


@functools.lru_cache(maxsize=None)
def pack_edge_case():
    """Gaussian weights with one all-zero row and one row whose largest
    magnitude is negative."""
    g = _gen(_seed(5))
    a = (torch.randn(PACK_EDGE_M, PACK_EDGE_K, generator=g) * 0.5).bfloat16()
    w = (torch.randn(PACK_EDGE_N, PACK_EDGE_K, generator=g) * 0.02).bfloat16()
    w[PACK_ZERO_ROW] = 0
    w[PACK_NEG_ROW] = -w[PACK_NEG_ROW].abs()
    w[PACK_NEG_ROW, 77] = -0.25             # the row's only extreme
    assert w[PACK_NEG_ROW].float().abs().max() == 0.25
    return a, w


def check_pack_edges(fns, to_dev=_ident):
    """fns: {"fp8": skinny fn, "batch": batch fn}.  The pack runs where
    to_dev puts the weights."""
    a, w = pack_edge_case()
    N, K = w.shape
    qf, s = D.pack_weight_fp8(to_dev(w))
    assert qf.device == to_dev(w).device
    s_c = s.cpu()
    assert torch.isfinite(s_c).all() and (s_c > 0).all()
    wd = D.unpack_weight_fp8(qf.cpu(), s_c, N, K)
    assert (wd[PACK_ZERO_ROW] == 0).all()
    # -max quantises to -448 and comes back as the bf16 value it was
    codes = D.unpack_weight_fp8(qf.cpu(), torch.ones(N), N, K)
    assert codes[PACK_NEG_ROW, 77] == -448 and \
        (codes[PACK_NEG_ROW] <= 0).all()
    assert wd[PACK_NEG_ROW, 77].bfloat16() == w[PACK_NEG_ROW, 77]
    a64 = a.double()
    ref = a64 @ wd.double().T
    S = a64.abs() @ wd.double().abs().T
    for kind, extra in (("fp8", ()), ("batch", (1,)), ("batch", (2,))):
        out = fns[kind](to_dev(a), qf, s, N, K, *extra)
        assert torch.isfinite(out.float()).all()
        assert (out[:, PACK_ZERO_ROW] == 0).all(), \
            f"{kind}: all-zero weight row gives non-zero outputs"
        assert gauss_ratio(out, ref, S, K) <= 1.0, kind
    return qf, s


def test_pack_edges_cpu():
    check_pack_edges(CPU_FN)


# ---------------------------------------------------------------------------
# 6. the checks are sharp: deliberately wrong implementations
# ---------------------------------------------------------------------------

MUTANTS = ("truncating_store", "next_scale", "swapped_k_halves",
           "dropped_last_chunk", "row_from_16_above", "dropped_last_split",
           "flushed_denormals")


def model_gemm(kind, mutant=None):
    """A CPU implementation with the call surface of `kind`'s kernel:
    f32 products per split, summed, scaled, one bf16 store -- and, if
    `mutant` names one, that defect."""
    def fn(a, *rest):
        if kind == "bf16":
            wf, n, k = rest
            q, s, splitk = unpack_frag(wf, n, k).float(), torch.ones(n), 1
        else:
            qf, s, n, k = rest[:4]
            splitk = rest[4] if kind == "batch" else 1
            q = D.unpack_weight_fp8(qf, torch.ones(n), n, k)
        q, a = q.clone(), a.float()
        if mutant == "flushed_denormals":       # e4m3 denormals: < 2^-6
            q[q.abs() < 2.0 ** -6] = 0
        if mutant == "swapped_k_halves":        # of the last 64-k block
            b = k - 64
            q[:, b:b + 64] = torch.cat([q[:, b + 32:b + 64], q[:, b:b + 32]],
                                       dim=1)
        if mutant == "dropped_last_chunk":
            q[:, k - 256:] = 0
        if mutant == "row_from_16_above" and a.shape[0] > 16:
            a = torch.cat([a[:16], a[:-16]])
        if mutant == "next_scale":
            s = torch.roll(s, -1)
        per = k // splitk
        splits = splitk - 1 if mutant == "dropped_last_split" else splitk
        acc = torch.zeros(a.shape[0], n)
        for i in range(splits):
            acc += a[:, i * per:(i + 1) * per] @ q[:, i * per:(i + 1) * per].T
        v = acc * s
        if mutant == "truncating_store":
            return (v.view(torch.int32) >> 16).to(torch.int16) \
                .view(torch.bfloat16)
        return v.bfloat16()
    return fn


def _mutant_checks():
    """(name, kind, check taking fn) of the integer and read-out checks."""
    return (
        ("integer", "bf16", lambda fn: check_exact(
            fn, int_bf16_case(48, 2304, SKINNY_ROWS), (32,))),
        ("integer", "fp8", lambda fn: check_exact(
            fn, int_fp8_case(48, 2304, FP8_ROWS), (64,))),
        ("integer", "batch", lambda fn: check_batch_exact(
            fn, (BATCH_EXTRA[1],))),
        ("read-out", "bf16", lambda fn: check_readout(fn, READOUT_BF16)),
        ("read-out", "fp8", lambda fn: check_readout(fn, READOUT_FP8[0])),
        ("read-out", "batch", lambda fn: check_readout(fn, READOUT_FP8[4])),
    )


def mutant_applies(mutant, check, kind):
    """Whether the defect changes what `check` looks at."""
    if mutant == "truncating_store":
        return check == "integer"       # read-out values are exact in bf16
    if mutant == "flushed_denormals":   # integer codes are normal numbers
        return check == "read-out" and kind != "bf16"
    if mutant == "next_scale":
        return kind != "bf16"
    if mutant == "dropped_last_split":
        return kind == "batch"
    return True


def test_checks_reject_mutants():
    """Every check passes the correct model and rejects every mutant that
    applies to it; each mutant is rejected by at least one integer or
    read-out check."""
    caught = {m: [] for m in MUTANTS}
    for name, kind, check in _mutant_checks():
        check(model_gemm(kind))
        for mutant in MUTANTS:
            if not mutant_applies(mutant, name, kind):
                continue
            with pytest.raises(AssertionError):
                check(model_gemm(kind, mutant))
            caught[mutant].append(f"{name}/{kind}")
    for mutant, by in caught.items():
        print(f"mutant {mutant}: rejected by {', '.join(by)}")
        assert by, mutant
    assert any(c.startswith("read-out") for c in caught["flushed_denormals"])
    assert all(any(c.startswith("integer") for c in caught[m])
               for m in MUTANTS if m != "flushed_denormals")
