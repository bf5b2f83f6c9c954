"""Exact-arithmetic and edge cases of the weight-streaming GEMM kernels:
the cases, references and assertions of test_gemm_edges.py, run through the
qsa_hip extension on the GPU, plus what only exists there -- the host checks
that refuse bad arguments before a launch, and the bit-invariance of the fp8
skinny kernel under its TILES and MT template parameters."""

import pytest
import torch

import test_gemm_edges as E
from quickstart_streaming_agents_amd.ops import dispatch as D

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def to_dev(t):
    return t.to(DEV)


@pytest.fixture(scope="module")
def ext():
    from quickstart_streaming_agents_amd.ops import ext as get_ext
    return get_ext()


@pytest.fixture(scope="module")
def fns(ext):
    return {"bf16": ext.skinny_gemm, "fp8": ext.skinny_gemm_fp8,
            "batch": ext.gemm_fp8_batch}


# ---- exact integers --------------------------------------------------------

@pytest.mark.parametrize("N,K", E.SKINNY_SHAPES)
def test_skinny_gemm_exact(ext, N, K):
    E.check_exact(ext.skinny_gemm, E.int_bf16_case(N, K, E.SKINNY_ROWS),
                  E.SKINNY_M, to_dev)


@pytest.mark.parametrize("N,K,cls,ms", E.FP8_SHAPES, ids=E.FP8_IDS)
def test_skinny_gemm_fp8_exact(ext, N, K, cls, ms):
    E.check_exact(ext.skinny_gemm_fp8, E.int_fp8_case(N, K, E.FP8_ROWS), ms,
                  to_dev)


@pytest.mark.parametrize("mf,sk,nt", E.BATCH_TRIPLES)
def test_gemm_fp8_batch_exact(ext, mf, sk, nt):
    E.check_batch_exact(ext.gemm_fp8_batch, E.batch_cases(mf, sk, nt), to_dev)


def test_gemm_fp8_batch_exact_extra(ext):
    E.check_batch_exact(ext.gemm_fp8_batch, E.BATCH_EXTRA, to_dev)


@pytest.mark.parametrize("kind", sorted(E.CPU_FN))
def test_strided_activations(fns, kind):
    E.check_strided(fns[kind], kind, to_dev)


# ---- one-hot read-out ------------------------------------------------------

@pytest.mark.parametrize("spec", E.READOUT_FP8 + (E.READOUT_BF16,),
                         ids=E.spec_id)
def test_readout(fns, spec):
    E.check_readout(fns[spec[0]], spec, to_dev)


# ---- Gaussian data ---------------------------------------------------------

@pytest.mark.parametrize("spec", E.GAUSS_CASES, ids=E.spec_id)
def test_gauss(fns, spec):
    E.check_gauss(fns[spec[0]], spec, to_dev)


# ---- invariance ------------------------------------------------------------

INV_N, INV_K = 128, 2304


def test_skinny_fp8_bits_do_not_depend_on_tiles_or_mt(ext):
    """For WAVES = 8 a row's bits are the same under every (TILES, MT), and
    the production launcher (wo class: 8 waves, 1 tile) gives those bits."""
    case = E.gauss_case("fp8", 64, INV_N, INV_K)
    assert D.skinny_fp8_class(INV_N, INV_K) == "wo"
    a = to_dev(case.a)
    wargs = E.weight_args(case, to_dev)
    base = ext.skinny_gemm_fp8_probe_mt(a, *wargs, 8, 1, 4).cpu()
    for tiles in (1, 2, 4):
        for mt in (2, 4):
            rows = 16 * mt
            out = ext.skinny_gemm_fp8_probe_mt(a[:rows], *wargs, 8, tiles, mt)
            E.assert_bits_equal(out, base[:rows],
                                f"probe waves=8 tiles={tiles} mt={mt}")
    for rows in (32, 64):
        E.assert_bits_equal(ext.skinny_gemm_fp8(a[:rows], *wargs),
                            base[:rows], f"production launcher M={rows}")


@pytest.mark.parametrize("N,splitk", E.BATCH_INVARIANCE)
def test_batch_row_invariance(ext, N, splitk):
    E.check_batch_row_invariance(ext.gemm_fp8_batch, N, splitk, to_dev)


# ---- pack edge cases -------------------------------------------------------

def test_pack_edges(fns):
    """Zero row and negative-maximum row, packed on the device."""
    qf, s = E.check_pack_edges(fns, to_dev)
    assert qf.is_cuda and s.is_cuda


@pytest.mark.parametrize("which", ("integer", "read-out"))
def test_device_pack_of_exact_data_matches_cpu_bytes(which):
    """q * 2^j with +-448 in every row has no rounding ties: the device
    pack is byte-identical to the CPU pack, scales included."""
    case = E.int_fp8_case(48, 2304, E.FP8_ROWS) if which == "integer" \
        else E.readout_case("fp8", 32)
    N, K = case.N, case.K
    w = D.unpack_weight_fp8(case.qf, case.s, N, K).bfloat16()
    qf, s = D.pack_weight_fp8(to_dev(w))
    assert qf.is_cuda
    assert torch.equal(s.cpu().view(torch.int32), case.s.view(torch.int32))
    assert torch.equal(qf.cpu(), case.qf)


# ---- host checks: every one raises before any launch -----------------------

@pytest.fixture(scope="module")
def small(ext):
    """Small valid operands of each kernel on the device."""
    bf = E.int_bf16_case(16, 256, E.SKINNY_ROWS)
    f8 = E.int_fp8_case(64, 256, E.BATCH_ROWS)
    return {
        "bf16": (ext.skinny_gemm, to_dev(bf.a),
                 (to_dev(bf.wf), 16, 256), ()),
        "fp8": (ext.skinny_gemm_fp8, to_dev(f8.a[:32].contiguous()),
                (to_dev(f8.qf), to_dev(f8.s), 64, 256), ()),
        "batch": (ext.gemm_fp8_batch, to_dev(f8.a),
                  (to_dev(f8.qf), to_dev(f8.s), 64, 256), (1,)),
    }


KINDS = ("bf16", "fp8", "batch")


@pytest.mark.parametrize("kind", KINDS)
def test_valid_small_operands_run(small, kind):
    fn, a, wargs, extra = small[kind]
    assert fn(a, *wargs, *extra).shape == (a.shape[0], wargs[-2])


@pytest.mark.parametrize("kind", KINDS)
def test_rejects_cpu_weight_stream(small, kind):
    fn, a, wargs, extra = small[kind]
    with pytest.raises(RuntimeError, match="must be on the GPU"):
        fn(a, wargs[0].cpu(), *wargs[1:], *extra)


@pytest.mark.parametrize("kind", KINDS)
def test_rejects_misaligned_activations(small, kind):
    fn, a, wargs, extra = small[kind]
    M, K = a.shape
    buf = torch.zeros(M, K + 8, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(RuntimeError, match="16-byte"):     # base + 2 bytes
        fn(buf[:, 1:1 + K], *wargs, *extra)
    odd = torch.zeros(M, K + 4, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(RuntimeError, match="16-byte"):     # stride % 8 != 0
        fn(odd[:, :K], *wargs, *extra)


def test_skinny_gemm_rejects_33_rows(small):
    fn, a, wargs, _ = small["bf16"]
    a33 = torch.cat([a, a[:1]])
    with pytest.raises(RuntimeError, match=r"M in \[1,32\]"):
        fn(a33, *wargs)


def test_gemm_fp8_batch_rejects_bad_shapes(small):
    fn, a, (qf, s, N, K), _ = small["batch"]
    a257 = torch.cat([a, a[:1]])
    with pytest.raises(RuntimeError, match=r"M in \[1,256\]"):
        fn(a257, qf, s, N, K, 1)
    with pytest.raises(RuntimeError, match="splitk"):
        fn(a, qf, s, N, K, 3)
    a192 = a[:, :192].contiguous()
    with pytest.raises(RuntimeError, match="splitk"):      # 192 % 128 != 0
        fn(a192, qf[:, :3].contiguous(), s, N, 192, 2)
    qf96 = torch.zeros(96 * K, dtype=torch.uint8, device=DEV)
    s96 = torch.ones(96, device=DEV)
    with pytest.raises(RuntimeError, match="N % 64"):
        fn(a, qf96, s96, 96, K, 1)


def test_skinny_kernels_reject_n_not_multiple_of_16(small):
    fn, a, (wf, _, K), _ = small["bf16"]
    wf24 = torch.zeros(24 * K, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(RuntimeError, match="N%16"):
        fn(a, wf24, 24, K)
    fn, a, (qf, s, _, K), _ = small["fp8"]
    qf24 = torch.zeros(24 * K, dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError, match="N%16"):
        fn(a, qf24, torch.ones(24, device=DEV), 24, K)


# ---- probes get the production checks and more ------------------------------

def test_probes_reject_before_launch(ext, small):
    """Every call raises in the host checks; none reaches a launch."""
    _, a, (qf, s, N, K), _ = small["fp8"]
    _, a16, (wf, N16, K16), _ = small["bf16"]
    assert (a.shape[0], N, K) == (32, 64, 256)
    for probe, cfg in ((ext.skinny_gemm_fp8_probe, (3, 1, 0)),
                       (ext.skinny_gemm_fp8_probe, (8, 2, 1)),
                       (ext.skinny_gemm_fp8_probe_mt, (3, 1, 2)),
                       (ext.skinny_gemm_fp8_probe_mt, (8, 1, 3))):
        with pytest.raises(RuntimeError, match="not instantiated"):
            probe(a, qf, s, N, K, *cfg)
    with pytest.raises(RuntimeError, match="not instantiated"):
        ext.skinny_gemm_probe(a16, wf, N16, K16, 8, 0, 1)
    for probe, last in ((ext.skinny_gemm_fp8_probe, 0),
                        (ext.skinny_gemm_fp8_probe_mt, 2)):
        with pytest.raises(RuntimeError, match=r"N%\(16\*tiles\)"):
            probe(a, qf, s, N, K, 8, 8, last)       # 64 % 128 != 0
        with pytest.raises(RuntimeError, match="must be on the GPU"):
            probe(a, qf.cpu(), s, N, K, 8, 1, last)
    a33 = torch.cat([a, a[:1]])
    with pytest.raises(RuntimeError, match=r"M in \[1,32\]"):
        ext.skinny_gemm_fp8_probe(a33, qf, s, N, K, 8, 1, 0)
    with pytest.raises(RuntimeError, match=r"M in \[1,32\]"):
        ext.skinny_gemm_fp8_probe_mt(a33, qf, s, N, K, 8, 1, 2)
    with pytest.raises(RuntimeError, match="must be on the GPU"):
        ext.skinny_gemm_probe(a16, wf.cpu(), N16, K16, 8, 0, 0)


# ---- one class function, one loop -------------------------------------------

CLASS_GRID = tuple((N, K)
                   for N in (6128, 6144, 16368, 16384, 16448, 65408, 65536)
                   for K in (256, 7936, 8192))


def test_skinny_fp8_class_agrees(ext):
    """The launcher's class function and its CPU-only copy in ops.dispatch,
    on the case table and across every class boundary.  No launch."""
    for N, K, cls, _ in E.FP8_SHAPES:
        assert ext.skinny_fp8_class(N, K) == cls
    for N, K in tuple(s[:2] for s in E.FP8_SHAPES) + CLASS_GRID:
        assert ext.skinny_fp8_class(N, K) == D.skinny_fp8_class(N, K), (N, K)
    assert {D.skinny_fp8_class(N, K) for N, K in CLASS_GRID} == \
        {"lm_head", "wgu", "qkv", "wo", "wdown"}


def test_bf16_and_fp8_skinny_are_one_loop(ext):
    """fp8 weights with unit scales, and the same weights dequantised to
    bf16 (exact) on the fragment-major pack: both kernels run 8 waves here
    (class wo), so they add the same products in the same order and the
    outputs are bit-equal."""
    case = E.gauss_case("fp8", 32, 48, 2304)
    N, K = case.N, case.K
    assert D.skinny_fp8_class(N, K) == "wo"
    ones = torch.ones(N)
    w32 = D.unpack_weight_fp8(case.qf, ones, N, K)
    w = w32.bfloat16()
    assert torch.equal(w.float(), w32)
    wf, qf, s1 = to_dev(D.pack_weight_frag(w)), to_dev(case.qf), to_dev(ones)
    for M in (1, 17, 32):
        a = to_dev(case.a[:M].contiguous())
        E.assert_bits_equal(ext.skinny_gemm_fp8(a, qf, s1, N, K),
                            ext.skinny_gemm(a, wf, N, K).cpu(),
                            f"fp8 vs bf16 skinny M={M}")
