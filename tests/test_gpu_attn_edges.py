"""Exact read-out and edge cases of the paged-attention kernels and the
KV-cache writers: the cases, expectations and assertions of
test_attn_edges.py, run through the qsa_hip extension on the GPU
(paged_attn_decode, decode_attn_fused at both waves_per_simd,
paged_attn_prefill, paged_attn_prefill_tiled at 32 and 64 rows and through
its fallback at R = 7, and the four writers), plus what only exists there:
the host checks of ops.cpp that refuse bad arguments before a launch, and the
empty batches that return without one.  No case compares a HIP kernel with
another HIP kernel; the tolerances are the ones derived in
test_attn_edges.py."""

import pytest
import torch

import test_attn_edges as E

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def to_dev(t):
    return t.to(DEV)


@pytest.fixture(scope="module")
def ext():
    from quickstart_streaming_agents_amd.ops import ext as get_ext
    return get_ext()


def _fused(ext, wps):
    return lambda *a: ext.decode_attn_fused(*a, wps)


def _tiled(ext, rows):
    return lambda *a: ext.paged_attn_prefill_tiled(*a, rows)


# ---- exact read-out ----------------------------------------------------------

@pytest.mark.parametrize("spec", E.DECODE_CASES, ids=E.case_id)
def test_decode_exact(ext, spec):
    E.check_decode(ext.paged_attn_decode, E.decode_case(*spec), to_dev)


@pytest.mark.parametrize("wps", (1, 2))
@pytest.mark.parametrize("tables", ("identity", "quarter"))
@pytest.mark.parametrize("spec", E.DECODE_CASES, ids=E.case_id)
def test_fused_exact(ext, spec, tables, wps):
    E.check_fused(_fused(ext, wps), E.fused_case(*spec, tables), to_dev)


@pytest.mark.parametrize("causal", (True, False))
@pytest.mark.parametrize("shape", E.ONE_WAVE_SHAPES, ids=E.case_id)
def test_prefill_one_wave_exact(ext, shape, causal):
    E.check_prefill(ext.paged_attn_prefill, E.prefill_case(*shape, causal),
                    16, to_dev)


@pytest.mark.parametrize("causal", (True, False))
@pytest.mark.parametrize("Dh,QH,KVH,rows",
                         E.TILED_SHAPES + [E.FALLBACK_SHAPE])
def test_prefill_tiled_exact(ext, Dh, QH, KVH, rows, causal):
    """The last shape (R = 7) runs the one-wave kernel through the tiled
    binding's fallback, with 16-row blocks past the items' ends."""
    E.check_prefill(_tiled(ext, rows), E.prefill_case(Dh, QH, KVH, causal),
                    rows, to_dev)


# ---- Gaussian data under the derived bound -----------------------------------

@pytest.mark.parametrize("spec", E.GAUSS_DECODE, ids=E.case_id)
def test_decode_gauss(ext, spec):
    E.check_gauss_decode(ext.paged_attn_decode, E.gauss_decode_case(*spec),
                         to_dev)


@pytest.mark.parametrize("wps", (1, 2))
@pytest.mark.parametrize("spec", E.GAUSS_DECODE, ids=E.case_id)
def test_fused_gauss(ext, spec, wps):
    """Real rope tables: the appended k row under the rope bound, the
    output under the attention bound."""
    E.check_gauss_fused(_fused(ext, wps), E.gauss_fused_case(*spec), to_dev)


@pytest.mark.parametrize("causal", (True, False))
@pytest.mark.parametrize("shape", E.ONE_WAVE_SHAPES, ids=E.case_id)
def test_prefill_one_wave_gauss(ext, shape, causal):
    E.check_gauss_prefill(ext.paged_attn_prefill,
                          E.gauss_prefill_case(*shape, causal), 16, to_dev)


@pytest.mark.parametrize("causal", (True, False))
@pytest.mark.parametrize("Dh,QH,KVH,rows",
                         E.TILED_SHAPES[:3] + [E.FALLBACK_SHAPE])
def test_prefill_tiled_gauss(ext, Dh, QH, KVH, rows, causal):
    E.check_gauss_prefill(_tiled(ext, rows),
                          E.gauss_prefill_case(Dh, QH, KVH, causal), rows,
                          to_dev)


# ---- writers ------------------------------------------------------------------

@pytest.mark.parametrize("spec", list(E.writer_specs()), ids=E.case_id)
def test_writers_exact(ext, spec):
    E.check_writer(getattr(ext, spec[0]), E.writer_case(*spec, "quarter"),
                   to_dev)


@pytest.mark.parametrize("kind,T", (("rope_kv_append", 0),
                                    ("rope_kv_scatter", 65)))
@pytest.mark.parametrize("Dh", (64, 128))
def test_rope_writers_gauss(ext, kind, Dh, T):
    E.check_writer(getattr(ext, kind), E.writer_case(kind, Dh, T, "real"),
                   to_dev)


# ---- host checks: every one raises before any launch --------------------------

ARGS = {
    "paged_attn_decode": ("q", "kc", "vc", "bt", "sl"),
    "decode_attn_fused": ("q", "k", "v", "kc", "vc", "cos", "sin", "bt", "sl"),
    "kv_append": ("k", "v", "kc", "vc", "bt", "sl"),
    "rope_kv_append": ("q", "k", "v", "kc", "vc", "cos", "sin", "bt", "sl"),
    "kv_scatter": ("k", "v", "kc", "vc", "slots"),
    "rope_kv_scatter": ("q", "k", "v", "kc", "vc", "cos", "sin", "pos",
                        "slots"),
    "paged_attn_prefill": ("pq", "kc", "vc", "pbt", "item", "pos0", "off",
                           "start", "len"),
    "paged_attn_prefill_tiled": ("pq", "kc", "vc", "pbt", "titem", "tpos0",
                                 "off", "start", "len"),
}
TAIL = {"paged_attn_decode": (1.0,), "decode_attn_fused": (1.0, 1),
        "paged_attn_prefill": (1.0, True),
        "paged_attn_prefill_tiled": (1.0, True, 32)}
B_, QH_, KVH_, D_, T_ = 2, 8, 2, 64, 20


@pytest.fixture(scope="module")
def small():
    """Small valid operands on the device, shared by all bindings."""
    i32 = lambda x: torch.tensor(x, dtype=torch.int32, device=DEV)
    buf = torch.ones(B_, (QH_ + 2 * KVH_) * D_, dtype=torch.bfloat16,
                     device=DEV)
    q, k, v = E.qkv_views(buf, QH_, KVH_, D_)
    return dict(
        q=q, k=k, v=v,
        kc=torch.zeros(6, KVH_, D_ // 8, 64, 8, dtype=torch.bfloat16,
                       device=DEV),
        vc=torch.zeros(6, KVH_, D_, 64, dtype=torch.bfloat16, device=DEV),
        cos=torch.ones(128, D_ // 2, device=DEV),
        sin=torch.zeros(128, D_ // 2, device=DEV),
        bt=i32([[0, 1], [2, 3]]), sl=i32([5, 70]), slots=i32([7, 200]),
        pos=i32([3, 4]),
        pq=torch.ones(T_, QH_, D_, dtype=torch.bfloat16, device=DEV),
        pbt=i32([[4, 5]]), item=i32([0, 0]), pos0=i32([0, 16]),
        titem=i32([0]), tpos0=i32([0]), off=i32([0]), start=i32([0]),
        len=i32([T_]))


def _misaligned(t):
    """The same [rows, heads, D] view one element into a wider buffer."""
    n, h, d = t.shape
    buf = torch.ones(n, h * d + 8, dtype=t.dtype, device=t.device)
    return buf[:, 1:1 + h * d].view(n, h, d)


def _misaligned_kv(k, v):
    """k and v views of one buffer, as the bindings require, one element
    off a 16-byte boundary."""
    n, h, d = k.shape
    buf = torch.ones(n, 2 * h * d + 8, dtype=k.dtype, device=k.device)
    return (buf[:, 1:1 + h * d].view(n, h, d),
            buf[:, 1 + h * d:1 + 2 * h * d].view(n, h, d))


HOW = {
    "cpu": lambda t: t.cpu(),
    "f32": lambda t: t.float(),
    "bf16": lambda t: t.bfloat16(),
    "i64": lambda t: t.long(),
    "longer": lambda t: torch.cat([t, t[:1]]),
    "more_heads": lambda t: torch.cat([t, t[:, :1]], dim=1),
    "misaligned": _misaligned,
    "strided": lambda t: torch.cat([t, t], dim=-1)[..., ::2],
    "flat": lambda t: t.reshape(t.shape[0], t.shape[1], 64, -1),
    "d32": lambda t: t[..., :32].contiguous(),
    "wider": lambda t: torch.cat([t, t], dim=1),
}

ATTN = ("paged_attn_decode", "decode_attn_fused", "paged_attn_prefill",
        "paged_attn_prefill_tiled")
WRITE = ("kv_append", "rope_kv_append", "kv_scatter", "rope_kv_scatter")
DECODE = ("paged_attn_decode", "decode_attn_fused", "kv_append",
          "rope_kv_append")
PREFILL = ATTN[2:]


def _rows():
    """(binding, argument, what is wrong with it, message fragment)."""
    for name, args in ARGS.items():
        for a in args:                      # every tensor on q's device
            yield name, a, "cpu", "must be on the GPU"
        yield name, "kc", "f32", "kc must be bf16"
        yield name, "vc", "f32", "vc must be bf16"
        yield name, "kc", "flat", "K cache layout"
        yield name, "vc", "more_heads", "same pages and kv heads"
        yield name, "vc", "longer", "same pages and kv heads"
        yield name, "vc", "d32", "V cache layout"
        first = args[0]
        yield name, first, "f32", "must be bf16"
        yield name, first, "strided", "contiguous heads"
    for name in ATTN:
        yield name, ARGS[name][0], "misaligned", "16-byte"
    for name in ("decode_attn_fused", "rope_kv_scatter"):
        yield name, "k", "misaligned_kv", "16-byte"
    for name in WRITE:
        # D = 32 rows against a D = 64 cache: refused on D itself
        yield name, ("q" if name.startswith("rope") else "k"), "d32", \
            "D must be 64/128"
    for name in DECODE:
        yield name, "sl", "longer", "seq_lens must have"
        yield name, "sl", "i64", "seq_lens must be i32"
        yield name, "bt", "longer", "block_table must be"
        yield name, "bt", "i64", "must be i32"
    for name in ("decode_attn_fused", "rope_kv_append", "rope_kv_scatter"):
        yield name, "cos", "wider", "rope tables"
        yield name, "sin", "bf16", "must be f32"
        yield name, "v", "more_heads", "k/v must be"
    for name in ("kv_scatter", "rope_kv_scatter"):
        yield name, "slots", "i64", "slots must be i32"
    yield "kv_scatter", "slots", "longer", "slots must have"
    yield "rope_kv_scatter", "slots", "longer", "slots longer than"
    yield "rope_kv_scatter", "pos", "longer", "pos must have"
    for name in PREFILL:
        yield name, "pbt", "longer", "block_table must be"
        for a in ("off", "start"):
            yield name, a, "longer", f"item_{a} must have"
        yield name, ARGS[name][5], "longer", "pos0 map must have"
        yield name, "len", "i64", "item_len must be i32"


@pytest.mark.parametrize("name", sorted(ARGS))
def test_valid_small_operands_run(ext, small, name):
    out = getattr(ext, name)(*(small[a].clone() for a in ARGS[name]),
                             *TAIL.get(name, ()))
    torch.cuda.synchronize()
    if name in ATTN:
        assert not torch.isnan(out.float()).any()


@pytest.mark.parametrize("name,arg,how,fragment", list(_rows()),
                         ids=lambda v: str(v).replace(" ", "_"))
def test_rejects_before_launch(ext, small, name, arg, how, fragment):
    bad = dict(small)
    if how == "misaligned_kv":
        bad["k"], bad["v"] = _misaligned_kv(small["k"], small["v"])
    else:
        bad[arg] = HOW[how](small[arg])
    args = [bad[a] for a in ARGS[name]]
    with pytest.raises(RuntimeError, match=fragment):
        getattr(ext, name)(*args, *TAIL.get(name, ()))


def test_fused_rejects_unknown_variant(ext, small):
    args = [small[a] for a in ARGS["decode_attn_fused"]]
    with pytest.raises(RuntimeError, match="waves_per_simd"):
        ext.decode_attn_fused(*args, 1.0, 3)


def test_tiled_rejects_64_rows_at_d128(ext, small):
    args = [small[a] for a in ARGS["paged_attn_prefill_tiled"]]
    args[0] = torch.ones(T_, QH_, 128, dtype=torch.bfloat16, device=DEV)
    args[1] = torch.zeros(6, KVH_, 16, 64, 8, dtype=torch.bfloat16,
                          device=DEV)
    args[2] = torch.zeros(6, KVH_, 128, 64, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(RuntimeError, match="rows must be 32"):
        ext.paged_attn_prefill_tiled(*args, 1.0, True, 64)


# ---- empty batches return without a launch -------------------------------------

def test_empty_decode_batches(ext, small):
    e = lambda t: t[:0]
    empty = {a: e(small[a]) for a in ("q", "k", "v", "bt", "sl")}
    get = lambda name: [empty.get(a, small[a]) for a in ARGS[name]]
    assert ext.paged_attn_decode(*get("paged_attn_decode"), 1.0).shape == \
        (0, QH_, D_)
    assert ext.decode_attn_fused(*get("decode_attn_fused"), 1.0, 1).shape \
        == (0, QH_, D_)
    kc, vc = small["kc"].clone(), small["vc"].clone()
    ext.kv_append(*get("kv_append"))
    ext.rope_kv_append(*get("rope_kv_append"))
    slots = small["slots"][:0]
    ext.kv_scatter(empty["k"], empty["v"], small["kc"], small["vc"], slots)
    ext.rope_kv_scatter(empty["q"], empty["k"], empty["v"], small["kc"],
                        small["vc"], small["cos"], small["sin"],
                        small["pos"][:0], slots)
    torch.cuda.synchronize()
    assert torch.equal(small["kc"], kc) and torch.equal(small["vc"], vc)


@pytest.mark.parametrize("QH,KVH", ((8, 2), (28, 4)))
def test_empty_prefill_maps(ext, small, QH, KVH):
    """No block and no tile: zeros, from the one-wave binding, the tiled
    one and (R = 7) the tiled binding's fallback."""
    q = torch.ones(T_, QH, D_, dtype=torch.bfloat16, device=DEV)
    kc = torch.zeros(6, KVH, D_ // 8, 64, 8, dtype=torch.bfloat16,
                     device=DEV)
    vc = torch.zeros(6, KVH, D_, 64, dtype=torch.bfloat16, device=DEV)
    none = small["item"][:0]
    rest = (small["off"], small["start"], small["len"], 1.0, True)
    for out in (ext.paged_attn_prefill(q, kc, vc, small["pbt"], none, none,
                                       *rest),
                ext.paged_attn_prefill_tiled(q, kc, vc, small["pbt"], none,
                                             none, *rest, 32)):
        assert out.shape == (T_, QH * D_) and not out.any()
    torch.cuda.synchronize()
