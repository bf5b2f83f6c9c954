"""Exact and edge cases of the routed MoE decode kernels (ops/hip/moe.hip):
the cases, references and assertions of test_moe_edges.py run through the
qsa_hip extension on the GPU, plus what only exists there -- the model's
routed _ffn at the limits of E and top-k against the dense loop and the
single-expert kernels, the row limit of the routed path, and the host checks
of the five bindings as a table of rejections raised before a launch."""

import dataclasses
import re

import pytest
import torch

import test_gemm_edges as G
import test_gpu_moe_routed as R
import test_moe_edges as M
from quickstart_streaming_agents_amd.ops import dispatch as D

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def to_dev(t):
    return t.to(DEV)


@pytest.fixture(scope="module")
def ext():
    from quickstart_streaming_agents_amd.ops import ext as get_ext
    return get_ext()


# ---- the shared cases ------------------------------------------------------

@pytest.mark.parametrize("spec", M.DISPATCH_SPECS, ids=G.spec_id)
def test_moe_dispatch(spec):
    case = M.dispatch_case(spec)
    counts, slot, _ = M.check_dispatch(D.moe_dispatch, case, to_dev)
    if spec == ("live", "all_dead"):
        assert counts.tolist() == [0] * case.E and (slot == -1).all()


@pytest.mark.parametrize("spec", M.COMBINE_SPECS, ids=G.spec_id)
def test_moe_combine(spec):
    M.check_combine(D.moe_combine, M.combine_case(spec), to_dev)


GEMM_FN = {"bf16": D.moe_skinny_linear, "fp8": D.moe_skinny_linear_fp8}


@pytest.mark.parametrize("spec", M.GEMM_SPECS, ids=G.spec_id)
def test_moe_gemm_exact(spec):
    M.check_moe_gemm(GEMM_FN[spec[0]], M.gemm_case(spec), to_dev)


@pytest.mark.parametrize("spec", M.SWIGLU_SPECS, ids=G.spec_id)
def test_moe_swiglu(spec):
    M.check_moe_swiglu(D.moe_swiglu, D.swiglu, M.swiglu_case(spec), to_dev)


@pytest.mark.parametrize("spec", M.COMPOSED_SPECS, ids=G.spec_id)
def test_composed_ffn_exact(spec):
    M.check_composed(D.moe_dispatch, GEMM_FN[spec[0]], D.moe_combine,
                     M.composed_case(spec), to_dev)


# ---- the model's routed _ffn at the limits of E and top-k ------------------

def build_limit_model(n_experts, top_k, env):
    from quickstart_streaming_agents_amd.models.mixtral import (MixtralConfig,
                                                                MixtralModel)
    cfg = dataclasses.replace(MixtralConfig.preset("tiny-moe"), n_layers=1,
                              n_experts=n_experts, top_k=top_k)
    assert (cfg.hidden, cfg.ffn) == (256, 512)
    with pytest.MonkeyPatch.context() as mp:
        for key in ("QSA_FP8", "QSA_MOE_ROUTED"):
            mp.delenv(key, raising=False)
        for key, val in env.items():
            mp.setenv(key, val)
        return MixtralModel(cfg, device=DEV, seed=5)


@pytest.fixture(scope="module", params=[(16, 4), (1, 1)],
                ids=["E16-k4", "E1-k1"])
def limit_models(request):
    """Same seed, same weights: routed on the bf16 stream, routed on the fp8
    stream, and the dense loop."""
    e, k = request.param
    return {"bf16": build_limit_model(e, k, {"QSA_FP8": "0"}),
            "fp8": build_limit_model(e, k, {}),
            "dense": build_limit_model(e, k, {"QSA_FP8": "0",
                                              "QSA_MOE_ROUTED": "0"})}


@pytest.mark.parametrize("T", [1, 17, 32])
def test_limit_model_equals_dense_loop(limit_models, T):
    """The dense loop adds every expert's term in ascending order: the
    combine's order with top_k terms, at the model level."""
    routed, dense = limit_models["bf16"], limit_models["dense"]
    assert "moe_wgu" in routed.layers[0]
    assert "moe_wgu" not in dense.layers[0]
    with torch.no_grad():
        h = R.rand_h(T, 500 + T)
        got = routed._ffn(routed.layers[0], h)
        want = dense._ffn(dense.layers[0], h)
    assert torch.isfinite(got.float()).all()
    G.assert_bits_equal(got, want.cpu(), f"routed vs dense T={T}")


@pytest.mark.parametrize("fmt", ["bf16", "fp8"])
@pytest.mark.parametrize("T", [33, 64])
def test_limit_model_equals_composition(limit_models, fmt, T):
    m = limit_models[fmt]
    with torch.no_grad():
        h = R.rand_h(T, 600 + T)
        L = m.layers[0]
        got = m._ffn(L, h)
        want = R.composed_ffn(m, L, h, fmt == "fp8")
    assert torch.isfinite(got.float()).all()
    G.assert_bits_equal(got, want.cpu(), f"routed vs composed {fmt} T={T}")


def test_routed_path_stops_at_64_rows(limit_models, monkeypatch):
    routed, dense = limit_models["bf16"], limit_models["dense"]
    calls = []
    real = D.moe_dispatch

    def spy(*args, **kwargs):
        calls.append(args[0].shape[0])
        return real(*args, **kwargs)

    monkeypatch.setattr(D, "moe_dispatch", spy)
    with torch.no_grad():
        routed._ffn(routed.layers[0], R.rand_h(64, 700))
        assert calls == [64]
        h = R.rand_h(65, 701)
        got = routed._ffn(routed.layers[0], h)
        assert calls == [64]            # 65 rows: not the routed path
        want = dense._ffn(dense.layers[0], h)
    G.assert_bits_equal(got, want.cpu(), "T=65")


# ---- host checks: every one raises before any launch -----------------------

def _z(*shape, dtype=torch.bfloat16, device=DEV):
    return torch.zeros(*shape, dtype=dtype, device=device)


def _idx(T, k=2):
    return torch.arange(k, device=DEV).repeat(T, 1).to(torch.int64)


ARG_ORDER = {
    "dispatch": ("h", "top_idx", "E", "row_live"),
    "gemm": ("xg", "counts", "wf", "N", "K"),
    "fp8": ("xg", "counts", "qf", "scale", "N", "K"),
    "swiglu": ("gu", "counts"),
    "combine": ("y", "slot", "top_idx", "top_w"),
}


def valid_args(binding):
    """Small valid operands of a binding on the device (counts of zero: the
    grouped kernels return at once)."""
    i32 = torch.int32
    if binding == "dispatch":
        return dict(h=_z(4, 256), top_idx=_idx(4), E=4,
                    row_live=torch.ones(4, dtype=i32, device=DEV))
    if binding == "gemm":
        return dict(xg=_z(4, 32, 256), counts=_z(4, dtype=i32),
                    wf=_z(4, 16 * 256), N=16, K=256)
    if binding == "fp8":
        return dict(xg=_z(4, 32, 256), counts=_z(4, dtype=i32),
                    qf=_z(4, 16 * 256, dtype=torch.uint8),
                    scale=torch.ones(4, 16, device=DEV), N=16, K=256)
    if binding == "swiglu":
        return dict(gu=_z(4, 32, 32), counts=_z(4, dtype=i32))
    return dict(y=_z(4, 32, 256), slot=_z(4, 2, dtype=i32), top_idx=_idx(4),
                top_w=torch.ones(4, 2, device=DEV))


def call(ext, binding, args):
    fn = {"dispatch": ext.moe_dispatch, "gemm": ext.moe_skinny_gemm,
          "fp8": ext.moe_skinny_gemm_fp8, "swiglu": ext.moe_swiglu,
          "combine": ext.moe_combine}[binding]
    return fn(*(args[name] for name in ARG_ORDER[binding]))


def _rows(T):
    """dispatch operands of T rows."""
    return dict(h=_z(T, 256), top_idx=_idx(T), row_live=None)


def _combine_rows(T, cap):
    return dict(y=_z(4, cap, 256), slot=_z(T, 2, dtype=torch.int32),
                top_idx=_idx(T), top_w=torch.ones(T, 2, device=DEV))


GPU_MSG = "must be on the GPU"
STACK_MSG = "stack of N*K streams"
SCALE_MSG = "scale must be f32 [E, N] on device"

# (binding, what is bad, the arguments it replaces, fragment of the message)
HOST_CHECKS = [
    ("dispatch", "h on the CPU", lambda a: dict(h=a["h"].cpu()), GPU_MSG),
    ("dispatch", "h f32", lambda a: dict(h=a["h"].float()), "must be bf16"),
    ("dispatch", "h not contiguous", lambda a: dict(h=_z(4, 512)[:, ::2]),
     "must be contiguous"),
    ("dispatch", "H % 8", lambda a: dict(h=_z(4, 260)), "16-byte aligned"),
    ("dispatch", "h 1-D", lambda a: dict(h=_z(256)), "h must be [T, H]"),
    ("dispatch", "T = 65", lambda a: _rows(65), "moe: T in [1,64]"),
    ("dispatch", "T = 0", lambda a: _rows(0), "moe: T in [1,64]"),
    ("dispatch", "top_idx i32", lambda a: dict(top_idx=a["top_idx"].int()),
     "top_idx must be i64 [T, k]"),
    ("dispatch", "top_idx of T - 1 rows", lambda a: dict(top_idx=_idx(3)),
     "top_idx must be i64 [T, k]"),
    ("dispatch", "top_idx on the CPU",
     lambda a: dict(top_idx=a["top_idx"].cpu()), GPU_MSG),
    ("dispatch", "k = 0", lambda a: dict(top_idx=_idx(4, 0)),
     "moe: top-k in [1,4]"),
    ("dispatch", "k = 5", lambda a: dict(top_idx=_idx(4, 5)),
     "moe: top-k in [1,4]"),
    ("dispatch", "E = 0", lambda a: dict(E=0), "moe: E in [1,16]"),
    ("dispatch", "E = 17", lambda a: dict(E=17), "moe: E in [1,16]"),
    ("dispatch", "row_live i64",
     lambda a: dict(row_live=a["row_live"].long()), "must be i32"),
    ("dispatch", "row_live of T - 1",
     lambda a: dict(row_live=a["row_live"][:3].contiguous()),
     "row_live must be [T]"),
    ("dispatch", "row_live on the CPU",
     lambda a: dict(row_live=a["row_live"].cpu()), GPU_MSG),
    ("swiglu", "2F % 16", lambda a: dict(gu=_z(4, 32, 24)),
     "gu cols (2F) % 16"),
    ("swiglu", "cap 48", lambda a: dict(gu=_z(4, 48, 32)),
     "cap must be 32/64"),
    ("swiglu", "counts of E - 1", lambda a: dict(counts=a["counts"][:3]),
     "counts must be [E]"),
    ("combine", "slot i64", lambda a: dict(slot=a["slot"].long()),
     "must be i32"),
    ("combine", "slot on the CPU", lambda a: dict(slot=a["slot"].cpu()),
     GPU_MSG),
    ("combine", "top_w f64", lambda a: dict(top_w=a["top_w"].double()),
     "must be f32"),
    ("combine", "top_w on the CPU", lambda a: dict(top_w=a["top_w"].cpu()),
     GPU_MSG),
    ("combine", "top_w [T, k + 1]",
     lambda a: dict(top_w=torch.ones(4, 3, device=DEV)),
     "must all be [T, k]"),
    ("combine", "cap 64 at T = 32", lambda a: _combine_rows(32, 64),
     "y cap does not match T"),
    ("combine", "cap 32 at T = 33", lambda a: _combine_rows(33, 32),
     "y cap does not match T"),
    ("combine", "y f32", lambda a: dict(y=a["y"].float()), "must be bf16"),
    ("fp8", "the lm_head class", lambda a: dict(
        xg=_z(1, 32, 256), counts=_z(1, dtype=torch.int32),
        qf=_z(1, 65536 * 256, dtype=torch.uint8),
        scale=torch.ones(1, 65536, device=DEV), N=65536),
     "lm_head shape class"),
    ("fp8", "qf int8", lambda a: dict(qf=a["qf"].view(torch.int8)),
     "qf must be uint8"),
    ("gemm", "wf f32", lambda a: dict(wf=a["wf"].float()), "must be bf16"),
]
for _b, _w in (("gemm", "wf"), ("fp8", "qf")):
    _dt = torch.bfloat16 if _b == "gemm" else torch.uint8
    HOST_CHECKS += [
        (_b, "cap 48", lambda a: dict(xg=_z(4, 48, 256)),
         "cap must be 32/64"),
        (_b, "counts i64", lambda a: dict(counts=a["counts"].long()),
         "must be i32"),
        (_b, "counts of E - 1", lambda a: dict(counts=a["counts"][:3]),
         "counts must be [E]"),
        (_b, "counts on the CPU", lambda a: dict(counts=a["counts"].cpu()),
         GPU_MSG),
        (_b, "K other than xg's", lambda a: dict(K=512), "K mismatch"),
        (_b, "K % 256", lambda a, w=_w, dt=_dt: {
            "xg": _z(4, 32, 128), "K": 128, w: _z(4, 16 * 128, dtype=dt)},
         "K%256==0"),
        (_b, "N % 16", lambda a, w=_w, dt=_dt: {
            "N": 24, w: _z(4, 24 * 256, dtype=dt),
            "scale": torch.ones(4, 24, device=DEV)}, "N%16==0"),
        (_b, "stream numel", lambda a, w=_w, dt=_dt: {
            w: _z(4, 16 * 256 - 16, dtype=dt)}, STACK_MSG),
        (_b, "stream leading dim", lambda a, w=_w, dt=_dt: {
            w: _z(2, 2 * 16 * 256, dtype=dt)}, STACK_MSG),
        (_b, "stream on the CPU", lambda a, w=_w: {w: a[w].cpu()}, GPU_MSG),
    ]
HOST_CHECKS += [
    ("fp8", "scale [N]", lambda a: dict(scale=torch.ones(16, device=DEV)),
     SCALE_MSG),
    ("fp8", "scale [E, N - 1]",
     lambda a: dict(scale=torch.ones(4, 15, device=DEV)), SCALE_MSG),
    ("fp8", "scale f64", lambda a: dict(scale=a["scale"].double()),
     SCALE_MSG),
    ("fp8", "scale on the CPU", lambda a: dict(scale=a["scale"].cpu()),
     SCALE_MSG),
]


@pytest.mark.parametrize("binding", sorted(ARG_ORDER))
def test_valid_small_operands_run(ext, binding):
    call(ext, binding, valid_args(binding))
    torch.cuda.synchronize()


@pytest.mark.parametrize("binding,what,replace,fragment", HOST_CHECKS,
                         ids=[f"{b}-{w}".replace(" ", "_")
                              for b, w, _, _ in HOST_CHECKS])
def test_host_check(ext, binding, what, replace, fragment):
    """One bad argument, every other one valid: the named check fires."""
    args = valid_args(binding)
    new = replace(args)
    # "scale" rides along in the shared gemm / fp8 rows
    args.update({k: v for k, v in new.items() if k in ARG_ORDER[binding]})
    with pytest.raises(RuntimeError, match=re.escape(fragment)):
        call(ext, binding, args)
