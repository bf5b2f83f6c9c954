"""Edge cases of the elementwise, top-k, window, AR and hash-join HIP
kernels: the cases, references and assertions of test_kernel_edges.py, run
through the qsa_hip extension on the GPU."""

import numpy as np
import pytest
import torch

import test_kernel_edges as E
from quickstart_streaming_agents_amd.ops import dispatch as D

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def to_dev(t):
    return t.to(DEV)


@pytest.fixture(scope="module")
def ext():
    from quickstart_streaming_agents_amd.ops import ext as get_ext
    return get_ext()


# ---- elementwise -----------------------------------------------------------

@pytest.mark.parametrize("H", E.RMSNORM_H)
def test_rmsnorm(ext, H):
    E.check_rmsnorm(ext.rmsnorm, ext.rmsnorm_residual, H, to_dev)


@pytest.mark.parametrize("name", E.SWIGLU_CASES)
def test_swiglu(ext, name):
    E.check_swiglu(ext.swiglu, name, to_dev)


def test_swiglu_rejects_misaligned_halves(ext):
    """gu[:, 1:1025] starts 2 bytes past a 16-byte boundary; the host check
    refuses it before any launch."""
    gu = to_dev(E.swiglu_case("strided_halves")[0])
    with pytest.raises(RuntimeError, match="16-byte"):
        ext.swiglu(gu[:, 1:1025], gu[:, 1024:])
    with pytest.raises(RuntimeError, match="16-byte"):
        ext.swiglu(gu[:, :1024], gu[:, 1:1025])
    odd = torch.zeros(4, 2 * 1024 + 4, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(RuntimeError, match="16-byte"):     # stride % 8 != 0
        ext.swiglu(odd[:, :1024], odd[:, 1024:2048])


@pytest.mark.parametrize("Dh", E.ROPE_D)
def test_rope_inplace(ext, Dh):
    E.check_rope(ext.rope_inplace, Dh, to_dev)


@pytest.mark.parametrize("name", sorted(E.SOFTMAX_CASES))
def test_softmax_rows(ext, name):
    E.check_softmax(ext.softmax_rows_, name, to_dev)


@pytest.mark.parametrize("scale", E.SOFTMAX_BF16_SCALES)
@pytest.mark.parametrize("cols", E.SOFTMAX_BF16_COLS)
def test_softmax_rows_bf16(ext, cols, scale):
    E.check_softmax_bf16(ext.softmax_rows_bf16_, cols, scale, to_dev)


# ---- top-k -----------------------------------------------------------------

@pytest.mark.parametrize("N,Dm,k,Q,seed", E.TOPK_CASES)
def test_topk(ext, N, Dm, k, Q, seed):
    queries, docs, ref = E.topk_case(N, Dm, k, Q, seed)
    E.check_topk(ext.topk_cosine, queries, docs, k, ref,
                 f"topk N={N} k={k}", to_dev)


def test_topk_all_negated(ext):
    q, docs, ref = E.topk_negated_case()
    E.check_topk(ext.topk_cosine, q, docs, 4, ref, "topk negated", to_dev)


@pytest.mark.parametrize("kind,k", E.TOPK_TIE_CASES)
def test_topk_ties_lowest_index_first(ext, kind, k):
    q, docs, ref = E.topk_tie_case(kind, k)
    E.check_topk(ext.topk_cosine, q, docs, k, ref,
                 f"topk ties {kind} k={k}", to_dev)


def test_topk_k_above_n_raises(ext):
    queries, docs, _ = E.topk_case(*E.TOPK_CASES[0])
    with pytest.raises(RuntimeError, match="k must not exceed"):
        ext.topk_cosine(to_dev(queries), to_dev(docs), 6)


# ---- window aggregation ----------------------------------------------------

@pytest.mark.parametrize("name", sorted(E.WINDOW_CASES))
def test_window_agg(ext, name):
    E.check_window(ext.window_agg, name, to_dev)


def test_window_agg_rejects_bad_arguments(ext):
    ts, key, value = (to_dev(t) for t in E.window_case("span")[:3])
    for args in ((ts, key, value, 0, 0, 4, 7), (ts, key, value, 0, 1000, 0, 7),
                 (ts, key[:-1], value, 0, 1000, 4, 7),
                 (ts, key, value[:-1], 0, 1000, 4, 7)):
        with pytest.raises(RuntimeError, match="window_agg"):
            ext.window_agg(*args)


# ---- AR anomaly scorer -----------------------------------------------------

@pytest.mark.parametrize("order", E.AR_ORDERS)
@pytest.mark.parametrize("family", E.AR_FAMILIES)
def test_anomaly_batch(ext, family, order):
    series, lengths = E.ar_case(family)
    fc, se, dof = ext.anomaly_batch(to_dev(torch.from_numpy(series)),
                                    to_dev(torch.from_numpy(lengths)), order)
    E.check_ar(family, order, fc.cpu().numpy().astype(np.float64),
               se.cpu().numpy().astype(np.float64), dof.cpu().numpy())


# ---- hash join -------------------------------------------------------------

@pytest.mark.parametrize("name", E.HASH_CASES)
def test_hash_join(name):
    """GPU table against the brute-force max-(ts, row) on every probe, and
    against the CPU dict path."""
    keys, ts, probe = E.hash_case(name)
    table = E.check_hash(name, to_dev)
    assert isinstance(table, tuple) and table[0].is_cuda
    cpu_table = D.hash_build(keys, ts)
    for min_ts in E.HASH_MIN_TS:
        assert torch.equal(D.hash_probe(table, to_dev(probe), min_ts).cpu(),
                           D.hash_probe(cpu_table, probe, min_ts))
