"""Steered read-out and edge cases of the two sampler kernels: the cases,
expectations and assertions of test_sampler_edges.py, run through
greedy_sample_step, sample_step and sample_tokens of the qsa_hip extension
on the GPU, every row of every case (the 16-byte phases of the rows are
the tables'), plus the host check on V.  No case compares a kernel with
another kernel or with the CPU branch; every comparison is exact."""

import pytest
import torch

import test_sampler_edges as E
from quickstart_streaming_agents_amd.ops import dispatch as D

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def run(c):
    E.check_case(c, DEV, all_rows=True)
    torch.cuda.synchronize()


# ---- 1. slots -------------------------------------------------------------------

@pytest.mark.parametrize("kind", E.EOS_KINDS)
def test_slots_one_hot(kind):
    for spec in E.SLOT_SPECS:
        run(E.slot_one_hot_case(kind, spec))


@pytest.mark.parametrize("kind", E.EOS_KINDS)
def test_slots_ties(kind):
    run(E.slot_tie_case(kind))


def test_empty_windows_and_dead_rows():
    run(E.empty_window_case())
    run(E.empty_window_no_eos_case())
    run(E.all_neg_inf_case())


@pytest.mark.parametrize("n", range(1, 8))
def test_no_body_windows(n):
    for hot in [None] + list(range(n)):
        run(E.no_body_case(n, hot))


# ---- 2. step scan ---------------------------------------------------------------

def test_step_scan_16k():
    run(E.scan_16k_case())


def test_step_scan_2m():
    run(E.scan_2m_case())


@pytest.mark.parametrize("lo", (0, 1))
def test_step_scan_max(lo):
    run(E.scan_max_case(lo))


# ---- 3, 4, 5. kept sets and weights ----------------------------------------------

@pytest.mark.parametrize("i", range(len(E.KEPT_TABLE)),
                         ids=[s.name for s in E.KEPT_TABLE])
def test_kept_sets(i):
    run(E.kept_case(i))


@pytest.mark.parametrize("i", range(5))
def test_weight_rows(i):
    run(E.weight_case(i))


def test_unit_weights():
    run(E.unit_weight_case())


@pytest.mark.parametrize("kind", E.EOS_KINDS)
@pytest.mark.parametrize("si", range(len(E.INF_SLOTS)))
def test_plus_inf_gives_the_greedy_token(si, kind):
    run(E.inf_case(si, kind))


# ---- 6. bookkeeping -------------------------------------------------------------

@pytest.mark.parametrize("ctr0", E.BK_CTRS)
def test_bookkeeping(ctr0):
    E.check_bookkeeping(D.greedy_sample_step, ctr0, DEV)
    E.check_bookkeeping(E.sampled_step(DEV), ctr0, DEV)
    torch.cuda.synchronize()


# ---- 7. host checks -------------------------------------------------------------

def test_host_check_on_v():
    """One LDS total per 2048 candidates, 2048 of them: V = 2046 * 2048 is
    the last size taken, 8 more is refused before a launch."""
    c = E.new_case("host", 8, 0, 8, -1, 1)
    p = E.params(c, [0], DEV)
    ok = torch.zeros(1, E.VMAX, dtype=torch.bfloat16, device=DEV)
    ok[0, E.VMAX - 1] = 1.0
    assert D.sample_tokens(ok, 0, E.VMAX, -1, *E.params(
        c, [0], DEV, greedy=True)).tolist() == [E.VMAX - 1]
    big = torch.zeros(1, E.VMAX + 8, dtype=torch.bfloat16, device=DEV)
    bk = E._books(1, DEV)
    with pytest.raises(RuntimeError, match="2046"):
        D.sample_tokens(big, 0, E.VMAX + 8, -1, *p)
    with pytest.raises(RuntimeError, match="2046"):
        D.sample_tokens(big, 0, 8, -1, *p)
    with pytest.raises(RuntimeError, match="2046"):
        D.sample_step(big, 0, 8, -1, *p, bk["script"], bk["mask"], bk["ctr"],
                      bk["hist"], bk["tokens"], bk["ticket"])
    torch.cuda.synchronize()
    assert int(bk["ctr"][0]) == 0 and bk["tokens"].tolist() == [-7]
