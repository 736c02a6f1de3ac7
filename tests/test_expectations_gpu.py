"""Expectations (K19) on the MI355X: the keys / sort / fold / stitch kernels (csrc/expect.hip)
against the numpy oracle of expect_cases.py and the host mirror, bit for bit."""
import pytest
import torch

import expect_cases as C
import records_cases as RC

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", C.TILE_CASES)
def test_tile_edges(gpu_device, name):
    C.check_tile()
    C.check_case(name, gpu_device)


@pytest.mark.parametrize("name", C.LONG_CASES)
def test_long_runs(gpu_device, name):
    C.check_case(name, gpu_device)


@pytest.mark.parametrize("name", C.OTHER_CASES)
def test_device_equals_oracle_and_host_mirror(gpu_device, name):
    C.check_case(name, gpu_device)


def test_values(gpu_device):
    C.check_values(gpu_device)


def test_slots_one_by_one(gpu_device):
    C.check_slots(gpu_device)


def test_guards_with_poisoned_priors_and_term_memory(gpu_device):
    # what the term buffer of the next call is likely to be handed: every word a huge term
    n = C.case("slots")[0].shape[0] * 6 * 8
    junk = torch.full((n,), 0x7F7F7F7F, dtype=torch.int32, device=gpu_device)
    del junk
    C.check_guards(gpu_device)


def test_carries(gpu_device):
    C.check_carries(gpu_device)


def test_invariance(gpu_device):
    C.check_invariance(gpu_device)


@pytest.mark.parametrize("name", ["three", "few:3", "tile:3:%d" % (2 * C.TILE + 3), "mixed:5:mode", "stitch"])
def test_same_bits_on_every_run(gpu_device, name):
    first = C.fold(name, gpu_device)
    C.assert_table(C.fold(name, gpu_device), (first.table.cpu(), first.bad), name)


def test_every_branch_of_game(gpu_device):
    C.check_branches(gpu_device)


@pytest.mark.parametrize("K", [3, 5])
def test_end_to_end(gpu_device, K):
    exp = C.check_end_to_end(K, gpu_device)
    assert exp.table.is_cuda and exp.lookup([0])["z"].is_cuda


def test_lookup_outliers_fairness(gpu_device):
    C.check_api(gpu_device)


def test_merge(gpu_device):
    C.check_merge(gpu_device)


def test_arena_expectations(gpu_device):
    C.check_arena(RC.SPEC3, gpu_device)


def test_bad_arguments_launch_nothing(gpu_device):
    rec, priors, pred, P, track = C.case("slots")
    exp = C.Table(P, gpu_device, track).exp
    d = gpu_device
    with pytest.raises(RuntimeError):
        exp.add_scored(rec.to(d), priors, pred.to(d))  # priors on another device
    with pytest.raises(RuntimeError):
        exp.add_scored(rec.to(d), priors.to(d), pred)  # pred on another device
    with pytest.raises(RuntimeError):
        exp.add_scored(rec, priors.to(d), pred.to(d))  # rec on another device
    with pytest.raises(RuntimeError):
        exp.add_scored(rec.to(d), priors.to(d).double(), pred.to(d))
    with pytest.raises(RuntimeError):
        exp.add_scored(rec.to(d), priors.to(d), pred.to(d).to(torch.int64))
    with pytest.raises(RuntimeError):
        C.native().expect_add(exp.table, exp._bad, rec.to(d), priors[:3].to(d), pred.to(d), P, 0)  # another M
    with pytest.raises(RuntimeError):
        C.native().expect_add(exp.table, exp._bad.cpu(), rec.to(d), priors.to(d), pred.to(d), P, 0)
    assert int(exp.table.abs().sum()) == 0 and exp.bad == 0


def test_cli(gpu_device):
    C.check_cli("cuda")
