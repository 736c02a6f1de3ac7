"""Pairs (K15) on the MI355X: the keys / sort / gather / count / scan / emit kernels
(csrc/pairs.hip) against the plain Python oracle of pairs_cases.py and the host mirror, bit
for bit."""
import pytest
import torch

from analyzer_amd.ops.native import native

import pairs_cases as C
import records_cases as RC

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("K", [1, 2, 3, 4, 5])
def test_hand_built_windows(gpu_device, K):
    C.check_hand_built(K, gpu_device)


def test_nothing_outside_the_bitmap_is_read(gpu_device):
    C.check_guarded_bitmap(gpu_device)


@pytest.mark.parametrize("name", C.RUN_CASES)
def test_run_edges(gpu_device, name):
    C.check_run_edges(name, gpu_device)


@pytest.mark.parametrize("name", C.WIDE_CASES)
def test_key_width(gpu_device, name):
    table = C.check_case(name, gpu_device)
    assert (table.keys.numel() == 0) == (name == "wide:p1")


def test_filter(gpu_device):
    table = C.check_case("filter", gpu_device)
    assert set((table.keys >> 32).tolist()) == {0, 7, 31, 44}
    assert C.check_case("nobody", gpu_device).keys.numel() == 0


def test_cut_invariance(gpu_device):
    C.check_cut_invariance(gpu_device)


@pytest.mark.parametrize("K", [3, 5])
def test_symmetries(gpu_device, K):
    C.check_symmetries(K, gpu_device)


@pytest.mark.parametrize("name", ["long", "sym:5:012", "cut", "hand:3"])
def test_same_bits_on_every_run(gpu_device, name):
    C.check_repeatable(name, gpu_device)


def test_queries(gpu_device):
    C.check_queries(gpu_device)


def test_merge_adds_tables(gpu_device):
    a, b = C.run("filter", gpu_device), C.run("cut", gpu_device)
    keys, counts = native().pairs_merge([a.keys, b.keys, a.keys], [a.counts, b.counts, a.counts])
    host = native().pairs_merge([a.keys.cpu(), b.keys.cpu(), a.keys.cpu()],
                                [a.counts.cpu(), b.counts.cpu(), a.counts.cpu()])
    assert keys.is_cuda and torch.equal(keys.cpu(), host[0]) and torch.equal(counts.cpu(), host[1])
    assert keys.numel() > C.TILE


@pytest.mark.parametrize("spec", [RC.SPEC3, RC.SPEC5], ids=["3v3", "5v5"])
def test_arena_pairs(gpu_device, spec):
    arena, table = C.check_arena_pairs(spec, gpu_device)
    assert table.keys.is_cuda and arena.rows.is_cuda


def test_cli_pairs(gpu_device):
    C.check_cli(gpu_device)
