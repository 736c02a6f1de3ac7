"""Matchmaking on the CPU (the host mirror of csrc/matchmake.hip, csrc/host.cpp): held to the
oracle of matchmake_cases.py -- the split choice exactly, quality and p_win0 within their
derived budgets."""
import numpy as np
import pytest
import torch

from analyzer_amd.ops import balance_lobbies
from analyzer_amd.ops import matchmake as MM

import matchmake_cases as C

CPU = torch.device("cpu")


@pytest.mark.parametrize("K", C.KS)
def test_split_tables_equal_the_enumeration(K):
    assert MM.split_masks(K) == C.oracle_masks(K)
    G, per_wave, per_block = C.geometry(K)
    assert G >= 2 * K + 2 and per_wave * G == 64 and per_block * G == 256


@pytest.mark.parametrize("K", C.KS)
def test_sizes(K):
    C.check_sizes(K, CPU)


def test_ties_keep_the_lower_index():
    C.check_ties(CPU)


def test_modes_fall_back_and_seeds():
    C.check_modes(CPU)


@pytest.mark.parametrize("K", C.KS)
def test_error_lobbies_leave_their_neighbours_alone(K):
    C.check_errors(K, CPU)


def test_the_roster_is_only_read():
    C.check_read_only(C.live_roster(), CPU)


@pytest.mark.parametrize("K", C.KS)
def test_preview_against_rate(K):
    C.check_preview(K, CPU)


@pytest.mark.parametrize("K", C.KS)
def test_balanced_records_are_rate_input(K):
    C.check_round_trip(K, CPU)


@pytest.mark.parametrize("Q", ("0", "1", "2K-1", "2K", "2K+1", "1000"))
@pytest.mark.parametrize("K", (1, 3, 5))
def test_make_lobbies(K, Q):
    C.check_make_lobbies(K, C.queue_size(K, Q), CPU)


def test_a_repeated_queue_id_fails_exactly_its_lobby():
    C.check_make_lobbies(3, 200, CPU, repeat=True)


def test_repeatable_empty_and_value_errors():
    C.check_repeatable(CPU)
    C.check_empty(CPU)
    C.check_value_errors(CPU)


def test_every_split_is_somewhere_the_answer():
    for K in C.KS:
        got = balance_lobbies(C.random_roster(), torch.as_tensor(C.random_lobbies(K)), "ranked", cfg=C.CFG)
        assert set(np.unique(got.split.numpy()).tolist()) == set(range(C.COUNTS[K]))


def test_cli_prints_the_matchmaking_line(capsys):
    C.check_cli(CPU, capsys)
