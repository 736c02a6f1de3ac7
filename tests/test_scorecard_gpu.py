"""Scorecard (K14) on the MI355X: the keys / sort / summaries / stitch / apply kernels and
the score kernel (csrc/score.hip) against the plain Python oracles of scorecard_cases.py and
the host mirror."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import records_cases as RC
import scorecard_cases as C

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", C.FEW_CASES)
def test_few_players_every_feature(gpu_device, name):
    C.check_constants()
    C.check_priors(name, gpu_device)


@pytest.mark.parametrize("name", C.TILE_CASES)
def test_tile_edges(gpu_device, name):
    C.check_priors(name, gpu_device)


@pytest.mark.parametrize("name", C.DEVICE_LONG_CASES)
def test_long_runs(gpu_device, name):
    C.check_priors(name, gpu_device)


def test_sparse_ids_and_ids_out_of_range(gpu_device):
    C.check_sparse(gpu_device)


def test_empty_window(gpu_device):
    C.check_empty(gpu_device)


@pytest.mark.parametrize("K", [3, 5])
def test_chain_is_the_roster(gpu_device, K):
    card = C.check_chain_is_roster(K, gpu_device)
    assert card.chain.is_cuda and card.table.is_cuda


@pytest.mark.parametrize("K", C.KS)
def test_first_appearances_equal_preview(gpu_device, K):
    C.check_first_appearances(K, gpu_device)


@pytest.mark.parametrize("K", [1, 3, 5])
def test_closing_the_loop(gpu_device, K):
    C.check_closing_the_loop(K, gpu_device)


def test_p_against_mpmath(gpu_device):
    C.check_p_against_mpmath(gpu_device)


def test_integer_log_device_equals_host_and_int_oracle(gpu_device):
    C.check_integer_log(gpu_device)
    C.check_integer_log("cpu")


@pytest.mark.parametrize("K", C.KS)
def test_table_from_own_pred_rows(gpu_device, K):
    C.check_table(K, gpu_device)


def test_table_modes_and_shared_track(gpu_device):
    C.check_table(3, gpu_device, modes=("ranked", "blitz"), track="shared")


def test_coin_flips_score_one_bit(gpu_device):
    C.check_coin(gpu_device)


@pytest.mark.parametrize("K", [1, 3])
def test_wrong_starting_roster_is_inconsistent(gpu_device, K):
    C.check_wrong_roster(K, gpu_device)


def test_invariance(gpu_device):
    C.check_invariance(gpu_device)


@pytest.mark.parametrize("name", ["every", "tile:3:%d" % (2 * C.TILE + 3), "few:5"])
def test_same_bits_on_every_run(gpu_device, name):
    first = C.run_priors(name, gpu_device)
    again = C.run_priors(name, gpu_device)
    assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1])


@pytest.mark.parametrize("spec", [RC.SPEC3, RC.SPEC5], ids=["3v3", "5v5"])
def test_arena_scorecard(gpu_device, spec):
    arena, card = C.check_arena(spec, gpu_device)
    assert card.table.is_cuda and arena.rows.is_cuda


def test_cli_score(gpu_device):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    ok = subprocess.run([sys.executable, "-m", "analyzer_amd.runtime.rerate", "--matches", "900", "--players", "120",
                         "--window", "400", "--records", "resident", "--score", "mode"],
                        capture_output=True, text=True, env=env, cwd=ROOT, timeout=300)
    assert ok.returncode == 0, ok.stderr
    lines = [json.loads(ln) for ln in ok.stdout.splitlines() if ln.startswith('{"scorecard"')]
    assert len(lines) == 1
    card = lines[0]["scorecard"]
    assert card["n"] > 500 and card["inconsistent"] == 0 and 0.9 < card["bits"] < 1.2
    bad = subprocess.run([sys.executable, "-m", "analyzer_amd.runtime.rerate", "--matches", "900", "--players", "120",
                          "--window", "400", "--score", "mode"], capture_output=True, text=True, env=env, cwd=ROOT,
                         timeout=300)
    assert bad.returncode == 2 and "--score needs --records resident" in bad.stderr
