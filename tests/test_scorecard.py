"""Scorecard (K14) on the CPU: the host mirrors of ``priors_add`` and ``score_add`` against
the plain Python oracles of scorecard_cases.py, ``Scorecard``, ``RecordArena.scorecard`` and
the ``--score`` command line."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from analyzer_amd.ops import Scorecard
from analyzer_amd.ops.rate import BatchRater
from analyzer_amd.ops.synth import StreamSpec, make_stream, play_out

import records_cases as RC
import scorecard_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_constants():
    C.check_constants()


@pytest.mark.parametrize("name", C.FEW_CASES + C.TILE_CASES + C.LONG_CASES + ["split"])
def test_host_priors_equal_oracle(name):
    C.check_priors(name, "cpu")


def test_sparse_ids_and_ids_out_of_range():
    C.check_sparse("cpu")


def test_empty_window():
    C.check_empty("cpu")


@pytest.mark.parametrize("K", [3, 5])
def test_chain_is_the_roster(K):
    C.check_chain_is_roster(K, "cpu")


@pytest.mark.parametrize("K", C.KS)
def test_first_appearances_equal_preview(K):
    C.check_first_appearances(K, "cpu")


@pytest.mark.parametrize("K", C.KS)
def test_closing_the_loop(K):
    C.check_closing_the_loop(K, "cpu")


def test_p_against_mpmath():
    C.check_p_against_mpmath("cpu")


def test_integer_log_host_equals_int_oracle():
    C.check_integer_log("cpu")


def test_integer_log_accuracy():
    """Against mpmath -log2 over the 4,096 random patterns the error R - T lies in
    [0.00077, 1.00015] units of 2^-20 (measured); the analytic bound of the 20-step
    recurrence on a 31-bit fraction is 0 <= R - T < 1 + 2^-10 (csrc/score_core.h)."""
    lo, hi = C.integer_log_error()
    print("nlog2_q20 error in units of 2^-20: min %.6g max %.6g" % (lo, hi))
    assert 0.0 <= lo and hi < 1.0 + 2.0 ** -10


@pytest.mark.parametrize("K", C.KS)
def test_table_from_own_pred_rows(K):
    C.check_table(K, "cpu")


def test_table_modes_and_shared_track():
    card, pred = C.check_table(3, "cpu", modes=("ranked", "blitz"), track="shared")
    assert set(card.summary()["modes"]) <= {"ranked", "blitz"}
    mode_card, mode_pred = C.check_table(3, "cpu")
    assert not torch.equal(pred.p_win0[pred.status == 0], mode_pred.p_win0[mode_pred.status == 0])


def test_coin_flips_score_one_bit():
    C.check_coin("cpu")


@pytest.mark.parametrize("K", [1, 3])
def test_wrong_starting_roster_is_inconsistent(K):
    C.check_wrong_roster(K, "cpu")


def test_invariance():
    C.check_invariance("cpu")


def test_it_means_something():
    """A latent-skill history (300 players, 20,000 3v3 matches, seed 5) rated at the defaults:
    over its second half the ratings beat the coin predictor, whose bits per match are
    exactly 1 and whose accuracy is 0.5.  Observed on the host mirror over the 9,808 scored matches:
    bits 0.9067, favourite_won / n 0.6463, Brier 0.2192, ECE 0.0222."""
    roster, rec = C.latent_history()
    half = rec.shape[0] // 2
    card = Scorecard(roster, cfg=C.CFG)
    rater = BatchRater(C.CFG)
    res = rater.rate(roster, rec[:half], 3)
    card.add(rec[:half], res.packed)
    card.table.zero_()  # the first half only warms the ratings up
    res = rater.rate(roster, rec[half:], 3)
    card.add(rec[half:], res.packed)
    s = card.summary()
    print("second half: bits %.4f accuracy %.4f brier %.4f ece %.4f n %d" % (
        s["bits"], s["accuracy"], s["brier"], s["ece"], s["n"]))
    assert s["inconsistent"] == 0 and s["n"] > 9000
    assert s["bits"] < 1.0
    assert s["accuracy"] > 0.5


def test_coin_stream_scores_one_bit_under_a_flat_roster():
    """``play_out`` against the generator's own winners: on a stream of fresh, equal players
    every prediction is 0.5 and scores exactly one bit whoever wins."""
    rec = make_stream(StreamSpec(team_size=1, seed=3, p_tie=0.0, p_afk=0.0), 50, 100, K=1)
    played = play_out(rec, torch.linspace(0.0, 3000.0, 100, dtype=torch.float64), 1000.0, 1)
    assert torch.equal(played[:, :3], rec[:, :3]) and set((played[:, 3] & 3).tolist()) == {1, 2}
    assert torch.equal(played, play_out(rec, torch.linspace(0.0, 3000.0, 100, dtype=torch.float64), 1000.0, 1))
    # the higher skill wins more often than not
    ids = rec[:, :2].long()
    better0 = ids[:, 0] > ids[:, 1]
    won0 = (played[:, 3] & 1).bool()
    assert int((better0 == won0).sum()) > 30


def test_bad_arguments():
    before, rec, rows, _ = C.few(2)
    with pytest.raises(ValueError):
        Scorecard(before, track="ranked")
    with pytest.raises(ValueError):
        Scorecard(before, modes=("chess",))
    card = Scorecard(before)
    with pytest.raises(ValueError):
        card.add(rec.to(torch.int64), rows)
    with pytest.raises(ValueError):
        card.add(rec, rows[:5])
    with pytest.raises(RuntimeError):
        card.add(rec, rows[:, :8].contiguous())  # not the packed rows


@pytest.mark.parametrize("spec", [RC.SPEC3, RC.SPEC5], ids=["3v3", "5v5"])
def test_arena_scorecard(spec):
    C.check_arena(spec, "cpu")


def test_arena_scorecard_needs_one_rank():
    from analyzer_amd.runtime.records import RecordArena

    arena = RecordArena(10, 3, "cpu", rank=1, size=2, window=5)
    with pytest.raises(ValueError):
        arena.scorecard(C.few(3)[0], lambda lo, hi: None)


CLI = ["--matches", "900", "--players", "120", "--window", "400"]


def _cli(*args):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-m", "analyzer_amd.runtime.rerate", "--device", "cpu", *CLI, *args],
                          capture_output=True, text=True, env=env, cwd=ROOT, timeout=300)


def test_cli_score():
    ok = _cli("--records", "resident", "--arena-free-bytes", str(1 << 30), "--score", "mode")
    assert ok.returncode == 0, ok.stderr
    lines = [json.loads(ln) for ln in ok.stdout.splitlines() if ln.startswith('{"scorecard"')]
    assert len(lines) == 1
    card = lines[0]["scorecard"]
    assert card["track"] == "mode" and card["n"] > 500 and card["inconsistent"] == 0
    assert 0.9 < card["bits"] < 1.2  # the stream's winners are coin flips
    assert sum(b["n"] for b in card["bins"]) == card["n"] == sum(m["n"] for m in card["modes"].values())


def test_cli_score_needs_resident_records():
    for args in (("--score", "mode"), ("--records", "resident", "--score-modes", "ranked")):
        bad = _cli(*args)
        assert bad.returncode == 2 and "--score" in bad.stderr, (args, bad.stderr)
