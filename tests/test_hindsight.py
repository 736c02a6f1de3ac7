"""Hindsight (K16) on the CPU: the host mirror of ``hindsight_add`` -- the plain backward loop
in fp64 -- against the 50-digit oracle of hindsight_cases.py within the error budget,
``Hindsight``, ``RecordArena.hindsight`` and the ``--hindsight`` command line."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from analyzer_amd.ops import Hindsight
from analyzer_amd.ops.native import native

import hindsight_cases as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_constants():
    H.check_constants()


def test_hand_built_chain():
    H.check_hand_chain("cpu")


@pytest.mark.parametrize("K", H.KS)
def test_team_sizes_and_invariants(K):
    H.check_team_size(K, "cpu")


def test_mode_track():
    H.check_mode_track(3, "cpu")


def test_tile_edges():
    H.check_tile_edges("cpu")


def test_one_player_in_every_match():
    H.check_every("cpu")


def test_many_tiles():
    H.check_stitch("cpu")


def test_window_cuts():
    H.check_window_cuts("cpu")


def test_rows_and_slots():
    H.check_rows_and_slots("cpu")


def test_bad_values():
    H.check_bad_values("cpu")


def test_degenerate_sigma():
    H.check_degenerate("cpu")


def test_tau_zero_is_exact():
    H.check_tau_zero("cpu")


def test_empty():
    H.check_empty("cpu")


def test_bad_arguments():
    with pytest.raises(ValueError):
        Hindsight(4, "cpu", track="mode")  # a mode track is named by its mode
    with pytest.raises(ValueError):
        Hindsight(4, "cpu", track="chess")
    with pytest.raises(ValueError):
        Hindsight(4, "cpu", cfg=H.cfg_tau(-1.0))
    with pytest.raises(ValueError):
        Hindsight(1 << 31, "cpu")
    rec, rows, P = H.messy()
    hs = Hindsight(P, "cpu")
    with pytest.raises(ValueError):
        hs.add(rec, rows, K=3)
    with pytest.raises(RuntimeError):
        hs.add(rec, rows[:, :8].contiguous())  # not the packed rows
    carry = torch.full((P, 2), float("nan"), dtype=torch.float64)
    for args in ((carry.float(), rec, rows, 10.0, 0, 0), (carry, rec, rows, float("nan"), 0, 0),
                 (carry, rec, rows, -1.0, 0, 0), (carry, rec, rows, 10.0, 2, 0), (carry, rec, rows, 10.0, 1, 6),
                 (carry[:, :1].contiguous(), rec, rows, 10.0, 0, 0)):
        with pytest.raises(RuntimeError):
            native().hindsight_add(*args)
    assert bool(torch.isnan(carry).all())


def test_arena_hindsight():
    arena = H.check_arena("cpu")
    arena.size = 2
    with pytest.raises(ValueError):
        arena.hindsight(120, lambda lo, hi: None, [5])


CLI = ["--matches", "900", "--players", "120", "--window", "400"]


def _cli(*args):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-m", "analyzer_amd.runtime.rerate", "--device", "cpu", *CLI, *args],
                          capture_output=True, text=True, env=env, cwd=ROOT, timeout=300)


def test_cli_hindsight():
    from analyzer_amd.runtime.rerate import RerateSpec, rerate_resident, stream_records

    ok = _cli("--records", "resident", "--arena-free-bytes", str(1 << 30), "--hindsight", "5,7",
              "--hindsight-track", "ranked")
    assert ok.returncode == 0, ok.stderr
    lines = [json.loads(ln) for ln in ok.stdout.splitlines() if ln.startswith('{"hindsight"')]
    assert [ln["hindsight"] for ln in lines] == [5, 7]
    spec = RerateSpec(total_matches=900, players=120, team_size=3, window=400, seed=2024)
    _, _, arena = rerate_resident(spec, "cpu", free_bytes=1 << 40)
    cols = arena.hindsight(120, stream_records(spec, "cpu"), [5, 7], track="ranked")
    for line in lines:
        sel = (cols["player"] == line["hindsight"]).nonzero().reshape(-1)
        assert line["track"] == "ranked" and line["records"] == sel.numel() > 0
        assert line["match"] == sorted(line["match"])
        for name in ("match", "mu", "sigma", "mu_s", "sigma_s"):
            assert line[name] == cols[name][sel].tolist(), name
        assert line["mu_s"][-1] == line["mu"][-1] and line["sigma_s"][-1] == line["sigma"][-1]


def test_cli_hindsight_argument_errors():
    for args in (("--hindsight", "5"), ("--records", "resident", "--hindsight", "5,120"),
                 ("--records", "resident", "--hindsight", "5", "--hindsight-track", "chess"),
                 ("--records", "resident", "--hindsight-track", "ranked")):
        bad = _cli(*args)
        assert bad.returncode == 2 and "--hindsight" in bad.stderr, (args, bad.stderr)
