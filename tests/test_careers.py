"""Careers (K13) on the CPU: the host mirror of ``careers_add`` against the plain Python
oracle of career_cases.py, ``CareerTable`` and ``RecordArena.careers``, and the
``--careers`` command line."""
import json
import os
import subprocess
import sys

import pytest
import torch

from analyzer_amd.ops import CareerTable
from analyzer_amd.runtime.rerate import RerateSpec, rerate_resident, stream_records

import career_cases as C
import records_cases as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_constants():
    C.check_tile()


@pytest.mark.parametrize("name", C.TILE_CASES + C.LONG_CASES + C.OTHER_CASES)
def test_host_mirror_equals_oracle(name):
    C.check_case(name, "cpu")


def test_hand_built_rows():
    C.check_hand_built("cpu")


def test_ids_out_of_range_touch_nothing():
    C.check_guarded_table("cpu")


def test_split_invariance():
    C.check_split_invariance("cpu")


def test_match_indices_are_64_bit():
    C.check_64_bit("cpu")


def test_empty_window_and_chunked_add():
    C.check_empty_window_and_chunks("cpu")


def test_columns_and_lookup():
    C.check_lookup("cpu")


def test_aliased_player_wins_and_loses_every_match():
    cols = C.check_case("alias", "cpu").columns()
    M = C.TILE + C.TILE // 2
    assert int(cols["games"][0]) == 2 * M and int(cols["wins"][0]) == M
    assert int(cols["best_win"][0]) == 2  # slot 1 of a match it wins there, then slot 0 of the next
    assert int(cols["streak"][0]) == -1 and (int(cols["first"][0]), int(cols["last"][0])) == (0, M - 1)
    assert float(cols["peak"][0]) == 9.0 and int(cols["peak_match"][0]) == 10


def test_bad_arguments():
    with pytest.raises(ValueError):
        CareerTable(4, "cpu", track="ranked")
    with pytest.raises(ValueError):
        CareerTable(4, "cpu", score="sigma")
    with pytest.raises(ValueError):
        CareerTable(4, "cpu", modes=("chess",))
    table = CareerTable(4, "cpu")
    rec, rows, base, _, _ = C.case("hand")
    with pytest.raises(ValueError):
        table.add(rec, rows, base, K=3)
    with pytest.raises(ValueError):
        table.lookup([4])
    with pytest.raises(RuntimeError):
        table.add(rec, rows[:, :8].contiguous(), base)  # not the packed rows
    with pytest.raises(RuntimeError):
        table.add(rec, rows, -1)


@pytest.mark.parametrize("spec", [RC.SPEC3, RC.SPEC5], ids=["3v3", "5v5"])
def test_arena_careers(spec):
    C.check_arena_careers(spec, "cpu")


CLI = ["--matches", "900", "--players", "120", "--window", "400"]


def _cli(*args):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-m", "analyzer_amd.runtime.rerate", "--device", "cpu", *CLI, *args],
                          capture_output=True, text=True, env=env, cwd=ROOT, timeout=300)


def test_cli_careers():
    ok = _cli("--records", "resident", "--arena-free-bytes", str(1 << 30), "--careers", "5,7",
              "--careers-track", "mode", "--careers-modes", "ranked,casual")
    assert ok.returncode == 0, ok.stderr
    lines = [json.loads(ln) for ln in ok.stdout.splitlines() if ln.startswith('{"career"')]
    assert [ln["career"] for ln in lines] == [5, 7]
    spec = RerateSpec(total_matches=900, players=120, team_size=3, window=400, seed=2024)
    _, _, arena = rerate_resident(spec, "cpu", free_bytes=RC.FREE)
    look = arena.careers(120, stream_records(spec, "cpu"), track="mode", modes=("ranked", "casual")).lookup([5, 7])
    for i, line in enumerate(lines):
        assert line["track"] == "mode" and line["score"] == "conservative" and line["rank"] == 0
        for name, col in look.items():
            v = col[i].item()
            assert line[name] == (None if v != v else v), name
    assert lines[0]["games"] > 0 and lines[0]["first"] >= 0


def test_cli_careers_argument_errors():
    for args in (("--careers", "5"), ("--records", "resident", "--careers", "5,120", "--careers-modes", "chess")):
        bad = _cli(*args)
        assert bad.returncode == 2 and "--careers" in bad.stderr, (args, bad.stderr)
