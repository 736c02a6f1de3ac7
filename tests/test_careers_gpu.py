"""Careers (K13) on the MI355X: the keys / sort / fold / stitch kernels (csrc/career.hip)
against the plain Python oracle of career_cases.py and the host mirror, bit for bit."""
import json
import os
import subprocess
import sys

import pytest
import torch

from analyzer_amd.runtime.rerate import stream_records

import career_cases as C
import records_cases as RC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", C.TILE_CASES)
def test_tile_edges(gpu_device, name):
    C.check_tile()
    C.check_case(name, gpu_device)


@pytest.mark.parametrize("name", C.DEVICE_LONG_CASES)
def test_long_runs(gpu_device, name):
    C.check_case(name, gpu_device)


@pytest.mark.parametrize("name", C.OTHER_CASES)
def test_device_equals_oracle_and_host_mirror(gpu_device, name):
    C.check_case(name, gpu_device)


def test_realistic_window_from_history_hits(gpu_device):
    """The oracle fed from the device's own K10 hits of every player."""
    rec, rows, base, P, _ = C.case("real")
    hits = RC.select(rec, rows, base, P, range(P), gpu_device).cpu()
    want = C.career_ref(hits, P, 3)
    table = C.run("real", gpu_device)
    assert torch.equal(table.table.cpu(), want)
    games = table.columns()["games"]
    assert int((games == 0).sum()) > 1000 and int((games > 0).sum()) > 1000


def test_hand_built_rows(gpu_device):
    C.check_hand_built(gpu_device)


def test_ids_out_of_range_touch_nothing(gpu_device):
    C.check_guarded_table(gpu_device)


def test_split_invariance(gpu_device):
    C.check_split_invariance(gpu_device)


def test_match_indices_are_64_bit(gpu_device):
    C.check_64_bit(gpu_device)


def test_empty_window_and_chunked_add(gpu_device):
    C.check_empty_window_and_chunks(gpu_device)


def test_columns_and_lookup(gpu_device):
    C.check_lookup(gpu_device)


@pytest.mark.parametrize("name", ["alias", "few:3", "tile:3:%d" % (2 * C.TILE + 3), "mixed", "stitch"])
def test_same_bits_on_every_run(gpu_device, name):
    first = C.run(name, gpu_device).table.cpu()
    assert torch.equal(C.run(name, gpu_device).table.cpu(), first)


@pytest.mark.parametrize("spec", [RC.SPEC3, RC.SPEC5], ids=["3v3", "5v5"])
def test_arena_careers(gpu_device, spec):
    arena, table = C.check_arena_careers(spec, gpu_device)
    assert table.table.is_cuda and arena.rows.is_cuda


def test_cli_careers(gpu_device):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    ok = subprocess.run([sys.executable, "-m", "analyzer_amd.runtime.rerate", "--matches", "900", "--players", "120",
                         "--window", "400", "--records", "resident", "--careers", "5,7"],
                        capture_output=True, text=True, env=env, cwd=ROOT, timeout=300)
    assert ok.returncode == 0, ok.stderr
    lines = [json.loads(ln) for ln in ok.stdout.splitlines() if ln.startswith('{"career"')]
    assert [ln["career"] for ln in lines] == [5, 7]
    from analyzer_amd.runtime.rerate import RerateSpec, rerate_resident

    spec = RerateSpec(total_matches=900, players=120, team_size=3, window=400, seed=2024)
    _, _, arena = rerate_resident(spec, gpu_device, free_bytes=RC.FREE)
    look = arena.careers(120, stream_records(spec, gpu_device)).lookup([5, 7])
    for i, line in enumerate(lines):
        for name, col in look.items():
            v = col[i].item()
            assert line[name] == (None if v != v else v), name
