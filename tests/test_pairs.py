"""Pairs (K15) on the CPU: the host mirror of ``pairs_window`` / ``pairs_merge`` against the
plain Python oracle of pairs_cases.py, ``PairTable`` and its queries, ``RecordArena.pairs``
and the ``--pairs`` command line."""
import os
import subprocess
import sys

import pytest
import torch

from analyzer_amd.ops import PairTable
from analyzer_amd.ops.native import native

import pairs_cases as C
import records_cases as RC


def test_constants():
    C.check_constants()


@pytest.mark.parametrize("K", [1, 2, 3, 4, 5])
def test_hand_built_windows(K):
    C.check_hand_built(K, "cpu")


def test_nothing_outside_the_bitmap_is_read():
    C.check_guarded_bitmap("cpu")


@pytest.mark.parametrize("name", C.RUN_CASES)
def test_run_edges(name):
    C.check_run_edges(name, "cpu")


@pytest.mark.parametrize("name", C.WIDE_CASES)
def test_key_width(name):
    table = C.check_case(name, "cpu")
    assert (table.keys.numel() == 0) == (name == "wide:p1")
    if name == "wide:max":
        assert int(table.keys[-1] >> 32) == (1 << 31) - 2  # the id next to P


def test_filter():
    table = C.check_case("filter", "cpu")
    assert set((table.keys >> 32).tolist()) == {0, 7, 31, 44}
    assert C.check_case("nobody", "cpu").keys.numel() == 0


def test_cut_invariance():
    C.check_cut_invariance("cpu")


@pytest.mark.parametrize("K", [3, 5])
def test_symmetries(K):
    C.check_symmetries(K, "cpu")


def test_queries():
    C.check_queries("cpu")


def test_merge_adds_tables():
    a, b = C.run("filter", "cpu"), C.run("cut", "cpu")
    keys, counts = native().pairs_merge([a.keys, b.keys, a.keys], [a.counts, b.counts, a.counts])
    want = dict(C.oracle("cut"))
    for k, v in C.oracle("filter").items():
        want[k] = [x + 2 * y for x, y in zip(want.get(k, [0, 0, 0, 0]), v)]
    assert torch.equal(keys, C.table_of(want)[0]) and torch.equal(counts, C.table_of(want)[1])


def test_bad_arguments():
    with pytest.raises(ValueError):
        PairTable(4, "cpu", modes=("chess",))
    with pytest.raises(ValueError):
        PairTable(1 << 31, "cpu")
    with pytest.raises(ValueError):
        PairTable(4, "cpu", max_entries=0)
    table = PairTable(C.HAND_P, "cpu")
    rec, rows, _, _ = C.case("hand:2")
    with pytest.raises(ValueError):
        table.add(rec, rows, K=3)
    with pytest.raises(RuntimeError):
        table.add(rec, rows[:, :8].contiguous())  # not the packed rows
    with pytest.raises(RuntimeError):
        native().pairs_window(rec, rows, C.HAND_P, 1 << 6, None)
    with pytest.raises(RuntimeError):
        native().pairs_merge([table.keys], [])
    table.matches = (1 << 31) - rec.shape[0]
    with pytest.raises(OverflowError):
        table.add(rec, rows)  # the counters are int32


@pytest.mark.parametrize("spec", [RC.SPEC3, RC.SPEC5], ids=["3v3", "5v5"])
def test_arena_pairs(spec):
    C.check_arena_pairs(spec, "cpu")


def test_cli_pairs():
    C.check_cli("cpu", "--device", "cpu", "--arena-free-bytes", str(1 << 30))


def test_cli_pairs_argument_errors():
    env = dict(os.environ, PYTHONPATH=C.ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    base = [sys.executable, "-m", "analyzer_amd.runtime.rerate", "--device", "cpu", "--matches", "900", "--players", "120",
            "--window", "400"]
    for args in (("--pairs", "5"), ("--records", "resident", "--pairs-top", "3"),
                 ("--records", "resident", "--pairs", "5,120"),
                 ("--records", "resident", "--pairs", "5", "--pairs-modes", "chess")):
        bad = subprocess.run(base + list(args), capture_output=True, text=True, env=env, cwd=C.ROOT, timeout=300)
        assert bad.returncode == 2 and "--pairs" in bad.stderr, (args, bad.stderr)
