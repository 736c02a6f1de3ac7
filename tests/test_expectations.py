"""Expectations (K19) on the CPU: the host mirror of ``expect_add`` against the numpy oracle of
expect_cases.py, bit for bit, ``Expectations``, ``RecordArena.expectations`` and the
``--expect`` command line."""
import os
import shutil
import subprocess

import pytest
import torch

from analyzer_amd.ops import Expectations

import expect_cases as C
import records_cases as RC


def test_constants():
    C.check_tile()


@pytest.mark.parametrize("name", C.TILE_CASES[::4] + ["three", "exact", "few:3"] + C.OTHER_CASES)
def test_host_mirror_equals_oracle(name):
    C.check_case(name, "cpu")


def test_values():
    C.check_values("cpu")


def test_slots_one_by_one():
    C.check_slots("cpu")


def test_guards_with_poisoned_priors():
    C.check_guards("cpu")


def test_carries():
    C.check_carries("cpu")


def test_invariance():
    C.check_invariance("cpu")


def test_every_branch_of_game():
    C.check_branches("cpu")


@pytest.mark.parametrize("K", [3, 5])
def test_end_to_end(K):
    C.check_end_to_end(K, "cpu")


def test_lookup_outliers_fairness():
    C.check_api("cpu")


def test_merge():
    C.check_merge("cpu")


def test_bad_arguments():
    rec, priors, pred, P, track = C.case("slots")
    exp = C.Table(P, "cpu", track).exp
    with pytest.raises(RuntimeError):
        exp.add_scored(rec, priors.double(), pred)
    with pytest.raises(RuntimeError):
        exp.add_scored(rec, priors, pred.to(torch.int64))
    with pytest.raises(RuntimeError):
        exp.add_scored(rec.to(torch.int64), priors, pred)
    with pytest.raises(ValueError):
        exp.add_scored(rec, priors[:3], pred)  # priors of another M
    with pytest.raises(RuntimeError):
        exp.add_scored(rec, priors[:, :, :4].contiguous(), pred)  # priors of another K
    with pytest.raises(RuntimeError):
        C.native().expect_add(exp.table, exp._bad, rec, priors[:3], pred, P, 0)
    with pytest.raises(RuntimeError):
        C.native().expect_add(exp.table, exp._bad, rec, priors, pred, P, 2)  # no such track
    with pytest.raises(RuntimeError):
        C.native().expect_add(exp.table, exp._bad, rec, priors, pred, P + 1, 0)  # not the table's P
    assert int(exp.table.abs().sum()) == 0 and exp.bad == 0
    with pytest.raises(ValueError):
        Expectations(C.rated(2, 120, 60)[0], track="ranked")


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host compiler")
def test_host_mirror_under_asan_ubsan(tmp_path):
    """tests/native/expect_selftest.cpp with csrc/host.cpp as a stand-alone executable: every
    word pattern of pred and priors through ``host_expect_add``, buffers of the exact sizes."""
    csrc = os.path.join(C.ROOT, "analyzer_amd", "csrc")
    exe = str(tmp_path / "expect_selftest")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-I" + csrc, os.path.join(C.ROOT, "tests", "native", "expect_selftest.cpp"),
           os.path.join(csrc, "host.cpp"), "-o", exe]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    assert "expect selftest ok" in run.stdout


def test_arena_expectations():
    C.check_arena(RC.SPEC3, "cpu")


def test_arena_expectations_needs_one_rank():
    from analyzer_amd.runtime.records import RecordArena

    arena = RecordArena(10, 3, "cpu", rank=1, size=2, window=5)
    with pytest.raises(ValueError):
        arena.expectations(C.rated(2, 120, 60)[0], lambda lo, hi: None)


def test_cli_expect():
    C.check_cli("cpu")


def test_cli_expect_needs_resident_records():
    for args in (("--expect", "5"), ("--records", "resident", "--arena-free-bytes", str(1 << 30), "--expect", "120")):
        bad = C.run_cli("cpu", *args)
        assert bad.returncode == 2 and "--expect" in bad.stderr, (args, bad.stderr)
