"""Profiles (K17) on the CPU: the host mirror of ``profiles_add`` against the numpy oracle of
profile_cases.py, the ``ProfileTable`` interface and the command line."""
import pytest

from analyzer_amd.ops import ProfileTable
from analyzer_amd.ops.profiles import default_edges

import profile_cases as C


def test_constants():
    C.check_tile()
    assert len(default_edges()) == 9 and ProfileTable(3, "cpu").brackets == 10


@pytest.mark.parametrize("name", C.TILE_CASES + C.LONG_CASES + C.OTHER_CASES)
def test_host_mirror_equals_oracle(name):
    C.check_case(name, "cpu")


def test_cells():
    C.check_cells("cpu")


def test_stat_values():
    C.check_stat_values("cpu")


def test_guards_with_poisoned_stats():
    C.check_guards("cpu")


def test_invariance():
    C.check_invariance("cpu")


def test_realistic_window():
    C.check_realistic("cpu")


def test_lookup_baselines_brackets_compare():
    C.check_api("cpu")


def test_bad_arguments():
    for kw in ({"track": "ranked"}, {"score": "sigma"}, {"modes": ("chess",)}, {"edges": (2.0, 1.0)},
               {"edges": (1.0, 1.0)}, {"edges": (1.0, float("nan"))}, {"edges": (0.0, float("inf"))},
               {"edges": (1.0e39,)}, {"edges": tuple(range(32))}, {"edges": (1.0, 1.0 + 2.0 ** -30)}):
        with pytest.raises(ValueError):
            ProfileTable(4, "cpu", **kw)
    assert ProfileTable(4, "cpu", edges=tuple(range(31))).brackets == 32
    table = ProfileTable(4, "cpu")
    rec, rows, stats, _, _ = C.case("api")
    with pytest.raises(ValueError):
        table.add(rec, rows, stats, K=3)
    with pytest.raises(ValueError):
        table.add(rec, rows, stats[:, :1])
    with pytest.raises(ValueError):
        table.add(rec, rows[:2], stats)
    for ids in ([4], [-1]):
        with pytest.raises(ValueError):
            table.lookup(ids)
    with pytest.raises(ValueError):
        table.compare([1, 2], [3.0])
    with pytest.raises(ValueError):
        table.merge(ProfileTable(4, "cpu", score="mu"))
    with pytest.raises(RuntimeError):
        table.add(rec, rows[:, :8].contiguous(), stats)  # not the packed rows
    assert int(table.table.abs().sum()) == 0 and int(table.cells.abs().sum()) == 0


def test_cli():
    C.check_cli("cpu")
    bad = C.run_cli("cpu", "--matches", "10", "--players", "5", "--ids", "5")
    assert bad.returncode == 2 and "--ids" in bad.stderr
