"""Profiles (K17) on the MI355X: the keys / sort / fold / stitch kernels (csrc/profile.hip)
against the numpy oracle of profile_cases.py and the host mirror, bit for bit."""
import pytest

from analyzer_amd.ops import ProfileTable

import profile_cases as C

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", C.TILE_CASES)
def test_tile_edges(gpu_device, name):
    C.check_tile()
    C.check_case(name, gpu_device)


@pytest.mark.parametrize("name", C.LONG_CASES)
def test_long_runs(gpu_device, name):
    C.check_case(name, gpu_device)


@pytest.mark.parametrize("name", C.OTHER_CASES)
def test_device_equals_oracle_and_host_mirror(gpu_device, name):
    C.check_case(name, gpu_device)


def test_cells(gpu_device):
    C.check_cells(gpu_device)


def test_stat_values(gpu_device):
    C.check_stat_values(gpu_device)


def test_guards_with_poisoned_stats(gpu_device):
    C.check_guards(gpu_device)


def test_invariance(gpu_device):
    C.check_invariance(gpu_device)


@pytest.mark.parametrize("name", ["alias", "few:3", "tile:3:%d" % (2 * C.TILE + 3), "allcells", "stitch"])
def test_same_bits_on_every_run(gpu_device, name):
    first = C.fold(name, gpu_device)
    C.assert_tables(C.fold(name, gpu_device), (first.table.cpu(), first.cells.cpu()), name)


def test_realistic_window(gpu_device):
    C.check_realistic(gpu_device)


def test_lookup_baselines_brackets_compare(gpu_device):
    C.check_api(gpu_device)
    table = C.fold("api", gpu_device)
    assert table.table.is_cuda and table.cells.is_cuda and table.lookup([0])["per_game"].is_cuda


def test_bad_arguments_launch_nothing(gpu_device):
    table = ProfileTable(4, gpu_device)
    rec, rows, stats, _, _ = C.case("api")
    with pytest.raises(RuntimeError):
        table.add(rec.to(gpu_device), rows.to(gpu_device), stats)  # stats on another device
    with pytest.raises(RuntimeError):
        table.add(rec.to(gpu_device), rows.to(gpu_device), stats.to(gpu_device).double())
    assert int(table.table.abs().sum()) == 0 and int(table.cells.abs().sum()) == 0


def test_cli(gpu_device):
    C.check_cli("cuda")
