"""Islands (K18) on the MI355X: the hook / edges / flatten / census kernels (csrc/islands.hip)
against the plain Python oracle of island_cases.py, the host mirror and, where it imports,
scipy's connected components, bit for bit."""
import pytest

import island_cases as C
import records_cases as RC

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("R", [1, 2, 7])
@pytest.mark.parametrize("K", [1, 2, 3, 4, 5])
def test_team_sizes_and_regions(gpu_device, K, R):
    isl, _ = C.check_stream(K, R, gpu_device)
    assert isl.parent.is_cuda and isl.table()["label"].is_cuda


@pytest.mark.parametrize("K,R", [(1, 1), (3, 7)])
def test_against_scipy(gpu_device, K, R):
    pytest.importorskip("scipy")
    C.check_scipy(K, R, gpu_device)


@pytest.mark.parametrize("order", C.PATH_ORDERS)
def test_deep_paths(gpu_device, order):
    C.check_path(order, gpu_device)


@pytest.mark.parametrize("order", C.PATH_ORDERS)
def test_deep_paths_as_edges(gpu_device, order):
    C.check_path(order, gpu_device, edges=True)


@pytest.mark.parametrize("player", [C.HOT_P - 1, 0])
def test_one_player_in_every_match_same_bits_three_times(gpu_device, player):
    C.check_hot(player, gpu_device, runs=3)


@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_bridge(gpu_device, where):
    C.check_bridge(where, gpu_device)


def test_cuts_order_and_repeats(gpu_device):
    C.check_cuts(gpu_device)


def test_liveness_and_guards(gpu_device):
    C.check_liveness(gpu_device)


def test_edges(gpu_device):
    C.check_edges(gpu_device)


def test_from_pairs(gpu_device):
    C.check_from_pairs(gpu_device)


def test_merge(gpu_device):
    C.check_merge(gpu_device)


def test_degenerate(gpu_device):
    C.check_degenerate(gpu_device)


def test_cache(gpu_device):
    C.check_cache(gpu_device)


def test_the_error_word_is_raised(gpu_device):
    C.check_error_word(gpu_device)


@pytest.mark.parametrize("spec", [RC.SPEC3, RC.SPEC5], ids=["3v3", "5v5"])
def test_arena_islands(gpu_device, spec):
    isl = C.check_arena_islands(spec, gpu_device)
    assert isl.parent.is_cuda


def test_cli_islands(gpu_device):
    C.check_cli(gpu_device)
