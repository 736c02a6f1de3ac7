"""Hindsight (K16) on the device: the kernels of csrc/hindsight.hip -- the composition of the
smoother's steps in a segmented scan -- against the 50-digit oracle of hindsight_cases.py
within the error budget, and against the host mirror at twice it."""
import numpy as np
import pytest

import hindsight_cases as H

pytestmark = pytest.mark.gpu


def test_hand_built_chain(gpu_device):
    H.check_hand_chain(gpu_device)


@pytest.mark.parametrize("K", H.KS)
def test_team_sizes_and_invariants(gpu_device, K):
    """Rated by ``BatchRater`` on the device; the mirror on the same rows at twice the budget."""
    out = H.check_team_size(K, gpu_device)
    rec, rows = H.rated(K, gpu_device)
    elem, ids, mu, sigma, _ = H.elements(rec, rows, H.RATED_P)
    host = H.run("cpu", rec, rows, H.RATED_P)[0]
    flat = np.flatnonzero(elem.ravel())
    who = ids.ravel()[flat]
    n = np.bincount(who, minlength=H.RATED_P).astype(np.float64)[who]
    top = np.zeros(H.RATED_P)
    np.maximum.at(top, who, np.abs(mu.ravel()[flat].astype(np.float64)))
    g, h = out.reshape(-1, 2)[flat].astype(np.float64), host.reshape(-1, 2)[flat].astype(np.float64)
    b_mu, b_sigma = H.budget(n, top[who], np.maximum(np.abs(g[:, 0]), np.abs(h[:, 0])), np.maximum(g[:, 1], h[:, 1]))
    assert (np.abs(g[:, 0] - h[:, 0]) <= 2 * b_mu).all() and (np.abs(g[:, 1] - h[:, 1]) <= 2 * b_sigma).all()


def test_mode_track(gpu_device):
    H.check_mode_track(3, gpu_device)


def test_tile_edges(gpu_device):
    H.check_tile_edges(gpu_device)


def test_one_player_in_every_match(gpu_device):
    H.check_every(gpu_device)


def test_stitch_takes_two_iterations(gpu_device):
    rec, rows, P = H.stitch()
    H.check_stitch(gpu_device, mirror=H.run("cpu", rec, rows, P))


@pytest.mark.parametrize("window", [H.tile_edges, H.stitch], ids=["tile_edges", "stitch"])
def test_same_bits_on_every_run(gpu_device, window):
    """No atomics on floats and one owner per carry row: a second run gives the first one's bits,
    NaNs included, in ``out`` (fp32), ``carry`` (fp64) and ``bad``."""
    rec, rows, P = window()
    first = H.run(gpu_device, rec, rows, P)
    again = H.run(gpu_device, rec, rows, P)
    assert np.array_equal(first[0].view(np.uint32), again[0].view(np.uint32))
    assert np.array_equal(first[1].view(np.uint64), again[1].view(np.uint64))
    assert first[2] == again[2]


def test_window_cuts(gpu_device):
    H.check_window_cuts(gpu_device)


def test_rows_and_slots(gpu_device):
    H.check_rows_and_slots(gpu_device)


def test_bad_values(gpu_device):
    H.check_bad_values(gpu_device)


def test_degenerate_sigma(gpu_device):
    H.check_degenerate(gpu_device, also_tau=H.TAU)


def test_tau_zero_is_exact(gpu_device):
    H.check_tau_zero(gpu_device)


def test_empty(gpu_device):
    H.check_empty(gpu_device)


def test_arena_hindsight(gpu_device):
    H.check_arena(gpu_device)
