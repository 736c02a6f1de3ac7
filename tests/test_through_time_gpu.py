"""Through time (K20) on the device: the kernels of csrc/ttt.hip -- both directions of every
chain as segmented scans over a Kalman element, and the match factors -- against the host mirror
at twice the bound of through_time_cases.py, and against its 50-digit oracle."""
import numpy as np
import pytest

import hindsight_cases as H
import through_time_cases as T

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("K", H.KS)
def test_oracle_and_mirror(gpu_device, K):
    """Rated by ``BatchRater`` on the device.  After 0 and 8 sweeps the kernels against the
    mirror on the same rows at twice the bound; after 3 against the oracle itself."""
    start, rec, rows, P = T.mixed(K, gpu_device)
    for s in (0, 8):
        out, res, tt = T.fit(gpu_device, start, rec, rows, s)
        ref, mres, mt = T.fit("cpu", start, rec, rows, s)
        assert (tt.bad, tt.flat, tt.inconsistent) == (mt.bad, mt.flat, mt.inconsistent)
        T.check_against_mirror(out, ref, "K=%d after %d sweeps" % (K, s))
        assert np.allclose(res.residual, mres.residual, rtol=0, atol=T.fp64_slack(rec, rows, P))
    ex = T.oracle(start, rec, rows, P, sweeps=3, snapshots=(3,))
    out, _, tt = T.fit(gpu_device, start, rec, rows, 3)
    assert (tt.bad, tt.flat, tt.inconsistent) == ex.counters
    T.check_against_oracle(out, ex, 3, "K=%d after 3 sweeps on the device" % K)


def test_mode_track_and_damping(gpu_device):
    start, rec, rows, P = T.mixed(3, gpu_device)
    out, _, _ = T.fit(gpu_device, start, rec, rows, 3, track="ranked", damping=0.5)
    ref, _, _ = T.fit("cpu", start, rec, rows, 3, track="ranked", damping=0.5)
    T.check_against_mirror(out, ref, "ranked track, damping 0.5")
    assert not np.isnan(ref).all()


def test_zero_sweeps_is_hindsight(gpu_device):
    T.check_equals_hindsight(gpu_device)


def test_one_element_per_player(gpu_device):
    """The kernels on the rows of ``T.singles``: the filter correctly rounded, nothing seeded."""
    T.check_singles(gpu_device)


def test_one_element_per_player_device_rated_is_the_exact_posterior(gpu_device):
    T.check_singles_exact(gpu_device)


@pytest.mark.parametrize("name", ["tiles", "every", "inner", "edges"])
def test_scan_shapes(gpu_device, name):
    T.check_shape(gpu_device, name)


def test_tau_zero(gpu_device):
    T.check_shape(gpu_device, "tiles", tau=0.0)


def test_small_histories(gpu_device):
    T.check_small(gpu_device)


def test_same_bits_on_every_run(gpu_device):
    """No float atomics, an integer max for the residual: a second fit gives the first one's bits."""
    start, rec, rows, P = T.shape("edges", gpu_device)
    first, fres, _ = T.fit(gpu_device, start, rec, rows, 2)
    again, ares, _ = T.fit(gpu_device, start, rec, rows, 2)
    assert np.array_equal(first.view(np.uint32), again.view(np.uint32)) and fres.residual == ares.residual


def test_convergence_and_not_hindsight(gpu_device):
    T.check_convergence(gpu_device)


def test_counters_and_wrong_roster(gpu_device):
    T.check_counters(gpu_device)


def test_arena_through_time(gpu_device):
    T.check_arena(gpu_device)
