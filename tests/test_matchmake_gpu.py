"""Matchmaking on the device (csrc/matchmake.hip): the split choice held bit for bit to the
oracle of matchmake_cases.py and to the host mirror, quality and p_win0 within their derived
budgets."""
import numpy as np
import pytest
import torch

from analyzer_amd.ops import balance_lobbies, preview_matches
from analyzer_amd.ops.rate import BatchRater
from analyzer_amd.ops.synth import RosterSpec, StreamSpec, make_roster, make_stream

import matchmake_cases as C

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("K", C.KS)
def test_sizes_on_device(gpu_device, K):
    C.check_sizes(K, gpu_device)


@pytest.mark.parametrize("K", C.KS)
def test_device_split_equals_host_mirror(gpu_device, K):
    lob = C.random_lobbies(K)
    dev = C.run_balance(C.random_roster(), lob, gpu_device)
    host = C.run_balance(C.random_roster(), lob, "cpu")
    for k in ("status", "split", "team0", "records"):
        assert np.array_equal(dev[k], host[k]), k
    assert set(np.unique(dev["split"]).tolist()) == set(range(C.COUNTS[K]))


def test_ties_keep_the_lower_index_on_device(gpu_device):
    C.check_ties(gpu_device)


def test_modes_fall_back_and_seeds_on_device(gpu_device):
    C.check_modes(gpu_device)


@pytest.mark.parametrize("K", C.KS)
def test_error_lobbies_leave_their_neighbours_alone_on_device(gpu_device, K):
    C.check_errors(K, gpu_device)


def test_a_roster_the_device_just_rated_is_only_read(gpu_device):
    roster = make_roster(RosterSpec(num_players=500, seed=7), device=gpu_device)
    rec = make_stream(StreamSpec(team_size=3, seed=8), 2000, 500, device=gpu_device)
    BatchRater().rate(roster, rec)
    torch.cuda.synchronize()
    assert (roster.state[:, 1::2].view(torch.int32) != 0).any(), "the launch left no live tag"
    C.check_read_only(roster, gpu_device)


@pytest.mark.parametrize("K", C.KS)
def test_preview_against_rate_on_device(gpu_device, K):
    C.check_preview(K, gpu_device)


@pytest.mark.parametrize("K", C.KS)
def test_balanced_records_are_rate_input_on_device(gpu_device, K):
    C.check_round_trip(K, gpu_device)


@pytest.mark.parametrize("Q", ("0", "1", "2K-1", "2K", "2K+1", "1000"))
@pytest.mark.parametrize("K", (1, 3, 5))
def test_make_lobbies_on_device(gpu_device, K, Q):
    C.check_make_lobbies(K, C.queue_size(K, Q), gpu_device)


def test_a_repeated_queue_id_fails_exactly_its_lobby_on_device(gpu_device):
    C.check_make_lobbies(3, 200, gpu_device, repeat=True)


def test_repeatable_empty_and_value_errors_on_device(gpu_device):
    C.check_repeatable(gpu_device)
    C.check_empty(gpu_device)
    C.check_value_errors(gpu_device)


def test_kernels_run_on_the_current_stream(gpu_device):
    K = 5
    orc = C.random_oracle(K)
    side = torch.cuda.Stream(gpu_device)
    with torch.cuda.stream(side):
        roster = C.random_roster().to(gpu_device)
        lob = torch.as_tensor(C.random_lobbies(K)).to(gpu_device)
        bal = balance_lobbies(roster, lob, "ranked", cfg=C.CFG)
        pv = preview_matches(roster, bal.records, cfg=C.CFG)
        side.synchronize()
    got = {k: getattr(bal, k).cpu().numpy() for k in bal._fields}
    C.assert_balance(got, orc, what="side stream", device=gpu_device)
    # the preview of a balanced record sees the same match: the same belief
    assert (pv.status == 0).all()
    r = C.ratio(pv.quality.cpu().numpy(), orc["q"], orc["B_q"])
    assert (r <= 1.0).all()
    r = C.ratio(pv.p_win0.cpu().numpy(), orc["p"], orc["B_p"])
    assert (r <= 1.0).all()


def test_cli_prints_the_matchmaking_line_on_device(gpu_device, capsys):
    C.check_cli(gpu_device, capsys)


def test_worst_ratios_are_reported(gpu_device):
    """Runs last in this file: the worst |error| / budget per output seen by the tests above."""
    print("worst |error| / budget:", {k: round(v, 4) for k, v in sorted(C.WORST.items())})
    assert all(v <= 1.0 for v in C.WORST.values())
