"""The ladder on the device (csrc/ladder.hip): held bit for bit to the host mirror and to
the oracle of ladder_cases.py."""
import numpy as np
import pytest
import torch

from analyzer_amd.ops import build_ladder
from analyzer_amd.ops.rate import BatchRater
from analyzer_amd.ops.synth import RosterSpec, StreamSpec, make_roster, make_stream

import ladder_cases as C

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("P", C.SIZES)
def test_device_ladder_equals_host_mirror_and_oracle(gpu_device, P):
    C.check_sizes(P, gpu_device)


def test_tag_words_never_matter_on_device(gpu_device):
    C.check_live_tags(gpu_device)


def test_ladder_of_a_roster_the_device_just_rated(gpu_device):
    roster = make_roster(RosterSpec(num_players=500, seed=7), device=gpu_device)
    rec = make_stream(StreamSpec(team_size=3, seed=8), 2000, 500, device=gpu_device)
    BatchRater().rate(roster, rec)
    torch.cuda.synchronize()
    host = roster.to("cpu")
    assert (host.state[:, 1::2].view(torch.int32) != 0).any(), "the launch left no live tag"
    dev_lad, host_lad = build_ladder(roster, C.TRACKS), build_ladder(host, C.TRACKS)
    st = host.state.numpy()
    for t in C.TRACKS:
        C.assert_same(C.outputs(dev_lad, t), C.outputs(host_lad, t), "rated roster, %s" % t)
        C.assert_same(C.outputs(dev_lad, t), C.oracle(st, t), "rated roster vs oracle, %s" % t)
    assert dev_lad.ranked("shared") > 0
    assert torch.equal(roster.state.cpu().view(torch.int32), host.state.view(torch.int32))


def test_all_null_on_device(gpu_device):
    C.check_all_null(gpu_device)


def test_all_tied_orders_by_id_across_tiles_on_device(gpu_device):
    C.check_all_tied(gpu_device)


def test_few_distinct_scores_on_device(gpu_device):
    C.check_few_distinct(gpu_device)


def test_special_values_on_device(gpu_device):
    C.check_specials(gpu_device)


def test_max_sigma_on_device(gpu_device):
    C.check_max_sigma(gpu_device)


def test_multi_track_builds_equal_single_track_builds_on_device(gpu_device):
    C.check_multi_track(gpu_device)


def test_round_trips_and_repeatability_on_device(gpu_device):
    C.check_repeatable(gpu_device)


def test_top_lookup_cutoff_on_device(gpu_device):
    C.check_api(gpu_device)


def test_random_bit_patterns_on_device(gpu_device):
    rng = np.random.default_rng(9)
    P = C.TILE + 1
    mu = rng.integers(0, 1 << 32, P, dtype=np.uint64).astype(np.uint32).view(np.float32)
    st = C.set_track(C.empty_state(P), "blitz", mu, np.zeros(P))
    C.check(st, gpu_device, tracks=("blitz",), what="random bits")


def test_ladder_runs_on_the_current_stream(gpu_device):
    st = C.random_state(C.TILE + 1)
    side = torch.cuda.Stream(gpu_device)
    with torch.cuda.stream(side):
        state = torch.from_numpy(st).to(gpu_device, non_blocking=False)
        lad = build_ladder(state, ("shared", "br"))
        side.synchronize()
    for t in ("shared", "br"):
        C.assert_same(C.outputs(lad, t), C.oracle(st, t), "side stream, %s" % t)


def test_value_errors_on_device(gpu_device):
    st = torch.from_numpy(C.random_state(64)).to(gpu_device)
    with pytest.raises(ValueError):
        build_ladder(st, ("rankd",))
    with pytest.raises(ValueError):
        build_ladder(st.to(torch.float64))
    with pytest.raises(ValueError):
        build_ladder(torch.zeros(128, 64, device=gpu_device)[:, :32])
    with pytest.raises(ValueError):
        build_ladder(st, score="sigma")


def test_cli_prints_the_ladder_on_device(gpu_device, capsys):
    C.check_cli(gpu_device, capsys)
