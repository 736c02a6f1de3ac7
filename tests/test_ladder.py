"""The ladder on the CPU: the host mirror (csrc/host.cpp host_ladder) held exactly to the
oracle of ladder_cases.py, the Python API and the re-rate command line."""
import numpy as np
import pytest
import torch

from analyzer_amd.ops import Ladder, build_ladder
from analyzer_amd.ops.rate import Roster

import ladder_cases as C


@pytest.mark.parametrize("P", C.SIZES)
def test_host_ladder_equals_oracle(P):
    C.check_sizes(P, "cpu")


def test_empty_roster_gives_empty_outputs():
    lad = build_ladder(Roster.empty(0), C.TRACKS)
    assert isinstance(lad, Ladder) and lad.num_players == 0
    for t in C.TRACKS:
        assert lad.ranked(t) == 0 and lad.order(t).shape == lad.score(t).shape == lad.rank(t).shape == (0,)
        assert lad.order(t).dtype == lad.rank(t).dtype == torch.int32 and lad.score(t).dtype == torch.float32


def test_tag_words_never_matter():
    C.check_live_tags("cpu")


def test_all_null():
    C.check_all_null("cpu")


def test_all_tied_orders_by_id_across_tiles():
    C.check_all_tied("cpu")


def test_few_distinct_scores():
    C.check_few_distinct("cpu")


def test_special_values():
    C.check_specials("cpu")


def test_max_sigma_is_inclusive_and_nan_sigma_is_unranked():
    C.check_max_sigma("cpu")


def test_multi_track_builds_equal_single_track_builds():
    C.check_multi_track("cpu")


def test_round_trips_and_repeatability():
    C.check_repeatable("cpu")


def test_top_lookup_cutoff():
    C.check_api("cpu")


def test_roster_object_and_default_track():
    st = C.random_state(65)
    roster = Roster(torch.from_numpy(st), torch.zeros(65, 4))
    lad = build_ladder(roster)
    assert lad.tracks == ("shared",)
    C.assert_same(C.outputs(lad, "trueskill"), C.oracle(st, "shared"), "default build")


def test_value_errors():
    st = torch.from_numpy(C.random_state(64))
    for bad in ("rankd", "trueskill_", "", "spare", 3):
        with pytest.raises(ValueError):
            build_ladder(st, (bad,))
    with pytest.raises(ValueError):
        build_ladder(st, ())
    with pytest.raises(ValueError):
        build_ladder(st.to(torch.float64))
    with pytest.raises(ValueError):
        build_ladder(st.to(torch.float16))
    with pytest.raises(ValueError):
        build_ladder(torch.from_numpy(C.random_state(64)).t().contiguous().t())  # [64, 32], column-major
    with pytest.raises(ValueError):
        build_ladder(torch.zeros(128, 64)[:, :32])
    with pytest.raises(ValueError):
        build_ladder(torch.zeros(64, 16))
    with pytest.raises(ValueError):
        build_ladder(st, score="sigma")
    lad = build_ladder(st, ("shared",))
    with pytest.raises(ValueError):
        lad.rank("ranked")  # not built
    with pytest.raises(ValueError):
        lad.lookup("shared", [64])
    with pytest.raises(ValueError):
        lad.cutoff("shared", 1.5)


def test_key_is_monotone_and_invertible_through_the_outputs():
    """Random bit patterns as mu (sigma 0, so the score is mu + 0): the output scores are
    the canonicalised inputs bit for bit, in the oracle's order."""
    rng = np.random.default_rng(9)
    P = C.TILE + 1
    mu = rng.integers(0, 1 << 32, P, dtype=np.uint64).astype(np.uint32).view(np.float32)
    st = C.set_track(C.empty_state(P), "blitz", mu, np.zeros(P))
    lad = C.check(st, "cpu", tracks=("blitz",), what="random bits")
    assert 0 < lad.ranked("blitz") < P  # the NaN patterns dropped out


def test_cli_prints_the_ladder(capsys):
    C.check_cli("cpu", capsys)
