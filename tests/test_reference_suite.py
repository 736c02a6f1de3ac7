"""API-parity gate: the four unit tests the reference project
keeps for its ``rater`` module (seeding, a rated match of new players, of
returning players, an AFK match), against this repository's drop-in ``rater.py``.

Their inputs and expected results are stored in
``tests/golden/reference_rater_cases.json``, so the gate needs nothing outside
the repository.  The stand-in objects below carry exactly the attributes the
reference's own test doubles carry (no ``trueskill_br_*`` / ``5v5`` columns on
the player or the participant items), and a roster holds ONE participant object
three times, as there."""
import json
import os
from types import SimpleNamespace

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "reference_rater_cases.json")) as f:
    CASES = json.load(f)

PLAYER_FIELDS = ("skill_tier", "rank_points_ranked", "rank_points_blitz", "trueskill_mu", "trueskill_sigma",
                 "trueskill_casual_mu", "trueskill_casual_sigma", "trueskill_ranked_mu", "trueskill_ranked_sigma",
                 "trueskill_blitz_mu", "trueskill_blitz_sigma")
ITEM_FIELDS = PLAYER_FIELDS[5:]


def _player(fields):
    assert set(fields) <= set(PLAYER_FIELDS), fields
    return SimpleNamespace(api_id="", **{k: fields.get(k) for k in PLAYER_FIELDS})


def _match(case):
    rosters = []
    for winner in (True, False):
        items = SimpleNamespace(api_id="", any_afk=False, **{k: None for k in ITEM_FIELDS})
        part = SimpleNamespace(api_id="", skill_tier=case["participant_skill_tier"], went_afk=case["went_afk"],
                               participant_items=[items], player=[_player(case["player"])])
        rosters.append(SimpleNamespace(api_id="", winner=winner, participants=[part] * case["team_size"]))
    return SimpleNamespace(api_id="", game_mode=case["game_mode"], rosters=rosters,
                           participants=[p for r in rosters for p in r.participants])


def _holds(value, bound):
    assert set(bound) <= {"gt", "lt", "eq"} and bound, bound
    return (("gt" not in bound or value > bound["gt"]) and ("lt" not in bound or value < bound["lt"])
            and ("eq" not in bound or value == bound["eq"]))


def _first_player(match, roster):
    return match.rosters[roster].participants[0].player[0]


def check_get_trueskill_seed(rater):
    assert len(CASES["seed"]) == 5
    for case in CASES["seed"]:
        mu, sigma = rater.get_trueskill_seed(_player(case["player"]))
        assert _holds(mu - sigma, case["mu_minus_sigma"]), (case, mu, sigma)


def check_rate_match(rater):
    case = CASES["matches"]["new"]
    match = _match(case)
    assert rater.rate_match(match) is None
    won, lost = _first_player(match, 0), _first_player(match, 1)
    assert won.trueskill_mu is not None
    assert won.trueskill_ranked_mu is not None
    assert won.trueskill_ranked_sigma < won.trueskill_ranked_mu
    assert _holds(won.trueskill_ranked_mu, case["winner_ranked_mu"]), won.trueskill_ranked_mu
    assert won.trueskill_casual_mu is None
    assert won.trueskill_mu > lost.trueskill_mu
    assert won.trueskill_ranked_mu > lost.trueskill_ranked_mu


def check_rate_match_returning(rater):
    case = CASES["matches"]["returning"]
    match = _match(case)
    rater.rate_match(match)
    won = _first_player(match, 0)
    assert _holds(won.trueskill_ranked_mu, case["winner_ranked_mu"]), won.trueskill_ranked_mu


def check_rate_match_afk(rater):
    match = _match(CASES["matches"]["afk"])
    rater.rate_match(match)
    assert _first_player(match, 0).trueskill_mu is None
    assert match.rosters[0].participants[0].participant_items[0].any_afk == True  # noqa: E712


@pytest.mark.parametrize("name", ["test_get_trueskill_seed", "test_rate_match",
                                  "test_rate_match_returning", "test_rate_match_afk"])
def test_reference_worker_test(name):
    import rater

    assert os.path.dirname(os.path.abspath(rater.__file__)) == os.path.dirname(HERE), \
        "must test this repo's rater.py"
    globals()["check_" + name[len("test_"):]](rater)
