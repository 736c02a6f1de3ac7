"""Islands (K18) on the CPU: the host mirror of the island kernels against the plain Python
oracle of island_cases.py (and scipy's connected components where it imports), ``Islands`` and
its queries, the partition's rules, ``RecordArena.islands`` and the ``--islands`` command
line."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from analyzer_amd.ops import Islands
from analyzer_amd.ops.islands import partition_table
from analyzer_amd.ops.native import native

import island_cases as C
import records_cases as RC


@pytest.mark.parametrize("R", [1, 2, 7])
@pytest.mark.parametrize("K", [1, 2, 3, 4, 5])
def test_team_sizes_and_regions(K, R):
    C.check_stream(K, R, "cpu")


@pytest.mark.parametrize("K,R", [(1, 1), (3, 1), (3, 7), (5, 2)])
def test_against_scipy(K, R):
    pytest.importorskip("scipy")
    C.check_scipy(K, R)


@pytest.mark.parametrize("order", C.PATH_ORDERS)
def test_deep_paths(order):
    C.check_path(order, "cpu")


@pytest.mark.parametrize("order", C.PATH_ORDERS)
def test_deep_paths_as_edges(order):
    C.check_path(order, "cpu", edges=True)


@pytest.mark.parametrize("player", [C.HOT_P - 1, 0])
def test_one_player_in_every_match(player):
    C.check_hot(player, "cpu")


@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_bridge(where):
    C.check_bridge(where, "cpu")


def test_cuts_order_and_repeats():
    C.check_cuts("cpu")


def test_liveness_and_guards():
    C.check_liveness("cpu")


def test_edges():
    C.check_edges("cpu")


def test_from_pairs():
    C.check_from_pairs("cpu")


def test_merge():
    C.check_merge("cpu")


def test_degenerate():
    C.check_degenerate("cpu")


def test_cache():
    C.check_cache("cpu")


def test_partition_rules():
    # largest first; ties: the smaller label first, onto the lower of the least loaded ranks
    label = np.array([2, 5, 9, 11, 20, 30], dtype=np.int64)
    matches = np.array([4, 7, 4, 0, 7, 1], dtype=np.int64)
    # order: 5 (7), 20 (7), 2 (4), 9 (4), 30 (1), 11 (0)
    # on 2 ranks: 5 -> r0 (7), 20 -> r1 (7), 2 -> r0 (11), 9 -> r1 (11), 30 -> r0 (12), 11 -> r1 (11)
    assert partition_table(label, matches, 2).tolist() == [0, 0, 1, 1, 1, 0]
    # on 3 ranks: 5 -> r0 (7), 20 -> r1 (7), 2 -> r2 (4), 9 -> r2 (8), 30 -> r0 (8), 11 -> r1 (7)
    assert partition_table(label, matches, 3).tolist() == [2, 0, 2, 1, 1, 0]
    assert partition_table(label, matches, 1).tolist() == [0] * 6
    assert partition_table(label[:0], matches[:0], 4).tolist() == []


def test_partition():
    rec, rows = C.stream_case(1, 7)  # many islands
    P = C.stream_players(7)
    isl = Islands(P, "cpu").add(rec, rows)
    table, labels = isl.table(), isl.labels()
    assert table["label"].numel() > 50
    for n in (1, 3, 8, 5000):
        part = isl.partition(n)
        ranks = part["rank_of_player"]
        assert ranks.dtype == torch.int32 and ranks.shape == (P,) and part["load"].dtype == torch.int64
        assert torch.equal(ranks < 0, labels < 0) and int(ranks.max()) < n
        # every island is on one rank: a player's rank is its label's
        seen = labels >= 0
        assert torch.equal(ranks[seen], ranks[labels[seen].long()])
        assert torch.equal(ranks[table["label"]], part["rank_of_island"])
        assert int(part["load"].sum()) == int(table["matches"].sum()) == isl.summary()["matches"]
        load = torch.zeros(n, dtype=torch.int64).index_add_(0, part["rank_of_island"].long(), table["matches"])
        assert torch.equal(load, part["load"])
        assert part["imbalance"] == float(load.max()) * n / float(load.sum()) >= 1.0
        assert torch.equal(part["rank_of_island"],
                           torch.from_numpy(partition_table(table["label"].numpy(), table["matches"].numpy(), n)))
        again = isl.partition(n)
        assert torch.equal(again["rank_of_player"], ranks) and torch.equal(again["load"], part["load"])
    assert isl.partition(1)["imbalance"] == 1.0
    with pytest.raises(ValueError):
        isl.partition(0)


def test_summary_and_largest():
    isl = C.check_bridge("middle", "cpu")
    t = isl.table()
    s = isl.summary()
    assert s["islands"] == t["label"].numel() and s["players_seen"] == int(t["players"].sum()) == int(isl.seen.sum())
    assert s["singletons"] == int((t["players"] == 1).sum())
    top = int(t["matches"].argmax())
    assert s["largest"] == {"label": int(t["label"][top]), "players": int(t["players"][top]),
                            "matches": int(t["matches"][top]),
                            "share_of_matches": int(t["matches"][top]) / int(t["matches"].sum())}
    assert [r["matches"] for r in isl.largest(3)] == sorted(t["matches"].tolist(), reverse=True)[:3]


def test_bad_arguments():
    with pytest.raises(ValueError):
        Islands(4, "cpu", modes=("chess",))
    with pytest.raises(ValueError):
        Islands(1 << 31, "cpu")
    isl = Islands(C.LIVE_P, "cpu")
    rec, rows = C.CC.window(2, C.live_matches())
    with pytest.raises(ValueError):
        isl.add(rec, rows, K=3)
    with pytest.raises(RuntimeError):
        isl.add(rec, rows[:, :8].contiguous())  # not the packed rows
    with pytest.raises(RuntimeError):
        native().islands_add(isl.parent, isl.slots, isl.credit, isl.ctrl, rec, rows, C.LIVE_P, 1 << 6)
    with pytest.raises(RuntimeError):
        native().islands_add(isl.parent[:4], isl.slots, isl.credit, isl.ctrl, rec, rows, C.LIVE_P, 1)
    with pytest.raises(ValueError):
        isl.add_edges([1, 2], [3])
    with pytest.raises(ValueError):
        isl.same([0], [C.LIVE_P])
    with pytest.raises(ValueError):
        Islands.from_pairs(C.PC.run("planted", "cpu"), "near")
    assert bool((isl.parent == torch.arange(C.LIVE_P)).all()) and not bool(isl.seen.any())


def test_a_broken_parent_table_is_an_error():
    """A parent word above its own index breaks the invariant everything rests on: the mirror
    refuses to follow it."""
    isl = Islands(4, "cpu")
    isl.parent[1] = 3
    with pytest.raises(RuntimeError):
        isl.add_edges([1], [2])


def test_the_error_word_is_raised():
    C.check_error_word("cpu")


@pytest.mark.parametrize("spec", [RC.SPEC3, RC.SPEC5], ids=["3v3", "5v5"])
def test_arena_islands(spec):
    C.check_arena_islands(spec, "cpu")


def test_cli_islands():
    C.check_cli("cpu", "--device", "cpu", "--arena-free-bytes", str(1 << 30))


def test_cli_islands_argument_errors():
    env = dict(os.environ, PYTHONPATH=C.ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    base = [sys.executable, "-m", "analyzer_amd.runtime.rerate", "--device", "cpu", "--matches", "900", "--players", "120",
            "--window", "400"]
    for args in (("--islands",), ("--records", "resident", "--islands-ranks", "3"),
                 ("--records", "resident", "--islands", "--islands-ranks", "0"),
                 ("--records", "resident", "--islands", "--islands-modes", "chess")):
        bad = subprocess.run(base + list(args), capture_output=True, text=True, env=env, cwd=C.ROOT, timeout=300)
        assert bad.returncode == 2 and "--islands" in bad.stderr, (args, bad.stderr)
