"""Islands: the connected components of the match graph (K18, csrc/islands.hip,
csrc/island_core.h).

The vertices are the players; an edge joins any two *live* slots of one match.  A slot is live
as ``ops/pairs.py`` has it: it is occupied, its id lies in [0, P), the match's mode is one of
the selected modes and the match was rated.  AFK, invalid, unsupported, failed and malformed
matches join nobody.  A rating only means something relative to the players it is connected to
through rated matches, so two islands carry ratings on unrelated scales.

    isl = Islands(P, device)                       # or arena.islands(P, rec_of)
    isl.add(rec, res.packed)                       # any window, any order, any number of times
    isl.labels()                                   # the smallest id of each player's island, -1: never seen
    isl.same([17, 4242], [99, 17])                 # comparable ratings?
    isl.table()                                    # label, players, matches, player_games per island
    isl.summary()                                  # how many islands, how big is the biggest
    isl.partition(8)                               # whole islands onto 8 ranks

The label of an island is the smallest id in it and every counter is an integer sum, so all of
this is the same bits on every run, on the device and in the host mirror, in any window order
and however a window is cut.  A match is credited to the player in its first live slot, so an
island's ``matches`` counts each rated match once.
"""
from __future__ import annotations

import heapq
from typing import Dict, Iterable, Optional

import numpy as np
import torch

from .careers import _window_chunks, modes_mask
from .native import native

RELATIONS = ("with", "against", "any")


def pair_edges(pairs, relation: str = "with", min_games: int = 1, min_win_rate: Optional[float] = None):
    """The rows (a, b) of a ``PairTable`` that met in ``relation`` at least ``min_games`` times,
    a winning at least ``min_win_rate`` of them (None: any): int32 tensors ``a``, ``b``."""
    if relation not in RELATIONS:
        raise ValueError("unknown relation %r: one of %s" % (relation, ", ".join(RELATIONS)))
    keys, counts = pairs.keys, pairs.counts.to(torch.int64)
    if relation == "with":
        games, wins = counts[:, 0], counts[:, 1]
    elif relation == "against":
        games, wins = counts[:, 2], counts[:, 3]
    else:
        games, wins = counts[:, 0] + counts[:, 2], counts[:, 1] + counts[:, 3]
    keep = games >= max(1, int(min_games))
    if min_win_rate is not None:
        keep &= wins.to(torch.float64) / games.to(torch.float64) >= float(min_win_rate)  # 0 / 0: no
    keys = keys[keep]
    return (keys >> 32).to(torch.int32), (keys & 0xFFFFFFFF).to(torch.int32)


class Islands:
    """The island forest of ``num_players`` players on ``device``, initially every player
    unseen and alone.  ``modes``: names of the modes whose matches count (None: all)."""

    def __init__(self, num_players: int, device, modes: Optional[Iterable[str]] = None):
        self.num_players = int(num_players)
        if not 0 <= self.num_players < 1 << 31:
            raise ValueError("an island forest holds fewer than 2^31 players")
        self.device = torch.device(device)
        self.modes = modes_mask(modes)
        self.max_slots = int(native().MAX_SLOTS)  # slots per kernel call; ``add`` splits above it
        self._seen_bit = int(native().ISLAND_SEEN_BIT)
        self.parent = torch.arange(self.num_players, dtype=torch.int32, device=self.device)
        self.slots = torch.zeros(self.num_players, dtype=torch.int32, device=self.device)
        self.credit = torch.zeros(self.num_players, dtype=torch.int32, device=self.device)
        self.ctrl = torch.zeros(2, dtype=torch.int64, device=self.device)  # sticky error, bad edges
        self._flat = True
        self._table: Optional[Dict[str, torch.Tensor]] = None

    # ------------------------------------------------------------------ building
    def _dirty(self) -> None:
        self._flat = False
        self._table = None

    def add(self, rec: torch.Tensor, rows: torch.Tensor, K: Optional[int] = None) -> "Islands":
        """Unite the live slots of every rated match of one window: its records ``rec``
        [M, 2K+2] and packed output rows ``rows`` [M, W].  Windows may come in any order.  A
        window above the kernels' slot limit is split into chunks, which is exact."""
        for a, b in _window_chunks(rec, rows, K, self.max_slots)[1]:
            native().islands_add(self.parent, self.slots, self.credit, self.ctrl, rec[a:b], rows[a:b],
                                 self.num_players, self.modes)
        self._dirty()
        return self

    def _edges(self, a, b, mark: bool) -> None:
        a = torch.as_tensor(a, dtype=torch.int32).reshape(-1).to(self.device).contiguous()
        b = torch.as_tensor(b, dtype=torch.int32).reshape(-1).to(self.device).contiguous()
        if a.numel() != b.numel():
            raise ValueError("one b per a")
        native().islands_edges(self.parent, self.slots, self.ctrl, a, b, self.num_players, mark)
        self._dirty()

    def add_edges(self, a, b) -> "Islands":
        """Unite a[i] with b[i] for arbitrary edges (int32 ids).  Both endpoints count as seen;
        a self loop unites nothing; an edge with an endpoint outside [0, P) is dropped and
        counted in ``bad``."""
        self._edges(a, b, True)
        return self

    @classmethod
    def from_pairs(cls, pairs, relation: str = "with", min_games: int = 1,
                   min_win_rate: Optional[float] = None) -> "Islands":
        """The islands of the rows of a ``PairTable`` that ``pair_edges`` keeps:
        ``from_pairs(pairs, "against", min_games=20, min_win_rate=0.9)`` are the rings behind
        ``PairTable.suspects``."""
        a, b = pair_edges(pairs, relation, min_games, min_win_rate)
        return cls(pairs.num_players, pairs.device).add_edges(a, b)

    def merge(self, other: "Islands") -> "Islands":
        """The union of this forest with ``other``, built with the same options: the counters
        add up."""
        if (self.num_players, self.modes) != (other.num_players, other.modes):
            raise ValueError("the forests were built with different options")
        ids = torch.arange(self.num_players, dtype=torch.int32, device=self.device)
        self._edges(ids, other.parent.to(self.device), False)  # i is of its parent's island there
        mine, theirs = self.slots.to(torch.int64), other.slots.to(self.device).to(torch.int64)
        low = self._seen_bit - 1
        words = ((mine & low) + (theirs & low)) | ((mine | theirs) & self._seen_bit)
        self.slots.copy_(((words + (1 << 31)) % (1 << 32) - (1 << 31)).to(torch.int32))
        self.credit += other.credit.to(self.device)
        theirs = other.ctrl.to(self.device)
        self.ctrl[0] |= theirs[0]  # error bits
        self.ctrl[1] += theirs[1]
        return self

    # ------------------------------------------------------------------ reading
    def _check(self) -> None:
        err = int(self.ctrl[0])
        if err:
            raise RuntimeError("islands: %s" % " and ".join(
                text for bit, text in ((int(native().ISLAND_ERR_STEPS), "a find or a union took more than P steps"),
                                       (int(native().ISLAND_ERR_PARENT), "a parent word lies outside [0, its index]"))
                if err & bit))

    @property
    def bad(self) -> int:
        """Edges of ``add_edges`` dropped for an endpoint outside [0, P)."""
        self._check()
        return int(self.ctrl[1])

    def _flatten(self) -> None:
        if not self._flat:
            native().islands_flatten(self.parent, self.ctrl, self.num_players)
        self._check()
        self._flat = True

    @property
    def seen(self) -> torch.Tensor:
        """bool [P]: the player held a live slot of a rated match or an end of an edge."""
        return self.slots != 0

    def labels(self) -> torch.Tensor:
        """int32 [P]: the smallest id of the player's island, -1 if the player was never seen."""
        self._flatten()
        return torch.where(self.seen, self.parent, torch.full_like(self.parent, -1))

    def same(self, a, b) -> torch.Tensor:
        """bool [n]: a[i] and b[i] are of one island; False if either was never seen."""
        a = torch.as_tensor(a, device=self.device).to(torch.int64).reshape(-1)
        b = torch.as_tensor(b, device=self.device).to(torch.int64).reshape(-1)
        if a.numel() != b.numel():
            raise ValueError("one b per a")
        for ids in (a, b):
            if ids.numel() and (int(ids.min()) < 0 or int(ids.max()) >= self.num_players):
                raise ValueError("player ids must lie in [0, %d)" % self.num_players)
        labels = self.labels()
        la, lb = labels.index_select(0, a), labels.index_select(0, b)
        return (la == lb) & (la >= 0)

    def table(self) -> Dict[str, torch.Tensor]:
        """One row per island in ascending ``label``: ``players``, ``matches`` (rated matches,
        each counted once) and ``player_games`` (live slots), all int64."""
        if self._table is None:
            self._flatten()
            census = native().islands_census(self.parent, self.slots, self.credit, self.ctrl, self.num_players)
            self._check()
            label = census[0].nonzero().reshape(-1)
            self._table = {"label": label, "players": census[0].index_select(0, label),
                           "matches": census[1].index_select(0, label),
                           "player_games": census[2].index_select(0, label)}
        return dict(self._table)

    def summary(self) -> dict:
        """``islands``, ``players_seen``, ``matches``, ``singletons`` and the ``largest`` island
        by matches (ties: the smaller label): label, players, matches, share_of_matches."""
        t = {k: v.cpu() for k, v in self.table().items()}
        n, total = int(t["label"].numel()), int(t["matches"].sum())
        out = {"islands": n, "players_seen": int(t["players"].sum()), "matches": total,
               "singletons": int((t["players"] == 1).sum()), "largest": None}
        if n:
            i = int((t["matches"] == t["matches"].max()).nonzero()[0])  # the first: the smallest label
            out["largest"] = {"label": int(t["label"][i]), "players": int(t["players"][i]),
                              "matches": int(t["matches"][i]),
                              "share_of_matches": int(t["matches"][i]) / total if total else None}
        return out

    def largest(self, top: int = 10) -> list:
        """The ``top`` islands by matches, ties by ascending label, as JSON-ready dicts."""
        t = {k: v.cpu() for k, v in self.table().items()}
        order = torch.sort(t["matches"], descending=True, stable=True).indices[:max(0, int(top))]
        return [{"label": int(t["label"][i]), "players": int(t["players"][i]), "matches": int(t["matches"][i]),
                 "player_games": int(t["player_games"][i])} for i in order.tolist()]

    def partition(self, n: int) -> Dict[str, object]:
        """Whole islands onto ``n`` ranks: the islands in descending ``matches`` (ties: the
        smaller label first), each onto the rank with the least load so far (ties: the lower
        rank).  ``rank_of_player`` int32 [P] (-1: never seen), ``rank_of_island`` int32 per
        table row, ``load`` int64 [n] (matches) and ``imbalance`` = max load / mean load (None
        without a match)."""
        n = int(n)
        if n < 1:
            raise ValueError("at least one rank")
        t = self.table()
        rank_of_island = partition_table(t["label"].cpu().numpy(), t["matches"].cpu().numpy(), n)
        load = np.zeros(n, dtype=np.int64)
        np.add.at(load, rank_of_island, t["matches"].cpu().numpy())
        labels = self.labels().to(torch.int64)
        of_label = torch.full((max(1, self.num_players),), -1, dtype=torch.int32, device=self.device)
        of_label[t["label"]] = torch.from_numpy(rank_of_island).to(self.device)
        rank_of_player = torch.where(labels >= 0, of_label[:self.num_players].index_select(0, labels.clamp(min=0)),
                                     torch.full_like(labels, -1, dtype=torch.int32))
        total = int(load.sum())
        return {"rank_of_player": rank_of_player, "rank_of_island": torch.from_numpy(rank_of_island),
                "load": torch.from_numpy(load), "imbalance": float(load.max()) * n / total if total else None}


def partition_table(label: np.ndarray, matches: np.ndarray, n: int) -> np.ndarray:
    """The rank int32 [islands] of each row of an island table under ``Islands.partition``'s
    rule: largest ``matches`` first (ties: the smaller label) onto the least loaded of ``n``
    ranks (ties: the lower rank)."""
    order = np.lexsort((label, -matches.astype(np.int64)))
    ranks = np.zeros(label.shape[0], dtype=np.int32)
    heap = [(0, r) for r in range(n)]  # (load, rank): the least load, then the lower rank
    for i in order.tolist():
        load, r = heapq.heappop(heap)
        ranks[i] = r
        heapq.heappush(heap, (load + int(matches[i]), r))
    return ranks


def islands_line(isl: Islands, top: int = 10, ranks: Optional[int] = None) -> dict:
    """The summary, the ``top`` largest islands and, with ``ranks``, the partition's loads and
    imbalance, as one JSON-ready dict."""
    line = {"islands": isl.summary(), "largest": isl.largest(top), "bad_edges": isl.bad}
    if ranks is not None:
        part = isl.partition(ranks)
        line["partition"] = {"ranks": int(ranks), "load": part["load"].tolist(), "imbalance": part["imbalance"]}
    return line
