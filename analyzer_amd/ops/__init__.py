"""Batched tensor operators of the rating engine (HIP kernels on MI355X)."""
from .native import native, is_built  # noqa: F401
from .ladder import Ladder, build_ladder  # noqa: F401
from .careers import CareerTable  # noqa: F401
from .scorecard import Scorecard, match_priors  # noqa: F401
from .pairs import PairTable  # noqa: F401
from .profiles import ProfileTable  # noqa: F401
from .matchmake import (Balanced, Preview, balance_lobbies, fill_winners, make_lobbies,  # noqa: F401
                        preview_matches)
from .hindsight import Hindsight  # noqa: F401
from .through_time import ThroughTime  # noqa: F401
from .islands import Islands  # noqa: F401
from .expectations import Expectations  # noqa: F401
