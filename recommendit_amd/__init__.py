"""recommendit_amd -- MI355X-native (gfx950) hot path of sarihammad/recommendit.

Same names as the reference's ``src/models/__init__.py:1-3`` so callers switch with one import:
``from recommendit_amd import TwoTowerModel, FAISSIndex, LightGBMRanker``.
"""
from .two_tower import ItemTower, TwoTowerModel, UserTower, N_GENRES  # noqa: F401
from .faiss_index import FAISSIndex  # noqa: F401
from .ranker import LightGBMRanker  # noqa: F401
from .sq8_index import SQ8Index  # noqa: F401  (not in the reference: 8-bit scalar-quantised index, sq8_index.py)
from .pq_index import PQIndex  # noqa: F401  (not in the reference: product-quantised index, pq_index.py)
from .seen import SeenItems  # noqa: F401  (not in the reference: per-user exclusion of seen items, seen.py)
from .coldstart import UserHistories  # noqa: F401  (not in the reference: cold-start users from rating histories, coldstart.py)
from .rerank import mmr_rerank_device  # noqa: F401  (not in the reference: diversified top-k, rerank.py)
from .validation import RankValidator  # noqa: F401  (not in the reference: validation while training, validation.py)
from ._lib import have_gpu  # noqa: F401  (the switch a caller guards the swap with: INTEGRATION.md §1)

__all__ = ["TwoTowerModel", "UserTower", "ItemTower", "FAISSIndex", "SQ8Index", "PQIndex", "LightGBMRanker", "SeenItems", "UserHistories", "mmr_rerank_device", "RankValidator", "N_GENRES",
           "have_gpu"]
