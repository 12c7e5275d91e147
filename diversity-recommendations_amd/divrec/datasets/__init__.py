from .base_datasets import (
    DevicePairWiseDataset,
    DevicePointWiseDataset,
    PairWiseDataset,
    PairWiseRow,
    PointWiseDataset,
    PointWiseRow,
    RankingDataset,
    RankingRow,
    interaction_csr,
)
from .storages import Features, UserItemInteractionsDataset

__all__ = [
    "DevicePairWiseDataset",
    "DevicePointWiseDataset",
    "Features",
    "UserItemInteractionsDataset",
    "PairWiseRow",
    "PairWiseDataset",
    "PointWiseRow",
    "PointWiseDataset",
    "RankingDataset",
    "RankingRow",
    "interaction_csr",
]
