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
from .feature_maps import FeatureCSR, feature_csr
from .storages import Features, UserItemInteractionsDataset

__all__ = [
    "DevicePairWiseDataset",
    "DevicePointWiseDataset",
    "FeatureCSR",
    "Features",
    "UserItemInteractionsDataset",
    "PairWiseRow",
    "PairWiseDataset",
    "PointWiseRow",
    "PointWiseDataset",
    "RankingDataset",
    "RankingRow",
    "feature_csr",
    "interaction_csr",
]
