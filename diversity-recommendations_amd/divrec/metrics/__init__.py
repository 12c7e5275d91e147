from divrec.losses.intra_list_diversity_score import IntraListDiversityScore

from .aspect_coverage_score import AspectCoverageScore, aspect_matrix
from .auc_score import AUCScore
from .average_precision_at_k import (
    AveragePrecisionAtKScore,
    MeanAveragePrecisionAtKScore,
    average_precision_at_k,
)
from .calibration_score import CalibrationScore
from .entropy_diversity_score import EntropyDiversityScore
from .normalized_discounted_cumulative_gain import NDCGScore, normalized_discounted_cumulative_gain
from .popularity_rank_correlation_for_items import PRI, avg_rank, rank
from .precision_at_k import HitRateScore, PrecisionAtKScore, precision_at_k
from .recall_at_k import RecallAtKScore, recall_at_k
from .serendipity_scores import (
    NoveltyScore,
    SerendipityScore,
    UnexpectednessScore,
    novelty_item_values,
    relevance_flags,
)

__all__ = [
    "AUCScore",
    "AspectCoverageScore",
    "AveragePrecisionAtKScore",
    "CalibrationScore",
    "EntropyDiversityScore",
    "HitRateScore",
    "IntraListDiversityScore",
    "MeanAveragePrecisionAtKScore",
    "NDCGScore",
    "NoveltyScore",
    "avg_rank",
    "rank",
    "PRI",
    "PrecisionAtKScore",
    "RecallAtKScore",
    "SerendipityScore",
    "UnexpectednessScore",
    "aspect_matrix",
    "average_precision_at_k",
    "normalized_discounted_cumulative_gain",
    "novelty_item_values",
    "precision_at_k",
    "recall_at_k",
    "relevance_flags",
]
