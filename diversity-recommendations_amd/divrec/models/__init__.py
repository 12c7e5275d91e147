from .base_models import RankingModel
from .feature_matrix_factorization import FeatureMatrixFactorization
from .matrix_factorization import MatrixFactorization
from .random_model import RandomModel

__all__ = ["FeatureMatrixFactorization", "MatrixFactorization", "RankingModel", "RandomModel"]
