"""WARP ranking loss (Weston, Bengio, Usunier 2011, as LightFM implements it;
not in the reference).

``divrec.train.warp_train_loop`` draws each pair's negatives itself, until one
violates the margin or ``max_trials`` draws are used up, and weights the
update by the rank the number of draws implies: the sampling, the loss and its
gradients are one dr_warp_fwd_bwd per batch, and this object carries the two
settings. On GIVEN (positive, negative) scores, as the generic
``pair_wise_train_loop`` and ``pair_wise_score_loop`` hand them over, the loss
is the plain hinge the violation test is made of."""
import torch

from .base_losses import PairWiseLoss


class WARPLoss(PairWiseLoss):
    def __init__(self, margin: float = 1.0, max_trials: int = 100, *args, **kwargs):
        PairWiseLoss.__init__(self, *args, **kwargs)
        self.margin = float(margin)
        self.max_trials = int(max_trials)
        if not torch.isfinite(torch.tensor(self.margin)):
            raise ValueError("margin must be finite")
        if self.max_trials < 1:
            raise ValueError("max_trials must be >= 1")

    def pair_wise(self, positives: torch.Tensor, negatives: torch.Tensor) -> torch.Tensor:
        return torch.clamp(self.margin - positives + negatives, min=0)
