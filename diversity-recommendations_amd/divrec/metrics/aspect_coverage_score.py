"""Expected aspect coverage of recommendation lists over a multi-hot item-aspect
matrix: the objective of the xQuAD re-rank (Santos, Macdonald, Ounis, WWW 2010;
Vargas & Castells, RecSys 2011) as a metric. Not in the reference; the aspects
are columns of its ``item_features`` (e.g. the 19 genre columns of its ML-100K
loader).

Per user: sum_a p_a (1 - prod_{j in list} (1 - c_{j,a})), c the items' aspect
values clamped to [0, 1] and p the aspect distribution of the user's
``history`` interactions (dr_aspect_profile over the history's CSR), or
p_a = 1 / G with ``uniform``: with binary aspects that is subtopic recall at k
(Zhai, Cohen, Lafferty, SIGIR 2003). dr_aspect_coverage, include/divrec_hip.h.
Higher is better; 1 is a list that covers every aspect the profile weighs.
"""
from __future__ import annotations

from typing import Optional, Sequence

import torch

from divrec import _backend, ops
from divrec.datasets import UserItemInteractionsDataset
from divrec.losses.base_losses import DatasetAwareLoss, RecommendationsAwareLoss


def aspect_matrix(dataset: UserItemInteractionsDataset, names: Sequence[str]) -> torch.Tensor:
    """fp32 [n_items, G]: the ``dataset.item_features`` columns ``names`` side
    by side, the item-aspect matrix of ``ops.xquad_rerank``. ValueError without
    names, for a column the dataset does not have, or for more columns than the
    xQuAD kernels hold (ops.XQUAD_MAX_ASPECTS)."""
    names = list(names)
    if not names:
        raise ValueError("items_aspect_features must name at least one item feature")
    if len(names) > ops.XQUAD_MAX_ASPECTS:
        raise ValueError(f"at most {ops.XQUAD_MAX_ASPECTS} aspect features, got {len(names)}")
    for name in names:
        if dataset.item_features is None or name not in dataset.item_features:
            raise ValueError(f"the dataset has no item feature {name!r} to form an aspect from")
    return torch.stack([dataset.item_features[name].to(torch.float32) for name in names],
                       dim=1).contiguous()


class AspectCoverageScore(RecommendationsAwareLoss, DatasetAwareLoss):
    """``AspectCoverageScore(dataset=..., items_aspect_features=[...],
    history=None, uniform=False)``: ``history`` (a UserItemInteractionsDataset)
    is where the users' profiles come from; it defaults to ``dataset``'s own
    interactions (pass the train set to score the lists of a test split).
    ``uniform`` scores against p_a = 1 / G instead. The device matrix and the
    profile are built on first use and kept (``refresh()`` drops them after
    the history or the features change)."""

    def __init__(self, *args, items_aspect_features: Sequence[str],
                 history: Optional[UserItemInteractionsDataset] = None, uniform: bool = False,
                 **kwargs):
        DatasetAwareLoss.__init__(self, *args, **kwargs)
        RecommendationsAwareLoss.__init__(self, *args, **kwargs)
        self.items_aspect_features = list(items_aspect_features)
        self.history = history if history is not None else self.dataset
        self.uniform = bool(uniform)
        self.aspects = aspect_matrix(self.dataset, self.items_aspect_features)
        self.n_aspects = self.aspects.size(1)
        self._dev_aspects = None
        self._dev_profile = None

    def refresh(self) -> None:
        self.aspects = aspect_matrix(self.dataset, self.items_aspect_features)
        self._dev_aspects = None
        self._dev_profile = None

    def device_aspects(self, device: torch.device) -> torch.Tensor:
        if self._dev_aspects is None or self._dev_aspects.device != device:
            self._dev_aspects = self.aspects.to(device).contiguous()
        return self._dev_aspects

    def profile(self, device: torch.device) -> torch.Tensor:
        """fp32 [number_of_users, n_aspects] on ``device``: each user's aspect
        shares over ``history`` (a zero row for a user without any), or ones
        with ``uniform`` (the kernel normalises the row)."""
        if self._dev_profile is None or self._dev_profile.device != device:
            n_users = int(self.dataset.number_of_users)
            if self.uniform:
                self._dev_profile = torch.ones((n_users, self.n_aspects), dtype=torch.float32,
                                               device=device)
            else:
                rowptr, items = self.history.user_item_csr(n_users)
                self._dev_profile = ops.aspect_profile(rowptr.to(device), items.to(device),
                                                       self.device_aspects(device))
        return self._dev_profile

    def per_user(self, recommendations: torch.Tensor) -> torch.Tensor:
        """Coverage per user on the device (no reduction); row u of the
        recommendations is user u."""
        dev = recommendations.device if recommendations.is_cuda else _backend.default_device()
        profile = self.profile(dev)
        if recommendations.dim() != 2 or recommendations.size(0) != profile.size(0):
            raise ValueError(f"expected one list per user ([{profile.size(0)}, k]), got "
                             f"{tuple(recommendations.shape)}")
        return ops.aspect_coverage(recommendations.to(dev), self.device_aspects(dev), profile)

    def recommendations_loss(self, interactions, recommendations) -> torch.Tensor:
        return self.per_user(recommendations).to(recommendations.device)
