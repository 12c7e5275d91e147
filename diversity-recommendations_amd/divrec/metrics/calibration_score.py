"""Calibration of recommendation lists against the users' history over item
partition labels (Steck, "Calibrated Recommendations", RecSys 2018). Not in
the reference; the labels are its ``item_features["partition"]``, the surface
of IntraListBinaryUnfairnessScore.

Per user: KL(p || q~), p the label distribution of the user's ``history``
interactions and q~ that of the recommended list, smoothed with p
(dr_calibration_kl, include/divrec_hip.h); 0 is a perfectly calibrated list.
The profile is one dr_label_profile over the history's CSR. Lower is better.
"""
from __future__ import annotations

from typing import Optional

import torch

from divrec import _backend, ops
from divrec.datasets import UserItemInteractionsDataset
from divrec.losses.base_losses import DatasetAwareLoss, RecommendationsAwareLoss


def partition_labels(dataset: UserItemInteractionsDataset, feature: str) -> torch.Tensor:
    """The int64 item labels ``dataset.item_features[feature]`` and their
    count G = max + 1; ValueError without the feature, for a negative label or
    for more labels than the calibration kernels hold (ops.CALIB_MAX_LABELS)."""
    if dataset.item_features is None or feature not in dataset.item_features:
        raise ValueError(f"the dataset has no item feature {feature!r} to calibrate against")
    labels = dataset.item_features[feature].to(torch.int64).contiguous()
    if labels.numel() == 0:
        raise ValueError(f"item feature {feature!r} is empty")
    lo, hi = int(labels.min()), int(labels.max())
    if lo < 0 or hi >= ops.CALIB_MAX_LABELS:
        raise ValueError(f"item feature {feature!r} must hold labels in [0, {ops.CALIB_MAX_LABELS}), "
                         f"got [{lo}, {hi}]")
    return labels


class CalibrationScore(RecommendationsAwareLoss, DatasetAwareLoss):
    """``CalibrationScore(dataset=..., items_partition_feature="partition",
    history=None)``: ``history`` (a UserItemInteractionsDataset) is where the
    users' profiles come from; it defaults to ``dataset``'s own interactions
    (pass the train set to score the lists of a test split). The device
    labels and the profile are built on first use and kept (``refresh()``
    drops them after the history or the labels change)."""

    def __init__(self, *args, items_partition_feature: str = "partition",
                 history: Optional[UserItemInteractionsDataset] = None, **kwargs):
        DatasetAwareLoss.__init__(self, *args, **kwargs)
        RecommendationsAwareLoss.__init__(self, *args, **kwargs)
        self.items_partition_feature = items_partition_feature
        self.history = history if history is not None else self.dataset
        self.labels = partition_labels(self.dataset, items_partition_feature)
        self.n_labels = int(self.labels.max()) + 1
        self._dev_labels = None
        self._dev_profile = None

    def refresh(self) -> None:
        self._dev_labels = None
        self._dev_profile = None

    def device_labels(self, device: torch.device) -> torch.Tensor:
        if self._dev_labels is None or self._dev_labels.device != device:
            self._dev_labels = self.labels.to(device=device, dtype=torch.int32).contiguous()
        return self._dev_labels

    def profile(self, device: torch.device) -> torch.Tensor:
        """fp32 [number_of_users, n_labels] on ``device``: each user's label
        histogram over ``history`` (a zero row for a user without any)."""
        if self._dev_profile is None or self._dev_profile.device != device:
            rowptr, items = self.history.user_item_csr(int(self.dataset.number_of_users))
            self._dev_profile = ops.label_profile(rowptr.to(device), items.to(device),
                                                  self.device_labels(device), self.n_labels)
        return self._dev_profile

    def per_user(self, recommendations: torch.Tensor) -> torch.Tensor:
        """KL per user on the device (no reduction); row u of the
        recommendations is user u."""
        dev = recommendations.device if recommendations.is_cuda else _backend.default_device()
        profile = self.profile(dev)
        if recommendations.dim() != 2 or recommendations.size(0) != profile.size(0):
            raise ValueError(f"expected one list per user ([{profile.size(0)}, k]), got "
                             f"{tuple(recommendations.shape)}")
        return ops.calibration_kl(recommendations.to(dev), self.device_labels(dev), profile)

    def recommendations_loss(self, interactions, recommendations) -> torch.Tensor:
        return self.per_user(recommendations).to(recommendations.device)
