"""Novelty, unexpectedness and serendipity of recommendation lists: the two
beyond-accuracy objectives (Kaminskas & Bridge, TiiS 2016) beside diversity and
coverage. Not in the reference.

NoveltyScore: per user the mean over the list of a per-item popularity value,
``-log2(pop_i / n_users)`` (mean self-information) or ``1 - pop_i / max pop``
(expected popularity complement); dr_list_item_mean.
UnexpectednessScore: per user the mean over the list positions of the min (or
mean) cosine distance of the item from the user's history rows;
dr_history_distance. SerendipityScore: the same with each position's distance
multiplied by its relevance flag (the item is in ``interactions`` for that
user). include/divrec_hip.h holds the kernels' contracts. Higher is better.
"""
from __future__ import annotations

from typing import Optional

import torch

from divrec import _backend, ops
from divrec.datasets import UserItemInteractionsDataset
from divrec.losses.base_losses import DatasetAwareLoss, RecommendationsAwareLoss

NOVELTY_KINDS = ("self_information", "popularity_complement")


def novelty_item_values(pop: torch.Tensor, n_users: int, kind: str) -> torch.Tensor:
    """fp32 [n_items] from the items' user counts ``pop``: ``-log2(pop / n_users)``
    with an item nobody has seen counted as ``pop = 1`` ("self_information"), or
    ``1 - pop / max pop`` (all ones when no item was seen;
    "popularity_complement")."""
    if kind not in NOVELTY_KINDS:
        raise ValueError(f"kind must be one of {list(NOVELTY_KINDS)}, got {kind!r}")
    pop = pop.to(torch.float64)
    if kind == "self_information":
        return (-torch.log2(pop.clamp(min=1.0) / float(max(int(n_users), 1)))).to(torch.float32)
    top = float(pop.max()) if pop.numel() else 0.0
    return (1.0 - pop / top if top > 0 else torch.ones_like(pop)).to(torch.float32)


def _lists_on(recommendations: torch.Tensor, n_users: int, dev: torch.device) -> torch.Tensor:
    if recommendations.dim() != 2 or recommendations.size(0) != n_users:
        raise ValueError(f"expected one list per user ([{n_users}, k]), got "
                         f"{tuple(recommendations.shape)}")
    return recommendations.to(dev)


class NoveltyScore(RecommendationsAwareLoss, DatasetAwareLoss):
    """``NoveltyScore(dataset=..., history=None, kind="self_information" |
    "popularity_complement")``: ``pop_i`` is the number of distinct users of
    ``history`` (default: ``dataset``) with item i. For self-information an
    item nobody has seen takes ``pop_i = 1``, the rarest an observed item can
    be. The device values are built on first use (``refresh()`` drops them)."""

    def __init__(self, *args, history: Optional[UserItemInteractionsDataset] = None,
                 kind: str = "self_information", **kwargs):
        DatasetAwareLoss.__init__(self, *args, **kwargs)
        RecommendationsAwareLoss.__init__(self, *args, **kwargs)
        if kind not in NOVELTY_KINDS:
            raise ValueError(f"kind must be one of {list(NOVELTY_KINDS)}, got {kind!r}")
        self.kind = kind
        self.history = history if history is not None else self.dataset
        self._dev_values = None

    def refresh(self) -> None:
        self._dev_values = None

    def item_values(self, device: torch.device) -> torch.Tensor:
        if self._dev_values is None or self._dev_values.device != device:
            n_users = int(self.dataset.number_of_users)
            n_items = int(self.dataset.number_of_items)
            _, items = self.history.user_item_csr(n_users)  # distinct (user, item) pairs
            pop, _ = ops.catalog_histogram(items.to(device).view(-1, 1), n_items)
            self._dev_values = novelty_item_values(pop, n_users, self.kind).to(device)
        return self._dev_values

    def per_user(self, recommendations: torch.Tensor) -> torch.Tensor:
        dev = recommendations.device if recommendations.is_cuda else _backend.default_device()
        recs = _lists_on(recommendations, int(self.dataset.number_of_users), dev)
        return ops.list_item_mean(recs, self.item_values(dev))

    def recommendations_loss(self, interactions, recommendations) -> torch.Tensor:
        return self.per_user(recommendations).to(recommendations.device)


class UnexpectednessScore(RecommendationsAwareLoss, DatasetAwareLoss):
    """``UnexpectednessScore(dataset=..., item_table=... or model=...,
    history=None, reduce="min" | "mean")``: ``item_table`` ([n_items, d], any
    float dtype, d <= 256) or a model with ``item_embeddings`` supplies the
    rows; ``history`` (default ``dataset``) the users' known items. The bf16
    device table and the CSR are built on first use and kept (``refresh()``
    drops them after the table or the history change). Lists of at most 1024
    positions; entries < 0 count as distance 0."""

    def __init__(self, *args, item_table: Optional[torch.Tensor] = None, model=None,
                 history: Optional[UserItemInteractionsDataset] = None, reduce: str = "min",
                 **kwargs):
        # ``reduce`` names the history reduction here; the scores' own reduction
        # over users is chosen with ``reduction`` ("mean", "sum", "none")
        DatasetAwareLoss.__init__(self, *args, **kwargs)
        RecommendationsAwareLoss.__init__(self, *args, **kwargs)
        if (item_table is None) == (model is None):
            raise ValueError("give exactly one of item_table and model")
        if model is not None and not hasattr(model, "item_embeddings"):
            raise ValueError("model must have item_embeddings (a MatrixFactorization)")
        if reduce not in ("min", "mean"):
            raise ValueError(f'reduce must be "min" or "mean", got {reduce!r}')
        self.item_table, self.model, self.hist_reduce = item_table, model, reduce
        self.history = history if history is not None else self.dataset
        self._dev_table = None
        self._dev_csr = None

    def refresh(self) -> None:
        self._dev_table = None
        self._dev_csr = None

    def _rows(self) -> torch.Tensor:
        rows = self.item_table if self.model is None else self.model.item_embeddings.weight
        rows = rows.detach()
        n_items = int(self.dataset.number_of_items)
        if rows.dim() != 2 or rows.size(0) < n_items:
            raise ValueError(f"the item table must be [n_items >= {n_items}, d], got "
                             f"{tuple(rows.shape)}")
        return rows[:n_items]

    def device_table(self, device: torch.device) -> torch.Tensor:
        if self._dev_table is None or self._dev_table.device != device:
            rows = self._rows().to(device=device, dtype=torch.bfloat16).contiguous()
            self._dev_table = ops.pad_columns(
                rows, ops._width_of(ops.HISTORY_WIDTHS, rows.size(1), "history distance"))
        return self._dev_table

    def device_csr(self, device: torch.device):
        if self._dev_csr is None or self._dev_csr[0].device != device:
            rowptr, items = self.history.user_item_csr(int(self.dataset.number_of_users))
            self._dev_csr = (rowptr.to(device), items.to(device))
        return self._dev_csr

    def distances(self, recommendations: torch.Tensor) -> torch.Tensor:
        """fp32 [n_users, k] on the device: each position's history distance."""
        dev = recommendations.device if recommendations.is_cuda else _backend.default_device()
        recs = _lists_on(recommendations, int(self.dataset.number_of_users), dev)
        rowptr, items = self.device_csr(dev)
        # a history item outside the table is skipped (check=False), as the profiles do
        return ops.history_distance(recs.to(torch.int32), self.device_table(dev), rowptr, items,
                                    self.hist_reduce, check=False)

    def per_user(self, recommendations: torch.Tensor) -> torch.Tensor:
        return self.distances(recommendations).mean(dim=1)

    def recommendations_loss(self, interactions, recommendations) -> torch.Tensor:
        return self.per_user(recommendations).to(recommendations.device)


def relevance_flags(interactions: torch.Tensor, recommendations: torch.Tensor,
                    n_items: int) -> torch.Tensor:
    """bool [n_users, k]: is (u, recommendations[u, p]) a row of ``interactions``
    ([N, 2] user, item)? A search over the sorted keys user * n_items + item, on
    the recommendations' device."""
    dev = recommendations.device
    recs = recommendations.to(torch.int64)
    inter = interactions.to(device=dev, dtype=torch.int64)
    keys = torch.unique(inter[:, 0] * n_items + inter[:, 1])
    users = torch.arange(recs.size(0), device=dev).unsqueeze(1)
    valid = (recs >= 0) & (recs < n_items)
    want = users * n_items + recs.clamp(0, max(n_items - 1, 0))
    if keys.numel() == 0:
        return torch.zeros_like(valid)
    at = torch.searchsorted(keys, want.contiguous()).clamp_(max=keys.numel() - 1)
    return valid & (keys[at] == want)


class SerendipityScore(UnexpectednessScore):
    """``UnexpectednessScore`` with each position's distance multiplied by its
    relevance flag: per user the mean over the k positions of dist * hit, hit =
    the item is in the ``interactions`` the score is called with for that user
    (Ge et al., RecSys 2010: unexpected and useful)."""

    def recommendations_loss(self, interactions, recommendations) -> torch.Tensor:
        dist = self.distances(recommendations)
        hit = relevance_flags(interactions, recommendations.to(dist.device),
                              int(self.dataset.number_of_items))
        return (dist * hit.to(dist.dtype)).mean(dim=1).to(recommendations.device)
