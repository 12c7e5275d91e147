"""Sample / candidate streams of the reference (host side).

Mirrors reference divrec/datasets/base_datasets.py: PointWiseDataset (:41-56),
PairWiseDataset (:59-110) and RankingDataset (:113-171). They are host-side
index streams; the GPU paths consume them as CSR (``exclusion_csr``).

PairWiseDataset draws its samples with Python ``random.choices`` over the same
populations, in the same order, as the reference, so a seeded ``random``
yields the same (user, positive, negative) triples.

Opt-in device-resident streams, whole batches as device tensors:
DevicePointWiseDataset (PointWiseDataset's rows) and DevicePairWiseDataset
(PairWiseDataset's populations, sampled by dr_sample_pairwise).

Divergences: RankingDataset accepts ``frozen=None`` (every
item is a candidate) where the reference raises TypeError (:151,168).
"""
from __future__ import annotations

import random
from typing import Iterator, Optional, Tuple

import torch
from torch.utils.data import DataLoader, Dataset, IterableDataset

from .storages import UserItemInteractionsDataset, get_item_features, get_user_features

PointWiseRow = Tuple[int, int, Optional[torch.Tensor], Optional[torch.Tensor], float]
PairWiseRow = Tuple[int, int, int, Optional[torch.Tensor], Optional[torch.Tensor],
                    Optional[torch.Tensor]]
RankingRow = Tuple[torch.LongTensor, torch.LongTensor, torch.LongTensor,
                   Optional[torch.Tensor], Optional[torch.Tensor]]


def _user_items(data: UserItemInteractionsDataset, user_id: int) -> torch.Tensor:
    inter = data.interactions
    return inter[inter[:, 0] == user_id, 1]


class PointWiseDataset(Dataset):
    """(user, item, user features, item features, score) per interaction."""

    def __init__(self, data: UserItemInteractionsDataset):
        self.data = data

    def __len__(self) -> int:
        return self.data.number_of_interactions

    def __getitem__(self, index: int) -> PointWiseRow:
        user_id, item_id = self.data.interactions[index]
        # the reference indexes the scores by item id, not by row (:52)
        score = self.data.interaction_scores[item_id]
        return (user_id, item_id, get_user_features(self.data, user_id),
                get_item_features(self.data, item_id), score)

    def loader(self, **loader_params) -> DataLoader:
        return DataLoader(self, **loader_params)


class PairWiseDataset(IterableDataset):
    """Per user: positives x negatives (the Cartesian product of two samples
    with replacement of ``max_sampled`` items each, pos-major)."""

    def __init__(self, data: UserItemInteractionsDataset,
                 frozen: Optional[UserItemInteractionsDataset] = None, max_sampled: int = 100):
        self.data = data
        self.frozen = frozen
        self.max_sampled = max_sampled

    def __iter__(self) -> Iterator[PairWiseRow]:
        catalog = frozenset(range(self.data.number_of_items))
        for user_id in range(self.data.number_of_users):
            ufeat = get_user_features(self.data, user_id)
            pos = frozenset(_user_items(self.data, user_id).tolist())
            neg = catalog - pos
            if self.frozen is not None:
                neg = neg - frozenset(_user_items(self.frozen, user_id).tolist())
            if self.max_sampled > 0:
                pos = random.choices(list(pos), k=self.max_sampled)
                neg = random.choices(list(neg), k=self.max_sampled)
            for p in pos:
                pfeat = get_item_features(self.data, p)
                for n in neg:
                    yield user_id, p, n, ufeat, pfeat, get_item_features(self.data, n)

    def loader(self, **loader_params) -> DataLoader:
        return DataLoader(self, **loader_params)


class RankingDataset(IterableDataset):
    """One row per user: the user id repeated over its candidates, its
    positives, and the candidates = every item except the user's ``frozen``
    interactions, in ascending item id."""

    def __init__(self, data: UserItemInteractionsDataset,
                 frozen: Optional[UserItemInteractionsDataset] = None):
        self.data = data
        self.frozen = frozen

    def candidates(self, user_id: int) -> torch.LongTensor:
        n = self.data.number_of_items
        if self.frozen is None:
            return torch.arange(n, dtype=torch.long)
        keep = torch.ones(n, dtype=torch.bool)
        f = _user_items(self.frozen, user_id)
        keep[f[f < n]] = False
        return torch.nonzero(keep).flatten()

    def __iter__(self) -> Iterator[RankingRow]:
        for user_id in range(self.data.number_of_users):
            positives = _user_items(self.data, user_id)
            cands = self.candidates(user_id)
            ufeat = ifeat = None
            if self.data.has_user_features():
                # as the reference (:153-163): the whole user table per candidate,
                # and item features gated on has_user_features()
                ufeat = torch.concatenate([self.data.user_features.features for _ in cands])
                ifeat = torch.concatenate([get_item_features(self.data, int(i)) for i in cands])
            yield torch.full((len(cands),), user_id), positives, cands, ufeat, ifeat

    def exclusion_csr(self) -> Optional[Tuple[torch.Tensor, torch.Tensor]]:
        """Frozen items per user as CSR (rowptr int64 [U+1], items int32), or
        None without ``frozen`` — what dr_score_topk excludes."""
        if self.frozen is None or not self.frozen.has_interactions():
            return None
        return self.frozen.user_item_csr(self.data.number_of_users)


def _device_csr(data: UserItemInteractionsDataset, n_users: int, n_items: int, device):
    """Unique (user, item) pairs of ``data`` as a CSR on ``device``: rowptr
    int64 [n_users + 1], items int32 sorted per user (frozenset semantics)."""
    inter = data.interactions.to(device=device, dtype=torch.int64)
    key = torch.unique(inter[:, 0] * n_items + inter[:, 1])  # sorted, unique
    users, items = key // n_items, key % n_items
    counts = torch.bincount(users, minlength=n_users)
    rowptr = torch.zeros(n_users + 1, dtype=torch.int64, device=device)
    rowptr[1:] = torch.cumsum(counts, 0)
    return rowptr, items.to(torch.int32).contiguous()


def interaction_csr(data: UserItemInteractionsDataset, n_users: int, n_items: int, device,
                    by: str = "user", use_scores: bool = False):
    """The interactions of ``data`` as the CSR ``ops.als_solve`` takes, on
    ``device`` (torch ops only, so ``"cpu"`` works): (rowptr int64 [rows + 1],
    cols int32, values fp32 or None) over the unique (user, item) pairs, the
    columns sorted per row. ``by="user"``: one row per user over item columns;
    ``by="item"``: the transpose. With ``use_scores`` the values are
    ``interaction_scores[row of the interaction]`` summed over the repeats of a
    pair (float64 sums in interaction order, rounded once); without it None
    (every pair counts 1). ``n_users`` / ``n_items`` may exceed the data's own
    counts (rows without entries); ValueError if they are below them."""
    if by not in ("user", "item"):
        raise ValueError(f'by must be "user" or "item", got {by!r}')
    n_users, n_items = int(n_users), int(n_items)
    if n_users < int(data.number_of_users) or n_items < int(data.number_of_items):
        raise ValueError(f"the data has {int(data.number_of_users)} users and "
                         f"{int(data.number_of_items)} items: more than n_users = {n_users}, "
                         f"n_items = {n_items}")
    n_rows, span = (n_users, n_items) if by == "user" else (n_items, n_users)
    values = None
    if data.interactions is None or data.interactions.numel() == 0:
        key = torch.zeros(0, dtype=torch.int64, device=device)
        if use_scores:
            values = torch.zeros(0, dtype=torch.float32, device=device)
    else:
        inter = data.interactions.to(device=device, dtype=torch.int64)
        r, c = (inter[:, 0], inter[:, 1]) if by == "user" else (inter[:, 1], inter[:, 0])
        key = r * span + c
        if use_scores:
            # stable sort, then each pair's sum as a difference of one running
            # float64 sum: no atomics, the same values on every run
            key, order = torch.sort(key, stable=True)
            run = torch.cumsum(data.interaction_scores.to(device=device, dtype=torch.float64)[order], 0)
            last = torch.ones_like(key, dtype=torch.bool)
            last[:-1] = key[1:] != key[:-1]
            ends = run[last]
            values = ends.clone()
            values[1:] -= ends[:-1]
            values = values.to(torch.float32)
            key = key[last]
        else:
            key = torch.unique(key)  # sorted, unique
    rows, cols = key // span, key % span
    counts = torch.bincount(rows, minlength=n_rows)
    rowptr = torch.zeros(n_rows + 1, dtype=torch.int64, device=device)
    rowptr[1:] = torch.cumsum(counts, 0)
    return rowptr, cols.to(torch.int32).contiguous(), values


class DevicePointWiseDataset:
    """PointWiseDataset resident on ``device``: ``loader`` yields whole batches
    ``(user_id, item_id, None, None, true_relevance)`` as device tensors (int64
    ids, targets in the dtype of ``interaction_scores``) with no per-row Python
    (features are not gathered: the MF fast path ignores them).

    Targets are ``interaction_scores[item_id]``, what PointWiseDataset yields
    (the reference indexes the scores by item id, base_datasets.py:52), so with
    ``shuffle=False`` the batches equal ``PointWiseDataset(data).loader(
    batch_size=B)``'s element for element, the last short batch included.
    ``by_row=True`` opts into ``interaction_scores[row]``, the score of each
    interaction itself (a deliberate divergence).

    ``shuffle=True``: each ``loader()`` call is a new epoch whose order is a
    ``torch.randperm`` on the device seeded from ``(seed, epoch)``. Works with
    ``device="cpu"`` too (only the training loops need the GPU)."""

    def __init__(self, data: UserItemInteractionsDataset, device="cuda", seed: int = 0,
                 by_row: bool = False):
        self.data = data
        self.device = torch.device(device)
        self.seed = int(seed)
        self.epoch = 0
        self.by_row = bool(by_row)
        inter = data.interactions.to(torch.int64)
        scores = data.interaction_scores
        if not by_row and inter.size(0) and int(inter[:, 1].max()) >= scores.size(0):
            # PointWiseDataset fails at that row; checked here on the host so
            # that no device gather ever reads outside the scores
            raise IndexError(f"index {int(inter[:, 1].max())} is out of bounds for dimension 0 "
                             f"with size {scores.size(0)} (interaction_scores[item_id])")
        self.user_id = inter[:, 0].contiguous().to(self.device)
        self.item_id = inter[:, 1].contiguous().to(self.device)
        scores = scores.to(self.device)
        self.true_relevance = scores if by_row else scores[self.item_id]

    def __len__(self) -> int:
        return self.user_id.numel()

    def loader(self, batch_size: int = 1, shuffle: bool = False, drop_last: bool = False,
               **_unused) -> Iterator[PointWiseRow]:
        n, batch_size = len(self), int(batch_size)
        if batch_size < 1:
            raise ValueError("batch_size must be >= 1")
        cols = (self.user_id, self.item_id, self.true_relevance)
        if shuffle:
            g = torch.Generator(device=self.device)
            g.manual_seed((self.seed * 0x9E3779B97F4A7C15 + self.epoch) & ((1 << 63) - 1))
            self.epoch += 1
            order = torch.randperm(n, device=self.device, generator=g)
            cols = tuple(c[order] for c in cols)
        end = n // batch_size * batch_size if drop_last else n

        def batches():
            for b0 in range(0, end, batch_size):
                b1 = min(b0 + batch_size, end)
                yield cols[0][b0:b1], cols[1][b0:b1], None, None, cols[2][b0:b1]

        return batches()


class DevicePairWiseDataset:
    """PairWiseDataset with the sampling on the GPU.

    Same populations, layout and order as the reference's PairWiseDataset
    (base_datasets.py:70-107): users 0..U-1, per user m positives drawn with
    replacement from its unique positives and m negatives from
    items - positives - frozen, yielded as the m x m product (positive-major).
    The draws come from dr_sample_pairwise's counter-based generator instead of
    Python's ``random`` (parity is distributional; each ``loader()`` call is a
    new epoch with fresh draws). ``loader(batch_size=B)`` yields batches of B
    consecutive triples as device tensors ``(user, positive, negative, None,
    None, None)`` (features are not gathered: the MF fast path ignores them).
    Requires ``max_sampled > 0``. A user without positives raises IndexError,
    as the reference does, when its chunk is sampled."""

    def __init__(self, data: UserItemInteractionsDataset,
                 frozen: Optional[UserItemInteractionsDataset] = None, max_sampled: int = 100,
                 device="cuda", seed: int = 0, triples_per_chunk: int = 1 << 22):
        if max_sampled <= 0:
            raise ValueError("DevicePairWiseDataset samples: max_sampled must be > 0")
        self.data = data
        self.frozen = frozen
        self.max_sampled = int(max_sampled)
        self.device = torch.device(device)
        self.seed = int(seed)
        self.epoch = 0
        self.n_users = int(data.number_of_users)
        self.n_items = int(data.number_of_items)
        self.pos_csr = _device_csr(data, self.n_users, self.n_items, self.device)
        self.excl_csr = None
        if frozen is not None:
            self.excl_csr = _device_csr(frozen, self.n_users, self.n_items, self.device)
        self.users_per_chunk = max(1, triples_per_chunk // (self.max_sampled ** 2))

    def __len__(self) -> int:
        return self.n_users * self.max_sampled ** 2

    def loader(self, batch_size: int = 1, **_unused) -> Iterator[PairWiseRow]:
        from .. import ops  # device path only

        seed = (self.seed * 0x9E3779B97F4A7C15 + self.epoch) & ((1 << 64) - 1)
        self.epoch += 1
        carry = None
        for u0 in range(0, self.n_users, self.users_per_chunk):
            users = torch.arange(u0, min(u0 + self.users_per_chunk, self.n_users),
                                 dtype=torch.int64, device=self.device)
            _, _, trip = ops.sample_pairwise(users, *self.pos_csr, self.n_items, self.max_sampled,
                                             seed, exclude=self.excl_csr)
            if carry is not None:
                trip = tuple(torch.cat([c, t]) for c, t in zip(carry, trip))
            n_full = trip[0].numel() // batch_size * batch_size
            for b0 in range(0, n_full, batch_size):
                yield (trip[0][b0:b0 + batch_size], trip[1][b0:b0 + batch_size],
                       trip[2][b0:b0 + batch_size], None, None, None)
            carry = tuple(t[n_full:] for t in trip)
        if carry is not None and carry[0].numel() > 0:
            yield carry[0], carry[1], carry[2], None, None, None
