"""Row -> feature maps for feature-composed models (host side, not in the
reference): the CSR that ``FeatureMatrixFactorization`` sums feature embeddings
over, built from the reference's ``Features`` container.

The feature space of a map, in this order:
  * ``identity``: one private feature per row, ids [0, n_rows);
  * each categorical column, in the order given: one id per distinct
    non-negative integer value of the column (ascending), weight 1. A value
    that is negative, not an integer, or absent from the column's vocabulary
    gives no entry;
  * each numeric column: one id, the weight is the row's value.
A row's entries keep that order. The returned ``offsets`` record the space
(where each block starts, each categorical column's vocabulary), so a second
call with ``offsets=`` maps NEW rows into the SAME space: they get no identity
entry (their private feature does not exist), known categorical values map to
the known ids, and a value never seen gives no entry.
"""
from __future__ import annotations

from typing import Dict, NamedTuple, Optional, Sequence, Union

import torch

from .storages import Features


class FeatureCSR(NamedTuple):
    """``feature_csr``'s result: the CSR (rowptr int64 [n + 1], cols int32,
    weights fp32) over ``n_features`` feature ids, and the space's layout."""

    rowptr: torch.Tensor
    cols: torch.Tensor
    weights: torch.Tensor
    n_features: int
    offsets: Dict


def feature_csr(features: Union[Features, int, None], categorical: Sequence[str] = (),
                numeric: Sequence[str] = (), identity: bool = True, device=None,
                offsets: Optional[Dict] = None) -> FeatureCSR:
    """The feature map of the rows of ``features`` (a ``Features`` table, or
    the number of rows when there are no columns). ``categorical`` / ``numeric``
    name its columns; ``identity=True`` adds one private feature per row: with
    it and no columns the map is the identity and the model over it IS matrix
    factorization. ``offsets`` (a former result's) maps new rows into that
    result's space; ``categorical``, ``numeric`` and ``identity`` are then
    taken from it. The tensors are built on the host and moved to ``device``."""
    categorical, numeric = list(categorical), list(numeric)
    if offsets is not None:
        categorical, numeric = list(offsets["categorical"]), list(offsets["numeric"])
    if isinstance(features, Features):
        n = len(features)
    else:
        if categorical or numeric:
            raise ValueError("feature columns need a Features table")
        if features is None or int(features) < 0:
            raise ValueError("features must be a Features table or a row count")
        n = int(features)
    for name in categorical + numeric:
        if name not in features:
            raise ValueError(f"no feature column {name!r}")
    if len(set(categorical + numeric)) != len(categorical + numeric):
        raise ValueError("a feature column is named twice")

    cand_cols, cand_w = [], []  # per candidate entry of a row: [n] feature id (-1: none), weight
    new = offsets is None
    space = {"identity": 0, "categorical": {}, "numeric": {}, "n_features": 0}
    next_id = 0
    if new and identity:
        cand_cols.append(torch.arange(n, dtype=torch.int64))
        cand_w.append(torch.ones(n))
        space["identity"] = next_id = n
    for name in categorical:
        raw = features[name].detach().cpu()
        value = raw.to(torch.int64)
        valid = (value >= 0) & (value.to(raw.dtype) == raw)
        if new:
            vocab = torch.unique(value[valid])
            space["categorical"][name] = {"offset": next_id, "values": vocab}
            start, next_id = next_id, next_id + vocab.numel()
        else:
            start, vocab = offsets["categorical"][name]["offset"], offsets["categorical"][name]["values"]
        if vocab.numel():
            at = torch.searchsorted(vocab, value.clamp(min=0)).clamp(max=vocab.numel() - 1)
            found = valid & (vocab[at] == value)
        else:
            at, found = torch.zeros_like(value), torch.zeros_like(valid)
        cand_cols.append(torch.where(found, start + at, torch.full_like(at, -1)))
        cand_w.append(torch.ones(n))
    for name in numeric:
        if new:
            space["numeric"][name] = next_id
            fid, next_id = next_id, next_id + 1
        else:
            fid = offsets["numeric"][name]
        cand_cols.append(torch.full((n,), fid, dtype=torch.int64))
        cand_w.append(features[name].detach().cpu().to(torch.float32))
    if new:
        space["n_features"] = next_id
    else:
        space = offsets

    rowptr = torch.zeros(n + 1, dtype=torch.int64)
    if cand_cols:
        C, W = torch.stack(cand_cols, 1), torch.stack(cand_w, 1)
        keep = C >= 0
        rowptr[1:] = torch.cumsum(keep.sum(1), 0)
        cols, weights = C[keep].to(torch.int32), W[keep].to(torch.float32)  # row-major: a row's order
    else:
        cols, weights = torch.zeros(0, dtype=torch.int32), torch.zeros(0, dtype=torch.float32)
    if device is not None:
        rowptr, cols, weights = rowptr.to(device), cols.to(device), weights.to(device)
    return FeatureCSR(rowptr, cols.contiguous(), weights.contiguous(), int(space["n_features"]), space)
