"""FeatureMatrixFactorization: a LightFM-style hybrid on the HIP path (not in
the reference, whose only trainable model ignores ``user_features`` and
``item_features``, divrec/models/matrix_factorization.py:19-28).

A row's embedding is the weighted sum of the embeddings of its features:
    user table = S_u @ user_feature_embeddings.weight     [no_users, d]
    item table = S_i @ item_feature_embeddings.weight     [no_items, d]
with S the row -> feature maps of ``divrec.datasets.feature_csr`` (CSR). The
sum is dr_csr_row_sum (``ops.feature_sum``), its backward the same kernel over
the transposed map: no atomics, bitwise reproducible. Everything downstream
takes the composed tables as it takes MatrixFactorization's parameters: the
shared scan code of ``_TableModel`` (``score_topk``, ``recommend_diverse``),
``_GatherDot`` for ``forward``, dr_bpr_fwd_bwd for the fused training step.

What the maps buy: an item without interactions is scored through the
features it shares with trained items; items of one genre share statistical
strength; a NEW catalog is ``compose_items(feature_csr(new_features,
offsets=item_map.offsets))`` passed as ``item_vectors=``, without retraining.
With identity maps (``feature_csr(n, identity=True)``) the model IS
MatrixFactorization, table for table.

The parameters must live on a ROCm device; there is no CPU path.
"""
from __future__ import annotations

from typing import Optional

import torch

from divrec import ops

from .matrix_factorization import _GatherDot, _ids_for, _TableModel


def _as_map(csr, n_features: int, what: str) -> ops.CsrMap:
    """``csr`` = an ``ops.CsrMap``, or (rowptr, cols, weights[, n_features,
    ...]) as ``feature_csr`` returns it, over a space of ``n_features``."""
    if isinstance(csr, ops.CsrMap):
        m = csr
    else:
        if not isinstance(csr, (tuple, list)) or len(csr) < 3:
            raise ValueError(f"{what} must be an ops.CsrMap or (rowptr, cols, weights, n_features)")
        if len(csr) > 3 and int(csr[3]) != n_features:
            raise ValueError(f"{what} is over {int(csr[3])} features, the model's space has "
                             f"{n_features}")
        m = ops.CsrMap(csr[0], csr[1], csr[2], n_features)
    if m.n_cols != n_features:
        raise ValueError(f"{what} is over {m.n_cols} features, the model's space has {n_features}")
    return m


class FeatureMatrixFactorization(_TableModel):
    """``user_map`` / ``item_map``: ``feature_csr`` results (or (rowptr, cols,
    weights, n_features) tuples, on any device): one row per user / item. The
    parameters are ``user_feature_embeddings.weight`` [Fu, d] and
    ``item_feature_embeddings.weight`` [Fi, d] (fp32 nn.Embedding, N(0, 1)
    init, dense gradients). The maps are not parameters or buffers: they move
    to the parameters' device on first use and stay there, with their
    ``row_sum_plan`` and their transpose, for the model's lifetime."""

    def __init__(self, user_map, item_map, embedding_dim: int):
        torch.nn.Module.__init__(self)
        if not 1 <= int(embedding_dim) <= ops.ROW_SUM_MAX_D:
            raise ValueError(f"embedding_dim must be in [1, {ops.ROW_SUM_MAX_D}]")
        for what, m in (("user_map", user_map), ("item_map", item_map)):
            if not isinstance(m, ops.CsrMap) and (not isinstance(m, (tuple, list)) or len(m) < 4):
                raise ValueError(f"{what} must be an ops.CsrMap or (rowptr, cols, weights, "
                                 f"n_features), e.g. a feature_csr result")
        fu = user_map.n_cols if isinstance(user_map, ops.CsrMap) else int(user_map[3])
        fi = item_map.n_cols if isinstance(item_map, ops.CsrMap) else int(item_map[3])
        self.user_map = _as_map(user_map, fu, "user_map")
        self.item_map = _as_map(item_map, fi, "item_map")
        _cols_in_space(self.user_map, "user_map")
        _cols_in_space(self.item_map, "item_map")
        self.no_users = self.user_map.n_rows
        self.no_items = self.item_map.n_rows
        self.embedding_dim = int(embedding_dim)
        self.user_feature_embeddings = torch.nn.Embedding(fu, self.embedding_dim)
        self.item_feature_embeddings = torch.nn.Embedding(fi, self.embedding_dim)

    def _device(self) -> torch.device:
        dev = self.user_feature_embeddings.weight.device
        if dev.type != "cuda":
            raise RuntimeError(
                "FeatureMatrixFactorization runs on the divrec HIP backend: move the model to a "
                "ROCm device first (model.to('cuda')); there is no CPU path"
            )
        return dev

    def _maps(self, dev: torch.device):
        """The model's own maps on ``dev`` (moved once, then kept)."""
        if self.user_map.rowptr.device != dev:
            self.user_map = self.user_map.to(dev)
        if self.item_map.rowptr.device != dev:
            self.item_map = self.item_map.to(dev)
        return self.user_map, self.item_map

    def _compose(self, weight: torch.Tensor, own: ops.CsrMap, csr, what: str) -> torch.Tensor:
        if csr is None:
            return ops.feature_sum(weight, own, checked=True)  # checked at construction
        m = _as_map(csr, weight.size(0), what).to(weight.device)
        return ops.feature_sum(weight, m)  # a caller's map: columns range-checked (one read)

    def compose_users(self, csr=None) -> torch.Tensor:
        """The user table, fp32 [rows, d]: the model's own users, or the rows
        of ``csr``, any map over the same user-feature space (users the model
        has never seen, known by attributes only). Differentiable in the
        feature embeddings."""
        dev = self._device()
        return self._compose(self.user_feature_embeddings.weight, self._maps(dev)[0], csr, "csr")

    def compose_items(self, csr=None) -> torch.Tensor:
        """The item table, fp32 [rows, d]: the model's own items, or the rows
        of ``csr`` over the same item-feature space: the cold-start door, e.g.
        ``feature_csr(new_items, offsets=item_map.offsets)``; pass the result
        to ``score_topk`` / ``recommend_diverse`` as ``item_vectors``."""
        dev = self._device()
        return self._compose(self.item_feature_embeddings.weight, self._maps(dev)[1], csr, "csr")

    def _tables(self, users: bool = True, items: bool = True):
        with torch.no_grad():
            return (self.compose_users() if users else None,
                    self.compose_items() if items else None)

    def forward(
        self,
        user_id: torch.LongTensor,
        item_id: torch.LongTensor,
        user_features: Optional[torch.Tensor] = None,
        item_features: Optional[torch.Tensor] = None,
    ) -> torch.Tensor:
        """s[n] = <user table[user_id[n]], item table[item_id[n]]>: both tables
        composed whole (two dr_csr_row_sum), then MatrixFactorization's fused
        gather + dot; differentiable end to end (dr_gather_dot_backward into
        the composed tables' gradients, then the transposed row sums)."""
        dev = self._device()
        uid, hu = _ids_for(dev, user_id, self.no_users, "user_id")
        iid, hi = _ids_for(dev, item_id, self.no_items, "item_id")
        return _GatherDot.apply(self.compose_users(), self.compose_items(), uid, iid, hu and hi)


def _cols_in_space(m: ops.CsrMap, what: str) -> None:
    """A model's own map is checked once, here, so its sums need no read-back."""
    if m.cols.numel() and (int(m.cols.min()) < 0 or int(m.cols.max()) >= m.n_cols):
        raise ValueError(f"{what} names a feature outside [0, {m.n_cols})")
