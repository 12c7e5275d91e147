"""MatrixFactorization on the HIP path (reference divrec/models/matrix_factorization.py:8-28).

Same constructor, attributes and state-dict keys (``user_embeddings.weight``,
``item_embeddings.weight``: fp32 nn.Embedding, N(0,1) init, dense gradients),
so reference checkpoints load unchanged. ``forward`` is the fused embedding
gather + row dot of libdivrec_hip (dr_gather_dot) with its backward
(dr_gather_dot_backward) into dense fp32 gradients; parameters must live on a
ROCm device (``model.to("cuda")``) — there is no CPU path.

New, non-breaking: ``score_topk`` — full-catalog MFMA scoring with a fused
top-k (dr_score_topk), the hot path of get_model_recommendations. Two
precisions:
  * ``"fp32"`` (default): the fp32 parameters themselves, scored on
    v_mfma_f32_32x32x2_f32 — each score an exact fp32 fmaf chain, i.e. the
    reference's fp32 arithmetic (matrix_factorization.py:26-28) up to the
    summation order;
  * ``"bf16"``: bf16 copies of the tables on the bf16 MFMA (16x the rate),
    ranking the tables' bf16 rounding — the explicit fast mode.
Any ``embedding_dim`` works: widths without a scan instance (e.g. the
reference experiments' 100) are zero-padded per call (a copy of O((U + I) d)
bytes, small beside the O(U I d) scan; no cache, so writes through ``.data``
or raw pointers, which bump no autograd version, are always seen).

``recommend_diverse`` composes ``score_topk`` with a diversity re-rank of the
top candidates (greedy DPP, dr_dpp_rerank, or MMR, dr_mmr_rerank) over the
bf16 item table, with the calibrated re-rank over item partition labels
(dr_calibrated_rerank), or with the xQuAD re-rank over a multi-hot item-aspect
matrix (dr_xquad_rerank).
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from divrec import ops

from .base_models import RankingModel

PRECISIONS = {"fp32": torch.float32, "bf16": torch.bfloat16}
RERANKERS = ("dpp", "mmr", "calibrated", "xquad")  # recommend_diverse methods
# C of dr_dpp_rerank / dr_mmr_rerank / dr_calibrated_rerank / dr_xquad_rerank
MAX_RERANK_CANDIDATES = 1024


class _GatherDot(torch.autograd.Function):
    @staticmethod
    def forward(ctx, user_table, item_table, user_id, item_id, checked):
        ctx.save_for_backward(user_table, item_table, user_id, item_id)
        # ids validated on the host need no device read-back of the counter
        return ops.gather_dot(user_table, item_table, user_id, item_id, check=not checked)

    @staticmethod
    def backward(ctx, grad_out):
        user_table, item_table, user_id, item_id = ctx.saved_tensors
        gu = torch.zeros_like(user_table) if ctx.needs_input_grad[0] else None
        gi = torch.zeros_like(item_table) if ctx.needs_input_grad[1] else None
        ops.gather_dot_backward(user_table, item_table, user_id, item_id, grad_out, gu, gi)
        return gu, gi, None, None, None


def _on_device(model_device: torch.device, ids: torch.Tensor) -> torch.Tensor:
    ids = torch.as_tensor(ids)
    if ids.dtype != torch.int64:
        ids = ids.to(torch.int64)
    return ids.to(model_device, non_blocking=True)


def _ids_for(model_device: torch.device, ids, n_rows: int, what: str):
    """(device ids, validated on the host?): host ids are range-checked before
    the upload (IndexError, as nn.Embedding raises), device ids in the kernel."""
    ids = torch.as_tensor(ids)
    host = ids.device.type == "cpu"
    if host:
        from divrec import _backend
        _backend.host_ids_in_range(ids, n_rows, what)
    return _on_device(model_device, ids), host


def _scan_form(table: torch.Tensor, dt: torch.dtype, w: int) -> torch.Tensor:
    """``table`` as a scan operand of dtype ``dt`` and width ``w``: itself when
    it already is one, else a converted / zero-padded copy."""
    if dt == table.dtype and w == table.size(1) and table.is_contiguous():
        return table.detach()
    with torch.no_grad():
        return ops.pad_columns(table.detach().to(dt).contiguous(), w)


class _TableModel(RankingModel):
    """A model whose score is the dot product of a user row and an item row of
    two fp32 tables of width ``embedding_dim``, ``no_users`` and ``no_items``
    rows long. ONE hook says what those tables are, ``_tables``; everything
    that scans them (``scoring_tables``, ``score_topk``, ``recommend_diverse``)
    is written once, here, for every such model."""

    def _device(self) -> torch.device:
        raise NotImplementedError

    def _tables(self, users: bool = True, items: bool = True):
        """The tables of this model: (user table or None, item table or None),
        fp32 [rows, embedding_dim] on the model's device, as the parameters
        stand now. A side not asked for may be None (it may cost a kernel)."""
        raise NotImplementedError

    def scoring_tables(self, precision: str = "fp32") -> Tuple[torch.Tensor, torch.Tensor]:
        """The (user, item) tables score_topk scans at ``precision``: the
        model's tables themselves when their dtype and width already have a
        scan instance, else a converted / zero-padded copy made by this call.
        Never cached, for any model: an update through ``weight.data`` or a
        raw-pointer optimizer bumps no version a cache could key on (ADVICE
        r2), so a kept copy, or a kept composed table of a feature model, could
        not know that it is stale."""
        if precision not in PRECISIONS:
            raise ValueError(f"precision must be one of {sorted(PRECISIONS)}")
        self._device()
        dt = PRECISIONS[precision]
        w = ops.score_width(dt, self.embedding_dim)
        U, I = self._tables()
        return _scan_form(U, dt, w), _scan_form(I, dt, w)

    def bf16_tables(self) -> Tuple[torch.Tensor, torch.Tensor]:
        """bf16 copies of both tables (the fast scoring mode's operands)."""
        return self.scoring_tables("bf16")

    def _side(self, vectors: torch.Tensor, what: str, dev: torch.device, dt: torch.dtype,
              w: int) -> torch.Tensor:
        """``vectors`` (fp32 [n, embedding_dim]) as one side of a scan beside
        the model's own table: on its device, of its dtype and padded width."""
        if (vectors.dim() != 2 or vectors.size(1) != self.embedding_dim
                or vectors.dtype != torch.float32):
            raise ValueError(f"{what} must be fp32 [n, {self.embedding_dim}], got "
                             f"{vectors.dtype} {tuple(vectors.shape)}")
        return ops.pad_columns(vectors.detach().to(dev, dt).contiguous(), w)

    def _scan_sides(self, precision: str, user_vectors, item_vectors, users: bool = True):
        """(user side, item side) of a scan at ``precision``: the caller's
        vectors where given, else the model's table (``users=False``: no user
        side at all)."""
        if precision not in PRECISIONS:
            raise ValueError(f"precision must be one of {sorted(PRECISIONS)}")
        dev = self._device()
        dt = PRECISIONS[precision]
        w = ops.score_width(dt, self.embedding_dim)
        U, I = self._tables(users=users and user_vectors is None, items=item_vectors is None)
        if users:
            U = (_scan_form(U, dt, w) if user_vectors is None
                 else self._side(user_vectors, "user_vectors", dev, dt, w))
        I = (_scan_form(I, dt, w) if item_vectors is None
             else self._side(item_vectors, "item_vectors", dev, dt, w))
        return U, I

    @torch.no_grad()
    def score_topk(
        self,
        k: int,
        user_ids: Optional[torch.Tensor] = None,
        exclude: Optional[Tuple[torch.Tensor, torch.Tensor]] = None,
        precision: str = "fp32",
        n_items: Optional[int] = None,
        *,
        user_vectors: Optional[torch.Tensor] = None,
        item_vectors: Optional[torch.Tensor] = None,
    ) -> Tuple[torch.Tensor, torch.Tensor]:
        """Top-k items of each user (all users, or ``user_ids``) over the
        catalog (the first ``n_items`` item rows; default all): (items int64
        [n, k], scores fp32 [n, k]) on the model's device, ordered by score
        desc then item id asc. ``exclude`` = (rowptr int64 [n+1], items int32)
        CSR of items never to return. ``precision`` "fp32" (default, the
        reference's arithmetic) or "bf16" (fast mode). ``user_vectors`` (fp32
        [n, embedding_dim], e.g. ``fold_in_users``): these rows are the user
        side of the scan instead of the model's user table, converted and
        padded like ``scoring_tables``; ``user_ids`` must then be None.
        ``item_vectors`` (fp32 [n, embedding_dim]): these rows are the CATALOG
        of the call instead of the model's item table, item id = row number
        (e.g. ``FeatureMatrixFactorization.compose_items(new_csr)``: items the
        model has never seen)."""
        if user_vectors is not None and user_ids is not None:
            raise ValueError("user_vectors are the users to score: user_ids must be None")
        dev = self._device()
        U, I = self._scan_sides(precision, user_vectors, item_vectors)
        if n_items is not None:
            I = I[: int(n_items)]
        uids = None if user_ids is None else _on_device(dev, user_ids)
        ex = None
        if exclude is not None:
            ex = (exclude[0].to(dev, torch.int64), exclude[1].to(dev, torch.int32))
        scores, items = ops.score_topk(U, I, int(k), user_ids=uids, exclude=ex)
        return items.to(torch.int64), scores

    @torch.no_grad()
    def recommend_diverse(
        self,
        k: int,
        candidates: int,
        method: str = "dpp",
        lam: float = 0.5,
        user_ids: Optional[torch.Tensor] = None,
        exclude: Optional[Tuple[torch.Tensor, torch.Tensor]] = None,
        precision: str = "fp32",
        n_items: Optional[int] = None,
        *,
        item_labels: Optional[torch.Tensor] = None,
        user_profile: Optional[torch.Tensor] = None,
        n_labels: Optional[int] = None,
        item_aspects: Optional[torch.Tensor] = None,
        aspect_profile: Optional[torch.Tensor] = None,
        user_vectors: Optional[torch.Tensor] = None,
        item_vectors: Optional[torch.Tensor] = None,
    ) -> Tuple[torch.Tensor, torch.Tensor]:
        """Diversity re-ranked lists: the top-``candidates`` items of each user
        (``score_topk`` with the same ``user_ids`` / ``exclude`` / ``precision``
        / ``n_items``) re-ranked to ``k`` picks by ``method`` "dpp"
        (``ops.dpp_rerank``) or "mmr" (``ops.mmr_rerank``) at trade-off ``lam``
        over the bf16 item table, or by "calibrated"
        (``ops.calibrated_rerank``), which needs ``item_labels`` (int [catalog],
        values in [0, G)) and ``user_profile`` (fp32 [n, G], one row per
        listed user, e.g. ``ops.label_profile`` of the users' history;
        ``n_labels``, when given, must equal G <= 64) and uses no item rows,
        or by "xquad" (``ops.xquad_rerank``), which needs ``item_aspects``
        (fp32 [catalog, G], G <= 64: the items' aspect memberships in [0, 1])
        and ``aspect_profile`` (fp32 [n, G], one row per listed user, e.g.
        ``ops.aspect_profile`` of the users' history), with ``candidates * G
        <= ops.XQUAD_MAX_CELLS``; there ``lam`` weights relevance as for every
        method (the xQuAD paper's lambda is ``1 - lam``).
        ``user_vectors`` (fp32 [n, embedding_dim], e.g. ``fold_in_users``)
        replaces the model's users as in ``score_topk``; ``user_ids`` must
        then be None; ``item_vectors`` (fp32 [n, embedding_dim]) replaces the
        model's items as the catalog, for the scan and for the re-rank's rows.
        Returns (items int64 [n, k] in pick order,
        scores fp32 [n, k]: the picks' scan scores). A list that ends early
        (fewer eligible candidates than ``k``) holds item -1 / score -inf.
        ``k <= candidates <= min(1024, catalog)``, else ValueError."""
        k, candidates = int(k), int(candidates)
        if user_vectors is not None and user_ids is not None:
            raise ValueError("user_vectors are the users to score: user_ids must be None")
        if method not in RERANKERS:
            raise ValueError(f"method must be one of {sorted(RERANKERS)}, got {method!r}")
        catalog = self.no_items if item_vectors is None else len(item_vectors)
        if n_items is not None:
            catalog = int(n_items)
        if not 1 <= k <= candidates <= min(MAX_RERANK_CANDIDATES, catalog):
            raise ValueError(f"need 1 <= k <= candidates <= min({MAX_RERANK_CANDIDATES}, catalog "
                             f"= {catalog}), got k = {k}, candidates = {candidates}")
        if method == "calibrated":
            if item_labels is None or user_profile is None:
                raise ValueError('method "calibrated" needs item_labels and user_profile')
            n_lists = self.no_users if user_ids is None else len(user_ids)
            if user_vectors is not None:
                n_lists = len(user_vectors)
            if user_profile.dim() != 2 or user_profile.size(0) != n_lists:
                raise ValueError(f"user_profile must be [{n_lists}, n_labels], one row per user, "
                                 f"got {tuple(user_profile.shape)}")
            G = user_profile.size(1)
            if n_labels is not None and int(n_labels) != G:
                raise ValueError(f"n_labels = {n_labels}, but user_profile has {G} columns")
            if not 1 <= G <= ops.CALIB_MAX_LABELS:
                raise ValueError(f"need 1 <= n_labels <= {ops.CALIB_MAX_LABELS}, got {G}")
            if item_labels.dim() != 1 or item_labels.size(0) < catalog:
                raise ValueError(f"item_labels must hold a label for each of the {catalog} items")
        elif item_labels is not None or user_profile is not None or n_labels is not None:
            raise ValueError(f'item_labels, user_profile and n_labels belong to method '
                             f'"calibrated", not {method!r}')
        if method == "xquad":
            if item_aspects is None or aspect_profile is None:
                raise ValueError('method "xquad" needs item_aspects and aspect_profile')
            n_lists = self.no_users if user_ids is None else len(user_ids)
            if user_vectors is not None:
                n_lists = len(user_vectors)
            if item_aspects.dim() != 2 or item_aspects.size(0) < catalog:
                raise ValueError(f"item_aspects must be [catalog, n_aspects] with a row for each "
                                 f"of the {catalog} items, got {tuple(item_aspects.shape)}")
            G = item_aspects.size(1)
            if not 1 <= G <= ops.XQUAD_MAX_ASPECTS:
                raise ValueError(f"need 1 <= n_aspects <= {ops.XQUAD_MAX_ASPECTS}, got {G}")
            if aspect_profile.dim() != 2 or tuple(aspect_profile.shape) != (n_lists, G):
                raise ValueError(f"aspect_profile must be [{n_lists}, {G}], one row per user, "
                                 f"got {tuple(aspect_profile.shape)}")
            if candidates * G > ops.XQUAD_MAX_CELLS:
                raise ValueError(f"candidates * n_aspects = {candidates} * {G} exceeds "
                                 f"{ops.XQUAD_MAX_CELLS}: at most "
                                 f"{ops.XQUAD_MAX_CELLS // G} candidates fit with {G} aspects")
        elif item_aspects is not None or aspect_profile is not None:
            raise ValueError(f'item_aspects and aspect_profile belong to method "xquad", '
                             f'not {method!r}')
        cand, cand_scores = self.score_topk(candidates, user_ids=user_ids, exclude=exclude,
                                            precision=precision, n_items=n_items,
                                            user_vectors=user_vectors, item_vectors=item_vectors)
        cand32 = cand.to(torch.int32)
        if method == "calibrated":
            dev = cand.device
            picks, _ = ops.calibrated_rerank(
                cand32, cand_scores, item_labels[:catalog].to(dev),
                user_profile.to(dev, torch.float32), k, lam)
        elif method == "xquad":
            dev = cand.device
            picks, _ = ops.xquad_rerank(
                cand32, cand_scores, item_aspects[:catalog].to(dev, torch.float32),
                aspect_profile.to(dev, torch.float32), k, lam)
        else:
            rows = self._scan_sides("bf16", None, item_vectors, users=False)[1][:catalog]
            if method == "dpp":
                picks, _ = ops.dpp_rerank(cand32, cand_scores, rows, k, lam)
            else:
                picks = ops.mmr_rerank(cand32, cand_scores, rows, k, lam)
        picks = picks.to(torch.int64)
        # the picks' scan scores: candidate ids are distinct per user, so a pick
        # is found by a search in the user's sorted ids
        ids_sorted, order = cand.sort(dim=1)
        at = torch.searchsorted(ids_sorted, picks.contiguous()).clamp_(max=candidates - 1)
        scores = cand_scores.gather(1, order.gather(1, at))
        return picks, scores.masked_fill_(picks < 0, float("-inf"))

    @torch.no_grad()
    def recommend_serendipitous(
        self,
        k: int,
        candidates: int,
        history: Tuple[torch.Tensor, torch.Tensor],
        lam: float = 0.5,
        reduce: str = "min",
        user_ids: Optional[torch.Tensor] = None,
        user_vectors: Optional[torch.Tensor] = None,
        item_vectors: Optional[torch.Tensor] = None,
        precision: str = "fp32",
        exclude: Optional[Tuple[torch.Tensor, torch.Tensor]] = None,
        n_items: Optional[int] = None,
    ) -> Tuple[torch.Tensor, torch.Tensor]:
        """Serendipity re-ranked lists: the top-``candidates`` items of each
        user (``score_topk`` with the same ``user_ids`` / ``exclude`` /
        ``precision`` / ``n_items`` / ``user_vectors`` / ``item_vectors``)
        re-ranked to the ``k`` best of lam * score + (1 - lam) * distance,
        distance the ``reduce`` ("min" or "mean") cosine distance of the
        candidate from the rows of the user's ``history``: a CSR (rowptr int64
        [n + 1], items int32) with one row per listed user, e.g.
        ``dataset.exclusion_csr()`` (``ops.serendipity_rerank`` over the bf16
        item table). ``lam`` weights relevance as in ``recommend_diverse``;
        ``lam = 1`` and a user without history give the plain top-k. A door of
        its own: its input is a history, not a ``method``. Returns (items
        int64 [n, k] in pick order, distances fp32 [n, k]). ``k <= candidates
        <= min(1024, catalog)`` and an embedding width <= 256, else
        ValueError."""
        k, candidates = int(k), int(candidates)
        if user_vectors is not None and user_ids is not None:
            raise ValueError("user_vectors are the users to score: user_ids must be None")
        if reduce not in ("min", "mean"):
            raise ValueError(f'reduce must be "min" or "mean", got {reduce!r}')
        if not 0.0 <= float(lam) <= 1.0:
            raise ValueError(f"lam must be in [0, 1], got {lam}")
        catalog = self.no_items if item_vectors is None else len(item_vectors)
        if n_items is not None:
            catalog = int(n_items)
        if not 1 <= k <= candidates <= min(MAX_RERANK_CANDIDATES, catalog):
            raise ValueError(f"need 1 <= k <= candidates <= min({MAX_RERANK_CANDIDATES}, catalog "
                             f"= {catalog}), got k = {k}, candidates = {candidates}")
        n_lists = self.no_users if user_ids is None else len(user_ids)
        if user_vectors is not None:
            n_lists = len(user_vectors)
        if (not isinstance(history, (tuple, list)) or len(history) != 2
                or history[0].dim() != 1 or history[0].numel() != n_lists + 1
                or history[1].dim() != 1):
            raise ValueError(f"history must be a CSR (rowptr [{n_lists + 1}], items), one row per "
                             f"listed user")
        cand, cand_scores = self.score_topk(candidates, user_ids=user_ids, exclude=exclude,
                                            precision=precision, n_items=n_items,
                                            user_vectors=user_vectors, item_vectors=item_vectors)
        dev = cand.device
        rows = self._scan_sides("bf16", None, item_vectors, users=False)[1][:catalog]
        # a history item outside the catalog has no row and is skipped; the
        # candidates come from the scan and are inside it
        picks, dist = ops.serendipity_rerank(
            cand.to(torch.int32), cand_scores, rows, history[0].to(dev, torch.int64),
            history[1].to(dev, torch.int32), k, lam, reduce, check=False)
        return picks.to(torch.int64), dist


class MatrixFactorization(_TableModel):
    def __init__(self, no_users: int, no_items: int, embedding_dim: int):
        torch.nn.Module.__init__(self)
        self.no_users = no_users
        self.no_items = no_items
        self.embedding_dim = embedding_dim
        self.user_embeddings = torch.nn.Embedding(no_users, embedding_dim)
        self.item_embeddings = torch.nn.Embedding(no_items, embedding_dim)

    def _device(self) -> torch.device:
        dev = self.user_embeddings.weight.device
        if dev.type != "cuda":
            raise RuntimeError(
                "MatrixFactorization runs on the divrec HIP backend: move the model to a "
                "ROCm device first (model.to('cuda')); there is no CPU path"
            )
        return dev

    def _tables(self, users: bool = True, items: bool = True):
        return self.user_embeddings.weight, self.item_embeddings.weight

    def forward(
        self,
        user_id: torch.LongTensor,
        item_id: torch.LongTensor,
        user_features: Optional[torch.Tensor] = None,
        item_features: Optional[torch.Tensor] = None,
    ) -> torch.Tensor:
        dev = self._device()
        uid, hu = _ids_for(dev, user_id, self.user_embeddings.num_embeddings, "user_id")
        iid, hi = _ids_for(dev, item_id, self.item_embeddings.num_embeddings, "item_id")
        return _GatherDot.apply(self.user_embeddings.weight, self.item_embeddings.weight, uid, iid,
                                hu and hi)

    @torch.no_grad()
    def fold_in_users(self, rowptr: torch.Tensor, items: torch.Tensor,
                      weights: Optional[torch.Tensor] = None, alpha: float = 40.0,
                      reg: float = 0.1) -> torch.Tensor:
        """Embeddings of users the model has never seen, from their histories
        (CSR: rowptr int64 [n + 1], items int32, ``weights`` fp32 or None):
        fp32 [n, embedding_dim], each row the ALS solve of that history against
        the model's item table (``ops.als_solve``; ``alpha`` and ``reg`` as in
        ``als_train_loop``). The rows go to ``score_topk`` and
        ``recommend_diverse`` as ``user_vectors``. An item id outside the item
        table raises IndexError."""
        dev = self._device()
        if self.embedding_dim > ops.ALS_WIDTHS[-1]:
            raise ValueError(f"fold_in_users supports embedding_dim <= {ops.ALS_WIDTHS[-1]}")
        w = None if weights is None else weights.to(dev, torch.float32)
        return ops.als_solve(self.item_embeddings.weight.detach(), rowptr.to(dev, torch.int64),
                             items.to(dev, torch.int32), w, alpha=alpha, reg=reg)
