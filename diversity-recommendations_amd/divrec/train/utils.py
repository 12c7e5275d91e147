"""Training / scoring loops (reference divrec/train/utils.py:10-216).

Same functions, arguments and return values as the reference. On the hot path:

* ``get_model_recommendations`` with a MatrixFactorization model runs ONE
  dr_score_topk over all users (fp32 MFMA scores by default, fused top-k,
  frozen items excluded through a CSR) instead of the reference's per-user
  loop of set differences, full-catalog forward and full argsort (:58-77).
  Ties are broken by item id ascending (the reference's argsort is unstable
  there, :73).
* ``pair_wise_train_loop`` with MatrixFactorization + LogSigmoidDifferenceLoss
  runs each batch as ONE dr_bpr_fwd_bwd (gather, loss, AUC flags and dense
  embedding gradients fused) followed by dr_adam_dense when the optimizer is a
  plain torch.optim.Adam (its state tensors are used and kept up to date, so
  the optimizer stays usable). Other combinations take the generic path: the
  model's HIP forward/backward under autograd and ``optimizer.step()``.
* ``point_wise_train_loop`` with MatrixFactorization + MSELoss on fp32 targets
  runs each batch as ONE dr_mse_fwd_bwd followed by the same optimizer steps,
  and ``point_wise_score_loop`` with MSELoss losses as its forward-only form.
* ``diversity_pair_wise_train_loop`` (not in the reference) trains the BPR
  objective minus a weighted ILD of the model's own top-k lists: the pairwise
  part as above, the regulariser's gradient by dr_ild_embedding_backward.
* ``als_train_loop`` (not in the reference) trains a MatrixFactorization by
  implicit-feedback alternating least squares: two dr_als_solve per iteration.
* FeatureMatrixFactorization (not in the reference) takes the one-launch
  recommendation paths like MatrixFactorization (its composed tables are
  scanned), and ``pair_wise_train_loop`` runs it with LogSigmoidDifferenceLoss
  as a fused step: two dr_csr_row_sum compose the tables, one dr_bpr_fwd_bwd,
  two transposed dr_csr_row_sum give the feature tables' gradients. The
  point-wise loops run it through its forward and autograd;
  ``diversity_pair_wise_train_loop`` and ``als_train_loop`` refuse it.
* ``warp_train_loop`` (not in the reference) trains either model with the
  WARP ranking loss: per batch of (user, positive) pairs ONE dr_warp_fwd_bwd,
  which draws each pair's negatives until one violates the margin.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import torch

from torch.autograd.graph import increment_version

from divrec import _backend, ops
from divrec.datasets import (
    PairWiseDataset,
    PointWiseDataset,
    RankingDataset,
    UserItemInteractionsDataset,
    interaction_csr,
)
from divrec.datasets.base_datasets import _device_csr
from divrec.losses import (
    EmbeddingDistance,
    IntraListDiversityScore,
    LogSigmoidDifferenceLoss,
    MSELoss,
    PairWiseLoss,
    PointWiseLoss,
    RecommendationsAwareLoss,
    WARPLoss,
)
from divrec.metrics import AUCScore
from divrec.metrics import _rank
from divrec.metrics.aspect_coverage_score import aspect_matrix
from divrec.metrics.calibration_score import partition_labels
from divrec.models import FeatureMatrixFactorization, MatrixFactorization, RankingModel
from divrec.models.matrix_factorization import MAX_RERANK_CANDIDATES, RERANKERS


def _model_device(model: torch.nn.Module) -> Optional[torch.device]:
    for p in model.parameters():
        return p.device
    return None


def _to(t, device):
    return t.to(device, non_blocking=True) if isinstance(t, torch.Tensor) and device else t


# --------------------------------------------------------------------------- shared steps
def _epoch_counter(epoch_err: Optional[torch.Tensor], device) -> torch.Tensor:
    """The epoch's id range counter: made on the first fused batch, read once
    after the epoch (``_backend.raise_if_out_of_range``)."""
    return _backend.error_counter(device) if epoch_err is None else epoch_err


def _device_ids_in_range(uid, n_users: int, item_ids, n_items: int) -> None:
    """Range check of a DEVICE batch (``item_ids``: the batch's item id
    tensors): one min/max reduction read back (one sync) BEFORE the kernel, so
    a bad batch raises IndexError with the weights, the optimizer state and
    the gradient tables as they were (the reference's nn.Embedding fails
    before any backward; the lazy path's all-zero gradient invariant holds)."""
    if not uid.numel():
        return
    lo, hi = item_ids[0].min(), item_ids[0].max()
    for t in item_ids[1:]:
        lo, hi = torch.minimum(lo, t.min()), torch.maximum(hi, t.max())
    mm = torch.stack([uid.min(), uid.max(), lo, hi]).cpu().tolist()
    if mm[0] < 0 or mm[1] >= n_users:
        raise IndexError("index out of range in self (user_id)")
    if mm[2] < 0 or mm[3] >= n_items:
        raise IndexError("index out of range in self (item_id)")


def _dense_grads(*params) -> None:
    """The dense gradient tables the fused kernels add into."""
    for p in params:
        if p.grad is None:
            p.grad = torch.zeros_like(p)


def _optimizer_step(optimizer, adam: bool, lazy: bool, rows) -> None:
    """The step after a fused batch: for a SparseAdam (``lazy``) dr_adam_rows
    over ``rows()``, parameter -> the unique rows the batch touched (computed
    only here; the kernel zeroes those gradient rows); for a plain Adam
    (``adam``) dr_adam_dense; ``optimizer.step()`` otherwise."""
    if lazy:
        lazy_adam_step(optimizer, rows())
        return
    if adam:
        fused_adam_step(optimizer)
    else:
        optimizer.step()
    optimizer.zero_grad()


# --------------------------------------------------------------------------- scoring
def _mse_pairs(model: MatrixFactorization, user_id, item_id, true_rel):
    """The MSE fast paths' batch on the model's device: (uid, iid, target).
    Host ids are range-checked here, before any compute; device ids are left
    to the caller (a min/max read-back, or the kernel's error counter)."""
    dev = model._device()
    U, I = model.user_embeddings.weight, model.item_embeddings.weight
    if user_id.device.type == "cpu":
        _backend.host_ids_in_range(user_id, U.size(0), "user_id")
    if item_id.device.type == "cpu":
        _backend.host_ids_in_range(item_id, I.size(0), "item_id")
    uid, iid = (t.to(dev, torch.int64, non_blocking=True) for t in (user_id, item_id))
    return uid, iid, true_rel.to(dev, non_blocking=True)


def _fp32_targets(true_rel) -> bool:
    return isinstance(true_rel, torch.Tensor) and true_rel.dtype == torch.float32


def point_wise_score_loop(dataset: PointWiseDataset, model: RankingModel,
                          losses: List[PointWiseLoss], **loader_params):
    """With MatrixFactorization, MSELoss-only ``losses`` and fp32 targets each
    batch is ONE forward-only dr_mse_fwd_bwd (no atomics) whose per-pair
    squared errors every loss then reduces as it says; anything else scores
    through the model's forward and ``loss.point_wise``."""
    model.eval()
    dev = _model_device(model)
    values = {loss.__class__.__name__: [] for loss in losses}
    fast = bool(losses) and _mf_scoring(model) and all(type(loss) is MSELoss for loss in losses)
    epoch_err = None  # id range errors of the kernel on device batches
    with torch.no_grad():
        for user_id, item_id, uf, itf, true_rel in dataset.loader(**loader_params):
            if fast and _fp32_targets(true_rel):
                uid, iid, target = _mse_pairs(model, user_id, item_id, true_rel)
                epoch_err = _epoch_counter(epoch_err, uid.device)
                _, sq = ops.mse_fwd_bwd(model.user_embeddings.weight.data,
                                        model.item_embeddings.weight.data, uid, iid, target, 0.0,
                                        None, None, err=epoch_err, check=False)
                for loss in losses:
                    values[loss.__class__.__name__].append(sq)
                continue
            pred = model(user_id, item_id, uf, itf)
            for loss in losses:
                values[loss.__class__.__name__].append(loss.point_wise(_to(true_rel, pred.device), pred))
    _backend.raise_if_out_of_range(epoch_err, "point_wise_score_loop")
    return [loss.reduce_loss_values(torch.concatenate(values[loss.__class__.__name__]))
            for loss in losses]


def pair_wise_score_loop(dataset: PairWiseDataset, model: RankingModel,
                         losses: List[PairWiseLoss], **loader_params):
    model.eval()
    values = {loss.__class__.__name__: [] for loss in losses}
    with torch.no_grad():
        for user_id, pos, neg, uf, pf, nf in dataset.loader(**loader_params):
            positives = model(user_id, pos, uf, pf)
            negatives = model(user_id, neg, uf, nf)
            for loss in losses:
                values[loss.__class__.__name__].append(loss.pair_wise(positives, negatives))
    return [loss.reduce_loss_values(torch.concatenate(values[loss.__class__.__name__]))
            for loss in losses]


def _mf_scoring(model: RankingModel) -> bool:
    """The MF fast path applies only to MatrixFactorization's own forward: a
    subclass that overrides forward is scored through its forward."""
    return (isinstance(model, MatrixFactorization)
            and type(model).forward is MatrixFactorization.forward)


def _feature_scoring(model: RankingModel) -> bool:
    """The same for FeatureMatrixFactorization (a sibling of
    MatrixFactorization, never a subclass: it has no ``user_embeddings``)."""
    return (isinstance(model, FeatureMatrixFactorization)
            and type(model).forward is FeatureMatrixFactorization.forward)


def _table_scoring(model: RankingModel) -> bool:
    """Models whose full-catalog scores are ONE scan of two tables
    (``score_topk`` / ``recommend_diverse`` of the shared ``_TableModel``)."""
    return _mf_scoring(model) or _feature_scoring(model)


def _list_length(dataset: RankingDataset, excl, n_users: int, n_items: int, k: int) -> int:
    """Length of the reference's recommendation lists: min(k, candidates),
    where the candidates of a user are the catalog minus its frozen items.
    Lists of different lengths make the reference's torch.LongTensor(...)
    raise (utils.py:77); so does this."""
    if excl is None:
        return min(k, n_items)
    rowptr, cols = excl
    inside = (cols.to(torch.int64) < n_items).to(torch.int64)
    csum = torch.zeros(cols.numel() + 1, dtype=torch.int64)
    csum[1:] = torch.cumsum(inside, 0)
    n_cands = n_items - (csum[rowptr[1:]] - csum[rowptr[:-1]])
    lengths = torch.clamp(n_cands, max=k)
    lo, hi = int(lengths.min()), int(lengths.max())
    if lo != hi:
        raise ValueError(f"expected sequence of length {hi} at dim 1 (got {lo}): a user has "
                         f"fewer than {k} candidates, so the recommendation lists are ragged")
    return lo


MAX_SCAN_K = 1024  # dr_score_topk's largest k (include/divrec_hip.h)


def get_model_recommendations(dataset: RankingDataset, model: RankingModel,
                              number_of_recommendations: int) -> torch.LongTensor:
    """Top-``number_of_recommendations`` candidates of every user of
    ``dataset`` (LongTensor [U, k] on the CPU, like the reference), scored in
    fp32 (MatrixFactorization.score_topk's faithful mode). A
    FeatureMatrixFactorization takes the same one-launch path over its
    composed tables; any other model the per-user loop."""
    k = int(number_of_recommendations)
    n_users = int(dataset.data.number_of_users)
    n_items = int(dataset.data.number_of_items)
    if _table_scoring(model) and n_users <= model.no_users and n_items <= model.no_items:
        if n_users == 0:
            return torch.LongTensor([])
        excl = dataset.exclusion_csr()
        k_len = _list_length(dataset, excl, n_users, n_items, k)
        if k_len == 0:
            return torch.zeros((n_users, 0), dtype=torch.int64)
        if k_len <= MAX_SCAN_K:
            user_ids = None if n_users == model.no_users else torch.arange(n_users)
            items, _ = model.score_topk(k_len, user_ids=user_ids, exclude=excl, n_items=n_items)
            return items.cpu()
        # lists longer than the scan's top-k bound: the loop below (the model's
        # HIP forward per user, full sort), as the reference returns any length
    # Generic RankingModel: the reference loop (model scores per user), with
    # the deterministic tie-break. Outside the MF hot path.
    recs = []
    with torch.no_grad():
        for rep_user, _, cands, uf, itf in dataset:
            scores = model(rep_user, cands, uf, itf).to("cpu")
            order = torch.sort(scores, descending=True, stable=True).indices
            recs.append(cands[order][:k].tolist())
    return torch.LongTensor(recs)


def get_diverse_recommendations(dataset: RankingDataset, model: RankingModel,
                                number_of_recommendations: int, candidates: int,
                                method: str = "dpp", lam: float = 0.5,
                                items_partition_feature: str = "partition",
                                items_aspect_features: Optional[Sequence[str]] = None,
                                ) -> torch.LongTensor:
    """Diversity re-ranked lists of every user of ``dataset`` (LongTensor
    [U, k] on the CPU, not in the reference): the top-``candidates``
    candidates of ``get_model_recommendations``' scan (fp32 scores, frozen
    items excluded) re-ranked to ``number_of_recommendations`` picks by
    ``MatrixFactorization.recommend_diverse`` (``method`` "dpp" or "mmr",
    trade-off ``lam``). ``method`` "calibrated" re-ranks towards each user's
    own mix of item partitions instead: the labels are
    ``dataset.data.item_features[items_partition_feature]`` (at most 64 of
    them), the user's profile the label histogram of its ``frozen`` items, its
    history (``ops.label_profile`` over ``dataset.exclusion_csr()``).
    ``method`` "xquad" re-ranks for coverage of the aspects a user's history
    weighs: the item-aspect matrix is the ``dataset.data.item_features``
    columns named by ``items_aspect_features`` (at most 64, e.g. the genre
    columns of ML-100K; ``candidates`` times their count at most
    ``ops.XQUAD_MAX_CELLS``), the user's profile the aspect shares of its
    ``frozen`` items (``ops.aspect_profile`` over the same CSR).
    A FeatureMatrixFactorization is served like a MatrixFactorization.
    ValueError for a model outside the MF fast path, for ragged candidate
    lists (as ``get_model_recommendations``), for a list that ends early
    (fewer eligible candidates than picks) and, for "calibrated" and "xquad",
    without ``frozen`` or without the feature(s)."""
    k, cands = int(number_of_recommendations), int(candidates)
    if method not in RERANKERS:
        raise ValueError(f"method must be one of {sorted(RERANKERS)}, got {method!r}")
    if not 1 <= k <= cands <= MAX_RERANK_CANDIDATES:
        raise ValueError(f"need 1 <= number_of_recommendations <= candidates <= "
                         f"{MAX_RERANK_CANDIDATES}, got {k} and {cands}")
    n_users = int(dataset.data.number_of_users)
    n_items = int(dataset.data.number_of_items)
    if not (_table_scoring(model) and n_users <= model.no_users and n_items <= model.no_items):
        raise ValueError("get_diverse_recommendations needs a MatrixFactorization model (its own "
                         "forward) that covers the dataset's users and items")
    if n_users == 0:
        return torch.LongTensor([])
    excl = dataset.exclusion_csr()
    labels = None
    if method == "calibrated":
        labels = partition_labels(dataset.data, items_partition_feature)
        if excl is None:
            raise ValueError('method "calibrated" takes the users\' profiles from the frozen '
                             'interactions: the dataset has none')
    aspects = None
    if method == "xquad":
        if items_aspect_features is None:
            raise ValueError('method "xquad" needs items_aspect_features: the item feature '
                             'columns that form the aspect matrix')
        aspects = aspect_matrix(dataset.data, items_aspect_features)
        if excl is None:
            raise ValueError('method "xquad" takes the users\' profiles from the frozen '
                             'interactions: the dataset has none')
    elif items_aspect_features is not None:
        raise ValueError(f'items_aspect_features belongs to method "xquad", not {method!r}')
    c_len = _list_length(dataset, excl, n_users, n_items, cands)
    if c_len < k:
        raise ValueError(f"a user has {c_len} candidates, fewer than the {k} recommendations asked for")
    user_ids = None if n_users == model.no_users else torch.arange(n_users)
    extra = {}  # the keyword arguments of the label- and aspect-aware methods
    if labels is not None:
        dev, n_labels = model._device(), int(labels.max()) + 1
        labels = labels.to(dev)
        # the labels are validated above; a frozen item outside the catalog has none and is skipped
        profile = ops.label_profile(excl[0].to(dev), excl[1].to(dev), labels, n_labels,
                                    check=False)
        extra = dict(item_labels=labels, user_profile=profile)
    if aspects is not None:
        dev = model._device()
        aspects = aspects.to(dev)
        # a frozen item outside the catalog has no aspects and is skipped
        profile = ops.aspect_profile(excl[0].to(dev), excl[1].to(dev), aspects, check=False)
        extra = dict(item_aspects=aspects, aspect_profile=profile)
    items, _ = model.recommend_diverse(k, c_len, method=method, lam=lam, user_ids=user_ids,
                                       exclude=excl, n_items=n_items, **extra)
    items = items.cpu()
    if bool((items < 0).any()):
        short = int((items < 0).any(dim=1).sum())
        raise ValueError(f"{short} lists end before {k} picks (fewer eligible candidates: "
                         f"duplicate or linearly dependent rows), so the lists are ragged")
    return items


def get_serendipitous_recommendations(dataset: RankingDataset, model: RankingModel,
                                      number_of_recommendations: int, candidates: int,
                                      lam: float = 0.5, reduce: str = "min") -> torch.LongTensor:
    """Serendipity re-ranked lists of every user of ``dataset`` (LongTensor
    [U, k] on the CPU, not in the reference): the top-``candidates`` candidates
    of ``get_model_recommendations``' scan (fp32 scores, frozen items excluded)
    re-ranked by ``MatrixFactorization.recommend_serendipitous`` to the
    ``number_of_recommendations`` best of lam * score + (1 - lam) * distance
    from the user's history, which is its ``frozen`` items
    (``dataset.exclusion_csr()``). ValueError without ``frozen``, for a model
    outside the MF fast path, for ragged candidate lists and for a list that
    ends early, as ``get_diverse_recommendations``."""
    k, cands = int(number_of_recommendations), int(candidates)
    if not 1 <= k <= cands <= MAX_RERANK_CANDIDATES:
        raise ValueError(f"need 1 <= number_of_recommendations <= candidates <= "
                         f"{MAX_RERANK_CANDIDATES}, got {k} and {cands}")
    n_users = int(dataset.data.number_of_users)
    n_items = int(dataset.data.number_of_items)
    if not (_table_scoring(model) and n_users <= model.no_users and n_items <= model.no_items):
        raise ValueError("get_serendipitous_recommendations needs a MatrixFactorization model "
                         "(its own forward) that covers the dataset's users and items")
    excl = dataset.exclusion_csr()
    if excl is None:
        raise ValueError("the users' histories are the frozen interactions: the dataset has none")
    if n_users == 0:
        return torch.LongTensor([])
    c_len = _list_length(dataset, excl, n_users, n_items, cands)
    if c_len < k:
        raise ValueError(f"a user has {c_len} candidates, fewer than the {k} recommendations asked for")
    user_ids = None if n_users == model.no_users else torch.arange(n_users)
    items, _ = model.recommend_serendipitous(k, c_len, excl, lam=lam, reduce=reduce,
                                             user_ids=user_ids, exclude=excl, n_items=n_items)
    items = items.cpu()
    if bool((items < 0).any()):
        short = int((items < 0).any(dim=1).sum())
        raise ValueError(f"{short} lists end before {k} picks, so the lists are ragged")
    return items


def recommendations_score_loop(dataset: RankingDataset, model: RankingModel,
                               losses: List[RecommendationsAwareLoss],
                               number_of_recommendations: int):
    model.eval()
    interactions = dataset.data.interactions
    recommendations = get_model_recommendations(dataset, model, number_of_recommendations)
    # P@k / R@k / MAP@k / NDCG@k of one (interactions, recommendations) pair
    # come from one dr_rank_metrics launch
    with _rank.shared_rank_metrics():
        return [loss(interactions, recommendations) for loss in losses]


# --------------------------------------------------------------------------- training
def point_wise_train_loop(dataset: PointWiseDataset, model: RankingModel, loss: PointWiseLoss,
                          optimizer: torch.optim.Optimizer,
                          scores: Optional[List[PointWiseLoss]] = None,
                          **loader_params) -> Tuple[float, List[float]]:
    """One epoch of point-wise training; returns (mean batch loss, [mean score]).

    MatrixFactorization + a reducing MSELoss (+ MSELoss scores) on fp32 targets
    runs each batch as ONE dr_mse_fwd_bwd (gather, squared error and dense
    embedding gradients fused) followed by dr_adam_dense (plain Adam),
    dr_adam_rows (SparseAdam) or ``optimizer.step()``, like the BPR path of
    pair_wise_train_loop. Anything else is the reference's loop."""
    assert scores is None or all(score.reduce for score in scores)
    model.train()
    n_scores = len(scores) if scores is not None else 0
    # per batch: the loss and the scores, as Python floats (generic path) or
    # as device tensors read back once after the epoch (fused path)
    batch_losses, batch_scores = [], []
    fused = _mse_fast_path(model, loss, scores)
    adam = _plain_adam(optimizer)
    lazy = fused and _plain_sparse_adam(optimizer)
    epoch_err = None  # id range errors of the fused kernel
    for user_id, item_id, uf, itf, true_rel in dataset.loader(**loader_params):
        if fused and _fp32_targets(true_rel):
            U, I = model.user_embeddings.weight, model.item_embeddings.weight
            host = user_id.device.type == "cpu" and item_id.device.type == "cpu"
            uid, iid, target = _mse_pairs(model, user_id, item_id, true_rel)
            if not host:
                _device_ids_in_range(uid, U.size(0), (iid,), I.size(0))
            _dense_grads(U, I)
            epoch_err = _epoch_counter(epoch_err, uid.device)
            B = uid.numel()
            grad_scale = 1.0 / B if loss.reduction == "mean" else 1.0
            _, sq = ops.mse_fwd_bwd(U.data, I.data, uid, iid, target, grad_scale, U.grad, I.grad,
                                    err=epoch_err, check=False)
            _optimizer_step(optimizer, adam, lazy,
                            lambda: {U: torch.unique(uid), I: torch.unique(iid)})
            batch_losses.append(loss.reduce_loss_values(sq))
            if n_scores:  # MSELoss.point_wise = the squared errors, reduced as each score says
                batch_scores.append(torch.stack([s.reduce_loss_values(sq) for s in scores]))
        else:
            pred = model(user_id, item_id, uf, itf)
            true_rel = _to(true_rel, pred.device)
            loss_value = loss(true_rel, pred)
            loss_value.backward()
            optimizer.step()
            optimizer.zero_grad()
            batch_losses.append(loss_value.item())
            if n_scores:
                batch_scores.append([score(true_rel, pred).item() for score in scores])
    _backend.raise_if_out_of_range(epoch_err, "point_wise_train_loop")
    # per-batch values added as Python floats in batch order, like the reference
    batch_count, mean_loss = len(batch_losses), 0.0
    mean_scores = [0.0] * n_scores
    for value in _host_floats(batch_losses):
        mean_loss += value
    for row in _host_floats(batch_scores):
        for i in range(n_scores):
            mean_scores[i] += row[i]
    return mean_loss / batch_count, [s / batch_count for s in mean_scores]


def _mse_fast_path(model, loss, scores) -> bool:
    return (_mf_scoring(model) and type(loss) is MSELoss and loss.reduce
            and (scores is None or all(type(s) is MSELoss for s in scores)))


def _host_floats(values: list) -> list:
    """``values`` with its device tensors (0-d or 1-D fp32) replaced by their
    Python float (or list of floats), read back in one transfer."""
    at = [k for k, v in enumerate(values) if isinstance(v, torch.Tensor)]
    if not at:
        return values
    got = torch.stack([values[k] for k in at]).cpu().tolist()
    out = list(values)
    for k, v in zip(at, got):
        out[k] = v
    return out


def _plain_adam(optimizer: torch.optim.Optimizer) -> bool:
    if type(optimizer) is not torch.optim.Adam:
        return False
    for g in optimizer.param_groups:
        if g.get("amsgrad") or g.get("maximize") or g.get("capturable") or g.get("differentiable"):
            return False
        if g.get("decoupled_weight_decay", False):
            return False
    return True


def fused_adam_step(optimizer: torch.optim.Adam) -> None:
    """optimizer.step() of a plain torch.optim.Adam done by dr_adam_dense, on
    the optimizer's own state (step / exp_avg / exp_avg_sq), so torch's
    optimizer remains consistent and resumable."""
    for group in optimizer.param_groups:
        beta1, beta2 = group["betas"]
        for p in group["params"]:
            if p.grad is None:
                continue
            st = optimizer.state[p]
            if len(st) == 0:
                st["step"] = torch.tensor(0.0, dtype=torch.float32)
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            st["step"] += 1
            ops.adam_dense(p.data, p.grad, st["exp_avg"], st["exp_avg_sq"], group["lr"], beta1,
                           beta2, group["eps"], group["weight_decay"], int(st["step"].item()))
            # the kernel wrote p through a raw pointer: bump its autograd
            # version, as a torch in-place update would
            increment_version(p)


def _plain_sparse_adam(optimizer: torch.optim.Optimizer) -> bool:
    return type(optimizer) is torch.optim.SparseAdam and not any(
        g.get("maximize") for g in optimizer.param_groups)


def lazy_adam_step(optimizer: torch.optim.SparseAdam, rows: dict) -> None:
    """optimizer.step() of torch.optim.SparseAdam done by dr_adam_rows on the
    optimizer's own state: for each parameter p, ``rows[p]`` holds the unique
    rows the batch touched (the indices a sparse embedding gradient would
    carry). The reference's embeddings are dense (sparse=False), so plain
    torch cannot run SparseAdam on them; this is the opt-in row-sparse
    ("lazy") alternative to dense Adam. The touched
    gradient rows are zeroed, so the dense gradient tables stay allocated and
    all-zero between batches (no full memset, no re-allocation)."""
    for group in optimizer.param_groups:
        beta1, beta2 = group["betas"]
        for p in group["params"]:
            if p.grad is None or p not in rows:
                continue
            st = optimizer.state[p]
            if len(st) == 0:
                st["step"] = 0
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            st["step"] += 1
            ops.adam_rows(p.data, p.grad, st["exp_avg"], st["exp_avg_sq"], rows[p],
                          group["lr"], beta1, beta2, group["eps"], st["step"])
            increment_version(p)  # raw-pointer update, as in fused_adam_step


def _bpr_fast_path(model, loss, scores) -> bool:
    return (isinstance(model, MatrixFactorization) and type(loss) is LogSigmoidDifferenceLoss
            and (scores is None or all(type(s) is AUCScore for s in scores)))


def _feature_bpr_fast_path(model, loss, scores) -> bool:
    return (_feature_scoring(model) and type(loss) is LogSigmoidDifferenceLoss
            and (scores is None or all(type(s) is AUCScore for s in scores)))


def _composed_grads(model: FeatureMatrixFactorization, U: torch.Tensor, I: torch.Tensor):
    """The two dense composed-gradient buffers of the fused feature step
    ([no_users, d] and [no_items, d] fp32): kept on the model, zeroed per batch."""
    bufs = getattr(model, "_composed_grad_buffers", None)
    if (bufs is None or bufs[0].shape != U.shape or bufs[1].shape != I.shape
            or bufs[0].device != U.device):
        bufs = (torch.empty_like(U), torch.empty_like(I))
        model._composed_grad_buffers = bufs
    bufs[0].zero_(), bufs[1].zero_()
    return bufs


def _feature_fused_step(model: FeatureMatrixFactorization, kernel):
    """The fused FeatureMatrixFactorization step around a step kernel, up to
    the optimizer step: (1) compose both tables WHOLE (two dr_csr_row_sum),
    like the reference's dense Adam over whole tables; (2)
    ``kernel(U, I, gU, gI)``: ONE step kernel (dr_bpr_fwd_bwd,
    dr_warp_fwd_bwd) over the composed tables into the two composed-gradient
    buffers; (3) two dr_csr_row_sum over the transposed maps into the feature
    tables' ``.grad`` (no atomics: given the composed gradients, bitwise
    reproducible). Returns what ``kernel`` returns.
    Bytes per step beyond the kernel's own, with nnz the maps' entries, R
    = no_users + no_items rows and F = Fu + Fi features, all times 4 d:
    compose reads nnz and writes R; the buffers' zeroing writes R; the
    transposed sums read nnz and write F; so 2 nnz + 2 R + F rows of d floats,
    whatever the batch touches (a row-subset compose is out of scope)."""
    dev = model._device()
    Wu, Wi = model.user_feature_embeddings.weight, model.item_feature_embeddings.weight
    with torch.no_grad():
        U, I = model._tables()
        gU, gI = _composed_grads(model, U, I)
        out = kernel(U, I, gU, gI)
        user_map, item_map = model._maps(dev)
        for W, g, m in ((Wu, gU, user_map), (Wi, gI, item_map)):
            grad = m.T.sum(g, check=False)  # columns of a transpose: row numbers, valid
            W.grad = grad if W.grad is None else W.grad.add_(grad)
    return out


def _feature_pair_wise_batch(model: FeatureMatrixFactorization, scores, batch, epoch_err):
    """One batch of the fused FeatureMatrixFactorization + BPR step, up to the
    optimizer step: ``_feature_fused_step`` (its docstring prices it) around
    ONE dr_bpr_fwd_bwd. Returns what ``_pair_wise_batch`` returns."""
    user_id, pos, neg, _, _, _ = batch
    dev = model._device()
    host = user_id.device.type == "cpu"
    if host:  # host batches: raise before any compute
        _backend.host_ids_in_range(user_id, model.no_users, "user_id")
        _backend.host_ids_in_range(pos, model.no_items, "positive item_id")
        _backend.host_ids_in_range(neg, model.no_items, "negative item_id")
    ids = tuple(t.to(dev, torch.int64, non_blocking=True) for t in (user_id, pos, neg))
    if not host:
        _device_ids_in_range(ids[0], model.no_users, ids[1:], model.no_items)
    epoch_err = _epoch_counter(epoch_err, dev)
    B = ids[0].numel()
    losses_b, hits = _feature_fused_step(model, lambda U, I, gU, gI: ops.bpr_fwd_bwd(
        U, I, *ids, 1.0 / B, gU, gI, err=epoch_err, check=False))
    loss_value = torch.sum(losses_b, dim=0) / B
    row = [s.reduce_loss_values(hits).double() for s in scores or ()]
    return ids, loss_value.detach(), torch.stack(row) if row else None, epoch_err


def _pair_wise_batch(model: RankingModel, loss: PairWiseLoss, scores, fused: bool, batch,
                     epoch_err):
    """One batch's pairwise part, up to the optimizer step (not taken here):
    the batch's gradients end up in ``.grad``. ``fused``: range checks, then
    ONE dr_bpr_fwd_bwd that adds the dense gradients of the 'mean' reduction
    into the embeddings' ``.grad``; otherwise the model's forward and autograd.
    Returns (ids, loss value, score row, epoch_err): ids = (uid, pid, nid) on
    the model's device (None on the generic path), the score row a tensor of
    the reduced ``scores`` (None without scores), epoch_err the epoch's id
    range counter (made here on the first fused batch)."""
    user_id, pos, neg, uf, pf, nf = batch
    if fused:
        dev = model._device()
        U, I = model.user_embeddings.weight, model.item_embeddings.weight
        host = user_id.device.type == "cpu"
        if host:  # host batches: raise before any compute
            _backend.host_ids_in_range(user_id, U.size(0), "user_id")
            _backend.host_ids_in_range(pos, I.size(0), "positive item_id")
            _backend.host_ids_in_range(neg, I.size(0), "negative item_id")
        ids = tuple(t.to(dev, torch.int64, non_blocking=True) for t in (user_id, pos, neg))
        if not host:
            _device_ids_in_range(ids[0], U.size(0), ids[1:], I.size(0))
        _dense_grads(U, I)
        epoch_err = _epoch_counter(epoch_err, dev)
        B = ids[0].numel()
        losses_b, hits = ops.bpr_fwd_bwd(U.data, I.data, *ids, 1.0 / B, U.grad, I.grad,
                                         err=epoch_err, check=False)
        loss_value = torch.sum(losses_b, dim=0) / B
        # AUCScore.pair_wise = the hit flags, reduced as each score says
        row = [s.reduce_loss_values(hits).double() for s in scores or ()]
    else:
        ids = None
        positives = model(user_id, pos, uf, pf)
        negatives = model(user_id, neg, uf, nf)
        loss_value = loss(positives, negatives)
        loss_value.backward()
        row = [s(positives.detach(), negatives.detach()).double() for s in scores or ()]
    return ids, loss_value.detach(), torch.stack(row) if row else None, epoch_err


def pair_wise_train_loop(dataset: PairWiseDataset, model: RankingModel, loss: PairWiseLoss,
                         optimizer: torch.optim.Optimizer,
                         scores: Optional[List[PairWiseLoss]] = None,
                         **loader_params) -> Tuple[float, List[float]]:
    """One epoch of pairwise training; returns (mean batch loss, [mean score]).

    A FeatureMatrixFactorization with LogSigmoidDifferenceLoss (+ AUCScore
    scores) runs the fused step of ``_feature_pair_wise_batch`` (its docstring
    prices it), then dr_adam_dense for a plain Adam or the optimizer's own
    step; with other losses it trains through its forward and autograd. The
    lazy SparseAdam path is not offered for it (ValueError): a feature row's
    gradient gathers every row that holds the feature, so no small set of
    touched rows exists."""
    assert scores is None or all(score.reduce for score in scores)
    if isinstance(model, FeatureMatrixFactorization) and isinstance(optimizer,
                                                                    torch.optim.SparseAdam):
        raise ValueError("pair_wise_train_loop: FeatureMatrixFactorization has dense gradients "
                         "(a feature gathers every row that holds it); the lazy SparseAdam path "
                         "is not offered for it, use torch.optim.Adam")
    model.train()
    n_scores = len(scores) if scores is not None else 0
    batch_losses, batch_scores = [], []
    featured = _feature_bpr_fast_path(model, loss, scores)
    fused = _bpr_fast_path(model, loss, scores)
    adam = (fused or featured) and _plain_adam(optimizer)  # the generic path steps the optimizer itself
    lazy = fused and _plain_sparse_adam(optimizer)
    epoch_err = None  # id range errors of the fused kernel on device batches
    for batch in dataset.loader(**loader_params):
        if featured:
            ids, loss_value, row, epoch_err = _feature_pair_wise_batch(model, scores, batch,
                                                                       epoch_err)
        else:
            ids, loss_value, row, epoch_err = _pair_wise_batch(model, loss, scores, fused, batch,
                                                               epoch_err)
        _optimizer_step(optimizer, adam, lazy, lambda: {
            model.user_embeddings.weight: torch.unique(ids[0]),
            model.item_embeddings.weight: torch.unique(torch.cat(ids[1:]))})
        batch_losses.append(loss_value)
        if n_scores:
            batch_scores.append(row)
    _backend.raise_if_out_of_range(epoch_err, "pair_wise_train_loop")
    return _pair_wise_epoch_means(batch_losses, batch_scores, n_scores)


def _pair_wise_epoch_means(batch_losses, batch_scores, n_scores) -> Tuple[float, List[float]]:
    count = len(batch_losses)
    # per-batch values summed as Python floats in batch order, like the reference
    mean_loss = sum(float(v) for v in torch.stack(batch_losses).double().cpu().tolist()) / count
    means = [0.0] * n_scores
    if n_scores:
        rows = torch.stack(batch_scores).double().cpu().tolist()
        means = [sum(r[i] for r in rows) / count for i in range(n_scores)]
    return mean_loss, means


_M64 = (1 << 64) - 1


def _mix64(z: int) -> int:
    """splitmix64 finaliser on a Python int (csrc/common.h mix64)."""
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def warp_batch_seed(seed: int, epoch: int, batch: int) -> int:
    """The uint64 seed warp_train_loop gives batch ``batch`` of epoch ``epoch``."""
    z = _mix64((int(seed) + 0x9E3779B97F4A7C15 * (int(epoch) + 1)) & _M64)
    return _mix64(z ^ ((0xD1B54A32D192ED03 * (int(batch) + 1)) & _M64))


def warp_train_loop(dataset: PointWiseDataset, model: RankingModel, loss: WARPLoss,
                    optimizer: torch.optim.Optimizer,
                    frozen: Optional[UserItemInteractionsDataset] = None, seed: int = 0,
                    **loader_params) -> Tuple[float, dict]:
    """One epoch of WARP training (not in the reference); returns (mean batch
    loss, {"mean_trials": draws per pair, "no_violator": share of the pairs
    that found no violator within ``loss.max_trials`` draws}).

    ``dataset`` is a DevicePointWiseDataset or a PointWiseDataset: each batch's
    first two columns are its (user, positive) pairs. Each batch is ONE
    dr_warp_fwd_bwd: per pair, negatives are drawn on the device until one
    scores above ``positive - loss.margin``; draws of the user's own items
    (``dataset.data``, as a CSR built once per call) and of its ``frozen``
    items are skipped but counted; the update is weighted by
    log((n_items - 1) // draws), 'mean' reduction (grad_scale 1/B). The draws
    of a batch depend on (``seed``, the dataset's ``epoch`` counter or 0, the
    batch number) only. Then the optimizer steps as in pair_wise_train_loop:
    dr_adam_dense for a plain Adam, dr_adam_rows for a plain SparseAdam over
    the batch's users and its positives and violators, ``optimizer.step()``
    otherwise. A FeatureMatrixFactorization runs the kernel inside
    ``_feature_fused_step`` (SparseAdam is refused for it, as in
    pair_wise_train_loop). Ids outside the tables raise IndexError after the
    epoch. TypeError for any other model and for a loss that is not a
    WARPLoss; ValueError when the tables do not cover the interactions."""
    featured = _feature_scoring(model)
    if not (featured or isinstance(model, MatrixFactorization)):
        raise TypeError("warp_train_loop needs a MatrixFactorization or a "
                        f"FeatureMatrixFactorization model, got {type(model).__name__}")
    if not isinstance(loss, WARPLoss):
        raise TypeError(f"warp_train_loop needs a WARPLoss, got {type(loss).__name__}")
    if featured and isinstance(optimizer, torch.optim.SparseAdam):
        raise ValueError("warp_train_loop: FeatureMatrixFactorization has dense gradients (a "
                         "feature gathers every row that holds it); the lazy SparseAdam path is "
                         "not offered for it, use torch.optim.Adam")
    n_users, n_items = int(model.no_users), int(model.no_items)
    for what, data in (("dataset.data", dataset.data), ("frozen", frozen)):
        if data is not None and (int(data.number_of_users) > n_users
                                 or int(data.number_of_items) > n_items):
            raise ValueError(f"the model's tables ({n_users} users, {n_items} items) do not cover "
                             f"{what} ({int(data.number_of_users)} users, "
                             f"{int(data.number_of_items)} items)")
    dev = model._device()
    positives = _device_csr(dataset.data, n_users, n_items, dev)
    exclude = None
    if frozen is not None and frozen.has_interactions() and frozen.interactions.numel():
        exclude = _device_csr(frozen, n_users, n_items, dev)
    model.train()
    adam = _plain_adam(optimizer)
    lazy = not featured and _plain_sparse_adam(optimizer)
    epoch = int(getattr(dataset, "epoch", 0))
    batch_losses, counts = [], []
    epoch_err = None  # id range errors of the kernel
    for k, batch in enumerate(dataset.loader(**loader_params)):
        uid, pid = (torch.as_tensor(t).to(dev, torch.int64, non_blocking=True) for t in batch[:2])
        B = uid.numel()
        epoch_err = _epoch_counter(epoch_err, dev)

        def step(U, I, gU, gI, err=epoch_err, batch_seed=warp_batch_seed(seed, epoch, k)):
            return ops.warp_fwd_bwd(U, I, uid, pid, positives, exclude, loss.max_trials,
                                    loss.margin, batch_seed, 0, 1.0 / B, gU, gI, err=err,
                                    check=False)

        if featured:
            losses_b, neg, trials = _feature_fused_step(model, step)
        else:
            U, I = model.user_embeddings.weight, model.item_embeddings.weight
            _dense_grads(U, I)
            losses_b, neg, trials = step(U.data, I.data, U.grad, I.grad)
        valid = trials > 0  # an out-of-range pair made no draw; its rows are not touched
        _optimizer_step(optimizer, adam, lazy, lambda: {
            model.user_embeddings.weight: torch.unique(uid[valid]),
            model.item_embeddings.weight: torch.unique(torch.cat([pid[valid], neg[neg >= 0]]))})
        batch_losses.append(torch.sum(losses_b, dim=0) / B)
        counts.append(torch.stack([trials.sum(), (valid & (neg < 0)).sum(), valid.sum()]))
    _backend.raise_if_out_of_range(epoch_err, "warp_train_loop")
    mean_loss, _ = _pair_wise_epoch_means(batch_losses, [], 0)
    n_trials, n_none, n_pairs = torch.stack(counts).sum(dim=0).cpu().tolist()
    return mean_loss, {"mean_trials": n_trials / max(n_pairs, 1),
                       "no_violator": n_none / max(n_pairs, 1)}


def diversity_pair_wise_train_loop(dataset: PairWiseDataset, model: MatrixFactorization,
                                   loss: PairWiseLoss, optimizer: torch.optim.Optimizer,
                                   diversity: IntraListDiversityScore, diversity_weight: float,
                                   number_of_recommendations: int,
                                   scores: Optional[List[PairWiseLoss]] = None,
                                   **loader_params) -> Tuple[float, List[float], float]:
    """One epoch of pairwise training with a diversity regulariser; returns
    (mean batch loss, [mean score], mean ILD of the batches' lists).

    Per batch the objective is
        loss(pos, neg) - diversity_weight * mean_{u in unique(batch users)} ILD_u(L_u)
    where L_u = model.score_topk(number_of_recommendations, user_ids=those
    users) under the current parameters. The lists are CONSTANTS of the step:
    no gradient flows through the selection, only through the embeddings of
    the items a list holds (dr_ild_embedding_backward on the fp32 item table).

    The pairwise part runs exactly as in pair_wise_train_loop (the fused
    dr_bpr_fwd_bwd for MatrixFactorization + LogSigmoidDifferenceLoss,
    autograd otherwise) and leaves its gradients in ``.grad``; the regulariser
    adds into ``item_embeddings.weight.grad``; then the optimizer steps as
    there (dr_adam_dense for a plain Adam, dr_adam_rows for SparseAdam over
    the batch's rows and the lists' items, ``optimizer.step()`` otherwise).
    ``model`` must be a MatrixFactorization and ``diversity`` an
    IntraListDiversityScore over EmbeddingDistance(model.item_embeddings.weight,
    kind, differentiable=True); anything else raises ValueError before any
    compute. The returned loss and scores are those of pair_wise_train_loop
    (the regulariser is not part of them)."""
    assert scores is None or all(score.reduce for score in scores)
    D = getattr(diversity, "distance_matrix", None)
    if not isinstance(model, MatrixFactorization):
        raise ValueError("diversity_pair_wise_train_loop needs a MatrixFactorization model")
    if not (isinstance(diversity, IntraListDiversityScore) and isinstance(D, EmbeddingDistance)
            and D.differentiable):
        raise ValueError("diversity must be an IntraListDiversityScore over "
                         "EmbeddingDistance(..., differentiable=True)")
    if D.item_table is not model.item_embeddings.weight:
        raise ValueError("diversity's EmbeddingDistance must be over model.item_embeddings.weight")
    k = int(number_of_recommendations)
    if not 2 <= k <= min(ops.ILD_GRAD_MAX_K, model.no_items):
        raise ValueError(f"number_of_recommendations must be in [2, "
                         f"{min(ops.ILD_GRAD_MAX_K, model.no_items)}], got {k}")
    model.train()
    n_scores = len(scores) if scores is not None else 0
    batch_losses, batch_scores, batch_ilds = [], [], []
    fused = _bpr_fast_path(model, loss, scores)
    adam = fused and _plain_adam(optimizer)  # the generic path steps the optimizer itself
    lazy = fused and _plain_sparse_adam(optimizer)
    dev = model._device()
    epoch_err = None  # id range errors of the kernels on device batches
    for batch in dataset.loader(**loader_params):
        U, I = model.user_embeddings.weight, model.item_embeddings.weight
        ids, loss_value, row, epoch_err = _pair_wise_batch(model, loss, scores, fused, batch,
                                                           epoch_err)
        uid = ids[0] if fused else batch[0].to(dev, torch.int64)
        batch_losses.append(loss_value)
        if n_scores:
            batch_scores.append(row)
        # the regulariser: the lists of the batch's users under the current
        # parameters, their ILD, and its gradient added to the item table's
        users = torch.unique(uid)
        with torch.no_grad():
            items, _ = model.score_topk(k, user_ids=users)
            batch_ilds.append(diversity.per_user(items).mean())
        _dense_grads(I)
        epoch_err = _epoch_counter(epoch_err, dev)
        ops.ild_embedding_backward(items, I.data, D.kind, I.grad,
                                   scale=-float(diversity_weight) / users.numel(),
                                   err=epoch_err, check=False)
        # the lists' items are touched rows too: their gradient rows are zeroed
        _optimizer_step(optimizer, adam, lazy, lambda: {
            U: users, I: torch.unique(torch.cat([*ids[1:], items.reshape(-1)]))})
    _backend.raise_if_out_of_range(epoch_err, "diversity_pair_wise_train_loop")
    mean_loss, means = _pair_wise_epoch_means(batch_losses, batch_scores, n_scores)
    ilds = torch.stack(batch_ilds).double().cpu().tolist()
    return mean_loss, means, sum(ilds) / len(ilds)


def als_train_loop(data: UserItemInteractionsDataset, model: MatrixFactorization,
                   iterations: int, alpha: float = 40.0, reg: float = 0.1,
                   use_scores: bool = False, compute_loss: bool = True) -> List[float]:
    """Implicit-feedback ALS (Hu, Koren, Volinsky 2008; not in the reference):
    ``iterations`` times, solve every user row against the item table, then
    every item row against the user table (``ops.als_solve``: a closed-form
    solve per row, no sampler, no learning rate, no atomics), writing
    ``weight.data`` of both embeddings in place. The confidence of a pair is
    1 + alpha (or 1 + alpha * its summed ``interaction_scores`` with
    ``use_scores``); users and items of the model beyond the data's get zero
    rows. Returns the objective ``ops.als_objective`` before the first
    half-step and after every half-step (1 + 2 * iterations floats, each a
    host sync), or [] without ``compute_loss``. ValueError for a model that is
    not a plain MatrixFactorization, for tables that do not cover ``data`` and
    for ``embedding_dim`` > 128; RuntimeError for a model on the CPU."""
    if not _mf_scoring(model):
        raise ValueError("als_train_loop needs a MatrixFactorization model (its own forward)")
    if model.embedding_dim > ops.ALS_WIDTHS[-1]:
        raise ValueError(f"als_train_loop supports embedding_dim <= {ops.ALS_WIDTHS[-1]}, "
                         f"got {model.embedding_dim}")
    if int(data.number_of_users) > model.no_users or int(data.number_of_items) > model.no_items:
        raise ValueError(f"the model's tables ({model.no_users} users, {model.no_items} items) do "
                         f"not cover the data ({int(data.number_of_users)} users, "
                         f"{int(data.number_of_items)} items)")
    if int(iterations) < 0:
        raise ValueError("iterations must be >= 0")
    dev = model._device()
    by_user = interaction_csr(data, model.no_users, model.no_items, dev, "user", use_scores)
    by_item = interaction_csr(data, model.no_users, model.no_items, dev, "item", use_scores)
    U, I = model.user_embeddings.weight, model.item_embeddings.weight
    history: List[float] = []

    def objective() -> None:
        if compute_loss:
            history.append(ops.als_objective(U.data, I.data, *by_user, alpha, reg))

    with torch.no_grad():
        objective()
        for _ in range(int(iterations)):
            for table, fixed, csr in ((U, I, by_user), (I, U, by_item)):
                # the ids come from the data, checked against the tables above
                ops.als_solve(fixed.data, *csr, alpha=alpha, reg=reg, out=table.data, check=False)
                increment_version(table)  # raw-pointer update, as in fused_adam_step
                objective()
    return history


def recommendations_train_loop(dataset: RankingDataset, model: RankingModel,
                               loss: RecommendationsAwareLoss, number_of_recommendations: int,
                               optimizer: torch.optim.Optimizer,
                               scores: Optional[List[RecommendationsAwareLoss]] = None
                               ) -> Tuple[float, List[float]]:
    """The reference's listwise loop (:167-216), kept for API completeness: it
    ranks ASCENDING and back-propagates through integer recommendations, so
    with the shipped losses it fails at backward() exactly as the reference."""
    assert scores is None or all(score.reduce for score in scores)
    model.train()
    batch_count, mean_loss = 0, 0.0
    mean_scores = [0.0] * (len(scores) if scores is not None else 0)
    for rep_user, _, cands, uf, itf in dataset:
        model_scores = model(rep_user, cands, uf, itf)
        inter = dataset.data.interactions
        interactions = inter[inter[:, 0] == rep_user[0]]
        recommendations = cands[torch.argsort(model_scores.cpu())][:number_of_recommendations]
        loss_value = loss(interactions, recommendations)
        loss_value.backward()
        optimizer.step()
        optimizer.zero_grad()
        batch_count += 1
        mean_loss += loss_value.item()
        if scores is not None:
            for i, score in enumerate(scores):
                mean_scores[i] += score(interactions, recommendations).item()
    return mean_loss / batch_count, [s / batch_count for s in mean_scores]
