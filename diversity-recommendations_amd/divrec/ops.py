"""Tensor-level entry points of the HIP hot path (one function per C-ABI call).

Every function takes device tensors, validates dtype / shape / contiguity on
the host, and enqueues the HIP kernel on the current stream of the tensors'
device. Outputs are freshly allocated by the PyTorch caching allocator; the
native library never allocates. There is no CPU implementation here.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from divrec import _backend as B


def _contig(t: torch.Tensor, name: str) -> torch.Tensor:
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    return t


def _need(cond: bool, msg: str) -> None:
    if not cond:
        raise ValueError(msg)


def _counter(dev: torch.device, err: Optional[torch.Tensor] = None, check: bool = True):
    """(the id-range counter a call counts in, the one ``_done`` reads after
    it): the caller's ``err`` and None when it gave one (it reads it when it
    chooses), else with ``check`` twice a fresh counter, else None twice."""
    own = B.error_counter(dev) if err is None and check else None
    return (err if own is None else own), own


def _done(rc: int, name: str, own: Optional[torch.Tensor] = None) -> None:
    """A C call's return code, then its own id-range counter (one host sync), if any."""
    B.check(rc, name)
    B.raise_if_out_of_range(own, name)


def _grad_like(grad: Optional[torch.Tensor], table: torch.Tensor, name: str) -> None:
    if grad is not None:
        _need(grad.shape == table.shape and grad.dtype == torch.float32 and grad.is_contiguous(),
              f"{name} must be a contiguous fp32 tensor shaped like its table")


def _table_pair(user_table: torch.Tensor, item_table: torch.Tensor, dtypes, dtype_msg: str) -> None:
    """Two contiguous 2-D tables of one width, each of a dtype in ``dtypes``."""
    _need(user_table.dim() == 2 and item_table.dim() == 2, "tables must be 2-D")
    _need(user_table.size(1) == item_table.size(1), "tables must share embedding_dim")
    _need(user_table.dtype in dtypes and item_table.dtype in dtypes, dtype_msg)
    _contig(user_table, "user_table"), _contig(item_table, "item_table")


_IDS_MSG = "ids must be 1-D int64 of equal length"


def _id_columns(ids, dtype_msg: str = _IDS_MSG, shape_msg: str = _IDS_MSG):
    """1-D int64 id tensors of equal length, made contiguous."""
    _need(all(t.dtype == torch.int64 for t in ids), dtype_msg)
    _need(all(t.dim() == 1 and t.shape == ids[0].shape for t in ids), shape_msg)
    return tuple(t.contiguous() for t in ids)


def _user_ids(user_ids: torch.Tensor) -> torch.Tensor:
    _need(user_ids.dtype == torch.int64 and user_ids.dim() == 1, "user_ids must be 1-D int64")
    return user_ids.contiguous()


# --------------------------------------------------------------------------- MF forward
def gather_dot(
    user_table: torch.Tensor,
    item_table: torch.Tensor,
    user_id: torch.Tensor,
    item_id: torch.Tensor,
    err: Optional[torch.Tensor] = None,
    check: bool = True,
) -> torch.Tensor:
    """s[n] = <U[user_id[n]], I[item_id[n]]> (MatrixFactorization.forward,
    reference divrec/models/matrix_factorization.py:26-28). fp32 or bf16 tables,
    int64 ids, fp32 output. Ids are range-checked on the device (an invalid
    pair reads nothing and gives NaN): with ``check`` and no ``err`` this call
    reads the count (one sync) and raises IndexError like nn.Embedding;
    otherwise the count goes to the caller's ``err`` (may be None), which the
    caller reads when it chooses (divrec._backend.raise_if_out_of_range)."""
    dev = B.require_device(user_table, item_table, user_id, item_id)
    _need(user_table.dtype == item_table.dtype, "tables must share dtype")
    _table_pair(user_table, item_table, (torch.float32, torch.bfloat16),
                "tables must be fp32 or bf16")
    user_id, item_id = _id_columns((user_id, item_id), "ids must be int64",
                                   "ids must be 1-D, same length")
    out = torch.empty(user_id.numel(), dtype=torch.float32, device=dev)
    err, own = _counter(dev, err, check)
    rc = B.lib().dr_gather_dot(
        user_table.data_ptr(), user_table.size(0), item_table.data_ptr(), item_table.size(0),
        B.dtype_code(user_table.dtype), user_table.size(1), user_id.data_ptr(), item_id.data_ptr(),
        user_id.numel(), out.data_ptr(), B.ptr(err), B.stream(dev),
    )
    _done(rc, "dr_gather_dot", own)
    return out


def gather_dot_backward(
    user_table: torch.Tensor,
    item_table: torch.Tensor,
    user_id: torch.Tensor,
    item_id: torch.Tensor,
    grad_out: torch.Tensor,
    grad_user: Optional[torch.Tensor],
    grad_item: Optional[torch.Tensor],
    err: Optional[torch.Tensor] = None,
) -> None:
    """Accumulate dense fp32 embedding gradients of gather_dot in place.
    Out-of-range pairs add nothing and count in ``err`` (if given)."""
    dev = B.require_device(user_table, item_table, user_id, item_id, grad_out, grad_user, grad_item)
    _need(user_table.dtype == torch.float32 and item_table.dtype == torch.float32,
          "backward needs fp32 tables")
    _grad_like(grad_user, user_table, "grad_user"), _grad_like(grad_item, item_table, "grad_item")
    grad_out = grad_out.to(torch.float32).contiguous()
    rc = B.lib().dr_gather_dot_backward(
        user_table.data_ptr(), user_table.size(0), item_table.data_ptr(), item_table.size(0),
        user_table.size(1), user_id.contiguous().data_ptr(), item_id.contiguous().data_ptr(),
        user_id.numel(), grad_out.data_ptr(), B.ptr(grad_user), B.ptr(grad_item), B.ptr(err),
        B.stream(dev),
    )
    B.check(rc, "dr_gather_dot_backward")


# --------------------------------------------------------------------------- top-K
# Widths with a scan instantiation per table dtype (include/divrec_hip.h); any
# other width is served by zero-padding both tables (zero columns add exact
# zeros to every dot product).
SCORE_WIDTHS = {torch.bfloat16: (32, 64, 128, 256, 512), torch.float32: (32, 64, 128, 256)}


def score_width(dtype: torch.dtype, d: int) -> int:
    """The scan width an embedding of width ``d`` runs at (d itself or the
    next supported width, reached by zero-padding)."""
    _need(dtype in SCORE_WIDTHS, "score_topk tables must be bf16 or fp32")
    for w in SCORE_WIDTHS[dtype]:
        if d <= w:
            return w
    raise ValueError(f"embedding_dim {d} is wider than the widest {dtype} scan "
                     f"({SCORE_WIDTHS[dtype][-1]})")


def pad_columns(table: torch.Tensor, width: int) -> torch.Tensor:
    """``table`` [rows, d] widened to ``width`` columns with zeros (a copy);
    the table itself when it already has that width."""
    if table.size(1) == width:
        return table
    out = torch.zeros((table.size(0), width), dtype=table.dtype, device=table.device)
    out[:, :table.size(1)] = table
    return out


def score_topk(
    user_table: torch.Tensor,
    item_table: torch.Tensor,
    k: int,
    user_ids: Optional[torch.Tensor] = None,
    n_users: Optional[int] = None,
    item_base: int = 0,
    exclude: Optional[Tuple[torch.Tensor, torch.Tensor]] = None,
    init_thr: Optional[torch.Tensor] = None,
    stats: Optional[dict] = None,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """Top-k items per user over the catalog slice ``item_table`` (global ids
    ``item_base + row``); order = score desc, item id asc.

    ``init_thr`` (fp32 [n], optional): only items scoring strictly above the
    user's threshold are ranked (dr_score_topk_seeded); slots past the last
    such item hold item -1 / score -inf. Used by the item-sharded multi-GPU
    top-k with thresholds from a sample of the whole catalog.

    The tables' dtype picks the arithmetic: bf16 tables run the bf16 MFMA scan
    (exact products, fp32 sums: the fast mode), fp32 tables the fp32 MFMA scan
    (an exact fp32 fmaf chain per score: the reference's arithmetic up to the
    summation order). Widths without a scan instance are zero-padded here: a
    copy of both tables on every call (O((U + I) d) bytes; pad once and pass
    the padded tables when calling repeatedly on a large catalog).

    ``user_ids`` (int64) selects user rows; if None the first ``n_users`` rows
    (default: all) are scored. ``exclude = (rowptr int64 [n+1], items int32)``
    is a CSR of GLOBAL item ids (sorted per row) never to recommend.
    Returns (scores fp32 [n, k], items int32 [n, k]).

    ``stats`` (a dict, optional): filled with ``guess_failures`` = [users the
    first-tier guessed threshold failed, users every guess failed] of this
    call (dr_score_topk_fail_counts; one synchronising read).
    """
    dev = B.require_device(user_table, item_table, user_ids)
    _need(user_table.dtype == item_table.dtype and user_table.dtype in SCORE_WIDTHS,
          "score_topk tables must both be bf16 or both fp32")
    _need(user_table.dim() == 2 and item_table.dim() == 2, "tables must be 2-D")
    d = user_table.size(1)
    _need(item_table.size(1) == d, "tables must share embedding_dim")
    _contig(user_table, "user_table"), _contig(item_table, "item_table")
    w = score_width(user_table.dtype, d)
    user_table, item_table = pad_columns(user_table, w), pad_columns(item_table, w)
    _need(1 <= k <= 1024, "k must be in [1, 1024]")
    if user_ids is not None:
        user_ids = _user_ids(user_ids)
        n = user_ids.numel()
        if n:
            lo, hi = int(user_ids.min()), int(user_ids.max())
            _need(0 <= lo and hi < user_table.size(0), "user_ids out of range")
    else:
        n = user_table.size(0) if n_users is None else int(n_users)
        _need(0 <= n <= user_table.size(0), "n_users out of range")
    n_items = item_table.size(0)
    _need(k <= n_items or exclude is not None or init_thr is not None or n_items == 0,
          "k must be <= number of items")
    rowptr = cols = None
    if exclude is not None:
        rowptr, cols = exclude
        B.require_device(rowptr, cols)
        _need(rowptr.dtype == torch.int64 and rowptr.numel() == n + 1, "rowptr must be int64 [n+1]")
        _need(cols.dtype == torch.int32, "excluded items must be int32")
        rowptr, cols = rowptr.contiguous(), cols.contiguous()
        if cols.numel() == 0:
            cols = torch.zeros(1, dtype=torch.int32, device=dev)
    scores = torch.empty((n, k), dtype=torch.float32, device=dev)
    items = torch.empty((n, k), dtype=torch.int32, device=dev)
    if n == 0:
        return scores, items
    L = B.lib()
    dt = B.dtype_code(user_table.dtype)
    if init_thr is not None:
        B.require_device(init_thr)
        _need(init_thr.dtype == torch.float32 and init_thr.numel() == n,
              "init_thr must be fp32 [n_users]")
        init_thr = init_thr.contiguous()
        ws_bytes = L.dr_score_topk_seeded_workspace(n, n_items, dt, w, k)
        ws = torch.empty(max(int(ws_bytes), 1), dtype=torch.uint8, device=dev)
        rc = L.dr_score_topk_seeded(
            user_table.data_ptr(), B.ptr(user_ids), n, item_table.data_ptr(), n_items,
            int(item_base), dt, w, int(k), init_thr.data_ptr(), B.ptr(rowptr), B.ptr(cols),
            scores.data_ptr(), items.data_ptr(), ws.data_ptr(), ws.numel(), B.stream(dev),
        )
        B.check(rc, "dr_score_topk_seeded")
        return scores, items
    ws_bytes = L.dr_score_topk_workspace(n, n_items, dt, w, k)
    ws = torch.empty(max(int(ws_bytes), 1), dtype=torch.uint8, device=dev)
    rc = L.dr_score_topk(
        user_table.data_ptr(), B.ptr(user_ids), n, item_table.data_ptr(), n_items, int(item_base),
        dt, w, int(k), B.ptr(rowptr), B.ptr(cols), scores.data_ptr(), items.data_ptr(),
        ws.data_ptr(), ws.numel(), B.stream(dev),
    )
    B.check(rc, "dr_score_topk")
    if stats is not None:
        import ctypes

        torch.cuda.synchronize(dev)
        fc = (ctypes.c_int32 * 2)()
        B.check(L.dr_score_topk_fail_counts(ws.data_ptr(), n, n_items, dt, w, int(k),
                                            ctypes.addressof(fc)), "dr_score_topk_fail_counts")
        stats["guess_failures"] = [int(fc[0]), int(fc[1])]
    return scores, items


PLAN_FIELDS = ("users_per_wg", "user_blocks", "head_blocks", "tail_chunks", "chunk_items", "grid",
               "cap", "sample_stride", "sample_rows", "sample_rank", "head_keys", "tail_keys",
               "first_tier_rank")


def score_topk_plan(n_users: int, n_items: int, dtype: torch.dtype, d: int, k: int) -> dict:
    """The launch plan dr_score_topk uses for this call shape on the current
    device (no device work): user blocks, head/tail split, guess stride, ...
    (PLAN_FIELDS). Tests use it to prove which plan they exercised.
    ``sample_rank`` is the guess's safe (second-tier) rank ks in the sample,
    ``first_tier_rank`` the rank ks1 <= ks the main scan starts from."""
    import ctypes

    w = score_width(dtype, d)
    n_f = len(PLAN_FIELDS)
    out = (ctypes.c_int64 * n_f)()
    rc = B.lib().dr_score_topk_plan(int(n_users), int(n_items), B.dtype_code(dtype), w, int(k),
                                    ctypes.addressof(out), n_f)
    B.check(rc, "dr_score_topk_plan")
    return dict(zip(PLAN_FIELDS, (int(x) for x in out)))


def sample_thresholds(user_table: torch.Tensor, sample_rows: torch.Tensor, ks1: int, ks: int,
                      user_ids: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The guessed thresholds of the item-sharded top-k (dr_sample_thresholds):
    ``sample_rows`` are the whole catalog's rows at the guess stride; returns
    fp32 [2, n]: strictly below each user's ks1-th (row 0, first tier) and
    ks-th (row 1, safe tier) best tile-max score of the sample (the
    dr_score_topk guess's tile-max sample scan; -inf when there are fewer)."""
    dev = B.require_device(user_table, sample_rows, user_ids)
    _need(user_table.dtype == sample_rows.dtype and user_table.dtype in SCORE_WIDTHS,
          "user table and sample rows must both be bf16 or both fp32")
    _need(user_table.dim() == 2 and sample_rows.dim() == 2 and
          sample_rows.size(1) == user_table.size(1), "2-D tables of one width")
    _need(1 <= ks1 <= ks <= 256, "need 1 <= ks1 <= ks <= 256")
    _contig(user_table, "user_table")
    w = score_width(user_table.dtype, user_table.size(1))
    user_table = pad_columns(user_table, w)
    sample_rows = pad_columns(sample_rows.contiguous(), w)
    if user_ids is not None:
        user_ids = _user_ids(user_ids)
        n = user_ids.numel()
    else:
        n = user_table.size(0)
    out = torch.empty((2, n), dtype=torch.float32, device=dev)
    if n == 0:
        return out
    L = B.lib()
    dt = B.dtype_code(user_table.dtype)
    ws_bytes = L.dr_sample_thresholds_workspace(n, sample_rows.size(0), dt, w, int(ks))
    ws = torch.empty(max(int(ws_bytes), 1), dtype=torch.uint8, device=dev)
    rc = L.dr_sample_thresholds(user_table.data_ptr(), B.ptr(user_ids), n,
                                sample_rows.data_ptr(), sample_rows.size(0), dt, w, int(ks1),
                                int(ks), out[0].data_ptr(), out[1].data_ptr(), ws.data_ptr(),
                                ws.numel(), B.stream(dev))
    B.check(rc, "dr_sample_thresholds")
    return out


def topk_merge(
    scores: torch.Tensor, items: torch.Tensor, k_out: Optional[int] = None
) -> Tuple[torch.Tensor, torch.Tensor]:
    """Merge per-part sorted top-k lists [parts, n, k_in] -> [n, k_out]."""
    dev = B.require_device(scores, items)
    _need(scores.dim() == 3 and scores.shape == items.shape, "expected [parts, n, k] inputs")
    _need(scores.dtype == torch.float32 and items.dtype == torch.int32, "fp32 scores, int32 items")
    parts, n, k_in = scores.shape
    k_out = k_in if k_out is None else int(k_out)
    _need(1 <= k_out <= parts * k_in, "k_out must be in [1, parts * k_in]")
    _need(parts * k_in <= 2048 or k_out <= 1024, "k_out must be <= 1024 when parts * k_in > 2048")
    out_s = torch.empty((n, k_out), dtype=torch.float32, device=dev)
    out_i = torch.empty((n, k_out), dtype=torch.int32, device=dev)
    if n == 0:
        return out_s, out_i
    rc = B.lib().dr_topk_merge(
        scores.contiguous().data_ptr(), items.contiguous().data_ptr(), parts, n, k_in, k_out,
        out_s.data_ptr(), out_i.data_ptr(), B.stream(dev),
    )
    B.check(rc, "dr_topk_merge")
    return out_s, out_i


# --------------------------------------------------------------------------- ILD
def _recs(recs: torch.Tensor) -> Tuple[torch.Tensor, int]:
    _need(recs.dim() == 2, "recommendations must be [n_users, k]")
    _need(recs.dtype in (torch.int32, torch.int64), "recommendations must be int32 or int64")
    return recs.contiguous(), B.dtype_code(recs.dtype)


def _dist_matrix(dist: torch.Tensor) -> torch.Tensor:
    _need(dist.dim() == 2 and dist.size(0) == dist.size(1), "distance matrix must be [I, I]")
    _need(dist.dtype in (torch.float32, torch.float64, torch.int32, torch.int64),
          "distance matrix dtype must be float32/float64/int32/int64")
    return dist.contiguous()


def _ild_dense(recs: torch.Tensor, dist: torch.Tensor, symbol: str,
               out_dtype: torch.dtype) -> torch.Tensor:
    """The two dense-matrix ILD calls: one C signature, two symbols and output types."""
    dev = B.require_device(recs, dist)
    recs, rc_dt = _recs(recs)
    dist = _dist_matrix(dist)
    n, k = recs.shape
    out = torch.empty(n, dtype=out_dtype, device=dev)
    if n == 0:
        return out
    err, own = _counter(dev)
    rc = getattr(B.lib(), symbol)(
        recs.data_ptr(), rc_dt, n, k, dist.data_ptr(), B.dtype_code(dist.dtype), dist.size(0),
        out.data_ptr(), err.data_ptr(), B.stream(dev),
    )
    _done(rc, symbol, own)
    return out


def ild_dense(recs: torch.Tensor, dist: torch.Tensor) -> torch.Tensor:
    """Per-user ILD against a dense [I, I] distance matrix (fp32/fp64/int32/int64)."""
    return _ild_dense(recs, dist, "dr_ild_dense", torch.float32)


def ild_dense_pair_sum(recs: torch.Tensor, dist: torch.Tensor) -> torch.Tensor:
    """Per-user UN-normalised pair sum sum_{p<q} D[r_p, r_q] (the reference's
    user_ild), accumulated in D's precision; float64 [n] (exact for fp32 and
    integer D)."""
    return _ild_dense(recs, dist, "dr_ild_dense_pair_sum", torch.float64)


def ild_labels(recs: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
    """Per-user ILD with D[i,j] = (labels[i] == labels[j]) computed on the fly."""
    dev = B.require_device(recs, labels)
    recs, rc_dt = _recs(recs)
    labels = labels.to(torch.int64).contiguous()
    n, k = recs.shape
    out = torch.empty(n, dtype=torch.float32, device=dev)
    if n == 0:
        return out
    err, own = _counter(dev)
    rc = B.lib().dr_ild_labels(
        recs.data_ptr(), rc_dt, n, k, labels.data_ptr(), labels.numel(), out.data_ptr(),
        err.data_ptr(), B.stream(dev),
    )
    _done(rc, "dr_ild_labels", own)
    return out


_KINDS = {"cosine": B.DR_ILD_COSINE, "dot": B.DR_ILD_DOT, "euclidean": B.DR_ILD_EUCLIDEAN}
ILD_WIDTHS = (32, 64, 128, 256)  # dr_ild_embedding instances; others are zero-padded
MMR_WIDTHS = (64, 128)           # dr_mmr_rerank instances; others are zero-padded
DPP_WIDTHS = (64, 128)           # dr_dpp_rerank instances; others are zero-padded


def _width_of(widths, d: int, what: str) -> int:
    for w in widths:
        if d <= w:
            return w
    raise ValueError(f"{what} supports embedding_dim <= {widths[-1]}, got {d}")


def _bf16_rows(item_table: torch.Tensor, widths, what: str) -> torch.Tensor:
    """A bf16 [rows, d] table, contiguous and zero-padded to the next of ``widths``."""
    _need(item_table.dtype == torch.bfloat16 and item_table.dim() == 2, "item_table must be bf16 2-D")
    return pad_columns(item_table.contiguous(), _width_of(widths, item_table.size(1), what))


def _candidates(cand_items: torch.Tensor, cand_scores: torch.Tensor):
    """The re-rankers' candidates, contiguous: (ids int32 [n, C], scores fp32 [n, C], n, C)."""
    _need(cand_items.dtype == torch.int32 and cand_scores.dtype == torch.float32,
          "int32 candidate ids, fp32 scores")
    _need(cand_items.dim() == 2 and cand_items.shape == cand_scores.shape, "[n, C] inputs")
    return cand_items.contiguous(), cand_scores.contiguous(), *cand_items.shape


def ild_embedding(recs: torch.Tensor, item_table: torch.Tensor, kind: str = "cosine",
                  check: bool = True) -> torch.Tensor:
    """Per-user ILD with D computed from bf16 item embeddings (cosine/dot/euclidean).
    A list with an id outside the table gives NaN; with ``check`` the call
    reads the count (one sync) and raises IndexError."""
    dev = B.require_device(recs, item_table)
    recs, rc_dt = _recs(recs)
    _need(item_table.dtype == torch.bfloat16 and item_table.dim() == 2, "item_table must be bf16 2-D")
    _contig(item_table, "item_table")
    _need(kind in _KINDS, f"kind must be one of {sorted(_KINDS)}")
    # a width without a kernel instance (e.g. d = 100) is zero-padded per call,
    # never cached: writes through .data or raw pointers bump no version a
    # cache could key on. Repeated callers pad once themselves
    # (EmbeddingDistance holds its padded table; pad_columns is public).
    item_table = pad_columns(item_table, _width_of(ILD_WIDTHS, item_table.size(1), "embedding ILD"))
    n, k = recs.shape
    _need(k <= 16384, "embedding ILD supports k <= 16384")
    out = torch.empty(n, dtype=torch.float32, device=dev)
    if n == 0:
        return out
    err, own = _counter(dev, check=check)
    rc = B.lib().dr_ild_embedding(
        recs.data_ptr(), rc_dt, n, k, item_table.data_ptr(), item_table.size(0),
        item_table.size(1), _KINDS[kind], out.data_ptr(), B.ptr(err), B.stream(dev),
    )
    _done(rc, "dr_ild_embedding", own)
    return out


ILD_GRAD_MAX_K, ILD_GRAD_MAX_D = 128, 256  # dr_ild_embedding_backward's bounds


def ild_embedding_backward(
    recs: torch.Tensor,
    item_table: torch.Tensor,
    kind: str,
    grad_item: torch.Tensor,
    grad_out: Optional[torch.Tensor] = None,
    scale: float = 1.0,
    err: Optional[torch.Tensor] = None,
    check: bool = True,
) -> None:
    """Adds to ``grad_item`` the gradient of ``scale * sum_u grad_out[u] * ILD_u``
    with respect to the fp32 ``item_table`` (dr_ild_embedding_backward; the
    closed forms are in include/divrec_hip.h). ``grad_out`` None means all
    ones. Lists of 1 <= k <= 128 ids, any width d <= 256. Ids are range-checked
    on the device (a list with an invalid id adds nothing): with ``check`` and
    no ``err`` the call reads the count (one sync) and raises IndexError;
    otherwise the count goes to the caller's ``err`` (may be None), checked by
    the caller."""
    dev = B.require_device(recs, item_table, grad_item, grad_out)
    recs, rc_dt = _recs(recs)
    _need(item_table.dtype == torch.float32 and item_table.dim() == 2, "item_table must be fp32 2-D")
    _contig(item_table, "item_table")
    _need(grad_item.shape == item_table.shape and grad_item.dtype == torch.float32
          and grad_item.is_contiguous(),
          "grad_item must be a contiguous fp32 tensor shaped like item_table")
    _need(kind in _KINDS, f"kind must be one of {sorted(_KINDS)}")
    n, k = recs.shape
    _need(1 <= k <= ILD_GRAD_MAX_K, f"embedding ILD gradient supports 1 <= k <= {ILD_GRAD_MAX_K}")
    _need(1 <= item_table.size(1) <= ILD_GRAD_MAX_D,
          f"embedding ILD gradient supports embedding_dim <= {ILD_GRAD_MAX_D}")
    if grad_out is not None:
        _need(grad_out.dim() == 1 and grad_out.numel() == n, "grad_out must be 1-D, one per list")
        grad_out = grad_out.to(torch.float32).contiguous()
    if n == 0:
        return
    err, own = _counter(dev, err, check)
    rc = B.lib().dr_ild_embedding_backward(
        recs.data_ptr(), rc_dt, n, k, item_table.data_ptr(), item_table.size(0),
        item_table.size(1), _KINDS[kind], B.ptr(grad_out), float(scale), grad_item.data_ptr(),
        B.ptr(err), B.stream(dev),
    )
    _done(rc, "dr_ild_embedding_backward", own)


# --------------------------------------------------------------------------- BPR
def bpr_fwd_bwd(
    user_table: torch.Tensor,
    item_table: torch.Tensor,
    user_id: torch.Tensor,
    pos_id: torch.Tensor,
    neg_id: torch.Tensor,
    grad_scale: float,
    grad_user: Optional[torch.Tensor],
    grad_item: Optional[torch.Tensor],
    err: Optional[torch.Tensor] = None,
    check: bool = True,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """Fused BPR forward + backward; returns per-triple (loss fp32, hit int32)
    and accumulates dense gradients into grad_user / grad_item. Ids are
    range-checked on the device (an invalid triple adds nothing): with
    ``check`` and no ``err`` the call reads the count (one sync) and raises
    IndexError; otherwise the count goes to the caller's ``err`` (may be None),
    checked by the caller (pair_wise_train_loop: once per epoch)."""
    dev = B.require_device(user_table, item_table, user_id, pos_id, neg_id, grad_user, grad_item)
    _table_pair(user_table, item_table, (torch.float32,), "fp32 tables")
    user_id, pos_id, neg_id = _id_columns((user_id, pos_id, neg_id))
    n = user_id.numel()
    _grad_like(grad_user, user_table, "grad_user"), _grad_like(grad_item, item_table, "grad_item")
    loss = torch.empty(n, dtype=torch.float32, device=dev)
    hit = torch.empty(n, dtype=torch.int32, device=dev)
    err, own = _counter(dev, err, check)
    rc = B.lib().dr_bpr_fwd_bwd(
        user_table.data_ptr(), user_table.size(0), item_table.data_ptr(), item_table.size(0),
        user_table.size(1), user_id.data_ptr(), pos_id.data_ptr(),
        neg_id.data_ptr(), n, float(grad_scale), loss.data_ptr(), hit.data_ptr(),
        B.ptr(grad_user), B.ptr(grad_item), B.ptr(err), B.stream(dev),
    )
    _done(rc, "dr_bpr_fwd_bwd", own)
    return loss, hit


# --------------------------------------------------------------------------- WARP
WARP_MAX_TRIALS = 4096  # dr_warp_fwd_bwd's largest max_trials (include/divrec_hip.h)


def _user_csr(csr, n_users: int, name: str):
    """An optional per-user CSR (rowptr int64 [n_users + 1], items int32): the
    two tensors, contiguous, or (None, None)."""
    if csr is None:
        return None, None
    rowptr, items = csr
    _need(rowptr.dtype == torch.int64 and items.dtype == torch.int32,
          f"{name} CSR must be int64 rowptr / int32 items")
    _need(rowptr.dim() == 1 and rowptr.numel() == n_users + 1 and items.dim() == 1,
          f"{name} CSR must have one row per user row of the table")
    return rowptr.contiguous(), items.contiguous()


def warp_fwd_bwd(
    user_table: torch.Tensor,
    item_table: torch.Tensor,
    user_id: torch.Tensor,
    pos_id: torch.Tensor,
    positives: Optional[Tuple[torch.Tensor, torch.Tensor]],
    exclude: Optional[Tuple[torch.Tensor, torch.Tensor]],
    max_trials: int,
    margin: float,
    seed: int,
    pair_base: int,
    grad_scale: float,
    grad_user: Optional[torch.Tensor],
    grad_item: Optional[torch.Tensor],
    err: Optional[torch.Tensor] = None,
    check: bool = True,
) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Fused WARP forward + backward (dr_warp_fwd_bwd, whose header comment is
    the specification); returns per-pair (loss fp32, neg_id int64, trials
    int32) and accumulates the violating triples' dense gradients into
    grad_user / grad_item (either may be None). ``positives`` / ``exclude``:
    per-user CSRs (rowptr int64 [n_users + 1], items int32 sorted per row) of
    items a draw skips, or None. A pair without a violator within
    ``max_trials`` draws has loss 0, neg_id -1 and adds nothing. Ids are
    range-checked on the device (an invalid pair adds nothing): with ``check``
    and no ``err`` the call reads the count (one sync) and raises IndexError;
    otherwise the count goes to the caller's ``err`` (may be None), checked by
    the caller (warp_train_loop: once per epoch)."""
    dev = B.require_device(user_table, item_table, user_id, pos_id, grad_user, grad_item,
                           *(positives or ()), *(exclude or ()))
    _table_pair(user_table, item_table, (torch.float32,), "fp32 tables")
    user_id, pos_id = _id_columns((user_id, pos_id))
    n = user_id.numel()
    _grad_like(grad_user, user_table, "grad_user"), _grad_like(grad_item, item_table, "grad_item")
    _need(1 <= int(max_trials) <= WARP_MAX_TRIALS, f"max_trials must be in [1, {WARP_MAX_TRIALS}]")
    _need(int(pair_base) >= 0, "pair_base must be >= 0")
    pr, pi = _user_csr(positives, user_table.size(0), "positives")
    er, ei = _user_csr(exclude, user_table.size(0), "exclude")
    loss = torch.empty(n, dtype=torch.float32, device=dev)
    neg = torch.empty(n, dtype=torch.int64, device=dev)
    trials = torch.empty(n, dtype=torch.int32, device=dev)
    err, own = _counter(dev, err, check)
    rc = B.lib().dr_warp_fwd_bwd(
        user_table.data_ptr(), user_table.size(0), item_table.data_ptr(), item_table.size(0),
        user_table.size(1), user_id.data_ptr(), pos_id.data_ptr(), n, B.ptr(pr), B.ptr(pi),
        B.ptr(er), B.ptr(ei), int(max_trials), float(margin), int(seed) & ((1 << 64) - 1),
        int(pair_base), float(grad_scale), loss.data_ptr(), neg.data_ptr(), trials.data_ptr(),
        B.ptr(grad_user), B.ptr(grad_item), B.ptr(err), B.stream(dev),
    )
    _done(rc, "dr_warp_fwd_bwd", own)
    return loss, neg, trials


def warp_candidates(seed: int, pair_base: int, n_pairs: int, max_trials: int,
                    n_items: int) -> torch.Tensor:
    """The candidate stream of ``warp_fwd_bwd`` as a CPU int32 tensor
    [n_pairs, max_trials] (dr_warp_candidates: host only, needs no GPU)."""
    out = torch.empty((int(n_pairs), int(max_trials)), dtype=torch.int32)
    rc = B.lib().dr_warp_candidates(int(seed) & ((1 << 64) - 1), int(pair_base), int(n_pairs),
                                    int(max_trials), int(n_items), out.data_ptr())
    B.check(rc, "dr_warp_candidates")
    return out


# --------------------------------------------------------------------------- point-wise MSE
def mse_fwd_bwd(
    user_table: torch.Tensor,
    item_table: torch.Tensor,
    user_id: torch.Tensor,
    item_id: torch.Tensor,
    target: torch.Tensor,
    grad_scale: float,
    grad_user: Optional[torch.Tensor],
    grad_item: Optional[torch.Tensor],
    err: Optional[torch.Tensor] = None,
    check: bool = True,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """Fused point-wise MSE forward + backward (dr_mse_fwd_bwd); returns
    per-pair (pred fp32, loss fp32) with loss = (target - pred)^2 and
    accumulates ``-2 (target - pred) grad_scale`` times the other side's row
    into the dense grad_user / grad_item. Both gradient tables None is the
    forward-only form (no atomics). Ids are range-checked on the device (an
    invalid pair adds nothing and gets NaN): with ``check`` and no ``err`` the
    call reads the count (one sync) and raises IndexError; otherwise the count
    goes to the caller's ``err`` (may be None), checked by the caller
    (point_wise_train_loop: once per epoch)."""
    dev = B.require_device(user_table, item_table, user_id, item_id, target, grad_user, grad_item)
    _table_pair(user_table, item_table, (torch.float32,), "fp32 tables")
    user_id, item_id = _id_columns((user_id, item_id))
    n = user_id.numel()
    _need(target.dtype == torch.float32 and target.dim() == 1 and target.numel() == n,
          "target must be 1-D fp32, one per pair")
    _grad_like(grad_user, user_table, "grad_user"), _grad_like(grad_item, item_table, "grad_item")
    target = target.contiguous()
    pred = torch.empty(n, dtype=torch.float32, device=dev)
    loss = torch.empty(n, dtype=torch.float32, device=dev)
    err, own = _counter(dev, err, check)
    rc = B.lib().dr_mse_fwd_bwd(
        user_table.data_ptr(), user_table.size(0), item_table.data_ptr(), item_table.size(0),
        user_table.size(1), user_id.data_ptr(), item_id.data_ptr(),
        target.data_ptr(), n, float(grad_scale), pred.data_ptr(), loss.data_ptr(),
        B.ptr(grad_user), B.ptr(grad_item), B.ptr(err), B.stream(dev),
    )
    _done(rc, "dr_mse_fwd_bwd", own)
    return pred, loss


def adam_dense(
    param: torch.Tensor, grad: torch.Tensor, exp_avg: torch.Tensor, exp_avg_sq: torch.Tensor,
    lr: float, beta1: float, beta2: float, eps: float, weight_decay: float, step: int,
) -> None:
    dev = B.require_device(param, grad, exp_avg, exp_avg_sq)
    for t in (param, grad, exp_avg, exp_avg_sq):
        _need(t.dtype == torch.float32 and t.is_contiguous() and t.numel() == param.numel(),
              "adam tensors must be contiguous fp32 of equal size")
    rc = B.lib().dr_adam_dense(
        param.data_ptr(), grad.data_ptr(), exp_avg.data_ptr(), exp_avg_sq.data_ptr(),
        param.numel(), float(lr), float(beta1), float(beta2), float(eps), float(weight_decay),
        int(step), B.stream(dev),
    )
    B.check(rc, "dr_adam_dense")


def adam_rows(
    param: torch.Tensor, grad: torch.Tensor, exp_avg: torch.Tensor, exp_avg_sq: torch.Tensor,
    rows: torch.Tensor, lr: float, beta1: float, beta2: float, eps: float, step: int,
    zero_grad: bool = True,
) -> None:
    """torch.optim.SparseAdam's update over the UNIQUE rows ``rows`` of 2-D
    fp32 tables (gradient values read from the dense ``grad``); with
    ``zero_grad`` the touched gradient rows are zeroed afterwards."""
    dev = B.require_device(param, grad, exp_avg, exp_avg_sq, rows)
    _need(param.dim() == 2, "adam_rows: param must be a 2-D table")
    for t in (param, grad, exp_avg, exp_avg_sq):
        _need(t.dtype == torch.float32 and t.is_contiguous() and t.shape == param.shape,
              "adam_rows tensors must be contiguous fp32 tables of equal shape")
    rows = rows.to(torch.int64).contiguous()
    _need(rows.dim() == 1, "adam_rows: rows must be 1-D")
    rc = B.lib().dr_adam_rows(
        param.data_ptr(), grad.data_ptr(), exp_avg.data_ptr(), exp_avg_sq.data_ptr(),
        param.size(1), rows.data_ptr(), rows.numel(), float(lr), float(beta1), float(beta2),
        float(eps), int(step), 1 if zero_grad else 0, B.stream(dev),
    )
    B.check(rc, "dr_adam_rows")


# --------------------------------------------------------------------------- pairwise sampler
def sample_pairwise(users: torch.Tensor, pos_rowptr: torch.Tensor, pos_items: torch.Tensor,
                    n_items: int, m: int, seed: int,
                    exclude: Optional[Tuple[torch.Tensor, torch.Tensor]] = None,
                    expand: bool = True):
    """PairWiseDataset's per-user sampling on the device (dr_sample_pairwise).
    Returns (pos [n, m] int32, neg [n, m] int32, triples) where triples is
    (uid, pid, nid) int64 [n*m*m] in the reference's pos-major order, or None
    without ``expand``. Raises IndexError, as the reference does, when a user
    has no positives or no allowed negative (this reads one device counter)."""
    dev = B.require_device(users, pos_rowptr, pos_items)
    _need(pos_items.dtype == torch.int32 and pos_rowptr.dtype == torch.int64,
          "positives CSR must be int64 rowptr / int32 items")
    users = users.to(torch.int64).contiguous()
    n = users.numel()
    pos = torch.empty((n, m), dtype=torch.int32, device=dev)
    neg = torch.empty((n, m), dtype=torch.int32, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    trip = None
    if expand:
        trip = tuple(torch.empty(n * m * m, dtype=torch.int64, device=dev) for _ in range(3))
    er, ei = (None, None) if exclude is None else exclude
    rc = B.lib().dr_sample_pairwise(
        users.data_ptr(), n, pos_rowptr.contiguous().data_ptr(), pos_items.contiguous().data_ptr(),
        B.ptr(er), B.ptr(ei), int(n_items), int(m), int(seed) & ((1 << 64) - 1),
        pos.data_ptr(), neg.data_ptr(), *(B.ptr(t) for t in (trip or (None,) * 3)),
        err.data_ptr(), B.stream(dev),
    )
    B.check(rc, "dr_sample_pairwise")
    if int(err.item()) != 0:
        raise IndexError("Cannot choose from an empty sequence (a user without positives, "
                         "or without any allowed negative)")
    return pos, neg, trip


# --------------------------------------------------------------------------- catalog histogram
def catalog_histogram(recs: torch.Tensor, n_items: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """(counts int32 [n_items], position sums int64 [n_items]) of the item ids
    in ``recs`` [n, k]; entries outside [0, n_items) are skipped."""
    dev = B.require_device(recs)
    recs, rc_dt = _recs(recs)
    n, k = recs.shape
    _need(n_items >= 1, "n_items must be >= 1")
    counts = torch.zeros(int(n_items), dtype=torch.int32, device=dev)
    pos_sum = torch.zeros(int(n_items), dtype=torch.int64, device=dev)
    if n == 0 or k == 0:
        return counts, pos_sum
    rc = B.lib().dr_catalog_histogram(recs.data_ptr(), rc_dt, n, k, int(n_items),
                                      counts.data_ptr(), pos_sum.data_ptr(), B.stream(dev))
    B.check(rc, "dr_catalog_histogram")
    return counts, pos_sum


# --------------------------------------------------------------------------- MMR
def mmr_rerank(
    cand_items: torch.Tensor, cand_scores: torch.Tensor, item_table: torch.Tensor, k_out: int,
    lam: float = 0.5, check: bool = True,
) -> torch.Tensor:
    """Greedy MMR over per-user candidates (int32 [n, C] + fp32 [n, C]) -> int32 [n, k_out].
    Candidate ids < 0 are empty slots; with ``check`` an id >= the table's row
    count raises IndexError after the call (one counter read), as indexing the
    table would (without it such candidates are silently never picked).
    -inf and NaN scores count as -FLT_MAX (such a candidate stays live and is
    picked last); an all-zero item row has cosine 0 with every row and stays
    eligible on its score; +inf scores and non-finite rows are outside the
    contract. Widths other than 64 / 128 are zero-padded per call (no cache, so every
    write to the table is seen; pass a pre-padded table to avoid the copy)."""
    dev = B.require_device(cand_items, cand_scores, item_table)
    cand_items, cand_scores, n, C = _candidates(cand_items, cand_scores)
    item_table = _bf16_rows(item_table, MMR_WIDTHS, "mmr_rerank")
    out = torch.empty((n, int(k_out)), dtype=torch.int32, device=dev)
    if n == 0:
        return out
    err, own = _counter(dev, check=check)
    rc = B.lib().dr_mmr_rerank(
        cand_items.data_ptr(), cand_scores.data_ptr(), n, C,
        item_table.data_ptr(), item_table.size(0), item_table.size(1), int(k_out),
        float(lam), out.data_ptr(), B.ptr(err), B.stream(dev),
    )
    _done(rc, "dr_mmr_rerank", own)
    return out


# --------------------------------------------------------------------------- DPP
def dpp_rerank(
    cand_items: torch.Tensor, cand_scores: torch.Tensor, item_table: torch.Tensor, k_out: int,
    lam: float = 0.5, check: bool = True,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """Greedy DPP MAP over per-user candidates (int32 [n, C] + fp32 [n, C]) ->
    (items int32 [n, k_out], resid fp32 [n, k_out]): each pick maximises
    lam * score + (1 - lam) * log(residual), the residual being the pick's
    det-ratio against the picked set under the cosine Gram (include/divrec_hip.h).
    ``resid`` holds each pick's residual when it was picked, so
    ``resid.log().sum(1)`` is the list's log-determinant. A list that runs out
    of eligible candidates (rank exhausted, duplicates only) ends in -1 / 0.
    Candidate ids < 0 are empty slots; with ``check`` an id >= the table's row
    count raises IndexError after the call (one counter read); without it such
    candidates are silently never picked. Widths other than 64 / 128 are
    zero-padded per call, as for ``mmr_rerank``."""
    dev = B.require_device(cand_items, cand_scores, item_table)
    cand_items, cand_scores, n, C = _candidates(cand_items, cand_scores)
    item_table = _bf16_rows(item_table, DPP_WIDTHS, "dpp_rerank")
    out = torch.empty((n, int(k_out)), dtype=torch.int32, device=dev)
    resid = torch.empty((n, int(k_out)), dtype=torch.float32, device=dev)
    if n == 0:
        return out, resid
    err, own = _counter(dev, check=check)
    rc = B.lib().dr_dpp_rerank(
        cand_items.data_ptr(), cand_scores.data_ptr(), n, C,
        item_table.data_ptr(), item_table.size(0), item_table.size(1), int(k_out),
        float(lam), out.data_ptr(), resid.data_ptr(), B.ptr(err), B.stream(dev),
    )
    _done(rc, "dr_dpp_rerank", own)
    return out, resid


# --------------------------------------------------------------------------- calibration
CALIB_MAX_LABELS = 64  # DR_CALIB_MAX_LABELS


def _labels32(labels: torch.Tensor) -> torch.Tensor:
    """Item labels as the int32 table the calibration kernels read. int64
    labels are clamped to [-1, 64] first, so a value no int32 holds stays
    outside [0, G) instead of wrapping into it."""
    _need(labels.dim() == 1 and labels.dtype in (torch.int32, torch.int64),
          "item labels must be 1-D int32 or int64")
    _need(labels.numel() >= 1, "item labels must not be empty")
    if labels.dtype == torch.int64:
        labels = labels.clamp(-1, CALIB_MAX_LABELS).to(torch.int32)
    return labels.contiguous()


def _n_labels(n_labels: int) -> int:
    n_labels = int(n_labels)
    _need(1 <= n_labels <= CALIB_MAX_LABELS, f"n_labels must be in [1, {CALIB_MAX_LABELS}]")
    return n_labels


def _profile(profile: torch.Tensor, n: int) -> torch.Tensor:
    _need(profile.dtype == torch.float32 and profile.dim() == 2 and profile.size(0) == n,
          "profile must be fp32 [n, n_labels]")
    _n_labels(profile.size(1))
    return profile.contiguous()


def calibrated_rerank(
    cand_items: torch.Tensor, cand_scores: torch.Tensor, item_labels: torch.Tensor,
    profile: torch.Tensor, k_out: int, lam: float = 0.5, check: bool = True,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """Greedy calibrated re-rank (Steck 2018) over per-user candidates (int32
    [n, C] + fp32 [n, C]) -> (items int32 [n, k_out], kl fp32 [n, k_out]): each
    pick maximises lam * score - (1 - lam) * KL(p || q~(list + pick)), p the
    normalised row of ``profile`` (fp32 [n, G], G <= 64, e.g. ``label_profile``
    of the user's history) and q~ the label shares of the list under
    ``item_labels`` (int32 or int64 [n_items], values in [0, G)), smoothed with
    p (include/divrec_hip.h). ``kl[:, t]`` is the list's KL after pick t, so
    ``kl[:, -1]`` is ``calibration_kl`` of the finished list. A list that runs
    out of live candidates ends in -1 with the KL repeated. Candidate ids < 0
    are empty slots; with ``check`` a candidate id past the label table or a
    candidate whose label is outside [0, G) raises IndexError after the call
    (one counter read); without it such candidates are silently never picked."""
    dev = B.require_device(cand_items, cand_scores, item_labels, profile)
    cand_items, cand_scores, n, C = _candidates(cand_items, cand_scores)
    labels, profile = _labels32(item_labels), _profile(profile, n)
    out = torch.empty((n, int(k_out)), dtype=torch.int32, device=dev)
    kl = torch.empty((n, int(k_out)), dtype=torch.float32, device=dev)
    if n == 0:
        return out, kl
    err, own = _counter(dev, check=check)
    rc = B.lib().dr_calibrated_rerank(
        cand_items.data_ptr(), cand_scores.data_ptr(), n, C,
        labels.data_ptr(), labels.numel(), profile.size(1), profile.data_ptr(), int(k_out),
        float(lam), out.data_ptr(), kl.data_ptr(), B.ptr(err), B.stream(dev),
    )
    _done(rc, "dr_calibrated_rerank", own)
    return out, kl


def label_profile(rowptr: torch.Tensor, items: torch.Tensor, item_labels: torch.Tensor,
                  n_labels: int, check: bool = True) -> torch.Tensor:
    """fp32 [n, n_labels]: the normalised label histogram of every row of the
    CSR (rowptr int64 [n + 1], items int32), the profile ``calibrated_rerank``
    and ``calibration_kl`` take; an empty row is a zero row. With ``check`` an
    item outside the label table or a label outside [0, n_labels) raises
    IndexError (one counter read); without it they are skipped."""
    dev = B.require_device(rowptr, items, item_labels)
    _need(rowptr.dtype == torch.int64 and rowptr.dim() == 1 and rowptr.numel() >= 1,
          "rowptr int64 [n + 1]")
    _need(items.dtype == torch.int32 and items.dim() == 1, "items must be int32 1-D")
    G, labels = _n_labels(n_labels), _labels32(item_labels)
    n = rowptr.numel() - 1
    out = torch.empty((n, G), dtype=torch.float32, device=dev)
    if n == 0:
        return out
    err, own = _counter(dev, check=check)
    rc = B.lib().dr_label_profile(
        rowptr.contiguous().data_ptr(), items.contiguous().data_ptr() if items.numel() else None,
        n, labels.data_ptr(), labels.numel(), G, out.data_ptr(), B.ptr(err), B.stream(dev),
    )
    _done(rc, "dr_label_profile", own)
    return out


def calibration_kl(recs: torch.Tensor, item_labels: torch.Tensor, profile: torch.Tensor,
                   check: bool = True) -> torch.Tensor:
    """fp32 [n]: KL(p || q~) of each list of ``recs`` [n, k] (int32 or int64;
    entries < 0, the tail of a list that ended early, are skipped) against the
    normalised rows of ``profile`` (fp32 [n, G]); 0 is a perfectly calibrated
    list. With ``check`` an entry past the label table or with a label outside
    [0, G) raises IndexError (one counter read); without it it is skipped."""
    dev = B.require_device(recs, item_labels, profile)
    recs, rc_dt = _recs(recs)
    n, k = recs.shape
    labels, profile = _labels32(item_labels), _profile(profile, n)
    out = torch.empty(n, dtype=torch.float32, device=dev)
    if n == 0:
        return out
    err, own = _counter(dev, check=check)
    rc = B.lib().dr_calibration_kl(
        recs.data_ptr() if k else None, rc_dt, n, k, labels.data_ptr(), labels.numel(),
        profile.size(1), profile.data_ptr(), out.data_ptr(), B.ptr(err), B.stream(dev),
    )
    _done(rc, "dr_calibration_kl", own)
    return out


# --------------------------------------------------------------------------- xQuAD
XQUAD_MAX_ASPECTS = 64   # DR_XQUAD_MAX_ASPECTS
XQUAD_MAX_CELLS = 32768  # DR_XQUAD_MAX_CELLS: candidates x aspects of one user in LDS


def _aspects(item_aspects: torch.Tensor) -> torch.Tensor:
    _need(item_aspects.dtype == torch.float32 and item_aspects.dim() == 2,
          "item aspects must be fp32 [n_items, n_aspects]")
    _need(item_aspects.size(0) >= 1, "item aspects must not be empty")
    _need(1 <= item_aspects.size(1) <= XQUAD_MAX_ASPECTS,
          f"n_aspects must be in [1, {XQUAD_MAX_ASPECTS}]")
    return item_aspects.contiguous()


def _aspect_profile(profile: torch.Tensor, n: int, G: int) -> torch.Tensor:
    _need(profile.dtype == torch.float32 and profile.dim() == 2 and profile.size(0) == n
          and profile.size(1) == G, "aspect profile must be fp32 [n, n_aspects]")
    return profile.contiguous()


def xquad_rerank(
    cand_items: torch.Tensor, cand_scores: torch.Tensor, item_aspects: torch.Tensor,
    aspect_profile: torch.Tensor, k_out: int, lam: float = 0.5,
    err: Optional[torch.Tensor] = None, check: bool = True,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """Greedy xQuAD re-rank (Santos et al. 2010) over per-user candidates (int32
    [n, C] + fp32 [n, C]) -> (items int32 [n, k_out], cov fp32 [n, k_out]): each
    pick maximises lam * score + (1 - lam) * sum_a m_a c_a, c the candidate's
    row of ``item_aspects`` (fp32 [n_items, G], G <= 64, values clamped to
    [0, 1]) and m the mass of the normalised row of ``aspect_profile`` (fp32
    [n, G], e.g. ``aspect_profile`` of the user's history) that the list has
    not covered yet (include/divrec_hip.h). ``lam`` weights relevance: the
    paper's lambda is 1 - lam. ``cov[:, t]`` is the list's expected aspect
    coverage after pick t, so ``cov[:, -1]`` is ``aspect_coverage`` of the
    finished list. A list that runs out of live candidates ends in -1 with the
    coverage repeated. ``C * G <= XQUAD_MAX_CELLS``. Candidate ids < 0 are
    empty slots; a candidate id past the matrix is never picked and counted:
    into the caller's ``err`` (an int32 device counter) when given, else with
    ``check`` the call reads the count (one sync) and raises IndexError."""
    dev = B.require_device(cand_items, cand_scores, item_aspects, aspect_profile, err)
    cand_items, cand_scores, n, C = _candidates(cand_items, cand_scores)
    aspects = _aspects(item_aspects)
    profile = _aspect_profile(aspect_profile, n, aspects.size(1))
    out = torch.empty((n, int(k_out)), dtype=torch.int32, device=dev)
    cov = torch.empty((n, int(k_out)), dtype=torch.float32, device=dev)
    if n == 0:
        return out, cov
    err, own = _counter(dev, err, check)
    rc = B.lib().dr_xquad_rerank(
        cand_items.data_ptr(), cand_scores.data_ptr(), n, C,
        aspects.data_ptr(), aspects.size(0), aspects.size(1), profile.data_ptr(), int(k_out),
        float(lam), out.data_ptr(), cov.data_ptr(), B.ptr(err), B.stream(dev),
    )
    _done(rc, "dr_xquad_rerank", own)
    return out, cov


def aspect_profile(rowptr: torch.Tensor, items: torch.Tensor, item_aspects: torch.Tensor,
                   err: Optional[torch.Tensor] = None, check: bool = True) -> torch.Tensor:
    """fp32 [n, G]: the normalised aspect sums of every row of the CSR (rowptr
    int64 [n + 1], items int32) over ``item_aspects`` (fp32 [n_items, G]), the
    profile ``xquad_rerank`` and ``aspect_coverage`` take; an empty or all-zero
    row is a zero row. An item outside the matrix is skipped and counted, into
    ``err`` when given, else with ``check`` it raises IndexError (one counter
    read). Bitwise reproducible (no atomics)."""
    dev = B.require_device(rowptr, items, item_aspects, err)
    _need(rowptr.dtype == torch.int64 and rowptr.dim() == 1 and rowptr.numel() >= 1,
          "rowptr int64 [n + 1]")
    _need(items.dtype == torch.int32 and items.dim() == 1, "items must be int32 1-D")
    aspects = _aspects(item_aspects)
    n, G = rowptr.numel() - 1, aspects.size(1)
    out = torch.empty((n, G), dtype=torch.float32, device=dev)
    if n == 0:
        return out
    err, own = _counter(dev, err, check)
    rc = B.lib().dr_aspect_profile(
        rowptr.contiguous().data_ptr(), items.contiguous().data_ptr() if items.numel() else None,
        n, aspects.data_ptr(), aspects.size(0), G, out.data_ptr(), B.ptr(err), B.stream(dev),
    )
    _done(rc, "dr_aspect_profile", own)
    return out


def aspect_coverage(recs: torch.Tensor, item_aspects: torch.Tensor, aspect_profile: torch.Tensor,
                    err: Optional[torch.Tensor] = None, check: bool = True) -> torch.Tensor:
    """fp32 [n]: the expected aspect coverage sum_a p_a (1 - prod_j (1 - c_{j,a}))
    of each list of ``recs`` [n, k] (int32 or int64; entries < 0, the tail of a
    list that ended early, are skipped) under the normalised rows p of
    ``aspect_profile`` (fp32 [n, G]); 1 is a list that covers every aspect the
    profile weighs, and with a uniform profile and binary aspects it is
    subtopic recall. An entry past the matrix is skipped and counted, into
    ``err`` when given, else with ``check`` it raises IndexError."""
    dev = B.require_device(recs, item_aspects, aspect_profile, err)
    recs, rc_dt = _recs(recs)
    n, k = recs.shape
    aspects = _aspects(item_aspects)
    profile = _aspect_profile(aspect_profile, n, aspects.size(1))
    out = torch.empty(n, dtype=torch.float32, device=dev)
    if n == 0:
        return out
    err, own = _counter(dev, err, check)
    rc = B.lib().dr_aspect_coverage(
        recs.data_ptr() if k else None, rc_dt, n, k, aspects.data_ptr(), aspects.size(0),
        aspects.size(1), profile.data_ptr(), out.data_ptr(), B.ptr(err), B.stream(dev),
    )
    _done(rc, "dr_aspect_coverage", own)
    return out


# --------------------------------------------------------------------------- history distance
HISTORY_WIDTHS = (32, 64, 128, 256)
HISTORY_MAX_C = 1024
_HIST_REDUCE = {"min": 0, "mean": 1}  # enum dr_hist_reduce


def _history_csr(rowptr: torch.Tensor, items: torch.Tensor, n: int):
    _need(rowptr.dtype == torch.int64 and rowptr.dim() == 1 and rowptr.numel() == n + 1,
          "history rowptr must be int64 [n + 1]")
    _need(items.dtype == torch.int32 and items.dim() == 1, "history items must be int32 1-D")
    return rowptr.contiguous(), items.contiguous()


def _hist_reduce(reduce: str) -> int:
    _need(reduce in _HIST_REDUCE, f"reduce must be one of {sorted(_HIST_REDUCE)}")
    return _HIST_REDUCE[reduce]


def history_distance(lists: torch.Tensor, item_table: torch.Tensor, hist_rowptr: torch.Tensor,
                     hist_items: torch.Tensor, reduce: str = "min",
                     err: Optional[torch.Tensor] = None, check: bool = True) -> torch.Tensor:
    """fp32 [n, C]: for every position of ``lists`` (int32 [n, C], C <= 1024) the
    ``reduce`` ("min" or "mean") over the user's history row of the CSR
    (rowptr int64 [n + 1], items int32) of 1 - cos(e_item, e_h) on the bf16
    ``item_table`` (include/divrec_hip.h, dr_history_distance). A user without a
    valid history entry gets 0, a list id < 0 gets 0, a list id past the table
    NaN. Ids outside the table (list or history) are counted: into ``err`` when
    given, else with ``check`` the call reads the count (one sync) and raises
    IndexError."""
    dev = B.require_device(lists, item_table, hist_rowptr, hist_items, err)
    _need(lists.dtype == torch.int32 and lists.dim() == 2, "lists must be int32 [n, C]")
    n, C = lists.shape
    _need(1 <= C <= HISTORY_MAX_C, f"C must be in [1, {HISTORY_MAX_C}]")
    red = _hist_reduce(reduce)
    table = _bf16_rows(item_table, HISTORY_WIDTHS, "history distance")
    _need(table.size(0) >= 1, "item_table must not be empty")
    rowptr, items = _history_csr(hist_rowptr, hist_items, n)
    out = torch.empty((n, C), dtype=torch.float32, device=dev)
    if n == 0:
        return out
    err, own = _counter(dev, err, check)
    rc = B.lib().dr_history_distance(
        lists.contiguous().data_ptr(), n, C, table.data_ptr(), table.size(0), table.size(1),
        rowptr.data_ptr(), items.data_ptr() if items.numel() else None, red, out.data_ptr(),
        B.ptr(err), B.stream(dev),
    )
    _done(rc, "dr_history_distance", own)
    return out


def serendipity_rerank(
    cand_items: torch.Tensor, cand_scores: torch.Tensor, item_table: torch.Tensor,
    hist_rowptr: torch.Tensor, hist_items: torch.Tensor, k_out: int, lam: float = 0.5,
    reduce: str = "min", err: Optional[torch.Tensor] = None, check: bool = True,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """Serendipity re-rank over per-user candidates (int32 [n, C] + fp32 [n, C])
    -> (items int32 [n, k_out], dist fp32 [n, k_out]): the first ``k_out``
    candidates in stable descending order of lam * score + (1 - lam) * dist,
    dist the ``history_distance`` of the candidate from the user's history row
    (include/divrec_hip.h, dr_serendipity_rerank); ties go to the lowest
    candidate position. ``lam`` weights relevance as in every re-ranker: lam =
    1, and a user without history, give the order by score. A list with fewer
    than ``k_out`` live candidates ends in -1 with dist 0. Ids outside the
    table are counted as in ``history_distance``."""
    dev = B.require_device(cand_items, cand_scores, item_table, hist_rowptr, hist_items, err)
    cand_items, cand_scores, n, C = _candidates(cand_items, cand_scores)
    _need(1 <= C <= HISTORY_MAX_C, f"C must be in [1, {HISTORY_MAX_C}]")
    _need(1 <= int(k_out) <= C, "k_out must be in [1, C]")
    _need(0.0 <= float(lam) <= 1.0, "lam must be in [0, 1]")
    red = _hist_reduce(reduce)
    table = _bf16_rows(item_table, HISTORY_WIDTHS, "serendipity re-rank")
    _need(table.size(0) >= 1, "item_table must not be empty")
    rowptr, items = _history_csr(hist_rowptr, hist_items, n)
    out = torch.empty((n, int(k_out)), dtype=torch.int32, device=dev)
    dist = torch.empty((n, int(k_out)), dtype=torch.float32, device=dev)
    if n == 0:
        return out, dist
    err, own = _counter(dev, err, check)
    rc = B.lib().dr_serendipity_rerank(
        cand_items.data_ptr(), cand_scores.data_ptr(), n, C, table.data_ptr(), table.size(0),
        table.size(1), rowptr.data_ptr(), items.data_ptr() if items.numel() else None, red,
        int(k_out), float(lam), out.data_ptr(), dist.data_ptr(), B.ptr(err), B.stream(dev),
    )
    _done(rc, "dr_serendipity_rerank", own)
    return out, dist


def list_item_mean(recs: torch.Tensor, item_values: torch.Tensor,
                   err: Optional[torch.Tensor] = None, check: bool = True) -> torch.Tensor:
    """fp32 [n]: the mean of ``item_values`` (fp32 [n_items]) over the valid
    entries of each list of ``recs`` [n, k] (int32 or int64; entries < 0 are
    skipped; a list without a valid entry scores 0), summed in position order.
    An entry past the table is skipped and counted, into ``err`` when given,
    else with ``check`` it raises IndexError."""
    dev = B.require_device(recs, item_values, err)
    recs, rc_dt = _recs(recs)
    n, k = recs.shape
    _need(item_values.dtype == torch.float32 and item_values.dim() == 1,
          "item_values must be fp32 [n_items]")
    values = item_values.contiguous()
    out = torch.empty(n, dtype=torch.float32, device=dev)
    if n == 0:
        return out
    err, own = _counter(dev, err, check)
    rc = B.lib().dr_list_item_mean(
        recs.data_ptr() if k else None, rc_dt, n, k, values.data_ptr() if values.numel() else None,
        values.numel(), out.data_ptr(), B.ptr(err), B.stream(dev),
    )
    _done(rc, "dr_list_item_mean", own)
    return out


# --------------------------------------------------------------------------- rank metrics
def rank_metrics(
    recs: torch.Tensor, pos_rowptr: torch.Tensor, pos_items: torch.Tensor
) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """(precision@k, recall@k, AP@k, NDCG@k) per user of ``recs`` [n, k] against
    positives given as CSR (rowptr int64 [n+1], items int32 sorted per row)."""
    dev = B.require_device(recs, pos_rowptr, pos_items)
    recs, rc_dt = _recs(recs)
    n, k = recs.shape
    _need(pos_rowptr.dtype == torch.int64 and pos_rowptr.numel() == n + 1, "rowptr int64 [n+1]")
    _need(pos_items.dtype == torch.int32, "positives must be int32")
    outs = [torch.empty(n, dtype=torch.float32, device=dev) for _ in range(4)]
    if n == 0:
        return tuple(outs)
    items = pos_items.contiguous() if pos_items.numel() else torch.zeros(1, dtype=torch.int32, device=dev)
    rc = B.lib().dr_rank_metrics(
        recs.data_ptr(), rc_dt, n, k, pos_rowptr.contiguous().data_ptr(), items.data_ptr(),
        *(o.data_ptr() for o in outs), B.stream(dev),
    )
    B.check(rc, "dr_rank_metrics")
    return tuple(outs)


# --------------------------------------------------------------------------- ALS
ALS_WIDTHS = (32, 64, 128)  # dr_als_solve instances; others are zero-padded
GRAM_CHUNK_ROWS = 1 << 20   # rows of a table converted to float64 at a time
GRAM_BLOCK_ROWS = 4096      # rows per product of the batched Gram sum


def _gram64(table: torch.Tensor) -> torch.Tensor:
    """table^T table in float64, [d, d], summed over row chunks."""
    _need(table.dim() == 2 and table.dtype == torch.float32, "table must be fp32 2-D")
    d = table.size(1)
    g = torch.zeros((d, d), dtype=torch.float64, device=table.device)
    for r0 in range(0, table.size(0), GRAM_CHUNK_ROWS):
        t = table[r0:r0 + GRAM_CHUNK_ROWS].to(torch.float64)
        # blocks of GRAM_BLOCK_ROWS rows as one batched product, then their sum:
        # a single [d, rows] x [rows, d] product keeps few workgroups busy
        whole = t.size(0) // GRAM_BLOCK_ROWS * GRAM_BLOCK_ROWS
        if whole:
            blocks = t[:whole].view(-1, GRAM_BLOCK_ROWS, d)
            g += torch.bmm(blocks.transpose(1, 2), blocks).sum(0)
        if whole < t.size(0):
            g += t[whole:].T @ t[whole:]
    return g


def gram(table: torch.Tensor) -> torch.Tensor:
    """G = table^T table, fp32 [d, d]: the Gram matrix ``als_solve`` takes. A
    torch product in float64 (row chunks of at most 2^20 rows, so the float64
    copy stays small), made exactly symmetric and rounded once to fp32. One
    d x d product per half-step, under 1 % of the solve's work."""
    g = _gram64(table)
    return ((g + g.T) * 0.5).to(torch.float32)


_gram_of = gram  # als_solve has an argument of that name


def _csr(rowptr: torch.Tensor, cols: torch.Tensor, weights: Optional[torch.Tensor]):
    """A CSR's (rowptr int64 [n + 1], cols int32 [nnz], weights fp32 [nnz] or
    None), contiguous, and n. rowptr is checked against cols (one host sync):
    the kernel reads cols[rowptr[r] : rowptr[r + 1]] as it is told."""
    _need(rowptr.dtype == torch.int64 and rowptr.dim() == 1 and rowptr.numel() >= 1,
          "rowptr int64 [n + 1]")
    _need(cols.dtype == torch.int32 and cols.dim() == 1, "cols must be int32 1-D")
    if weights is not None:
        _need(weights.dtype == torch.float32 and weights.shape == cols.shape,
              "weights must be fp32, one per entry of cols")
        weights = weights.contiguous()
    rowptr, cols = rowptr.contiguous(), cols.contiguous()
    n = rowptr.numel() - 1
    first, last, falls = torch.stack(
        [rowptr[0], rowptr[-1], (rowptr[1:] < rowptr[:-1]).sum()]).tolist()
    _need(first == 0 and last == cols.numel() and falls == 0,
          "rowptr must rise from 0 to the number of entries of cols")
    return rowptr, cols, weights, n


def als_solve(
    fixed_table: torch.Tensor, rowptr: torch.Tensor, cols: torch.Tensor,
    weights: Optional[torch.Tensor] = None, alpha: float = 1.0, reg: float = 0.1,
    gram: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None, check: bool = True,
) -> torch.Tensor:
    """One implicit-feedback ALS half-step (dr_als_solve, Hu, Koren, Volinsky
    2008): fp32 [n, d], row r the exact minimiser of
    ``sum_i c_ri (p_ri - x^T y_i)^2 + reg |x|^2`` over the fp32 ``fixed_table``
    [m, d], with c = 1 + alpha * w and p = 1 on the entries of row r of the CSR
    (rowptr int64 [n + 1], cols int32, ``weights`` fp32 or None = 1) and c = 1,
    p = 0 elsewhere: ``x = (G + alpha sum_i w_i y_i y_i^T + reg I)^-1
    sum_i (1 + alpha w_i) y_i`` by an fp32 Cholesky. ``gram`` is G =
    ``ops.gram(fixed_table)`` (computed here when None; pass it when solving
    several CSRs against one table). ``out`` (fp32 [n, d], contiguous) is
    written in place and returned. An empty row is exactly 0; a repeated column
    counts once per occurrence; a row with a non-positive or non-finite pivot
    (negative or non-finite weights) is all NaN. With ``check`` a cols entry
    outside [0, m) raises IndexError after the call (one counter read);
    without it the entry contributes nothing. Widths other than 32 / 64 / 128
    are zero-padded per call, which is exact: the padded coordinates solve to 0.
    Results are bitwise reproducible and independent of the grid."""
    dev = B.require_device(fixed_table, rowptr, cols, weights, gram, out)
    _need(fixed_table.dim() == 2 and fixed_table.dtype == torch.float32,
          "fixed_table must be fp32 2-D")
    _contig(fixed_table, "fixed_table")
    m, d = fixed_table.shape
    _need(d >= 1, "fixed_table must have columns")
    w = _width_of(ALS_WIDTHS, d, "als_solve")
    alpha, reg = float(alpha), float(reg)
    _need(0.0 <= alpha < float("inf"), "alpha must be >= 0 and finite")
    _need(0.0 < reg < float("inf"), "reg must be > 0 and finite")
    rowptr, cols, weights, n = _csr(rowptr, cols, weights)
    if out is not None:
        _need(out.dtype == torch.float32 and out.shape == (n, d) and out.is_contiguous(),
              "out must be a contiguous fp32 [n, d] tensor")
    if gram is None:
        gram = _gram_of(fixed_table)
    _need(gram.dtype == torch.float32 and gram.shape == (d, d), "gram must be fp32 [d, d]")
    if w != d:
        fixed_table = pad_columns(fixed_table, w)
        padded = torch.zeros((w, w), dtype=torch.float32, device=dev)
        padded[:d, :d] = gram
        gram = padded
    gram = gram.contiguous()
    res = out if out is not None and w == d else torch.empty((n, w), dtype=torch.float32, device=dev)
    if n:
        err, own = _counter(dev, check=check)
        rc = B.lib().dr_als_solve(
            fixed_table.data_ptr() if m else None, m, w, gram.data_ptr(), rowptr.data_ptr(),
            cols.data_ptr() if cols.numel() else None, B.ptr(weights) if cols.numel() else None,
            n, alpha, reg, res.data_ptr(), B.ptr(err), B.stream(dev),
        )
        _done(rc, "dr_als_solve", own)
    if w == d:
        return res
    if out is None:
        return res[:, :d].contiguous()
    out.copy_(res[:, :d])
    return out


def als_objective(
    row_table: torch.Tensor, fixed_table: torch.Tensor, rowptr: torch.Tensor, cols: torch.Tensor,
    weights: Optional[torch.Tensor], alpha: float, reg: float,
) -> float:
    """The implicit-feedback objective ALS descends, as a Python float:
    ``J = sum_r [x_r^T G x_r + sum_{i in r} (c_ri (1 - s_ri)^2 - s_ri^2)]
    + reg (|X|^2 + |Y|^2)`` with X = ``row_table`` [n, d], Y = ``fixed_table``
    [m, d] (both fp32), G = Y^T Y, s_ri = x_r^T y_i (``gather_dot``) and
    c = 1 + alpha * w over the CSR's entries; every sum in float64 on the
    device. Equal to the sum over ALL (r, i) of c (p - s)^2 plus the
    regulariser, without visiting the unobserved pairs."""
    B.require_device(row_table, fixed_table, rowptr, cols, weights)
    _need(row_table.dim() == 2 and fixed_table.dim() == 2 and
          row_table.dtype == torch.float32 and fixed_table.dtype == torch.float32 and
          row_table.size(1) == fixed_table.size(1), "fp32 2-D tables of one width")
    row_table, fixed_table = row_table.contiguous(), fixed_table.contiguous()
    rowptr, cols, weights, n = _csr(rowptr, cols, weights)
    _need(n == row_table.size(0), "one CSR row per row of row_table")
    total = torch.zeros((), dtype=torch.float64, device=row_table.device)
    if cols.numel():
        rows = torch.repeat_interleave(torch.arange(n, device=cols.device), rowptr[1:] - rowptr[:-1])
        s = gather_dot(row_table, fixed_table, rows, cols.to(torch.int64)).to(torch.float64)
        c = 1.0 if weights is None else weights.to(torch.float64)
        c = 1.0 + float(alpha) * c
        total += (c * (1.0 - s) ** 2 - s * s).sum()
    g = _gram64(fixed_table)
    sq = torch.zeros((), dtype=torch.float64, device=row_table.device)
    for r0 in range(0, n, GRAM_CHUNK_ROWS):
        x = row_table[r0:r0 + GRAM_CHUNK_ROWS].to(torch.float64)
        total += ((x @ g) * x).sum()
        sq += (x * x).sum()
    total += float(reg) * (sq + torch.diagonal(g).sum())
    return float(total.item())


# --------------------------------------------------------------------------- CSR row sum
ROW_SUM_CHUNK = 512  # DR_ROW_SUM_CHUNK: entries of a chunk (Appendix-B split rule)
ROW_SUM_MAX_D = 512  # DR_ROW_SUM_MAX_D


class RowSumPlan:
    """What ``csr_row_sum`` needs from a CSR's ``rowptr`` beyond the pointer,
    computed once per CSR (``row_sum_plan``): the checked ``rowptr`` itself,
    the host-side sizes (rows, entries, chunks, long rows) and ``lists``, the
    int64 tensor of dr_csr_row_sum's five plan lists (include/divrec_hip.h;
    a single 0 for a CSR without long rows).
    Keep it as long as the CSR: a call with a plan reads nothing back."""

    __slots__ = ("rowptr", "n_rows", "nnz", "n_chunks", "n_long", "lists")

    def __init__(self, rowptr, n_rows, nnz, n_chunks, n_long, lists):
        self.rowptr, self.n_rows, self.nnz = rowptr, n_rows, nnz
        self.n_chunks, self.n_long, self.lists = n_chunks, n_long, lists


def row_sum_plan(rowptr: torch.Tensor) -> RowSumPlan:
    """The plan of ``csr_row_sum`` for the CSR with this ``rowptr`` (int64
    [n + 1], on any device; torch ops only, so it also runs on the host): the
    rows longer than ``ROW_SUM_CHUNK`` cut into chunks of that many entries.
    ONE read-back: rowptr's checks (it rises from 0) and the two list sizes."""
    _need(rowptr.dtype == torch.int64 and rowptr.dim() == 1 and rowptr.numel() >= 1,
          "rowptr int64 [n + 1]")
    rowptr = rowptr.contiguous()
    n, L, dev = rowptr.numel() - 1, ROW_SUM_CHUNK, rowptr.device
    lens = rowptr[1:] - rowptr[:-1]
    is_long = lens > L
    per_row = torch.where(is_long, (lens + (L - 1)) // L, torch.zeros_like(lens))
    first, nnz, falls, n_long, n_chunks = torch.stack(
        [rowptr[0], rowptr[-1], (lens < 0).sum(), is_long.sum(), per_row.sum()]).tolist()
    _need(first == 0 and falls == 0, "rowptr must rise from 0")
    if n_long == 0:  # nothing to split: the kernel strides over the rows, no lists
        return RowSumPlan(rowptr, n, nnz, 0, 0, torch.zeros(1, dtype=torch.int64, device=dev))
    # long rows first, then the others, each in ascending order, without a
    # second read-back: one stable sort, cut at the count read above
    by_kind = torch.sort(is_long.to(torch.int8), descending=True, stable=True).indices
    long_row, short_row = by_kind[:n_long], by_kind[n_long:]
    per = per_row[long_row]
    long_first = torch.zeros(n_long + 1, dtype=torch.int64, device=dev)
    long_first[1:] = torch.cumsum(per, 0)
    chunk_row = torch.repeat_interleave(long_row, per, output_size=n_chunks)
    slot = torch.arange(n_chunks, dtype=torch.int64, device=dev)
    chunk_k = slot - torch.repeat_interleave(long_first[:-1], per, output_size=n_chunks)
    chunk_beg = rowptr[chunk_row] + chunk_k * L
    chunk_len = torch.clamp(rowptr[chunk_row + 1] - chunk_beg, max=L)
    # every work item (a chunk -> its partial row, a short row -> out), longest first
    item_row = torch.cat([chunk_row, short_row])
    item_beg = torch.cat([chunk_beg, rowptr[short_row]])
    item_slot = torch.cat([slot, torch.full_like(short_row, -1)])
    order = torch.sort(torch.cat([chunk_len, lens[short_row]]), descending=True, stable=True).indices
    lists = torch.cat([item_row[order], item_beg[order], item_slot[order], long_row,
                       long_first]).contiguous()
    return RowSumPlan(rowptr, n, nnz, n_chunks, n_long, lists)


def csr_row_sum(
    table: torch.Tensor, rowptr: torch.Tensor, cols: torch.Tensor,
    weights: Optional[torch.Tensor] = None, plan: Optional[RowSumPlan] = None,
    out_dtype: torch.dtype = torch.float32, err: Optional[torch.Tensor] = None,
    check: bool = True, out: Optional[torch.Tensor] = None,
) -> torch.Tensor:
    """``out[r] = sum_e weights[e] * table[cols[e]]`` over the entries of row r
    of the CSR (rowptr int64 [n + 1], cols int32, ``weights`` fp32 or None = 1)
    over the fp32 ``table`` [m, d], 1 <= d <= 512 (dr_csr_row_sum): fp32 or
    bf16 [n, d] (``out_dtype``; bf16 is the fp32 sum rounded once). No atomics:
    a row is summed in entry order in chunks of ``ROW_SUM_CHUNK`` entries whose
    sums are added in chunk order, so it depends, bitwise, on its own entries
    only. An empty row is exactly 0; a repeated column counts once per
    occurrence. ``out`` (contiguous [n, d] of ``out_dtype``) is written in
    place, every row of it, and returned. ``plan`` = ``row_sum_plan(rowptr)``, made once per CSR and
    passed with the very ``rowptr`` it was made from: the call then reads
    nothing back from the device (with ``check=False`` or a caller's ``err``).
    Without a plan one is made here (one read-back). A cols entry outside
    [0, m) adds nothing and is counted: with ``check`` and no ``err`` this call
    reads the count (one sync) and raises IndexError; otherwise the count goes
    to the caller's ``err`` (may be None), read when the caller chooses."""
    dev = B.require_device(table, rowptr, cols, weights, err)
    _need(table.dim() == 2 and table.dtype == torch.float32, "table must be fp32 2-D")
    _contig(table, "table")
    m, d = table.shape
    _need(1 <= d <= ROW_SUM_MAX_D, f"table must have 1 to {ROW_SUM_MAX_D} columns")
    _need(out_dtype in (torch.float32, torch.bfloat16), "out_dtype must be fp32 or bf16")
    _need(cols.dtype == torch.int32 and cols.dim() == 1, "cols must be int32 1-D")
    if weights is not None:
        _need(weights.dtype == torch.float32 and weights.shape == cols.shape,
              "weights must be fp32, one per entry of cols")
        weights = weights.contiguous()
    cols = cols.contiguous()
    if plan is None:
        plan = row_sum_plan(rowptr)
    else:
        _need(isinstance(plan, RowSumPlan) and rowptr.dtype == torch.int64
              and rowptr.data_ptr() == plan.rowptr.data_ptr()
              and rowptr.numel() == plan.n_rows + 1,
              "plan must be row_sum_plan(rowptr) of this very rowptr tensor")
    _need(plan.nnz == cols.numel(), "rowptr must rise from 0 to the number of entries of cols")
    _need(plan.lists.device == dev, "plan and tensors on different devices")
    n = plan.n_rows
    if out is None:
        out = torch.empty((n, d), dtype=out_dtype, device=dev)
    else:
        _need(out.dtype == out_dtype and out.shape == (n, d) and out.is_contiguous()
              and out.device == dev, "out must be a contiguous [n, d] tensor of out_dtype")
    if n == 0:
        return out
    ws = torch.empty((plan.n_chunks, d), dtype=torch.float32, device=dev) if plan.n_chunks else None
    err, own = _counter(dev, err, check)
    rc = B.lib().dr_csr_row_sum(
        table.data_ptr() if m else None, m, d, plan.rowptr.data_ptr(),
        cols.data_ptr() if cols.numel() else None, B.ptr(weights) if cols.numel() else None, n,
        plan.lists.data_ptr(), plan.n_chunks, plan.n_long, out.data_ptr(), B.dtype_code(out_dtype),
        B.ptr(ws), ws.numel() * 4 if ws is not None else 0, B.ptr(err), B.stream(dev),
    )
    _done(rc, "dr_csr_row_sum", own)
    return out


def csr_transpose(rowptr: torch.Tensor, cols: torch.Tensor, weights: Optional[torch.Tensor],
                  n_cols: int) -> Tuple[torch.Tensor, torch.Tensor, Optional[torch.Tensor]]:
    """(rowptr_t int64 [n_cols + 1], cols_t int32, weights_t) of the transposed
    CSR, on the same device (torch ops; the host works too). The entries are
    ordered by a STABLE sort by column, so transposed row c lists its source
    rows in ascending order (a repeated entry in its original order): the
    fixed order ``csr_row_sum``'s reproducibility rests on. Every column must
    lie in [0, n_cols) (ValueError; one read-back, once per CSR)."""
    _need(rowptr.dtype == torch.int64 and rowptr.dim() == 1 and rowptr.numel() >= 1,
          "rowptr int64 [n + 1]")
    _need(cols.dtype == torch.int32 and cols.dim() == 1, "cols must be int32 1-D")
    if weights is not None:
        _need(weights.shape == cols.shape, "weights: one per entry of cols")
    n, nnz, n_cols, dev = rowptr.numel() - 1, cols.numel(), int(n_cols), cols.device
    _need(n_cols >= 0, "n_cols must be >= 0")
    lens = rowptr[1:] - rowptr[:-1]
    checks = [rowptr[0], rowptr[-1], (lens < 0).sum()]
    if nnz:
        checks += [cols.min().to(torch.int64), cols.max().to(torch.int64)]
    got = torch.stack(checks).tolist()
    _need(got[0] == 0 and got[1] == nnz and got[2] == 0,
          "rowptr must rise from 0 to the number of entries of cols")
    _need(not nnz or (got[3] >= 0 and got[4] < n_cols), "cols must lie in [0, n_cols)")
    rows = torch.repeat_interleave(torch.arange(n, dtype=torch.int64, device=dev), lens,
                                   output_size=nnz)
    order = torch.sort(cols, stable=True).indices
    counts = torch.bincount(cols.to(torch.int64), minlength=n_cols)
    rowptr_t = torch.zeros(n_cols + 1, dtype=torch.int64, device=dev)
    rowptr_t[1:] = torch.cumsum(counts, 0)
    return (rowptr_t, rows[order].to(torch.int32).contiguous(),
            None if weights is None else weights[order].contiguous())


class CsrMap:
    """A row -> table-row map kept for a model's lifetime: the CSR (rowptr
    int64 [n_rows + 1], cols int32, ``weights`` fp32 or None) over a table of
    ``n_cols`` rows, its ``row_sum_plan`` and, made on first use and kept, the
    transposed map ``.T`` with its own plan, which ``feature_sum``'s backward
    sums over. Built from tensors on any device; ``to(device)`` moves it."""

    def __init__(self, rowptr: torch.Tensor, cols: torch.Tensor,
                 weights: Optional[torch.Tensor], n_cols: int, _transposed: "CsrMap" = None):
        if weights is not None:
            _need(weights.dtype == torch.float32, "weights must be fp32")
        self.plan = row_sum_plan(rowptr)
        self.rowptr, self.cols = self.plan.rowptr, cols.contiguous()
        self.weights = None if weights is None else weights.contiguous()
        self.n_rows, self.n_cols = self.plan.n_rows, int(n_cols)
        _need(self.cols.dtype == torch.int32 and self.cols.dim() == 1
              and self.cols.numel() == self.plan.nnz,
              "cols must be int32 1-D, rowptr[-1] of them")
        _need(self.weights is None or self.weights.shape == self.cols.shape,
              "weights: one per entry of cols")
        self._t = _transposed

    @property
    def T(self) -> "CsrMap":
        if self._t is None:
            rt, ct, wt = csr_transpose(self.rowptr, self.cols, self.weights, self.n_cols)
            self._t = CsrMap(rt, ct, wt, self.n_rows, _transposed=self)
        return self._t

    def to(self, device) -> "CsrMap":
        device = torch.device(device)
        if self.rowptr.device == device:
            return self
        return CsrMap(self.rowptr.to(device), self.cols.to(device),
                      None if self.weights is None else self.weights.to(device), self.n_cols)

    def sum(self, table: torch.Tensor, out_dtype: torch.dtype = torch.float32,
            err: Optional[torch.Tensor] = None, check: bool = True) -> torch.Tensor:
        """``csr_row_sum`` of ``table`` [n_cols, d] over this map, with its plan."""
        _need(table.dim() == 2 and table.size(0) == self.n_cols,
              f"table must have the map's {self.n_cols} rows")
        return csr_row_sum(table, self.rowptr, self.cols, self.weights, plan=self.plan,
                           out_dtype=out_dtype, err=err, check=check)


class _FeatureSum(torch.autograd.Function):
    @staticmethod
    def forward(ctx, table, csr_map, checked):
        ctx.csr_map = csr_map
        return csr_map.sum(table, check=not checked)

    @staticmethod
    def backward(ctx, grad_out):
        # d out[r] / d table[c] = sum of the weights of (r, c): the same sum
        # over the transposed map; its columns are row numbers, valid by construction
        grad = ctx.csr_map.T.sum(grad_out.to(torch.float32).contiguous(), check=False)
        return grad, None, None


def feature_sum(table: torch.Tensor, csr_map: CsrMap, checked: bool = False) -> torch.Tensor:
    """``csr_map.sum(table)`` (fp32), differentiable in ``table`` only: the
    backward is the same kernel over the transposed map, no atomics, bitwise
    reproducible. ``checked``: the map's columns are known to lie in the table
    (no read-back of the range counter)."""
    return _FeatureSum.apply(table, csr_map, checked)
