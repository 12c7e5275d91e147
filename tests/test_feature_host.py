"""Feature-composed factorization without a GPU: the numpy restatements of
tests/feature_checks.py against each other (the tolerance rule is satisfiable
before the kernel is judged by it), csr_transpose / row_sum_plan / feature_csr
on CPU tensors against the numpy builders, dr_csr_row_sum's argument checks,
and the value errors of the model and loop doors, which come before any
device use."""
import ctypes

import numpy as np
import pytest
import torch

import feature_checks as fc
from divrec import _backend, datasets, losses, models, ops, train
from divrec.datasets import feature_csr
from divrec.models import FeatureMatrixFactorization


def t_csr(rowptr, cols, weights):
    return (torch.from_numpy(rowptr), torch.from_numpy(cols),
            None if weights is None else torch.from_numpy(weights))


# --------------------------------------------------------------------------- restatements
def test_chunk_length_is_the_librarys():
    assert ops.ROW_SUM_CHUNK == fc.L == _backend.load_library().dr_csr_row_sum_chunk()


@pytest.mark.parametrize("n_rows", fc.ROW_COUNTS)
@pytest.mark.parametrize("d", fc.WIDTHS)
def test_f32_restatement_is_inside_the_bound(d, n_rows):
    """The rule admits a correct fp32 sum in the kernel's order on every GPU
    case, fp32 and bf16 output alike, and rejects a sum that drops one entry."""
    T, rowptr, cols, w = fc.case(d, n_rows)
    ref = fc.case_ref(d, n_rows)
    out32 = fc.row_sum_f32_sequential(T, rowptr, cols, w)
    fc.check_row_sum(out32, ref, what=f"f32 restatement d={d}")
    bf16 = torch.from_numpy(out32).to(torch.bfloat16).to(torch.float64).numpy()
    fc.check_row_sum(bf16, ref, bf16=True, what=f"f32 restatement, bf16 d={d}")
    lens = np.diff(rowptr)
    r = int(np.argmax(lens))
    e = int(rowptr[r]) + int(lens[r]) - 1  # the long row's last entry, weight made non-zero
    w2 = np.ones(len(cols), fc.F) if w is None else w.copy()
    w2[e] = 1.5
    full = fc.row_sum_f64(T, rowptr, cols, w2)
    w2[e] = 0.0
    with pytest.raises(AssertionError):
        fc.check_row_sum(fc.row_sum_f32_sequential(T, rowptr, cols, w2), full, what="dropped entry")


@pytest.mark.parametrize("d,n_rows", [(8, 7), (128, 4097)])
def test_integer_cases_are_exact_in_fp32(d, n_rows):
    """On the integer-valued cases every partial sum is an integer below 2^24:
    the fp32 restatement equals the float64 reference bit for bit, so the GPU
    test may ask the kernel for the same."""
    T, rowptr, cols, w = fc.case(d, n_rows, integer=True)
    out64, mag, _ = fc.case_ref(d, n_rows, integer=True)
    assert mag.max() < 2 ** 24
    assert np.array_equal(fc.row_sum_f32_sequential(T, rowptr, cols, w), out64.astype(fc.F))


def test_case_generator_covers_the_lengths_and_edges():
    seen, nulls = set(), set()
    for d in fc.WIDTHS:
        for n in fc.ROW_COUNTS:
            T, rowptr, cols, w = fc.case(d, n)
            lens = np.diff(rowptr)
            seen |= set(lens.tolist())
            nulls.add(w is None)
            if n > 1:
                assert lens[-1] == 3 * fc.L + 5  # a long row LAST
                assert any(cols[rowptr[r]] == cols[rowptr[r] + 1] for r in range(n) if lens[r] >= 2)
            if w is not None and n > 1:
                assert (w == 0).any()
    assert set(fc.SPECIAL) <= seen and nulls == {True, False}


# --------------------------------------------------------------------------- transpose, plan
def test_csr_transpose_matches_the_numpy_builder():
    rng = np.random.default_rng(0)
    rows = [rng.integers(0, 9, n) for n in (3, 0, 5, 1, 0, 7)]
    rows[2][1] = rows[2][0]  # a repeat
    w = [rng.uniform(-1, 1, len(r)).astype(fc.F) for r in rows]
    for weights in (w, None):
        rowptr, cols, wt = fc.csr(rows, weights)
        want = fc.transpose(rowptr, cols, wt, 11)  # columns 9 and 10: empty transposed rows
        got = ops.csr_transpose(*t_csr(rowptr, cols, wt), 11)
        assert got[0].dtype == torch.int64 and got[1].dtype == torch.int32
        assert np.array_equal(got[0].numpy(), want[0]) and np.array_equal(got[1].numpy(), want[1])
        assert (got[2] is None) == (weights is None)
        if weights is not None:
            assert np.array_equal(got[2].numpy(), want[2])
        # each transposed row lists its source rows ascending
        for c in range(11):
            assert np.all(np.diff(got[1].numpy()[want[0][c]:want[0][c + 1]]) >= 0)
        S = fc.dense(rowptr, cols, wt, 11)
        assert np.allclose(fc.dense(want[0], want[1], want[2], 6), S.T)
    with pytest.raises(ValueError, match="n_cols"):
        ops.csr_transpose(*t_csr(rowptr, cols, wt), 5)
    with pytest.raises(ValueError, match="rowptr"):
        ops.csr_transpose(torch.tensor([0, 2, 1]), torch.zeros(1, dtype=torch.int32), None, 3)


def test_row_sum_plan_lists_exactly_the_long_rows():
    L = ops.ROW_SUM_CHUNK
    lens = [0, 1, L - 1, L, L + 1, 3 * L + 5, 2, 2 * L, 7 * L + 1]
    rowptr = torch.zeros(len(lens) + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(torch.tensor(lens), 0)
    plan = ops.row_sum_plan(rowptr)
    assert (plan.n_rows, plan.nnz, plan.n_long, plan.n_chunks) == (9, sum(lens), 4, 2 + 4 + 2 + 8)
    n_items = 9 - 4 + 16
    item_row, item_beg, item_slot, long_row, long_first = torch.split(
        plan.lists, [n_items, n_items, n_items, plan.n_long, plan.n_long + 1])
    assert long_row.tolist() == [4, 5, 7, 8]
    assert long_first.tolist() == [0, 2, 6, 8, 16]
    # every entry of the CSR is covered once: chunks by their partial row, short rows whole
    item_len = torch.minimum(rowptr[item_row + 1] - item_beg, torch.tensor(L))
    assert (item_len[:-1] >= item_len[1:]).all()  # longest first
    covered = torch.zeros(sum(lens), dtype=torch.int64)
    for b, n in zip(item_beg.tolist(), item_len.tolist()):
        covered[b:b + n] += 1
    assert (covered == 1).all()
    chunks = item_slot >= 0
    assert sorted(item_slot[chunks].tolist()) == list(range(16))
    by_slot = torch.argsort(item_slot[chunks])
    assert item_row[chunks][by_slot].tolist() == [4] * 2 + [5] * 4 + [7] * 2 + [8] * 8
    k = (item_beg[chunks] - rowptr[item_row[chunks]])[by_slot] // L
    assert k.tolist() == [0, 1, 0, 1, 2, 3, 0, 1] + list(range(8))
    assert sorted(item_row[~chunks].tolist()) == [0, 1, 2, 3, 6]
    empty = ops.row_sum_plan(torch.tensor([0, 3, 3]))
    assert (empty.n_long, empty.n_chunks, empty.lists.tolist()) == (0, 0, [0])
    with pytest.raises(ValueError, match="rise from 0"):
        ops.row_sum_plan(torch.tensor([0, 5, 3]))
    with pytest.raises(ValueError, match="rise from 0"):
        ops.row_sum_plan(torch.tensor([1, 5]))


# --------------------------------------------------------------------------- feature_csr
def _features(n=9, seed=4):
    rng = np.random.default_rng(seed)
    genre = rng.integers(0, 4, n).astype(np.float32) * 3  # values 0, 3, 6, 9: a sparse vocabulary
    genre[2] = -1.0                                       # missing
    decade = rng.integers(0, 3, n).astype(np.float32)
    price = rng.uniform(-1, 1, n).astype(np.float32)
    table = torch.from_numpy(np.stack([genre, decade, price], 1))
    return datasets.Features(table, ["genre", "decade", "price"]), (genre, decade, price)


def test_feature_csr_matches_the_numpy_builder():
    feats, (genre, decade, price) = _features()
    got = feature_csr(feats, categorical=("genre", "decade"), numeric=("price",))
    want = fc.feature_csr_np(9, [genre, decade], [price])
    assert got.rowptr.dtype == torch.int64 and got.cols.dtype == torch.int32
    assert got.weights.dtype == torch.float32
    assert np.array_equal(got.rowptr.numpy(), want[0]) and np.array_equal(got.cols.numpy(), want[1])
    assert np.array_equal(got.weights.numpy(), want[2]) and got.n_features == want[3]
    # row 2's genre is missing: identity, decade, price only
    assert int(got.rowptr[3] - got.rowptr[2]) == 3
    assert got.n_features == 9 + len(set(genre[genre >= 0])) + len(set(decade)) + 1
    no_id = feature_csr(feats, categorical=("genre",), identity=False)
    want = fc.feature_csr_np(9, [genre], identity=False)
    assert np.array_equal(no_id.cols.numpy(), want[1]) and no_id.n_features == want[3]
    with pytest.raises(ValueError, match="no feature column"):
        feature_csr(feats, categorical=("colour",))
    with pytest.raises(ValueError, match="Features table"):
        feature_csr(4, numeric=("price",))


def test_feature_csr_maps_new_rows_through_saved_offsets():
    feats, (genre, decade, price) = _features()
    first = feature_csr(feats, categorical=("genre", "decade"), numeric=("price",))
    _, _, _, _, vocab = fc.feature_csr_np(9, [genre, decade], [price])
    new_genre = np.asarray([3.0, 12.0, 0.0, -1.0], np.float32)  # 12 was never seen
    new_decade = np.asarray([1.0, 2.0, 7.0, 0.0], np.float32)   # nor decade 7
    new_price = np.asarray([0.5, -0.25, 0.0, 2.0], np.float32)
    new = datasets.Features(torch.from_numpy(np.stack([new_genre, new_decade, new_price], 1)),
                            ["genre", "decade", "price"])
    got = feature_csr(new, offsets=first.offsets)
    want = fc.feature_csr_np(4, [new_genre, new_decade], [new_price], vocab=vocab)
    assert got.n_features == first.n_features == want[3]
    assert np.array_equal(got.rowptr.numpy(), want[0]) and np.array_equal(got.cols.numpy(), want[1])
    assert np.array_equal(got.weights.numpy(), want[2])
    assert np.diff(got.rowptr.numpy()).tolist() == [3, 2, 2, 2]  # no identity entry, unknowns dropped
    assert int(got.cols.min()) >= 9  # nothing lands in the old rows' private features
    # a known value maps to the id the first call gave it
    r = int(np.nonzero(genre == 3.0)[0][0])
    assert int(got.cols[0]) == int(first.cols[first.rowptr[r] + 1])


def test_identity_alone_is_the_identity():
    m = feature_csr(6)
    assert m.rowptr.tolist() == list(range(7)) and m.cols.tolist() == list(range(6))
    assert m.weights.tolist() == [1.0] * 6 and m.n_features == 6
    feats, _ = _features()
    same = feature_csr(feats)
    assert same.cols.tolist() == list(range(9)) and same.n_features == 9
    none = feature_csr(3, identity=False)
    assert none.rowptr.tolist() == [0, 0, 0, 0] and none.n_features == 0


# --------------------------------------------------------------------------- argument checks
def test_csr_row_sum_argument_errors_without_gpu():
    lib = _backend.load_library()
    f32, bf16, one = _backend.DR_F32, _backend.DR_BF16, ctypes.c_void_p(64)

    def call(d=128, n_table=10, n_rows=4, n_chunks=0, n_long=0, out_dtype=f32, table=one,
             rowptr=one, out=one, plan=None, ws=None, ws_bytes=0):
        return lib.dr_csr_row_sum(table, n_table, d, rowptr, one, None, n_rows, plan, n_chunks,
                                  n_long, out, out_dtype, ws, ws_bytes, None, None)

    for d in (0, 513, -4):
        assert call(d=d) == -1 and b"d must be in [1, 512]" in lib.dr_last_error()
    assert call(n_rows=-1) == -1 and b"n_rows" in lib.dr_last_error()
    assert call(n_table=-1) == -1 and b"n_table_rows" in lib.dr_last_error()
    assert call(n_chunks=-1) == -1 and b"n_long" in lib.dr_last_error()
    assert call(n_chunks=1, n_long=2, plan=one, ws=one, ws_bytes=512) == -1
    assert call(out_dtype=_backend.DR_I32) == -1 and b"DR_F32 or DR_BF16" in lib.dr_last_error()
    for kw in (dict(table=None), dict(rowptr=None), dict(out=None)):
        assert call(**kw) == -1 and b"null pointer" in lib.dr_last_error()
    assert call(n_chunks=2, n_long=1) == -1 and b"null pointer" in lib.dr_last_error()
    assert call(n_chunks=2, n_long=1, plan=one, ws=one, ws_bytes=2 * 128 * 4 - 1) == -1
    assert b"workspace" in lib.dr_last_error()
    # no rows: a no-op success, whatever the pointers; bf16 output is a valid request
    assert call(n_rows=0, table=None, rowptr=None, out=None) == 0
    assert call(n_rows=0, out_dtype=bf16) == 0
    assert lib.dr_csr_row_sum_workspace(3, 100) == 3 * 100 * 4
    assert lib.dr_csr_row_sum_workspace(0, 100) == 0 == lib.dr_csr_row_sum_workspace(3, 513)


def test_ops_row_sum_has_no_cpu_path():
    T, rowptr, cols, w = fc.case(8, 7)
    with pytest.raises(RuntimeError, match="ROCm"):
        ops.csr_row_sum(torch.from_numpy(T), *t_csr(rowptr, cols, w))


# --------------------------------------------------------------------------- model and loop doors
def _cpu_model(d=16):
    return FeatureMatrixFactorization(feature_csr(12), feature_csr(20), d)


def test_model_shapes_state_dict_and_value_errors():
    m = _cpu_model()
    assert (m.no_users, m.no_items, m.embedding_dim) == (12, 20, 16)
    assert sorted(m.state_dict()) == ["item_feature_embeddings.weight",
                                      "user_feature_embeddings.weight"]
    assert m.user_feature_embeddings.weight.shape == (12, 16)
    assert m.item_feature_embeddings.weight.dtype == torch.float32
    assert not isinstance(m, models.MatrixFactorization)  # a sibling: no MF fast path takes it
    feats, (genre, _, _) = _features()
    hybrid = FeatureMatrixFactorization(feature_csr(5), feature_csr(feats, categorical=("genre",)), 8)
    assert hybrid.item_feature_embeddings.weight.shape == (9 + len(set(genre[genre >= 0])), 8)
    with pytest.raises(ValueError, match="embedding_dim"):
        FeatureMatrixFactorization(feature_csr(3), feature_csr(3), 513)
    with pytest.raises(ValueError, match="user_map"):
        FeatureMatrixFactorization(None, feature_csr(3), 8)
    bad = feature_csr(3)
    with pytest.raises(ValueError, match="outside"):
        FeatureMatrixFactorization((bad.rowptr, bad.cols, bad.weights, 2), feature_csr(3), 8)
    with pytest.raises(ValueError, match="features"):  # a map over another space
        m._compose(m.item_feature_embeddings.weight, m.item_map, feature_csr(7), "csr")


def test_model_has_no_cpu_path():
    m = _cpu_model()
    ids = torch.zeros(2, dtype=torch.int64)
    for door in (lambda: m(ids, ids), m.compose_users, m.compose_items, lambda: m.score_topk(3),
                 lambda: m.scoring_tables("bf16"), lambda: m.recommend_diverse(2, 4)):
        with pytest.raises(RuntimeError, match="no CPU path"):
            door()
    with pytest.raises(ValueError, match="precision"):
        m.scoring_tables("fp16")
    with pytest.raises(ValueError, match="user_vectors"):
        m.score_topk(3, user_ids=ids, user_vectors=torch.zeros(2, 16))
    with pytest.raises(ValueError, match="method"):
        m.recommend_diverse(2, 4, method="nope")


def test_loop_doors_value_errors_come_before_the_device():
    m = _cpu_model()
    data = datasets.UserItemInteractionsDataset(
        torch.tensor([[0, 1], [2, 3], [1, 5]]), number_of_users=12, number_of_items=20,
        user_features=datasets.Features(torch.zeros(12, 1), ["x"]),
        item_features=datasets.Features(torch.zeros(20, 1), ["x"]))
    pw =datasets.PairWiseDataset(data, max_sampled=2)
    sparse = torch.optim.SparseAdam(list(m.parameters()), lr=1e-2)
    with pytest.raises(ValueError, match="SparseAdam"):
        train.pair_wise_train_loop(pw, m, losses.LogSigmoidDifferenceLoss(), sparse, batch_size=4)
    with pytest.raises(ValueError, match="MatrixFactorization"):
        train.als_train_loop(data, m, 1)
    with pytest.raises(ValueError, match="MatrixFactorization"):
        train.diversity_pair_wise_train_loop(pw, m, losses.LogSigmoidDifferenceLoss(), sparse,
                                             None, 0.1, 5)
    # the fused step itself: a CPU model is refused loudly, not scored on the host
    adam = torch.optim.Adam(m.parameters(), lr=1e-2)
    with pytest.raises(RuntimeError, match="no CPU path"):
        train.pair_wise_train_loop(pw, m, losses.LogSigmoidDifferenceLoss(), adam, batch_size=4)
    ranking = datasets.RankingDataset(data)
    with pytest.raises(RuntimeError, match="no CPU path"):
        train.get_model_recommendations(ranking, m, 3)


# --------------------------------------------------------------------------- training, float64
def test_f64_training_descends_on_the_planted_data():
    """Three epochs of the float64 step (compose -> BPR -> transposed sum ->
    Adam) over genre features lower the epoch-mean loss each time: the GPU
    descent test asks the same of the kernels."""
    pairs, genre = fc.planted()
    rng = np.random.default_rng(0)
    users = fc.feature_csr_np(200)
    items = fc.feature_csr_np(300, [genre])
    Su, Si = fc.dense(*users[:3], users[3]), fc.dense(*items[:3], items[3])
    assert Si.shape == (300, 300 + 12)
    Wu = rng.standard_normal((users[3], 32)) * 0.1
    Wi = rng.standard_normal((items[3], 32)) * 0.1
    hist = fc.train_f64(Wu, Wi, Su, Si, fc.planted_triples(pairs, 300), 3, 1024, 0.05)
    print("float64 epoch-mean BPR losses:", hist)
    assert hist[0] > hist[1] > hist[2]
