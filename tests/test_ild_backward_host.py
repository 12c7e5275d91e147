"""Embedding-ILD gradient, host side: the dr_ild_embedding_backward ABI and its
argument checks (they run before any HIP call), the differentiable
EmbeddingDistance's own checks, and the float64 autograd reference of
tests/ild_grad_checks.py against the header's closed forms. No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import oracle
from divrec import _backend, ops, train
from divrec.losses import EmbeddingDistance
from ild_grad_checks import KINDS, closed_form_grad_f64, ild_f64, ild_grad_f64

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include",
                      "divrec_hip.h")
I32, I64 = _backend.DR_I32, _backend.DR_I64


def test_symbol_is_declared_bound_and_exported():
    text = open(HEADER).read()
    assert re.search(r"^int dr_ild_embedding_backward\(", text, re.M)
    res, args = _backend.SIGNATURES["dr_ild_embedding_backward"]
    assert res is ctypes.c_int and len(args) == 13
    assert args[9] is ctypes.c_float and args[2] is ctypes.c_int64  # scale, n_users
    assert hasattr(_backend.load_library(), "dr_ild_embedding_backward")
    assert callable(ops.ild_embedding_backward)
    assert callable(train.diversity_pair_wise_train_loop)


def test_argument_errors_without_gpu():
    lib = _backend.load_library()
    one = ctypes.c_void_p(8)  # a non-NULL pointer the checks never dereference

    def call(recs=one, rec_dtype=I64, n_users=5, k=10, table=one, n_items=50, d=64, kind=0,
             grad=one):
        return lib.dr_ild_embedding_backward(recs, rec_dtype, n_users, k, table, n_items, d, kind,
                                             None, 1.0, grad, None, None)

    for k in (0, 129, -1):
        assert call(k=k) == -1 and b"k must be in [1, 128]" in lib.dr_last_error()
    for d in (0, 257):
        assert call(d=d) == -1 and b"d must be in [1, 256]" in lib.dr_last_error()
    for kind in (3, -1):
        assert call(kind=kind) == -1 and b"unknown distance kind" in lib.dr_last_error()
    for dt in (_backend.DR_F32, _backend.DR_BF16, 7):
        assert call(rec_dtype=dt) == -1 and b"rec_dtype" in lib.dr_last_error()
    for null in ("table", "recs", "grad"):
        assert call(**{null: None}) == -1 and b"null pointer" in lib.dr_last_error()
    # no lists: a no-op success, whatever the pointers; bad k / d / kind still refused
    assert call(n_users=0) == 0
    assert call(n_users=0, recs=None, table=None, grad=None, rec_dtype=I32) == 0
    assert call(n_users=0, k=129) == -1


def test_differentiable_distance_rejects_what_the_kernel_cannot_take():
    with pytest.raises(ValueError, match="fp32"):
        EmbeddingDistance(torch.zeros(10, 32, dtype=torch.bfloat16), "cosine", differentiable=True)
    with pytest.raises(ValueError, match="fp32"):
        EmbeddingDistance(torch.zeros(10, 32, dtype=torch.float64), "dot", differentiable=True)
    with pytest.raises(ValueError, match="256"):
        EmbeddingDistance(torch.zeros(10, 257), "euclidean", differentiable=True)
    # the default is the metric as it was: any float table, any width, no flag set
    D = EmbeddingDistance(torch.zeros(10, 300, dtype=torch.float64), "cosine")
    assert D.differentiable is False


@pytest.mark.parametrize("kind", KINDS)
def test_autograd_reference_equals_the_closed_forms(kind):
    """k = 10, d = 100, position 1 repeating position 0 (a zero distance, two
    positions of one row), a zero row in some lists (cosine's mask) and a
    random grad_out: float64 autograd of the dense pair formula against the
    header's closed forms, to 1e-12 of the largest entry."""
    rng = np.random.default_rng(5)
    table = rng.standard_normal((60, 100))
    table[7] = 0.0
    recs = np.stack([rng.permutation(60)[:10] for _ in range(12)])
    recs[:, 1] = recs[:, 0]
    recs[::3, 4] = 7
    go = rng.standard_normal(12)
    auto = ild_grad_f64(table, recs, kind, go, scale=0.7)
    closed = closed_form_grad_f64(table, recs, kind, go, scale=0.7)
    assert np.isfinite(auto).all() and np.abs(auto).max() > 0
    assert np.abs(auto - closed).max() <= 1e-12 * np.abs(closed).max()
    if kind == "cosine":
        assert not auto[7].any()  # the zero row gets no gradient


@pytest.mark.parametrize("kind", KINDS)
def test_reference_value_is_the_oracles_ild(kind):
    """The formula that is differentiated is the one oracle.ild_embedding_f64 evaluates."""
    rng = np.random.default_rng(6)
    table = rng.standard_normal((40, 24))
    recs = np.stack([rng.permutation(40)[:9] for _ in range(5)])
    got = ild_f64(torch.from_numpy(table)[torch.from_numpy(recs)], kind).numpy()
    assert np.allclose(got, oracle.ild_embedding_f64(recs, table, kind), rtol=1e-12, atol=1e-14)


def test_reference_skips_lists_with_bad_ids():
    rng = np.random.default_rng(8)
    table = rng.standard_normal((20, 8))
    recs = np.stack([rng.permutation(20)[:5] for _ in range(4)])
    bad = recs.copy()
    bad[1, 2], bad[3, 0] = 20, -1
    assert np.array_equal(ild_grad_f64(table, bad, "dot"), ild_grad_f64(table, recs[[0, 2]], "dot"))
