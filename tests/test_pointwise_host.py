"""Point-wise MSE path, host side: the dr_mse_fwd_bwd ABI and its argument
checks (they run before any HIP call), the float64 restatement of the step
against the reference's ``mse_step`` fixture, and DevicePointWiseDataset's
batching on the CPU. No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from divrec import _backend, datasets, ops
from pointwise_checks import load, loop_data, mse_step_f64

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include",
                      "divrec_hip.h")


def test_mse_symbol_is_declared_bound_and_exported():
    text = open(HEADER).read()
    assert re.search(r"^int dr_mse_fwd_bwd\(", text, re.M)
    res, args = _backend.SIGNATURES["dr_mse_fwd_bwd"]
    assert res is ctypes.c_int and len(args) == 16
    assert args[9] is ctypes.c_float and args[8] is ctypes.c_int64  # grad_scale, batch
    assert hasattr(_backend.load_library(), "dr_mse_fwd_bwd")
    assert callable(ops.mse_fwd_bwd)


def test_mse_argument_errors_without_gpu():
    lib = _backend.load_library()
    one = ctypes.c_void_p(8)  # a non-NULL pointer the checks never dereference

    def call(ut=one, nu=10, it=one, ni=10, d=64, uid=one, iid=one, tgt=one, batch=3):
        return lib.dr_mse_fwd_bwd(ut, nu, it, ni, d, uid, iid, tgt, batch, 1.0, None, None, None,
                                  None, None, None)

    assert call(batch=0) == 0  # empty batch: a no-op success ...
    assert call(ut=None, it=None, uid=None, iid=None, tgt=None, batch=0) == 0  # ... whatever else
    for bad in (dict(batch=-1), dict(nu=-1), dict(ni=-1)):
        assert call(**bad) == -1 and b"sizes" in lib.dr_last_error()
    for d in (0, 513, -4):
        assert call(d=d) == -1 and b"d must be in [1, 512]" in lib.dr_last_error()
    for null in ("ut", "it", "uid", "iid", "tgt"):
        assert call(**{null: None}) == -1 and b"null pointer" in lib.dr_last_error()


def test_restatement_reproduces_the_reference_step():
    """mse_step_f64 against what the reference's MatrixFactorization forward,
    MSELoss() and autograd gave (fp32): forward and loss within fp32 rounding
    of a 16-term dot product, gradients at the golden step's tolerances."""
    g = load("mse_step")
    B = g["uid"].size
    pred, loss, gU, gI = mse_step_f64(g["U0"], g["I0"], g["uid"], g["iid"], g["target"], 1.0 / B)
    assert np.allclose(pred, g["pred"], rtol=1e-5, atol=1e-6)
    assert loss.sum() / B == pytest.approx(float(g["loss"]), rel=1e-6)
    assert np.allclose(gU, g["gU"], rtol=1e-5, atol=1e-8)
    assert np.allclose(gI, g["gI"], rtol=1e-5, atol=1e-8)
    # rows no pair touched have exactly zero gradient in both
    assert not gU[np.setdiff1d(np.arange(30), g["uid"])].any()


def test_restatement_skips_bad_ids():
    U, I = np.ones((3, 4), np.float32), np.ones((5, 4), np.float32)
    pred, loss, gU, gI = mse_step_f64(U, I, [0, -1, 2, 1], [4, 0, 5, 1], [1, 1, 1, 1], 1.0)
    assert np.isnan(pred[[1, 2]]).all() and np.isnan(loss[[1, 2]]).all()
    assert np.array_equal(pred[[0, 3]], [4.0, 4.0]) and np.array_equal(loss[[0, 3]], [9.0, 9.0])
    assert np.array_equal(gU[:, 0], [6.0, 6.0, 0.0])


# --------------------------------------------------------------------------- DevicePointWiseDataset
def _rows(batches):
    """Batches -> (user ids, item ids, targets) concatenated, plus batch sizes."""
    batches = list(batches)
    cat = [torch.cat([b[k] for b in batches]) for k in (0, 1, 4)]
    return cat, [b[0].numel() for b in batches]


@pytest.mark.parametrize("drop_last", [False, True])
@pytest.mark.parametrize("batch_size", [1, 64, 150, 200])
def test_device_dataset_equals_pointwise_loader(batch_size, drop_last):
    data = loop_data(load("mse_loop"))
    ref = list(datasets.PointWiseDataset(data).loader(batch_size=batch_size, drop_last=drop_last))
    ds = datasets.DevicePointWiseDataset(data, device="cpu")
    got = list(ds.loader(batch_size=batch_size, drop_last=drop_last))
    assert len(ds) == 150 and len(got) == len(ref)
    for (u, i, uf, itf, t), (ru, ri, _, _, rt) in zip(got, ref):
        assert uf is None and itf is None
        assert u.dtype == torch.int64 and i.dtype == torch.int64 and t.dtype == rt.dtype
        assert torch.equal(u, ru) and torch.equal(i, ri) and torch.equal(t, rt)


def test_device_dataset_targets():
    g = load("mse_loop")
    data = loop_data(g, torch.float64)
    (u, i, t), _ = _rows(datasets.DevicePointWiseDataset(data, device="cpu").loader(batch_size=64))
    assert t.dtype == torch.float64  # the scores' own dtype
    assert np.array_equal(t.numpy(), g["scores"][g["interactions"][:, 1]])  # by item id
    (u, i, t), sizes = _rows(datasets.DevicePointWiseDataset(data, device="cpu", by_row=True)
                             .loader(batch_size=64))
    assert sizes == [64, 64, 22]
    assert np.array_equal(t.numpy(), g["scores"])  # by row: the interactions' own scores
    assert np.array_equal(torch.stack([u, i], 1).numpy(), g["interactions"])


def test_device_dataset_item_id_beyond_scores_raises():
    """PointWiseDataset raises IndexError at the row whose item id is not an
    index of interaction_scores; the device data set raises when it is built."""
    data = datasets.UserItemInteractionsDataset(torch.tensor([[0, 1], [1, 7]]))
    with pytest.raises(IndexError):
        datasets.PointWiseDataset(data)[1]
    with pytest.raises(IndexError):
        datasets.DevicePointWiseDataset(data, device="cpu")
    assert len(datasets.DevicePointWiseDataset(data, device="cpu", by_row=True)) == 2


def test_device_dataset_shuffle():
    g = load("mse_loop")
    data = loop_data(g)
    key = lambda u, i, t: (u * 40 + i) * 8 + t.long()  # one sortable key per row
    ds = datasets.DevicePointWiseDataset(data, device="cpu", seed=5)
    plain, _ = _rows(ds.loader(batch_size=64))
    e0, sizes = _rows(ds.loader(batch_size=64, shuffle=True))
    e1, _ = _rows(ds.loader(batch_size=64, shuffle=True))
    assert sizes == [64, 64, 22]
    for epoch in (e0, e1):  # a permutation of all rows, each with its own target
        assert torch.equal(torch.sort(key(*epoch)).values, torch.sort(key(*plain)).values)
    assert not torch.equal(key(*e0), key(*plain))
    assert not torch.equal(key(*e0), key(*e1))  # a new order every epoch
    twin = datasets.DevicePointWiseDataset(data, device="cpu", seed=5)
    for epoch in (e0, e1):  # same seed: the same epochs
        again, _ = _rows(twin.loader(batch_size=64, shuffle=True))
        assert all(torch.equal(a, b) for a, b in zip(again, epoch))
    other, _ = _rows(datasets.DevicePointWiseDataset(data, device="cpu", seed=6)
                     .loader(batch_size=64, shuffle=True))
    assert not torch.equal(key(*other), key(*e0))
