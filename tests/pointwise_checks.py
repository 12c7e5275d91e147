"""Helpers of the point-wise (MSE) tests: the fixtures' loader and a float64
numpy restatement of dr_mse_fwd_bwd (include/divrec_hip.h), pinned to the
reference by tests/test_pointwise_host.py against the ``mse_step`` fixture."""
import os

import numpy as np
import torch

from divrec import datasets

GOLD = os.path.join(os.path.dirname(__file__), "golden")


def load(name):
    return np.load(os.path.join(GOLD, f"{name}.npz"), allow_pickle=False)


def mse_step_f64(U, I, uid, iid, target, grad_scale):
    """(pred, loss, grad_user, grad_item) in float64. A pair with an id outside
    its table gets pred / loss NaN and adds nothing."""
    U, I = np.asarray(U, np.float64), np.asarray(I, np.float64)
    uid, iid = np.asarray(uid, np.int64), np.asarray(iid, np.int64)
    target = np.asarray(target, np.float64)
    ok = (uid >= 0) & (uid < U.shape[0]) & (iid >= 0) & (iid < I.shape[0])
    u, i = uid[ok], iid[ok]
    pred = np.full(uid.shape, np.nan)
    loss = np.full(uid.shape, np.nan)
    pred[ok] = np.sum(U[u] * I[i], axis=1)
    e = target[ok] - pred[ok]
    loss[ok] = e * e
    g = (-2.0 * e * grad_scale)[:, None]
    gU, gI = np.zeros_like(U), np.zeros_like(I)
    np.add.at(gU, u, g * I[i])
    np.add.at(gI, i, g * U[u])
    return pred, loss, gU, gI


def loop_data(g, score_dtype=torch.float32):
    """The ``mse_loop`` fixture's data set (zero one-column feature tables:
    a DataLoader cannot collate None features)."""
    return datasets.UserItemInteractionsDataset(
        torch.from_numpy(g["interactions"]), torch.from_numpy(g["scores"]).to(score_dtype),
        user_features=datasets.Features(torch.zeros(12, 1), ["x"]),
        item_features=datasets.Features(torch.zeros(40, 1), ["x"]))
