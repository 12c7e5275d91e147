"""Generate the point-wise (MSE) golden vectors by running the REFERENCE divrec.

Run with the reference package on PYTHONPATH, like make_golden.py (the
reference tree is not on the GPU box):

    PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=<reference checkout> \
        python tests/golden/make_golden_pointwise.py

Nothing from the reference is copied: only data (inputs and the values its
code returned), written as .npz fixtures next to this script.

Fixtures:
  mse_step   one point_wise_train_loop batch by hand: MatrixFactorization
             forward, MSELoss() value, both gradients, the tables after one
             Adam(lr=1e-3) step (train/utils.py:108-115, losses/mse_loss.py:6-10)
  mse_loop   point_wise_train_loop over PointWiseDataset (three batches of
             64, 64, 22) with an MSELoss score, and point_wise_score_loop of
             the final tables (train/utils.py:10-28,94-127)
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))


def _import_reference():
    import divrec

    # the reference package has no HIP backend module; this project's has
    assert not os.path.exists(os.path.join(os.path.dirname(divrec.__file__), "_backend.py")), \
        f"not the reference package: {divrec.__file__}"
    from divrec import datasets, losses, models, train

    return datasets, losses, models, train


def save(name: str, **arrays):
    out = {}
    for k, v in arrays.items():
        if isinstance(v, torch.Tensor):
            v = v.detach().cpu().numpy()
        out[k] = np.asarray(v)
    np.savez_compressed(os.path.join(HERE, f"{name}.npz"), **out)
    print(f"wrote {name}.npz: " + ", ".join(f"{k}{list(np.shape(v))}" for k, v in out.items()))


def main():
    datasets, losses, models, train = _import_reference()

    # ---------------------------------------------------------------- MSE step
    g = torch.Generator().manual_seed(6)
    nu, ni, d, B = 30, 60, 16, 100
    mf = models.MatrixFactorization(nu, ni, d)
    with torch.no_grad():
        mf.user_embeddings.weight.copy_(torch.randn(nu, d, generator=g) * 0.5)
        mf.item_embeddings.weight.copy_(torch.randn(ni, d, generator=g) * 0.5)
    U0 = mf.user_embeddings.weight.detach().clone()
    I0 = mf.item_embeddings.weight.detach().clone()
    uid = torch.randint(0, nu, (B,), generator=g)
    iid = torch.randint(0, ni, (B,), generator=g)
    target = torch.randint(1, 6, (B,), generator=g).float()
    opt = torch.optim.Adam(mf.parameters(), lr=1e-3)
    pred = mf(uid, iid)
    loss = losses.MSELoss()(target, pred)
    loss.backward()
    gU = mf.user_embeddings.weight.grad.detach().clone()
    gI = mf.item_embeddings.weight.grad.detach().clone()
    opt.step()
    save("mse_step", U0=U0, I0=I0, uid=uid, iid=iid, target=target, pred=pred.detach(),
         loss=loss.detach(), gU=gU, gI=gI, U1=mf.user_embeddings.weight,
         I1=mf.item_embeddings.weight)

    # ---------------------------------------------------------------- MSE loop
    # scores are indexed by ITEM id in the reference (base_datasets.py:52): 150
    # of them, more than the 40 items, so every lookup is in range
    rng = np.random.default_rng(11)
    n_users, n_items, n_inter = 12, 40, 150
    inter = np.stack([rng.integers(0, n_users, n_inter), rng.integers(0, n_items, n_inter)], axis=1)
    inter[0], inter[1] = (n_users - 1, 0), (0, n_items - 1)  # both tables' last rows occur
    scores = rng.integers(1, 6, n_inter).astype(np.float32)
    data = datasets.UserItemInteractionsDataset(
        torch.from_numpy(inter).long(), torch.from_numpy(scores),
        user_features=datasets.Features(torch.zeros(n_users, 1), ["x"]),
        item_features=datasets.Features(torch.zeros(n_items, 1), ["x"]))
    torch.manual_seed(3)
    mf = models.MatrixFactorization(n_users, n_items, 16)
    U0 = mf.user_embeddings.weight.detach().clone()
    I0 = mf.item_embeddings.weight.detach().clone()
    opt = torch.optim.Adam(mf.parameters(), lr=1e-2)
    mean_loss, (mean_score,) = train.point_wise_train_loop(
        datasets.PointWiseDataset(data), mf, losses.MSELoss(), opt, scores=[losses.MSELoss()],
        batch_size=64)
    with torch.no_grad():
        (final_loss,) = train.point_wise_score_loop(
            datasets.PointWiseDataset(data), mf, [losses.MSELoss()], batch_size=64)
    save("mse_loop", interactions=inter.astype(np.int64), scores=scores, U0=U0, I0=I0,
         U1=mf.user_embeddings.weight, I1=mf.item_embeddings.weight,
         mean_loss=np.float64(mean_loss), mean_score=np.float64(mean_score),
         final_loss=np.float64(float(final_loss)), batch_size=np.int64(64), lr=np.float64(1e-2))


if __name__ == "__main__":
    sys.exit(main())
