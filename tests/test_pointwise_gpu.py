"""Point-wise MSE path on the GPU: dr_mse_fwd_bwd against the float64
restatement (tests/pointwise_checks.py, pinned to the reference by the host
tests), the reference's golden step and loop, the loops' path selection, the
optimizers and the id range contract.

Tolerances are the BPR tests' (tests/test_hip_kernels.py, test_api_gpu.py):
the kernel against float64 mean loss rel 1e-5, gradients rtol 1e-4 / atol
1e-7, per-pair pred and loss rtol 1e-5 / atol 1e-6; the golden step loss rel
1e-6, gradients rtol 1e-5 / atol 1e-8, tables atol 1e-6; the loops mean loss
and score rel 1e-5, tables atol 1e-5."""
import numpy as np
import pytest
import torch

from divrec import _backend, datasets, losses, models, ops, train
from divrec.train import utils as train_utils
from pairwise_checks import BPR_WIDTHS
from pointwise_checks import load, loop_data, mse_step_f64

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def tables(rng, nu, ni, d, scale=0.3):
    return ((rng.standard_normal((nu, d)) * scale).astype(np.float32),
            (rng.standard_normal((ni, d)) * scale).astype(np.float32))


def run_kernel(U, I, uid, iid, target, grad_scale, **kw):
    """ops.mse_fwd_bwd on numpy inputs -> numpy (pred, loss, grad_user, grad_item)."""
    gU, gI = torch.zeros(U.shape, device=DEV), torch.zeros(I.shape, device=DEV)
    pred, loss = ops.mse_fwd_bwd(dev(U), dev(I), dev(uid), dev(iid), dev(target), grad_scale,
                                 gU, gI, **kw)
    return tuple(t.cpu().numpy() for t in (pred, loss, gU, gI))


def check_against_f64(U, I, uid, iid, target, what=""):
    B = len(uid)
    got = run_kernel(U, I, uid, iid, target, 1.0 / B)
    ref = mse_step_f64(U, I, uid, iid, target, 1.0 / B)
    errs = [float(np.max(np.abs(g - r))) for g, r in zip(got, ref)]
    print(f"{what} B={B} d={U.shape[1]}: max abs err pred {errs[0]:.3g} loss {errs[1]:.3g} "
          f"gU {errs[2]:.3g} gI {errs[3]:.3g}; mean loss {got[1].sum() / B:.8g} "
          f"vs {ref[1].sum() / B:.8g}")
    assert np.allclose(got[0], ref[0], rtol=1e-5, atol=1e-6)
    assert np.allclose(got[1], ref[1], rtol=1e-5, atol=1e-6)
    assert float(got[1].astype(np.float64).sum() / B) == pytest.approx(ref[1].sum() / B, rel=1e-5)
    assert np.allclose(got[2], ref[2], rtol=1e-4, atol=1e-7)
    assert np.allclose(got[3], ref[3], rtol=1e-4, atol=1e-7)
    return got, ref


def random_batch(rng, nu, ni, B):
    return (rng.integers(0, nu, B), rng.integers(0, ni, B),
            rng.integers(1, 6, B).astype(np.float32))


# --------------------------------------------------------------------------- kernel
@pytest.mark.parametrize("d", sorted({*BPR_WIDTHS, 100, 128, 256}))
def test_mse_kernel_against_float64(d):
    """Every instance, as for bpr_kernel (pairwise_checks.BPR_WIDTHS: 1 to 3, 5
    to 7, 12 and 16 elements per lane, with masked tails), and 4 and 8
    elements: the reference's width (100), 128 and 256."""
    rng = np.random.default_rng(d)
    U, I = tables(rng, 200, 300, d)
    check_against_f64(U, I, *random_batch(rng, 200, 300, 4096), what="random")


@pytest.mark.parametrize("B", [1, 17, 4097])
def test_mse_kernel_batch_sizes(B):
    """One pair, one span plus one pair, and a last group with a single pair."""
    rng = np.random.default_rng(B)
    U, I = tables(rng, 200, 300, 100)
    check_against_f64(U, I, *random_batch(rng, 200, 300, B), what="batch size")


def test_mse_kernel_sorted_by_user_run_crosses_spans():
    """One user for the first 2000 pairs (125 spans of 16: that many groups
    flush into one gradient row), then other users in sorted order; items
    random, then item runs too."""
    rng = np.random.default_rng(7)
    U, I = tables(rng, 200, 300, 100)
    uid, iid, t = random_batch(rng, 200, 300, 4096)
    uid = np.concatenate([np.full(2000, 5), np.sort(uid[2000:])])
    check_against_f64(U, I, uid, iid, t, what="user runs")
    check_against_f64(U, I, iid % 200, np.sort(iid), t, what="item runs")


def test_mse_kernel_all_identical_pairs():
    rng = np.random.default_rng(9)
    U, I = tables(rng, 200, 300, 100)
    B = 1000
    uid, iid, t = np.full(B, 17), np.full(B, 250), np.full(B, 4.0, np.float32)
    got, _ = check_against_f64(U, I, uid, iid, t, what="identical")
    one = mse_step_f64(U, I, uid[:1], iid[:1], t[:1], 1.0 / B)
    assert np.allclose(got[2], B * one[2], rtol=1e-4, atol=1e-7)
    assert np.allclose(got[3], B * one[3], rtol=1e-4, atol=1e-7)
    assert np.count_nonzero(got[2].any(axis=1)) == 1 and np.count_nonzero(got[3].any(axis=1)) == 1


def test_mse_forward_only_and_null_outputs():
    """Both gradient tables None: no gradient is written anywhere (tables
    poisoned with NaN stay as they are) and pred / loss are the training
    call's, bit for bit. The C call accepts pred = NULL and loss = NULL."""
    rng = np.random.default_rng(21)
    Un, In = tables(rng, 200, 300, 100)
    uid, iid, t = (dev(a) for a in random_batch(rng, 200, 300, 4096))
    U, I = dev(Un), dev(In)
    gU, gI = torch.zeros_like(U), torch.zeros_like(I)
    pred_t, loss_t = ops.mse_fwd_bwd(U, I, uid, iid, t, 1.0 / 4096, gU, gI)
    assert gU.any() and gI.any()
    pU, pI = torch.full_like(U, float("nan")), torch.full_like(I, float("nan"))
    pred_f, loss_f = ops.mse_fwd_bwd(U, I, uid, iid, t, 1.0 / 4096, None, None)
    torch.cuda.synchronize()
    assert torch.isnan(pU).all() and torch.isnan(pI).all()
    assert torch.equal(pred_f, pred_t) and torch.equal(loss_f, loss_t)
    assert torch.equal(U, dev(Un)) and torch.equal(I, dev(In))
    # one table only: the other side's gradient is the training call's
    only_u = torch.zeros_like(U)
    ops.mse_fwd_bwd(U, I, uid, iid, t, 1.0 / 4096, only_u, None)
    assert np.allclose(only_u.cpu().numpy(), gU.cpu().numpy(), rtol=1e-4, atol=1e-7)
    lib = _backend.lib()
    for skip in ("pred", "loss"):
        out = torch.full((4096,), -7.0, device=DEV)
        rc = lib.dr_mse_fwd_bwd(U.data_ptr(), 200, I.data_ptr(), 300, 100, uid.data_ptr(),
                                iid.data_ptr(), t.data_ptr(), 4096, 0.0,
                                None if skip == "pred" else out.data_ptr(),
                                None if skip == "loss" else out.data_ptr(), None, None, None,
                                _backend.stream(DEV))
        assert rc == 0
        assert torch.equal(out, loss_t if skip == "pred" else pred_t)


def test_mse_bad_ids_are_skipped_and_counted():
    rng = np.random.default_rng(33)
    U, I = tables(rng, 200, 300, 100)
    uid, iid, t = random_batch(rng, 200, 300, 4096)
    uid[100], iid[3000] = -1, 300
    err = _backend.error_counter(DEV)
    got = run_kernel(U, I, uid, iid, t, 1.0 / 4096, err=err)
    assert int(err.item()) == 2
    bad = np.zeros(4096, bool)
    bad[[100, 3000]] = True
    assert np.isnan(got[0][bad]).all() and np.isnan(got[1][bad]).all()
    assert np.isfinite(got[0][~bad]).all() and np.isfinite(got[1][~bad]).all()
    ref = mse_step_f64(U, I, uid[~bad], iid[~bad], t[~bad], 1.0 / 4096)
    assert np.allclose(got[0][~bad], ref[0], rtol=1e-5, atol=1e-6)
    assert np.allclose(got[2], ref[2], rtol=1e-4, atol=1e-7)
    assert np.allclose(got[3], ref[3], rtol=1e-4, atol=1e-7)
    with pytest.raises(IndexError):
        run_kernel(U, I, uid, iid, t, 1.0 / 4096)  # check=True, no err: raises


# --------------------------------------------------------------------------- golden fixtures
def mf_from(U, I):
    mf = models.MatrixFactorization(U.shape[0], I.shape[0], U.shape[1])
    with torch.no_grad():
        mf.user_embeddings.weight.copy_(torch.from_numpy(U))
        mf.item_embeddings.weight.copy_(torch.from_numpy(I))
    return mf.to(DEV)


def weights(mf):
    return (mf.user_embeddings.weight.detach().cpu().numpy(),
            mf.item_embeddings.weight.detach().cpu().numpy())


def test_mse_step_golden():
    g = load("mse_step")
    mf = mf_from(g["U0"], g["I0"])
    opt = torch.optim.Adam(mf.parameters(), lr=1e-3)
    U, I = mf.user_embeddings.weight, mf.item_embeddings.weight
    U.grad, I.grad = torch.zeros_like(U), torch.zeros_like(I)
    B = g["uid"].size
    pred, sq = ops.mse_fwd_bwd(U.data, I.data, dev(g["uid"]), dev(g["iid"]), dev(g["target"]),
                               1.0 / B, U.grad, I.grad)
    assert float(sq.sum() / B) == pytest.approx(float(g["loss"]), rel=1e-6)
    assert np.allclose(pred.cpu().numpy(), g["pred"], rtol=1e-5, atol=1e-6)
    assert np.allclose(U.grad.cpu().numpy(), g["gU"], rtol=1e-5, atol=1e-8)
    assert np.allclose(I.grad.cpu().numpy(), g["gI"], rtol=1e-5, atol=1e-8)
    train.fused_adam_step(opt)
    U1, I1 = weights(mf)
    assert np.allclose(U1, g["U1"], rtol=0, atol=1e-6)
    assert np.allclose(I1, g["I1"], rtol=0, atol=1e-6)


class Calls:
    """Counts the calls of ops.mse_fwd_bwd made through divrec.train.utils."""

    def __init__(self, monkeypatch):
        self.n = 0
        real = ops.mse_fwd_bwd

        def counted(*a, **kw):
            self.n += 1
            return real(*a, **kw)

        monkeypatch.setattr(train_utils.ops, "mse_fwd_bwd", counted)


def loop_dataset(g, kind, **kw):
    data = loop_data(g, **kw)
    if kind == "device":
        return datasets.DevicePointWiseDataset(data, device=DEV)
    return datasets.PointWiseDataset(data)


def check_loop_golden(g, mf, mean_loss, mean_scores):
    assert mean_loss == pytest.approx(float(g["mean_loss"]), rel=1e-5)
    for s in mean_scores:
        assert s == pytest.approx(float(g["mean_score"]), rel=1e-5)
    U1, I1 = weights(mf)
    assert np.allclose(U1, g["U1"], atol=1e-5) and np.allclose(I1, g["I1"], atol=1e-5)


@pytest.mark.parametrize("kind", ["host", "device"])
def test_point_wise_loops_golden(kind, monkeypatch):
    """point_wise_train_loop over the reference's 150 interactions (batches of
    64, 64, 22) on the fused path, one kernel call per batch, then
    point_wise_score_loop of the trained tables on the forward-only form."""
    g = load("mse_loop")
    calls = Calls(monkeypatch)
    mf = mf_from(g["U0"], g["I0"])
    opt = torch.optim.Adam(mf.parameters(), lr=float(g["lr"]))
    mean_loss, mean_scores = train.point_wise_train_loop(
        loop_dataset(g, kind), mf, losses.MSELoss(), opt, scores=[losses.MSELoss()],
        batch_size=int(g["batch_size"]))
    assert calls.n == 3 and len(mean_scores) == 1
    check_loop_golden(g, mf, mean_loss, mean_scores)
    assert opt.state[mf.user_embeddings.weight]["step"].item() == 3  # torch's own Adam state
    (final,) = train.point_wise_score_loop(loop_dataset(g, kind), mf, [losses.MSELoss()],
                                           batch_size=int(g["batch_size"]))
    assert calls.n == 6
    assert float(final) == pytest.approx(float(g["final_loss"]), rel=1e-5)
    # the score loop of the fixture's own final tables
    (final,) = train.point_wise_score_loop(loop_dataset(g, kind), mf_from(g["U1"], g["I1"]),
                                           [losses.MSELoss()], batch_size=int(g["batch_size"]))
    assert float(final) == pytest.approx(float(g["final_loss"]), rel=1e-5)


def test_point_wise_train_loop_sum_reduction_and_no_scores(monkeypatch):
    """reduction='sum': grad_scale 1 and the loss value the batch's sum; with
    scores=None the loop returns an empty score list. Against the generic path
    (a user-defined loss of the same arithmetic)."""
    g = load("mse_loop")
    calls = Calls(monkeypatch)
    out = []
    for loss in (losses.MSELoss(reduction="sum"), _MyMSE(reduction="sum")):
        mf = mf_from(g["U0"], g["I0"])
        opt = torch.optim.Adam(mf.parameters(), lr=1e-2)
        out.append((train.point_wise_train_loop(loop_dataset(g, "host"), mf, loss, opt,
                                                batch_size=64), weights(mf)))
    assert calls.n == 3
    (fast, fw), (gen, gw) = out
    assert fast[1] == [] and gen[1] == []
    assert fast[0] == pytest.approx(gen[0], rel=1e-5)
    assert np.allclose(fw[0], gw[0], atol=1e-5) and np.allclose(fw[1], gw[1], atol=1e-5)


# --------------------------------------------------------------------------- path selection
class _MyMF(models.MatrixFactorization):
    def forward(self, user_id, item_id, user_features=None, item_features=None):
        return super().forward(user_id, item_id, user_features, item_features)


class _MyMSE(losses.PointWiseLoss):
    def point_wise(self, true_relevance, predicted_relevance):
        return (true_relevance - predicted_relevance) ** 2


def _generic_train_cases():
    yield "forward override", dict(model_cls=_MyMF)
    yield "float64 targets", dict(score_dtype=torch.float64)
    yield "user-defined loss", dict(loss=_MyMSE())
    yield "user-defined score", dict(scores=[_MyMSE()])


@pytest.mark.parametrize("name,case", list(_generic_train_cases()))
def test_generic_train_path_is_kept_and_agrees(name, case, monkeypatch):
    g = load("mse_loop")
    calls = Calls(monkeypatch)
    mf = mf_from(g["U0"], g["I0"])
    if "model_cls" in case:
        sub = case["model_cls"](12, 40, 16).to(DEV)
        sub.load_state_dict(mf.state_dict())
        mf = sub
    opt = torch.optim.Adam(mf.parameters(), lr=float(g["lr"]))
    data = loop_dataset(g, "host", score_dtype=case.get("score_dtype", torch.float32))
    mean_loss, mean_scores = train.point_wise_train_loop(
        data, mf, case.get("loss", losses.MSELoss()), opt,
        scores=case.get("scores", [losses.MSELoss()]), batch_size=64)
    assert calls.n == 0, name
    check_loop_golden(g, mf, mean_loss, mean_scores)


def test_train_loop_reduction_none_fails_at_backward_like_the_reference(monkeypatch):
    g = load("mse_loop")
    calls = Calls(monkeypatch)
    mf = mf_from(g["U0"], g["I0"])
    opt = torch.optim.Adam(mf.parameters(), lr=1e-2)
    with pytest.raises(RuntimeError, match="grad can be implicitly created only for scalar"):
        train.point_wise_train_loop(loop_dataset(g, "host"), mf, losses.MSELoss(reduction="none"),
                                    opt, batch_size=64)
    assert calls.n == 0


def test_score_loop_path_selection(monkeypatch):
    g = load("mse_loop")
    calls = Calls(monkeypatch)
    mf = mf_from(g["U1"], g["I1"])
    ds = loop_dataset(g, "host")
    (per_pair,) = train.point_wise_score_loop(ds, mf, [losses.MSELoss(reduction="none")],
                                              batch_size=64)
    assert calls.n == 3 and per_pair.shape == (150,)
    assert float(per_pair.sum() / 150) == pytest.approx(float(g["final_loss"]), rel=1e-5)
    # a second, non-MSE loss: every loss goes through the model's forward
    generic = train.point_wise_score_loop(ds, mf, [losses.MSELoss(reduction="none"), _MyMSE()],
                                          batch_size=64)
    assert calls.n == 3
    assert np.allclose(generic[0].cpu().numpy(), per_pair.cpu().numpy(), rtol=1e-5, atol=1e-6)
    assert float(generic[1]) == pytest.approx(float(g["final_loss"]), rel=1e-5)
    # float64 targets and a forward override: generic too
    train.point_wise_score_loop(loop_dataset(g, "host", score_dtype=torch.float64), mf,
                                [losses.MSELoss()], batch_size=64)
    sub = _MyMF(12, 40, 16).to(DEV)
    sub.load_state_dict(mf.state_dict())
    (v,) = train.point_wise_score_loop(ds, sub, [losses.MSELoss()], batch_size=64)
    assert calls.n == 3
    assert float(v) == pytest.approx(float(g["final_loss"]), rel=1e-5)
    # two MSELoss objects share one value list, as in the reference (keyed by class name)
    both = train.point_wise_score_loop(ds, mf, [losses.MSELoss(), losses.MSELoss(reduction="sum")],
                                       batch_size=64)
    assert calls.n == 6
    assert float(both[0]) == pytest.approx(float(g["final_loss"]), rel=1e-5)
    assert float(both[1]) == pytest.approx(300 * float(g["final_loss"]), rel=1e-5)


def test_score_loop_bad_ids_raise():
    mf = models.MatrixFactorization(12, 40, 16).to(DEV)
    t = torch.ones(4, device=DEV)
    ok = torch.zeros(4, dtype=torch.int64, device=DEV)
    bad = torch.tensor([0, 1, 40, 2], device=DEV)
    with pytest.raises(IndexError):  # device ids: the kernel's counter, read after the epoch
        train.point_wise_score_loop(_DeviceBatches([(ok, bad, t)]), mf, [losses.MSELoss()])
    with pytest.raises(IndexError):  # host ids: before any compute
        train.point_wise_score_loop(_DeviceBatches([(ok.cpu(), bad.cpu(), t.cpu())]), mf,
                                    [losses.MSELoss()])


# --------------------------------------------------------------------------- optimizers
def test_point_wise_train_loop_sparse_adam():
    """torch.optim.SparseAdam takes the fused kernel + dr_adam_rows. Reference:
    the same batches through nn.Embedding(sparse=True) tables and torch's
    SparseAdam on the CPU (as test_pair_wise_train_loop_sparse_adam). Both
    gradient tables are all-zero afterwards."""
    g = load("mse_loop")
    lr = 1e-2
    mf = mf_from(g["U0"], g["I0"])
    opt = torch.optim.SparseAdam(list(mf.parameters()), lr=lr)
    mean_loss, _ = train.point_wise_train_loop(loop_dataset(g, "host"), mf, losses.MSELoss(), opt,
                                               batch_size=64)
    for p in mf.parameters():
        assert p.grad is not None and not p.grad.any()

    Ue = torch.nn.Embedding(12, 16, sparse=True)
    Ie = torch.nn.Embedding(40, 16, sparse=True)
    with torch.no_grad():
        Ue.weight.copy_(torch.from_numpy(g["U0"]))
        Ie.weight.copy_(torch.from_numpy(g["I0"]))
    ref_opt = torch.optim.SparseAdam(list(Ue.parameters()) + list(Ie.parameters()), lr=lr)
    ref_losses = []
    for u, i, _, _, t in loop_dataset(g, "host").loader(batch_size=64):
        loss = ((t - torch.sum(Ue(u) * Ie(i), dim=1)) ** 2).mean()
        loss.backward()
        ref_opt.step()
        ref_opt.zero_grad()
        ref_losses.append(float(loss.detach()))
    assert mean_loss == pytest.approx(sum(ref_losses) / len(ref_losses), rel=1e-5)
    U1, I1 = weights(mf)
    assert np.allclose(U1, Ue.weight.detach().numpy(), rtol=0, atol=1e-5)
    assert np.allclose(I1, Ie.weight.detach().numpy(), rtol=0, atol=1e-5)


def test_point_wise_train_loop_sgd_uses_optimizer_step(monkeypatch):
    g = load("mse_loop")
    calls = Calls(monkeypatch)
    out = []
    for loss in (losses.MSELoss(), _MyMSE()):
        mf = mf_from(g["U0"], g["I0"])
        opt = torch.optim.SGD(mf.parameters(), lr=1e-2, momentum=0.9)
        out.append((train.point_wise_train_loop(loop_dataset(g, "host"), mf, loss, opt,
                                                scores=[losses.MSELoss()], batch_size=64),
                    weights(mf), opt))
    assert calls.n == 3  # the MSELoss run only
    (fast, fw, fopt), (gen, gw, _) = out
    assert fast[0] == pytest.approx(gen[0], rel=1e-5)
    assert fast[1][0] == pytest.approx(gen[1][0], rel=1e-5)
    assert np.allclose(fw[0], gw[0], atol=1e-5) and np.allclose(fw[1], gw[1], atol=1e-5)
    assert not np.array_equal(fw[0], g["U0"])
    assert all("momentum_buffer" in st for st in fopt.state.values())  # torch's step ran


# --------------------------------------------------------------------------- bad device batch
class _DeviceBatches:
    """A PointWiseDataset stand-in whose loader yields whole batches (as
    DevicePointWiseDataset does): (user, item, None, None, target)."""

    def __init__(self, batches):
        self.batches = batches

    def loader(self, **_):
        for u, i, t in self.batches:
            yield u, i, None, None, t


@pytest.mark.parametrize("sparse", [False, True])
def test_point_wise_train_loop_bad_device_batch_leaves_no_trace(sparse):
    """A device batch with an out-of-range id raises IndexError before the
    fused kernel runs: weights, optimizer state and gradient tables stay as
    they were, so training on gives exactly an untouched twin's weights."""
    torch.manual_seed(3)
    nu, ni, d = 50, 80, 32
    a = models.MatrixFactorization(nu, ni, d).to(DEV)
    b = models.MatrixFactorization(nu, ni, d).to(DEV)
    b.load_state_dict(a.state_dict())
    mk = (lambda m: torch.optim.SparseAdam(m.parameters(), lr=1e-2)) if sparse else \
        (lambda m: torch.optim.Adam(m.parameters(), lr=1e-2))
    oa, ob = mk(a), mk(b)
    # batches of one span (16 pairs): one 32-lane group adds every gradient in
    # program order, so the twins' fp32 atomic sums are bit-identical (across
    # groups the order of the adds into a row is not fixed)
    gen = torch.Generator(device=DEV).manual_seed(5)
    good = [(torch.randint(0, nu, (16,), generator=gen, device=DEV),
             torch.randint(0, ni, (16,), generator=gen, device=DEV),
             torch.randint(1, 6, (16,), generator=gen, device=DEV).float()) for _ in range(4)]
    before = [p.detach().clone() for p in a.parameters()]
    loss = losses.MSELoss()
    for col, value in ((1, ni + 3), (0, -1)):
        bad = [t.clone() for t in good[0]]
        bad[col][11] = value
        with pytest.raises(IndexError):
            train.point_wise_train_loop(_DeviceBatches([tuple(bad)]), a, loss, oa)
    for p_, p0 in zip(a.parameters(), before):
        assert torch.equal(p_, p0)
        assert p_.grad is None or not p_.grad.any()  # nothing was accumulated
    assert len(oa.state) == 0
    train.point_wise_train_loop(_DeviceBatches(good), a, loss, oa)
    train.point_wise_train_loop(_DeviceBatches(good), b, loss, ob)
    for pa, pb, p0 in zip(a.parameters(), b.parameters(), before):
        assert torch.equal(pa, pb)
        assert not torch.equal(pa, p0)
