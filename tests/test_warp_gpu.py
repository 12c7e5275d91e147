"""WARP step on the GPU: dr_warp_fwd_bwd against the float64 restatement of
its specification (tests/warp_checks.py; the reference project has no WARP),
under check_warp, whose bounds tests/test_warp_host.py shows on the CPU to
admit a correct kernel and to reject six broken ones; the catalog and calling
edges; and warp_train_loop end to end."""
import numpy as np
import pytest
import torch

from divrec import _backend, datasets, losses, metrics, models, ops, train
from divrec.train.utils import warp_batch_seed
from pairwise_checks import adam_ref, check_adam, csr
from warp_checks import WARP_WIDTHS, check_warp, warp_case, warp_ref, warp_step_f64

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def dev_csr(c):
    return None if c is None else (dev(c[0]), dev(c[1]))


def run_kernel(case, grad_user=True, grad_item=True, **kw):
    """ops.warp_fwd_bwd on a warp_checks case -> numpy (loss, neg, trials,
    grad_user, grad_item), a gradient None where it was not asked for."""
    gU = torch.zeros(case["U"].shape, device=DEV) if grad_user else None
    gI = torch.zeros(case["I"].shape, device=DEV) if grad_item else None
    out = ops.warp_fwd_bwd(dev(case["U"]), dev(case["I"]), dev(case["uid"]), dev(case["pid"]),
                           dev_csr(case.get("pos")), dev_csr(case.get("excl")),
                           case["max_trials"], case["margin"], case["seed"], case["pair_base"],
                           case["grad_scale"], gU, gI, **kw)
    return tuple(None if t is None else t.cpu().numpy() for t in (*out, gU, gI))


# --------------------------------------------------------------------------- kernel
@pytest.mark.parametrize("exclude", [False, True], ids=["", "excl"])
@pytest.mark.parametrize("regime", ["random", "planted"])
@pytest.mark.parametrize("d", WARP_WIDTHS)
def test_warp_against_the_restatement(d, regime, exclude):
    case, ref = warp_ref(d, regime, exclude)
    got = run_kernel(case)
    check_warp(got, ref, what=f"{regime} excl={exclude}")
    assert got[1].dtype == np.int64 and got[2].dtype == np.int32


@pytest.mark.parametrize("grad_user,grad_item", [(True, False), (False, True), (False, False)])
def test_warp_without_a_gradient_table(grad_user, grad_item):
    """Either gradient table may be NULL: the other side's gradient and the
    per-pair outputs are those of the full call."""
    case, ref = warp_ref(100, "planted", True)
    full = run_kernel(case)
    got = run_kernel(case, grad_user, grad_item)
    check_warp(got, ref, what=f"gU={grad_user} gI={grad_item}")
    assert (got[3] is None) == (not grad_user) and (got[4] is None) == (not grad_item)
    for a, b in zip(got[:3], full[:3]):
        assert np.array_equal(a, b)


def test_warp_null_outputs():
    """loss, neg_id and trials may each be NULL in the C call."""
    case, _ = warp_ref(64, "planted", False)
    full = run_kernel(case)
    U, I, uid, pid = (dev(case[k]) for k in ("U", "I", "uid", "pid"))
    pr, pi = dev_csr(case["pos"])
    lib = _backend.lib()
    for skip in range(3):
        outs = [torch.full((4096,), -7, dtype=t, device=DEV)
                for t in (torch.float32, torch.int64, torch.int32)]
        ptrs = [None if k == skip else o.data_ptr() for k, o in enumerate(outs)]
        rc = lib.dr_warp_fwd_bwd(U.data_ptr(), 200, I.data_ptr(), 300, 64, uid.data_ptr(),
                                 pid.data_ptr(), 4096, pr.data_ptr(), pi.data_ptr(), None, None,
                                 32, 1.0, case["seed"], 0, case["grad_scale"], *ptrs, None, None,
                                 None, _backend.stream(DEV))
        assert rc == 0
        for k, o in enumerate(outs):
            if k == skip:
                assert (o == -7).all()
            else:
                assert np.array_equal(o.cpu().numpy(), full[k])


def test_warp_integer_tables_are_exact():
    """Integer-valued tables in [-3, 3], d = 128, margin 1: every score and
    every comparison is exact in fp32, so neg and trials equal the
    restatement on EVERY pair, none left out."""
    case = dict(warp_case(128, "random", True))
    rng = np.random.default_rng(128)
    case["U"] = rng.integers(-3, 4, (200, 128)).astype(np.float32)
    case["I"] = rng.integers(-3, 4, (300, 128)).astype(np.float32)
    ref = warp_step_f64(case)
    got = run_kernel(case)
    assert np.array_equal(got[1], ref["neg"]) and np.array_equal(got[2], ref["trials"])
    assert (ref["neg"] < 0).any() and len(np.unique(ref["trials"])) > 16
    assert np.allclose(got[0], ref["loss"], rtol=1e-5, atol=1e-6)
    assert np.allclose(got[3], ref["gU"], rtol=1e-4, atol=1e-7)
    assert np.allclose(got[4], ref["gI"], rtol=1e-4, atol=1e-7)


# --------------------------------------------------------------------------- catalog edges
def test_warp_small_catalog_reaches_weight_zero():
    """n_items = 8, max_trials = 16: from trial 4 on (7 // trials <= 1) the
    weight is log 1 = 0: the violator is reported with loss 0 and adds no
    gradient."""
    case = dict(warp_case(64, B=1024), max_trials=16, pos=None)
    case["I"] = case["I"][:8].copy()
    case["pid"] = case["pid"] % 8
    ref = warp_step_f64(case)
    got = run_kernel(case)
    check_warp(got, ref, what="8 items")
    late = (ref["neg"] >= 0) & (ref["trials"] >= 4) & ~ref["undecided"]
    assert late.sum() > 10 and (got[0][late] == 0).all() and (got[1][late] >= 0).all()
    # such a pair alone, at its own position: nothing is added anywhere
    for b in np.flatnonzero(late)[:8]:
        one = run_kernel(dict(case, uid=case["uid"][b:b + 1], pid=case["pid"][b:b + 1],
                              pair_base=int(b)))
        assert one[1][0] == got[1][b] and not one[3].any() and not one[4].any()


def test_warp_user_without_any_candidate_and_one_item_catalog():
    """A user whose positives and exclusions cover the catalog has no
    violator; neither has any pair of a one-item catalog (the only draw is
    the positive itself)."""
    case = dict(warp_case(33, B=256))
    rows = [np.arange(0, 300, 2) if u == 7 else np.arange(3) for u in range(200)]
    ex = [np.arange(1, 300, 2) if u == 7 else np.zeros(0, np.int64) for u in range(200)]
    case.update(pos=csr(rows), excl=csr(ex))
    case["uid"] = case["uid"].copy()
    case["uid"][::4] = 7
    got = run_kernel(case)
    check_warp(got, warp_step_f64(case), what="covered user")
    mine = case["uid"] == 7
    assert (got[1][mine] == -1).all() and (got[2][mine] == 32).all() and (got[0][mine] == 0).all()
    assert (got[1][~mine] >= 0).any()
    one = dict(warp_case(33, B=64), pos=None)
    one["I"] = one["I"][:1].copy()
    one["pid"] = np.zeros(64, np.int64)
    got = run_kernel(one)
    check_warp(got, warp_step_f64(one), what="one item")
    assert (got[1] == -1).all() and (got[2] == 32).all() and not got[3].any() and not got[4].any()


# --------------------------------------------------------------------------- calling edges
@pytest.mark.parametrize("B", [1, 33])
def test_warp_batch_sizes(B):
    """One pair; two spans of 16 and a tail of one pair."""
    case = warp_case(100, "planted", True, B=B)
    check_warp(run_kernel(case), warp_step_f64(case), what="batch size")


def test_warp_halves_with_pair_base_equal_the_whole_call():
    case, ref = warp_ref(128, "planted", True)
    whole = run_kernel(case)
    gU, gI = np.zeros_like(whole[3]), np.zeros_like(whole[4])
    for lo, hi in ((0, 2048), (2048, 4096)):
        part = run_kernel(dict(case, uid=case["uid"][lo:hi], pid=case["pid"][lo:hi], pair_base=lo))
        for k in range(3):  # per pair bit for bit: the same arithmetic on the same draws
            assert np.array_equal(part[k], whole[k][lo:hi])
        gU += part[3]
        gI += part[4]
    assert np.allclose(gU, whole[3], rtol=1e-4, atol=1e-7)
    assert np.allclose(gI, whole[4], rtol=1e-4, atol=1e-7)
    # and a pair_base above 2^32 is a different, valid stream
    far = dict(case, pair_base=2 ** 33 + 5)
    check_warp(run_kernel(far), warp_step_f64(far), what="pair_base 2^33 + 5")


def test_warp_bad_ids_are_skipped_and_counted():
    case = dict(warp_case(100, "planted", True))
    case["uid"], case["pid"] = case["uid"].copy(), case["pid"].copy()
    case["uid"][[3, 900]] = [-1, 200]
    case["pid"][[17, 4095]] = [300, -5]
    err = _backend.error_counter(DEV)
    got = run_kernel(case, err=err)
    assert int(err.item()) == 4
    ref = warp_step_f64(case)
    assert (~ref["valid"]).sum() == 4
    check_warp(got, ref, what="bad ids")
    with pytest.raises(IndexError):
        run_kernel(case)  # check=True, no err: raises


def test_warp_wrapper_validates():
    case, _ = warp_ref(64, "random", False)
    U, I, uid, pid = (dev(case[k]) for k in ("U", "I", "uid", "pid"))
    pos = dev_csr(case["pos"])
    args = lambda **kw: {**dict(user_table=U, item_table=I, user_id=uid, pos_id=pid, positives=pos,
                                exclude=None, max_trials=8, margin=1.0, seed=1, pair_base=0,
                                grad_scale=1.0, grad_user=None, grad_item=None), **kw}
    for bad in (dict(max_trials=0), dict(max_trials=4097), dict(pair_base=-1),
                dict(user_table=U.double()), dict(pos_id=pid[:10]), dict(user_id=uid.int()),
                dict(positives=(pos[0][:-1], pos[1])), dict(exclude=(pos[0], pos[1].long())),
                dict(grad_item=torch.zeros(300, 65, device=DEV))):
        with pytest.raises(ValueError):
            ops.warp_fwd_bwd(**args(**bad))
    loss, neg, trials = ops.warp_fwd_bwd(**args())
    assert loss.shape == neg.shape == trials.shape == (4096,)
    empty = ops.warp_fwd_bwd(**args(user_id=uid[:0], pos_id=pid[:0]))
    assert all(t.numel() == 0 for t in empty)


def test_warp_user_runs_and_runs_of_one():
    """A batch sorted by user (runs that cross the 16-pair spans: RowRun sums
    a run in registers) against the same pairs one call each, in shuffled
    order, each at its own pair_base (runs of 1): per pair bit for bit, the
    gradients within the atomics' order; and the shuffled batch as one call
    against its own restatement."""
    case = dict(warp_case(100, "planted", True, B=512))
    order = np.argsort(case["uid"] % 20, kind="stable")
    case["uid"], case["pid"] = (case["uid"] % 20)[order], case["pid"][order]
    rows = csr([np.unique(case["pid"][case["uid"] == u]) for u in range(200)])
    case["pos"] = rows
    ref = warp_step_f64(case)
    got = run_kernel(case)
    check_warp(got, ref, what="sorted by user")
    U, I = dev(case["U"]), dev(case["I"])
    pos, excl = dev_csr(case["pos"]), dev_csr(case["excl"])
    uid, pid = dev(case["uid"]), dev(case["pid"])
    gU, gI = torch.zeros_like(U), torch.zeros_like(I)
    outs = {}
    for b in np.random.default_rng(0).permutation(512).tolist():
        outs[b] = ops.warp_fwd_bwd(U, I, uid[b:b + 1], pid[b:b + 1], pos, excl, 32, 1.0,
                                   case["seed"], b, case["grad_scale"], gU, gI, check=False)
    single = [torch.cat([outs[b][k] for b in range(512)]).cpu().numpy() for k in range(3)]
    for k in range(3):
        assert np.array_equal(single[k], got[k])
    assert np.allclose(gU.cpu().numpy(), got[3], rtol=1e-4, atol=1e-7)
    assert np.allclose(gI.cpu().numpy(), got[4], rtol=1e-4, atol=1e-7)
    perm = np.random.default_rng(1).permutation(512)
    mixed = dict(case, uid=case["uid"][perm], pid=case["pid"][perm])
    check_warp(run_kernel(mixed), warp_step_f64(mixed), what="shuffled")


# --------------------------------------------------------------------------- the train loop
N_USERS, N_ITEMS, BLOCKS = 64, 200, 4


def planted_split(seed=0):
    """64 users x 200 items in 4 blocks: a user's 20 interactions lie in its
    own block of 50 items; 12 train, 8 test."""
    rng = np.random.default_rng(seed)
    tr, te = [], []
    for u in range(N_USERS):
        blk = u % BLOCKS
        items = blk * 50 + rng.choice(50, 20, replace=False)
        tr += [(u, i) for i in items[:12]]
        te += [(u, i) for i in items[12:]]
    mk = lambda x: datasets.UserItemInteractionsDataset(
        torch.tensor(x, dtype=torch.int64), number_of_users=N_USERS, number_of_items=N_ITEMS)
    return mk(tr), mk(te)


def precision_at_10(model, train_data, test_data):
    ds = datasets.RankingDataset(test_data, frozen=train_data)
    (p,) = train.recommendations_score_loop(ds, model, [metrics.PrecisionAtKScore()], 10)
    return float(p)


def make_model(kind):
    torch.manual_seed(0)
    if kind == "feature":
        m = models.FeatureMatrixFactorization(datasets.feature_csr(N_USERS),
                                              datasets.feature_csr(N_ITEMS), 32)
        tables = (m.user_feature_embeddings, m.item_feature_embeddings)
    else:
        m = models.MatrixFactorization(N_USERS, N_ITEMS, 32)
        tables = (m.user_embeddings, m.item_embeddings)
    with torch.no_grad():
        for t in tables:
            t.weight.mul_(0.1)
    m = m.to(DEV)
    if kind == "sparse_adam":
        return m, torch.optim.SparseAdam(list(m.parameters()), lr=0.05)
    return m, torch.optim.Adam(m.parameters(), lr=0.05)


@pytest.mark.parametrize("kind", ["adam", "sparse_adam", "feature"])
def test_warp_train_loop_learns_the_planted_blocks(kind):
    """After a few epochs violators are harder to find than in the first
    epoch (mean_trials grows) and P@10 on held-out interactions exceeds the
    untrained model's on the same split."""
    tr, te = planted_split()
    model, opt = make_model(kind)
    before = precision_at_10(model, tr, te)
    ds = datasets.DevicePointWiseDataset(tr, device=DEV, seed=1)
    loss = losses.WARPLoss(margin=1.0, max_trials=50)
    history = [train.warp_train_loop(ds, model, loss, opt, seed=3, batch_size=128, shuffle=True)
               for _ in range(8)]
    after = precision_at_10(model, tr, te)
    first, last = history[0][1], history[-1][1]
    print(f"{kind}: P@10 {before:.3f} -> {after:.3f}; mean trials {first['mean_trials']:.2f} -> "
          f"{last['mean_trials']:.2f}; no violator {first['no_violator']:.3f} -> "
          f"{last['no_violator']:.3f}; loss {history[0][0]:.4f} -> {history[-1][0]:.4f}")
    assert all(np.isfinite(h[0]) for h in history)
    assert last["mean_trials"] > first["mean_trials"] >= 1.0
    assert 0.0 <= last["no_violator"] <= 1.0
    assert after > before
    if kind == "sparse_adam":  # the touched gradient rows were zeroed
        assert all(p.grad is not None and not p.grad.any() for p in model.parameters())


def test_warp_train_loop_takes_a_host_dataset_and_frozen_items(monkeypatch):
    """PointWiseDataset batches (host tensors through a DataLoader), and
    ``frozen``: no violator is ever one of the user's frozen items."""
    tr, te = planted_split()
    feats = lambda n: datasets.Features(torch.zeros(n, 1), ["x"])  # a DataLoader cannot collate None
    host = datasets.UserItemInteractionsDataset(tr.interactions, number_of_users=N_USERS,
                                                number_of_items=N_ITEMS,
                                                user_features=feats(N_USERS),
                                                item_features=feats(N_ITEMS))
    model, opt = make_model("adam")
    seen = []
    real = ops.warp_fwd_bwd

    def spy(*a, **kw):
        out = real(*a, **kw)
        seen.append((a[2].cpu(), out[1].cpu()))
        assert a[5] is not None  # the exclusion CSR built from ``frozen``
        return out

    monkeypatch.setattr(train.utils.ops, "warp_fwd_bwd", spy)
    mean_loss, stats = train.warp_train_loop(datasets.PointWiseDataset(host), model,
                                             losses.WARPLoss(max_trials=20), opt, frozen=te,
                                             batch_size=256)
    assert len(seen) == 3 and np.isfinite(mean_loss) and stats["mean_trials"] >= 1.0
    barred = {(int(u), int(i)) for u, i in torch.cat([tr.interactions, te.interactions]).tolist()}
    for uid, neg in seen:
        assert not any((int(u), int(n)) in barred for u, n in zip(uid.tolist(), neg.tolist()))


def test_warp_train_loop_refuses_and_reports():
    tr, _ = planted_split()
    ds = datasets.DevicePointWiseDataset(tr, device=DEV)
    model, _ = make_model("feature")
    with pytest.raises(ValueError, match="SparseAdam"):
        train.warp_train_loop(ds, model, losses.WARPLoss(),
                              torch.optim.SparseAdam(list(model.parameters())))
    small = models.MatrixFactorization(N_USERS, N_ITEMS - 1, 32).to(DEV)
    with pytest.raises(ValueError, match="do not cover"):
        train.warp_train_loop(ds, small, losses.WARPLoss(), torch.optim.Adam(small.parameters()))

    class Stray:  # a loader whose ids leave the tables: counted, raised after the epoch
        data = tr

        def loader(self, **_):
            yield (torch.tensor([0, 1, N_USERS], device=DEV), torch.tensor([0, 1, 2], device=DEV))

    model, opt = make_model("sparse_adam")
    with pytest.raises(IndexError):
        train.warp_train_loop(Stray(), model, losses.WARPLoss(), opt)


def test_warp_train_loop_step_is_the_kernel_plus_adam():
    """One step of the loop = ops.warp_fwd_bwd on the same batch with the
    loop's seed, then oracle.adam_step (float64) within check_adam's bounds.
    The batch is one 16-pair span: one group adds every gradient in program
    order, so both runs' atomic sums are the same bits."""
    tr, _ = planted_split()
    sixteen = datasets.UserItemInteractionsDataset(tr.interactions[:16], number_of_users=N_USERS,
                                                   number_of_items=N_ITEMS)
    model, opt = make_model("adam")
    U0 = model.user_embeddings.weight.detach().clone()
    I0 = model.item_embeddings.weight.detach().clone()
    loss = losses.WARPLoss(margin=0.5, max_trials=30)
    ds = datasets.DevicePointWiseDataset(sixteen, device=DEV, by_row=True)
    mean_loss, stats = train.warp_train_loop(ds, model, loss, opt, seed=11, batch_size=16)
    pos = datasets.base_datasets._device_csr(sixteen, N_USERS, N_ITEMS, DEV)
    gU, gI = torch.zeros_like(U0), torch.zeros_like(I0)
    uid, pid = (sixteen.interactions[:, k].to(DEV) for k in (0, 1))
    lv, neg, trials = ops.warp_fwd_bwd(U0, I0, uid, pid, pos, None, 30, 0.5,
                                       warp_batch_seed(11, 0, 0), 0, 1.0 / 16, gU, gI)
    assert mean_loss == pytest.approx(float(lv.sum() / 16), rel=1e-6)
    assert stats["mean_trials"] == pytest.approx(float(trials.sum()) / 16)
    assert stats["no_violator"] == pytest.approx(float((neg < 0).sum()) / 16)
    assert gU.any() and gI.any()
    z = np.zeros_like
    for p, p0, g in ((model.user_embeddings.weight, U0, gU), (model.item_embeddings.weight, I0, gI)):
        st = opt.state[p]
        p0n, gn = p0.cpu().numpy(), g.cpu().numpy()
        check_adam((p.detach().cpu().numpy(), st["exp_avg"].cpu().numpy(),
                    st["exp_avg_sq"].cpu().numpy()),
                   adam_ref(p0n, gn, z(p0n), z(p0n), 1, lr=0.05), what="loop step")
        assert int(st["step"].item()) == 1
