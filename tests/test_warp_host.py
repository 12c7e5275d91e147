"""WARP step, host side (no GPU): the library's candidate stream against the
numpy restatement of the draw hash; check_warp (tests/warp_checks.py) shown to
admit the fp32 emulation of the kernel and to reject each of six broken
kernels; the undecided share of the GPU tests' inputs; dr_warp_fwd_bwd's
argument checks (they run before any HIP call); WARPLoss on CPU tensors; and
warp_train_loop's refusals."""
import ctypes

import numpy as np
import pytest
import torch

from divrec import _backend, losses, models, ops, train
from warp_checks import (BUGS, UNDECIDED_CAP, WARP_WIDTHS, candidates, check_warp, warp_case,
                         warp_emulate_f32, warp_ref, warp_step_f64)


# --------------------------------------------------------------------------- the draw hash
@pytest.mark.parametrize("n_items", [1, 2, 300, 1_000_003, 2 ** 31 - 2])
def test_candidates_equal_the_numpy_restatement(n_items):
    for seed, base in ((0, 0), (1, 7), (2 ** 64 - 1, 2 ** 40 + 3), (0x123456789ABCDEF, 4096)):
        got = ops.warp_candidates(seed, base, 37, 19, n_items)
        assert got.dtype == torch.int32 and got.shape == (37, 19) and got.device.type == "cpu"
        ref = candidates(seed, base, 37, 19, n_items)
        assert np.array_equal(got.numpy().astype(np.int64), ref)
        assert ref.min() >= 0 and ref.max() < n_items
    # pair b of a call at pair_base k is pair k + b of a call at 0
    whole = ops.warp_candidates(5, 0, 40, 8, n_items)
    assert torch.equal(ops.warp_candidates(5, 25, 15, 8, n_items), whole[25:])


def test_candidates_argument_errors():
    lib = _backend.load_library()
    out = (ctypes.c_int32 * 4)()
    assert lib.dr_warp_candidates(1, 0, 0, 4, 10, None) == 0  # no pairs: no-op
    for args, msg in (((1, 0, 1, 0, 10, out), b"max_trials"), ((1, 0, 1, 4097, 10, out), b"max_trials"),
                      ((1, 0, 1, 4, 0, out), b"n_items"), ((1, 0, 1, 4, 2 ** 31 - 1, out), b"n_items"),
                      ((1, -1, 1, 4, 10, out), b"pair_base"), ((1, 0, 1, 4, 10, None), b"null pointer")):
        assert lib.dr_warp_candidates(*args) == -1 and msg in lib.dr_last_error(), args
    assert lib.dr_warp_round() >= 1


# --------------------------------------------------------------------------- check_warp
CASES = [(d, regime, exclude) for d in WARP_WIDTHS for regime in ("random", "planted")
         for exclude in (False, True)]


@pytest.mark.parametrize("d,regime,exclude", CASES)
def test_check_warp_admits_the_fp32_emulation(d, regime, exclude):
    """The kernel's operation order in numpy fp32 passes every bound, on the
    inputs the GPU test runs; their undecided share is under the cap, and the
    planted regime reaches long runs and pairs without a violator."""
    case, ref = warp_ref(d, regime, exclude)
    share = check_warp(warp_emulate_f32(case), ref, what=f"emulation {regime} excl={exclude}")
    assert share <= UNDECIDED_CAP
    if regime == "planted":  # long runs, and pairs that use up every trial
        assert (ref["neg"] < 0).mean() >= 0.005 and len(np.unique(ref["trials"])) >= 28
        assert ref["trials"].mean() > warp_ref(d, "random", exclude)[1]["trials"].mean()


# the random regime has no pair without a violator to leave a gradient on
@pytest.mark.parametrize("bug,regime", [(b, r) for b in BUGS for r in ("random", "planted")
                                        if (b, r) != ("gradient_without_violator", "random")])
def test_check_warp_rejects_a_broken_kernel(bug, regime):
    case, ref = warp_ref(100, regime, True)
    with pytest.raises(AssertionError):
        check_warp(warp_emulate_f32(case, bug=bug), ref, what=bug)


def test_check_warp_rejects_wrong_invalid_pairs_and_an_impossible_undecided_outcome():
    case = dict(warp_case(64, "planted"))
    case["uid"] = case["uid"].copy()
    case["uid"][[5, 700]] = [-1, 200]
    ref = warp_step_f64(case)
    assert not ref["valid"][[5, 700]].any() and np.isnan(ref["loss"][[5, 700]]).all()
    good = warp_emulate_f32(case)
    check_warp(good, ref)
    for field, value in ((0, 0.0), (1, 3), (2, 1)):  # loss not NaN, a neg, a trial count
        bad = [np.array(a, copy=True) for a in good]
        bad[field][5] = value
        with pytest.raises(AssertionError):
            check_warp(tuple(bad), ref)
    # an undecided pair may stop elsewhere, but only at a draw that was made and scored
    forged = dict(ref, undecided=ref["undecided"].copy())
    b = int(np.flatnonzero(ref["valid"] & (ref["neg"] >= 0))[0])
    forged["undecided"][b] = True
    bad = [np.array(a, copy=True) for a in good]
    bad[1][b] = (bad[1][b] + 1) % 300  # not the candidate of its trial
    with pytest.raises(AssertionError):
        check_warp(tuple(bad), forged)


def test_restatement_edges():
    """log 1 = 0 once (n_items - 1) // trials <= 1; a positive, an excluded
    item and the pair's own positive are never violators; the split of a
    batch at pair_base gives the whole call's outcome."""
    case, ref = warp_ref(100, "planted", True)
    cand = candidates(case["seed"], 0, 4096, 32, 300)
    has = ref["neg"] >= 0
    assert np.array_equal(cand[has, ref["trials"][has] - 1], ref["neg"][has])
    for csr_ in (case["pos"], case["excl"]):
        rowptr, items = csr_
        for b in np.flatnonzero(has)[:500]:
            u = case["uid"][b]
            assert ref["neg"][b] not in items[rowptr[u]:rowptr[u + 1]]
    assert (ref["neg"] != case["pid"]).all()
    half = dict(case, uid=case["uid"][2048:], pid=case["pid"][2048:], pair_base=2048)
    r2 = warp_step_f64(half)
    assert np.array_equal(r2["neg"], ref["neg"][2048:])
    assert np.array_equal(r2["trials"], ref["trials"][2048:])
    small = dict(warp_case(32), I=case["I"][:8, :32].copy(), pos=None, max_trials=16)
    small["pid"] = small["pid"] % 8
    r = warp_step_f64(small)
    late = r["trials"] >= 4
    assert late.any() and (r["loss"][late] == 0).all()


# --------------------------------------------------------------------------- the C ABI
def test_warp_argument_errors_without_gpu():
    lib = _backend.load_library()

    def call(batch=4, d=64, max_trials=10, pr=1, pi=1, er=None, ei=None, margin=1.0, base=0,
             tables=1):
        return lib.dr_warp_fwd_bwd(tables or None, 10, tables or None, 20, d, 1, 1, batch, pr, pi,
                                   er, ei, max_trials, margin, 7, base, 1.0, None, None, None,
                                   None, None, None, None)

    def fails(rc, msg):
        return rc == -1 and msg in lib.dr_last_error()

    assert fails(call(max_trials=0), b"max_trials must be in [1, 4096]")
    assert fails(call(max_trials=4097), b"max_trials must be in [1, 4096]")
    assert fails(call(d=513), b"d must be in [1, 512]") and fails(call(d=0), b"d must be")
    assert fails(call(pr=None), b"pos_rowptr and pos_items")
    assert fails(call(pi=None), b"pos_rowptr and pos_items")
    assert fails(call(er=1), b"excl_rowptr and excl_items")
    assert fails(call(ei=1), b"excl_rowptr and excl_items")
    assert fails(call(margin=float("inf")), b"margin must be finite")
    assert fails(call(margin=float("nan")), b"margin must be finite")
    assert fails(call(base=-1), b"pair_base")
    assert fails(call(batch=-1), b"sizes must be >= 0")
    assert fails(call(tables=0), b"null pointer")
    assert call(batch=0) == 0 and call(batch=0, tables=0, pr=None, pi=None) == 0  # a no-op
    assert fails(call(batch=0, max_trials=0), b"max_trials")  # settings are checked first


def test_warp_header_and_table_agree():
    res, args = _backend.SIGNATURES["dr_warp_fwd_bwd"]
    assert res is ctypes.c_int and len(args) == 24
    assert args[14] is ctypes.c_uint64 and args[13] is ctypes.c_float
    assert ops.WARP_MAX_TRIALS == 4096


# --------------------------------------------------------------------------- Python doors
def test_warp_loss_pair_wise_is_the_hinge():
    pos = torch.tensor([2.0, 0.5, 1.0, -1.0])
    neg = torch.tensor([0.5, 0.5, 0.0, 1.0])
    loss = losses.WARPLoss()
    assert (loss.margin, loss.max_trials) == (1.0, 100)
    assert isinstance(loss, losses.PairWiseLoss) and "WARPLoss" in losses.__all__
    assert torch.equal(loss.pair_wise(pos, neg), torch.tensor([0.0, 1.0, 0.0, 3.0]))
    assert float(loss(pos, neg)) == pytest.approx(1.0)
    wide = losses.WARPLoss(margin=0.25, max_trials=7, reduction="sum")
    assert (wide.margin, wide.max_trials) == (0.25, 7)
    assert float(wide(pos, neg)) == pytest.approx(0.25 + 2.25)
    assert losses.WARPLoss(reduction="none")(pos, neg).shape == (4,)
    for bad in (dict(margin=float("nan")), dict(max_trials=0)):
        with pytest.raises(ValueError):
            losses.WARPLoss(**bad)


def test_warp_train_loop_refusals():
    assert "warp_train_loop" in train.__all__
    opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=0.1)
    with pytest.raises(TypeError, match="MatrixFactorization"):
        train.warp_train_loop(None, models.RandomModel(4, 5), losses.WARPLoss(), opt)
    mf = models.MatrixFactorization(4, 5, 8)
    with pytest.raises(TypeError, match="WARPLoss"):
        train.warp_train_loop(None, mf, losses.LogSigmoidDifferenceLoss(), opt)


def test_warp_batch_seeds_differ_and_are_reproducible():
    from divrec.train.utils import warp_batch_seed

    seeds = {warp_batch_seed(s, e, k) for s in (0, 1) for e in (0, 1, 2) for k in range(50)}
    assert len(seeds) == 300 and all(0 <= s < 2 ** 64 for s in seeds)
    assert warp_batch_seed(3, 1, 2) == warp_batch_seed(3, 1, 2)
