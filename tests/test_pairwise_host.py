"""Pairwise training and ranking metrics, host side: the float64 restatements
of tests/pairwise_checks.py against the reference's fixtures; the argument
checks of dr_bpr_fwd_bwd, dr_adam_dense, dr_adam_rows, dr_rank_metrics,
dr_catalog_histogram and dr_sample_pairwise (they run before any HIP call);
and, for every assertion helper that tests/test_pairwise_gpu.py applies to a
kernel, that an fp32 emulation of the kernel's operation order passes it and a
deliberately wrong output does not. No GPU."""
import ctypes

import numpy as np
import pytest

from divrec import _backend
from pairwise_checks import (ADAM_CASES, ADAM_SIZES, BPR_WIDTHS, F, LOG2, adam_emulate_f32,
                             adam_inputs, adam_ref, bpr_case, bpr_emulate_f32,
                             bpr_runs_case, bpr_step_f64, check_adam, check_bpr, check_rank, csr,
                             load, rank_case, rank_emulate_f32, rank_metrics_f64)


# --------------------------------------------------------------------------- restatements
def test_bpr_restatement_reproduces_the_reference_step():
    """bpr_step_f64 against what the reference's forward, loss, AUCScore and
    autograd gave (fp32), at test_oracle_golden.test_bpr_step's tolerances."""
    g = load("bpr_step")
    B = g["uid"].size
    sp, sn, loss, gU, gI, margin = bpr_step_f64(g["U0"], g["I0"], g["uid"], g["pid"], g["nid"],
                                                1.0 / B)
    assert loss.sum() / B == pytest.approx(float(g["loss"]), rel=1e-6)
    assert np.mean(sp >= sn) == pytest.approx(float(g["auc"]), abs=1e-7)
    assert np.allclose(gU, g["gU"], rtol=1e-5, atol=1e-8)
    assert np.allclose(gI, g["gI"], rtol=1e-5, atol=1e-8)
    # no flag of the fixture is in doubt but those of triples with pid == nid
    assert (margin > 0).all() and ((np.abs(sp - sn) > margin) | (g["pid"] == g["nid"])).all()
    assert not gU[np.setdiff1d(np.arange(30), g["uid"])].any()


def test_bpr_restatement_skips_bad_ids():
    U, I = np.ones((3, 4), F), np.ones((5, 4), F)
    I[2] = 2.0
    uid, pid, nid = [0, -1, 2, 1, 3, 1], [2, 0, 5, 1, 0, -1], [0, 0, 1, 5, 0, 0]
    sp, sn, loss, gU, gI, margin = bpr_step_f64(U, I, uid, pid, nid, 1.0)
    assert np.isnan(loss[1:]).all() and np.isnan(sp[1:]).all() and np.isnan(margin[1:]).all()
    assert sp[0] == 8.0 and sn[0] == 4.0
    assert loss[0] == pytest.approx(np.log1p(np.exp(-4.0)), rel=1e-12)
    s = 1.0 / (1.0 + np.exp(4.0))  # sigmoid(-x): the one valid triple's weight
    assert np.allclose(gU, [[-s] * 4, [0] * 4, [0] * 4], rtol=1e-12)
    assert np.allclose(gI[[0, 2]], [[s] * 4, [-s] * 4], rtol=1e-12) and not gI[[1, 3, 4]].any()
    # every id valid but pid == nid: x = 0, loss log 2, no user gradient
    sp, sn, loss, gU, gI, _ = bpr_step_f64(U, I, [1], [2], [2], 1.0)
    assert loss[0] == pytest.approx(LOG2, rel=1e-12) and not gU.any() and not gI.any()


def positives_of(inter, n_users):
    """interactions [N, 2] -> CSR as metrics._rank.positives_csr builds it."""
    return csr([inter[inter[:, 0] == u, 1] for u in range(n_users)])


@pytest.mark.parametrize("name", ["ml100k_d100", "ml100k_cfg1"])
def test_rank_restatement_reproduces_the_reference_metrics(name):
    g = load(name)
    recs = g["recs"]
    got = rank_metrics_f64(recs, *positives_of(g["test"], recs.shape[0]))
    for mine, key in zip(got, ("precision", "recall", "ap", "ndcg")):
        assert np.allclose(mine, g[key], rtol=1e-6, atol=1e-7, equal_nan=True), key
    assert got[0].max() > 0  # the fixture has hits at all


def test_rank_restatement_by_hand():
    recs = np.array([[5, 7, 9, 7], [1, 2, 3, 4], [-1, 0, (1 << 32) + 3, 3]])
    rowptr, items = csr([[7, 7, 9], [], [3, 0]])
    p, r, ap, nd = rank_metrics_f64(recs, rowptr, items)
    assert np.array_equal(p, [0.75, 0.0, 0.5])
    assert r[0] == 1.0 and np.isnan(r[1]) and r[2] == 1.0  # raw count 3: duplicates kept
    assert ap[0] == pytest.approx((0 + 1 / 2 + 2 / 3 + 3 / 4) / 4)
    disc = 1 / np.log2(np.arange(2, 6))
    assert nd[2] == pytest.approx((disc[1] + disc[3]) / disc.sum())
    assert ap[1] == 0.0 and nd[1] == 0.0


# --------------------------------------------------------------------------- C argument checks
ONE = ctypes.c_void_p(8)  # a non-NULL pointer the checks never dereference


def _fails(lib, rc, text):
    return rc == -1 and text in lib.dr_last_error()


def test_bpr_argument_errors_without_gpu():
    lib = _backend.load_library()

    def call(ut=ONE, nu=10, it=ONE, ni=10, d=64, uid=ONE, pid=ONE, nid=ONE, batch=3):
        return lib.dr_bpr_fwd_bwd(ut, nu, it, ni, d, uid, pid, nid, batch, 1.0, None, None, None,
                                  None, None, None)

    assert call(batch=0) == 0
    assert call(ut=None, it=None, uid=None, pid=None, nid=None, d=0, batch=0) == 0
    for bad in (dict(batch=-1), dict(nu=-1), dict(ni=-1)):
        assert _fails(lib, call(**bad), b"dr_bpr_fwd_bwd: sizes must be >= 0")
    for d in (0, 513, -4):
        assert _fails(lib, call(d=d), b"d must be in [1, 512]")
    for null in ("ut", "it", "uid", "pid", "nid"):
        assert _fails(lib, call(**{null: None}), b"dr_bpr_fwd_bwd: null pointer")


def test_adam_argument_errors_without_gpu():
    lib = _backend.load_library()

    def dense(p=ONE, g=ONE, m=ONE, v=ONE, n=5, step=1):
        return lib.dr_adam_dense(p, g, m, v, n, 1e-3, 0.9, 0.999, 1e-8, 0.0, step, None)

    assert dense(n=0) == 0 and dense(p=None, g=None, m=None, v=None, n=0) == 0
    for bad in (dict(n=-1), dict(step=0), dict(step=-3), dict(n=0, step=0)):
        assert _fails(lib, dense(**bad), b"dr_adam_dense: n must be >= 0 and step >= 1")
    for null in ("p", "g", "m", "v"):
        assert _fails(lib, dense(**{null: None}), b"dr_adam_dense: null pointer")

    def rows(p=ONE, g=ONE, m=ONE, v=ONE, d=8, r=ONE, n_rows=5, step=1, zero_grad=1):
        return lib.dr_adam_rows(p, g, m, v, d, r, n_rows, 1e-3, 0.9, 0.999, 1e-8, step, zero_grad,
                                None)

    assert rows(n_rows=0) == 0 and rows(p=None, g=None, m=None, v=None, r=None, n_rows=0) == 0
    for bad in (dict(n_rows=-1), dict(d=0), dict(step=0), dict(n_rows=0, d=0)):
        assert _fails(lib, rows(**bad), b"dr_adam_rows: n_rows must be >= 0, d >= 1, step >= 1")
    for null in ("p", "g", "m", "v", "r"):
        assert _fails(lib, rows(**{null: None}), b"dr_adam_rows: null pointer")


def test_rank_metrics_argument_errors_without_gpu():
    lib = _backend.load_library()

    def call(recs=ONE, dt=_backend.DR_I64, n=4, k=10, rowptr=ONE, items=ONE):
        return lib.dr_rank_metrics(recs, dt, n, k, rowptr, items, None, None, None, None, None)

    assert call(n=0) == 0 and call(recs=None, rowptr=None, items=None, n=0) == 0
    for k in (0, -1):
        assert _fails(lib, call(k=k), b"dr_rank_metrics: k must be >= 1")
        assert _fails(lib, call(k=k, n=0), b"k must be >= 1")  # before the empty-input return
    for dt in (_backend.DR_F32, _backend.DR_BF16, _backend.DR_F64, 9, -1):
        assert _fails(lib, call(dt=dt), b"rec_dtype must be DR_I32/DR_I64")
    for null in ("recs", "rowptr", "items"):
        for dt in (_backend.DR_I32, _backend.DR_I64):
            assert _fails(lib, call(dt=dt, **{null: None}), b"dr_rank_metrics: null pointer")


def test_catalog_histogram_argument_errors_without_gpu():
    lib = _backend.load_library()

    def call(recs=ONE, dt=_backend.DR_I32, n=4, k=10, n_items=100, counts=ONE, pos_sum=ONE):
        return lib.dr_catalog_histogram(recs, dt, n, k, n_items, counts, pos_sum, None)

    assert call(n=0) == 0 and call(recs=None, counts=None, pos_sum=None, n=0) == 0
    for bad in (dict(n=-1), dict(k=0), dict(k=-2), dict(n_items=0), dict(n_items=-5)):
        assert _fails(lib, call(**bad), b"dr_catalog_histogram: bad sizes")
    for dt in (_backend.DR_F32, _backend.DR_F64, 7):
        assert _fails(lib, call(dt=dt), b"recs must be int32 or int64")
    for null in ("recs", "counts"):
        assert _fails(lib, call(**{null: None}), b"dr_catalog_histogram: null pointer")
        assert _fails(lib, call(pos_sum=None, **{null: None}), b"null pointer")


def test_sample_pairwise_argument_errors_without_gpu():
    lib = _backend.load_library()

    def call(users=ONE, n=4, rowptr=ONE, items=ONE, er=None, ei=None, n_items=100, m=3, pos=ONE,
             neg=ONE, uid=None, pid=None, nid=None, err=ONE):
        return lib.dr_sample_pairwise(users, n, rowptr, items, er, ei, n_items, m, 5, pos, neg, uid,
                                      pid, nid, err, None)

    assert call(n=0) == 0 and call(n=0, er=ONE, ei=ONE, uid=ONE, pid=ONE, nid=ONE) == 0
    assert call(users=None, rowptr=None, items=None, pos=None, neg=None, err=None, n=0) == 0
    for bad in (dict(n=-1), dict(n_items=0), dict(n_items=-1), dict(n_items=2 ** 31 - 1),
                dict(n_items=2 ** 31), dict(n_items=2 ** 40)):
        assert _fails(lib, call(**bad), b"n_users >= 0 and 1 <= n_items < 2^31 required")
    assert call(n=0, n_items=2 ** 31 - 2) == 0  # the largest catalog
    for m in (0, -1, 65537):
        assert _fails(lib, call(m=m), b"m (max_sampled) must be in [1, 65536]")
    assert call(n=0, m=65536) == 0 and call(n=0, m=1) == 0
    for one_set in (dict(er=ONE), dict(ei=ONE)):
        assert _fails(lib, call(**one_set), b"excl_rowptr and excl_items must both be set")
        assert _fails(lib, call(n=0, **one_set), b"must both be set")
    for null in ("users", "rowptr", "items", "pos", "neg", "err"):
        assert _fails(lib, call(**{null: None}), b"dr_sample_pairwise: null pointer")
    for some in (dict(uid=ONE), dict(pid=ONE), dict(nid=ONE), dict(uid=ONE, pid=ONE),
                 dict(uid=ONE, nid=ONE), dict(pid=ONE, nid=ONE)):
        assert _fails(lib, call(**some), b"uid, pid and nid must all be set (expand) or all be NULL")


# --------------------------------------------------------------------------- BPR: inputs and teeth
def _bpr_inputs_hold(U, I, uid, pid, nid, cap, what):
    """The fp32 emulation passes check_bpr on these inputs; returns (triples
    inside the margin, how many of those have pid == nid)."""
    ref = bpr_step_f64(U, I, uid, pid, nid, 1.0 / len(uid))
    loss, hit = bpr_emulate_f32(U, I, uid, pid, nid)
    check_bpr((loss, hit, None, None), ref, pid, nid, cap=cap, what=what)
    inside = np.abs(ref[0] - ref[1]) <= ref[5]
    assert not (hit != (ref[0] >= ref[1]))[~inside].any()
    return int(inside.sum()), int((inside & (pid == nid)).sum())


@pytest.mark.parametrize("d", BPR_WIDTHS)
def test_bpr_inputs_leave_the_bounds_room(d):
    """The inputs test_pairwise_gpu.py gives every instance, through an fp32
    emulation of the kernel's lane-strided sum: every loss inside rtol 1e-5 /
    atol 1e-6, no flag differs outside the margin, and the margin leaves out
    9 to 19 of the 4096 triples (far below the 1 % cap), all but a few of them
    triples with pid == nid, which have their own exact assertion."""
    inside, same = _bpr_inputs_hold(*bpr_case(d), cap=0.01, what="emulation")
    assert 9 <= inside <= 19 and inside - same <= 2


def test_bpr_eight_element_inputs_leave_the_bounds_room():
    _bpr_inputs_hold(*bpr_case(256), cap=0.01, what="d=256 emulation")


def test_bpr_saturated_inputs_leave_the_bounds_room():
    """d = 32 with tables scaled by 3.0: |x| reaches about 260, where
    exp(-|x|) underflows to 0 and the loss is -x or 0."""
    U, I, uid, pid, nid = bpr_case(32, scale=3.0)
    sp, sn = bpr_step_f64(U, I, uid, pid, nid, 1.0)[:2]
    assert np.abs(sp - sn).max() > 250 and (sp - sn).min() < -200 and (sp - sn).max() > 200
    assert np.exp(-F(np.abs(sp - sn).max())) == 0  # past expf's underflow in fp32
    _bpr_inputs_hold(U, I, uid, pid, nid, cap=0.01, what="saturated emulation")


@pytest.mark.parametrize("B", [1, 15, 16, 17, 4097])
def test_bpr_batch_size_inputs_leave_the_bounds_room(B):
    _bpr_inputs_hold(*bpr_case(100, B=B, seed=B), cap=0.01, what="batch emulation")


def test_bpr_long_and_run_inputs_leave_the_bounds_room():
    _bpr_inputs_hold(*bpr_case(33, B=262145, nu=64, ni=200), cap=0.01, what="long emulation")
    U, I, uid, pid, nid = bpr_runs_case()
    assert (np.diff(uid[4000:6000]) == 0).all() and uid.size == 18000
    assert ((pid == nid) & (uid == uid[7 * 400])).any()
    _bpr_inputs_hold(U, I, uid, pid, nid, cap=0.01, what="runs emulation")


def test_bpr_checks_reject_wrong_kernels():
    """check_bpr on deliberately wrong outputs (in place of ever running a
    broken kernel): losses rotated by one slot, hit flags rotated by one slot,
    one 32-element slice of every row ignored (forward, then gradients alone),
    a flag written for an invalid triple."""
    d = 96
    U, I, uid, pid, nid = bpr_case(d)
    ref = bpr_step_f64(U, I, uid, pid, nid, 1.0 / 4096)
    loss, hit = bpr_emulate_f32(U, I, uid, pid, nid)
    gU, gI = ref[3].astype(F), ref[4].astype(F)
    check_bpr((loss, hit, gU, gI), ref, pid, nid)  # the correct output passes
    for wrong in ((np.roll(loss, 1), hit, gU, gI), (loss, np.roll(hit, 1), gU, gI)):
        with pytest.raises(AssertionError):
            check_bpr(wrong, ref, pid, nid)
    Uc, Ic = U.copy(), I.copy()
    Uc[:, 32:64] = 0  # the second of three slices never read
    cut = bpr_step_f64(Uc, Ic, uid, pid, nid, 1.0 / 4096)
    cut_loss, cut_hit = bpr_emulate_f32(Uc, Ic, uid, pid, nid)
    with pytest.raises(AssertionError):
        check_bpr((cut_loss, hit, gU, gI), ref, pid, nid)
    with pytest.raises(AssertionError):
        check_bpr((loss, cut_hit, gU, gI), ref, pid, nid)
    with pytest.raises(AssertionError):
        check_bpr((loss, hit, cut[3].astype(F), gI), ref, pid, nid)
    with pytest.raises(AssertionError):
        check_bpr((loss, hit, gU, cut[4].astype(F)), ref, pid, nid)
    # a slice of the gradient never added (the rows are read in full)
    miss = gI.copy()
    miss[:, 64:] = 0
    with pytest.raises(AssertionError):
        check_bpr((loss, hit, gU, miss), ref, pid, nid)
    # bad ids: the loss must be NaN and the flag 0 exactly there
    bad_uid = uid.copy()
    bad_uid[17] = 200
    ref_b = bpr_step_f64(U, I, bad_uid, pid, nid, 1.0 / 4096)
    loss_b, hit_b = loss.copy(), hit.copy()
    loss_b[17], hit_b[17] = np.nan, 0
    check_bpr((loss_b, hit_b, None, None), ref_b, pid, nid)
    with pytest.raises(AssertionError):
        check_bpr((loss, hit_b, None, None), ref_b, pid, nid)
    hit_b[17] = 1
    with pytest.raises(AssertionError):
        check_bpr((loss_b, hit_b, None, None), ref_b, pid, nid)
    # the cap is a condition: all triples alike leaves every flag in doubt
    with pytest.raises(AssertionError):
        check_bpr((np.full(8, LOG2, F), np.ones(8, np.int32), None, None),
                  bpr_step_f64(U, I, uid[:8], pid[:8], pid[:8], 1.0), pid[:8], pid[:8])


# --------------------------------------------------------------------------- rank metrics: teeth
def _rank_wrong(recs, rowptr, items, drop_carry=False, unmasked=False):
    """rank_metrics_f64 with one of the kernel's block-walk mistakes: the
    count of earlier hits lost at every 64-position block, or the last block
    not masked at k (it then reads on into the next user's list; past the
    last user, empty slots)."""
    n, k = recs.shape
    width = -(-k // 64) * 64 if unmasked else k
    flat = np.concatenate([recs.reshape(-1), np.full(64, -1)])
    out = np.zeros((4, n))
    for u in range(n):
        pos = items[rowptr[u]:rowptr[u + 1]].astype(np.int64)
        rel = np.isin(flat[u * k:u * k + width], pos).astype(np.float64)
        cum = np.cumsum(rel)
        if drop_carry:
            cum = np.concatenate([np.cumsum(rel[b:b + 64]) for b in range(0, width, 64)])
        disc = 1.0 / np.log2(np.arange(2, width + 2))
        hits = cum[-1]
        out[0, u] = hits / k
        out[1, u] = hits / len(pos) if len(pos) else np.nan
        out[2, u] = (cum / np.arange(1, width + 1)).sum() / k
        out[3, u] = (rel * disc).sum() / disc.sum()
    return tuple(out)


@pytest.mark.parametrize("k", [1, 63, 64, 65, 128, 129, 200, 1000])
def test_rank_emulation_passes_the_check(k):
    """The kernel's fp32 lane-strided sums are within 1.5e-7 of float64 for
    every list length of the GPU tests, a fiftieth of the AP / NDCG bound."""
    recs, rowptr, items = rank_case(k, 27)
    ref = rank_metrics_f64(recs, rowptr, items)
    got = rank_emulate_f32(recs, rowptr, items)
    check_rank(got, ref, what=f"emulation k={k}")
    for g, r in zip(got, ref):
        assert np.nanmax(np.abs(g - r)) <= 1.5e-7
    # the mutants' base, with neither mistake, is the restatement
    assert np.array_equal(np.array(_rank_wrong(recs, rowptr, items)), np.array(ref), equal_nan=True)


@pytest.mark.parametrize("k", [65, 128, 129, 200, 1000])
def test_rank_check_rejects_a_lost_carry(k):
    recs, rowptr, items = rank_case(k, 27)
    ref = rank_metrics_f64(recs, rowptr, items)
    wrong = _rank_wrong(recs, rowptr, items, drop_carry=True)
    assert np.nanmax(np.abs(wrong[2] - ref[2])) > 1e-2  # off by percents, not by roundings
    with pytest.raises(AssertionError):
        check_rank(wrong, ref)
    for i in (0, 1, 2):  # each of precision, recall and AP alone gives it away
        mixed = list(ref)
        mixed[i] = wrong[i]
        with pytest.raises(AssertionError):
            check_rank(mixed, ref)


@pytest.mark.parametrize("k", [1, 63, 65, 129, 200, 1000])
def test_rank_check_rejects_an_unmasked_last_block(k):
    """Positives that hold the NEXT user's first items: a block that runs past
    k counts them."""
    recs, rowptr, items = rank_case(k, 27)
    rows = [items[rowptr[u]:rowptr[u + 1]] for u in range(27)]
    for u in range(26):
        rows[u] = np.concatenate([rows[u], recs[u + 1, :5]])
    rowptr, items = csr(rows)
    ref = rank_metrics_f64(recs, rowptr, items)
    with pytest.raises(AssertionError):
        check_rank(_rank_wrong(recs, rowptr, items, unmasked=True), ref)
    # without any stray hit the ideal DCG alone (summed past k) gives it away
    recs, rowptr, items = rank_case(k, 27)
    wrong = _rank_wrong(recs, rowptr, items, unmasked=True)
    with pytest.raises(AssertionError):
        check_rank(wrong, rank_metrics_f64(recs, rowptr, items))


def test_rank_check_rejects_a_truncating_compare_and_nan_mistakes():
    recs = np.array([[(1 << 32) + 3, 5, -1, 8]])
    rowptr, items = csr([[3, 8]])
    ref = rank_metrics_f64(recs, rowptr, items)
    assert ref[0][0] == 0.25
    trunc = rank_metrics_f64(recs & 0xFFFFFFFF, rowptr, items)
    with pytest.raises(AssertionError):
        check_rank(trunc, ref)
    # recall of a user without positives must be NaN, and only there
    empty = rank_metrics_f64(recs, *csr([[]]))
    assert np.isnan(empty[1][0])
    with pytest.raises(AssertionError):
        check_rank((empty[0], np.zeros(1), empty[2], empty[3]), empty)
    with pytest.raises(AssertionError):
        check_rank((ref[0], np.full(1, np.nan), ref[2], ref[3]), ref)


# --------------------------------------------------------------------------- Adam: teeth
@pytest.mark.parametrize("beta1,beta2,wd", ADAM_CASES)
@pytest.mark.parametrize("n", ADAM_SIZES)
def test_adam_emulation_passes_the_check_and_mutants_fail(n, beta1, beta2, wd):
    """An fp32 numpy emulation of adam_kernel's operation sequence is inside
    check_adam's bounds (three chained steps and step 1000 from given
    moments); an update scaled by 1.001 and swapped moments are not."""
    hp = dict(lr=1e-3, beta1=beta1, beta2=beta2, eps=1e-8, wd=wd)
    p, grads, m_late, v_late = adam_inputs(n, n)
    m, v = np.zeros(n, F), np.zeros(n, F)
    steps = [(s, g) for s, g in enumerate(grads, 1)] + [(1000, grads[0])]
    for step, g in steps:
        if step == 1000:
            m, v = m_late, v_late
        ref = adam_ref(p, g, m, v, step, **hp)
        got = adam_emulate_f32(p, g, m, v, step, **hp)
        check_adam(got, ref, what=f"emulation {beta1} {beta2} {wd} step {step}")
        scaled = (p + (got[0] - p) * F(1.001), got[1], got[2])
        swapped = (got[0], got[2], got[1])
        for wrong in (scaled, swapped):
            with pytest.raises(AssertionError):
                check_adam(wrong, ref)
        if n > 1:  # one element alone wrong, in each output
            for i in range(3):
                wrong = [a.copy() for a in got]
                wrong[i][n // 2] *= F(1.001)
                with pytest.raises(AssertionError):
                    check_adam(wrong, ref)
        p, m, v = got


def test_adam_emulation_takes_both_lerp_branches():
    p, g = np.ones(4, F), np.full(4, 0.5, F)
    m, v = np.full(4, 0.25, F), np.ones(4, F)
    for beta1 in (0.9, 0.5, 0.3):
        got = adam_emulate_f32(p, g, m, v, 5, beta1=beta1)
        assert np.allclose(got[1], beta1 * 0.25 + (1 - beta1) * 0.5, rtol=1e-6)
