"""Pairwise training and ranking-metric kernels on the GPU: bpr_kernel (every
instance), adam_kernel, adam_rows_kernel, rank_metrics_kernel,
catalog_hist_kernel and the sampler's draw / expand kernels, each against a
plain reference at the shapes where it takes another path.

The references and the assertion helpers are tests/pairwise_checks.py's; the
host file (tests/test_pairwise_host.py) pins the references to the reference
project's fixtures, shows on the CPU that an fp32 emulation of each kernel's
operation order passes every helper on these very inputs, and that the wrong
outputs a broken kernel would give (a lost carry, an unmasked last block,
rotated losses, an ignored row slice, an update scaled by 1.001, swapped
moments) do not.

Bounds: BPR per-triple loss rtol 1e-5 / atol 1e-6, gradients rtol 1e-4 / atol
1e-7, hit flags exact outside the fp32 margin of sp - sn (at most 1 % of the
triples inside it); dense Adam within the rounding bounds of
pairwise_checks.adam_ref; row-sparse Adam, the histogram and the sampler
exact; precision / recall rel 1e-6, AP / NDCG rel 1e-5 / abs 1e-7.

Not covered: user ids outside the positives CSR given to sample_pairwise.
The kernel does not guard them (the caller builds both), and passing one
would read out of bounds."""
import functools

import numpy as np
import pytest
import torch

import oracle
from divrec import _backend, ops
from pairwise_checks import (ADAM_CASES, ADAM_SIZES, BPR_WIDTHS, F, adam_inputs, adam_ref,
                             bpr_case, bpr_runs_case, bpr_step_f64, check_adam, check_bpr,
                             check_rank, csr, rank_case, rank_metrics_f64)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype=dtype)


def host(*ts):
    return tuple(None if t is None else t.cpu().numpy() for t in ts)


# --------------------------------------------------------------------------- BPR
def run_bpr(U, I, uid, pid, nid, grad_scale, grads="ui", **kw):
    """ops.bpr_fwd_bwd on numpy inputs -> numpy (loss, hit, grad_user, grad_item);
    ``grads`` names the gradient tables asked for."""
    Ut, It = dev(U), dev(I)
    gU = torch.zeros_like(Ut) if "u" in grads else None
    gI = torch.zeros_like(It) if "i" in grads else None
    loss, hit = ops.bpr_fwd_bwd(Ut, It, dev(uid), dev(pid), dev(nid), grad_scale, gU, gI, **kw)
    assert torch.equal(Ut, dev(U)) and torch.equal(It, dev(I))  # the tables are inputs only
    return host(loss, hit, gU, gI)


def bpr_against_f64(case, what, **kw):
    U, I, uid, pid, nid = case
    got = run_bpr(U, I, uid, pid, nid, 1.0 / len(uid), **kw)
    ref = bpr_step_f64(U, I, uid, pid, nid, 1.0 / len(uid))
    check_bpr(got, ref, pid, nid, cap=0.01, what=what)
    return got, ref


@pytest.mark.parametrize("d", BPR_WIDTHS)
def test_bpr_every_instance(d):
    """E = 1 (d = 1, 31, 32), 2 with a masked tail (33), 2, 3, 5, 6, 7 (64 to
    224), the 12-element instance at its first width, with a tail and full
    (257, 300, 384), and the 16-element one at its first width and full (385,
    512): per-triple loss, both gradients and every hit flag."""
    bpr_against_f64(bpr_case(d), f"instance d={d}")


def test_bpr_eight_element_instance():
    """d = 256, E = 8: the instance no width of BPR_WIDTHS reaches (E = 4 runs
    at d = 100 below)."""
    bpr_against_f64(bpr_case(256), "instance d=256")


def test_bpr_saturated_scores():
    """|x| up to about 260: exp(-|x|) underflows, the loss is -x or 0 and the
    gradient weight 1 or 0; nothing becomes NaN or Inf."""
    got, _ = bpr_against_f64(bpr_case(32, scale=3.0), "saturated")
    assert all(np.isfinite(a).all() for a in got)
    assert got[0].max() > 200 and (got[0] == 0).any()


@pytest.mark.parametrize("B", [1, 15, 16, 17, 4097])
def test_bpr_batch_sizes(B):
    """One triple, one short of a span, a span, a span plus one, and a last
    group with a single triple."""
    bpr_against_f64(bpr_case(100, B=B, seed=B), f"batch {B}")


def test_bpr_long_batch_with_a_short_last_span():
    """262145 triples: spans of 17, the last group holds 5."""
    bpr_against_f64(bpr_case(33, B=262145, nu=64, ni=200), "long batch")


def test_bpr_runs_flush_into_one_row():
    """The m x m layout with one user held for 2000 triples and an item that
    is a positive run and a negative of the same user."""
    bpr_against_f64(bpr_runs_case(), "runs")


def test_bpr_null_outputs():
    """Gradient tables None (both, each one alone) and, through the C call,
    loss, hit or err NULL: what is written equals the training call's, loss
    and hit bit for bit, and nothing else is touched."""
    U, I, uid, pid, nid = bpr_case(100, seed=21)
    B = len(uid)
    full = run_bpr(U, I, uid, pid, nid, 1.0 / B)
    ref = bpr_step_f64(U, I, uid, pid, nid, 1.0 / B)
    check_bpr(full, ref, pid, nid, what="training call")
    for grads in ("", "u", "i"):
        got = run_bpr(U, I, uid, pid, nid, 1.0 / B, grads=grads)
        assert np.array_equal(got[0], full[0]) and np.array_equal(got[1], full[1])
        check_bpr(got, ref, pid, nid, what=f"grads '{grads}'")
        for g, f in zip(got[2:], full[2:]):
            assert g is None or np.allclose(g, f, rtol=1e-4, atol=1e-7)
    lib = _backend.lib()
    Ut, It, ids = dev(U), dev(I), [dev(a) for a in (uid, pid, nid)]
    for skip in ("loss", "hit", "err"):
        loss = torch.full((B,), -7.0, device=DEV)
        hit = torch.full((B,), -7, dtype=torch.int32, device=DEV)
        err = _backend.error_counter(DEV)
        gU, gI = torch.zeros_like(Ut), torch.zeros_like(It)
        out = dict(loss=loss, hit=hit, err=err)
        out[skip] = None
        rc = lib.dr_bpr_fwd_bwd(Ut.data_ptr(), 200, It.data_ptr(), 300, 100,
                                *(t.data_ptr() for t in ids), B, 1.0 / B, _backend.ptr(out["loss"]),
                                _backend.ptr(out["hit"]), gU.data_ptr(), gI.data_ptr(),
                                _backend.ptr(out["err"]), _backend.stream(DEV))
        assert rc == 0
        l, h, u, i = host(loss, hit, gU, gI)
        assert np.array_equal(l, full[0]) if skip != "loss" else (l == -7).all()
        assert np.array_equal(h, full[1]) if skip != "hit" else (h == -7).all()
        assert np.allclose(u, ref[3], rtol=1e-4, atol=1e-7)
        assert np.allclose(i, ref[4], rtol=1e-4, atol=1e-7)
        assert int(err.item()) == 0
        assert torch.equal(Ut, dev(U)) and torch.equal(It, dev(I))


def _bad_id_cases():
    """-1 and n in each id column: at the first and last triple of a span, at
    the first and last triple of the batch, two bad ids in one triple (counted
    once), and inside runs of the m x m layout."""
    U, I, uid, pid, nid = (a.copy() for a in bpr_case(100, seed=33))  # spans of 16
    uid[0], uid[31] = -1, 200
    pid[32], pid[47] = 300, -1
    nid[4080], nid[4095] = -1, 300
    uid[100], nid[100] = 200, -1
    yield "spans", (U, I, uid, pid, nid), 7
    U, I, uid, pid, nid = (a.copy() for a in bpr_runs_case())  # 400 triples per user
    pid[5 * 400 + 7] = 403       # inside a positive run of 20
    nid[6 * 400 + 45] = -1
    uid[4100:4103] = [50, -1, 50]  # inside the user held for 2000 triples
    yield "runs", (U, I, uid, pid, nid), 5


@pytest.mark.parametrize("name,case,n_bad", list(_bad_id_cases()), ids=["spans", "runs"])
def test_bpr_bad_ids_are_skipped_and_counted(name, case, n_bad):
    err = _backend.error_counter(DEV)
    got, ref = bpr_against_f64(case, f"bad ids, {name}", err=err)
    assert int(err.item()) == n_bad == int(np.isnan(ref[2]).sum())
    assert np.isnan(got[0]).sum() == n_bad and not got[1][np.isnan(got[0])].any()
    again = _backend.error_counter(DEV)
    run_bpr(*case, 1.0 / len(case[2]), err=again, check=False)  # counted with check=False too
    assert int(again.item()) == n_bad
    with pytest.raises(IndexError):
        run_bpr(*case, 1.0 / len(case[2]))  # check=True, no err: raises


def test_bpr_wrapper_validates_tables_and_gradients():
    """ops.bpr_fwd_bwd raises ValueError before any launch for tables of
    different width, non-contiguous or non-2-D tables and gradient tables that
    are not contiguous fp32 tensors of their table's shape. Every input here
    would keep even a wrapper without these checks inside its allocations."""
    rng = np.random.default_rng(5)
    U, I = dev(rng.standard_normal((200, 64)).astype(F)), dev(rng.standard_normal((300, 64)).astype(F))
    uid, pid, nid = (dev(rng.integers(0, 150, 64)) for _ in range(3))
    zero = torch.zeros_like(uid)

    def raises(match, *a):
        with pytest.raises(ValueError, match=match):
            ops.bpr_fwd_bwd(*a)

    narrow = dev(rng.standard_normal((300, 32)).astype(F))  # read at stride 64: rows < 150 stay inside
    raises("embedding_dim", U, narrow, uid, pid, nid, 1.0, None, None)
    raises("embedding_dim", narrow, I, uid, pid, nid, 1.0, None, None)
    wide = dev(rng.standard_normal((300, 128)).astype(F))
    raises("contiguous", wide[:200, :64], I, uid, pid, nid, 1.0, None, None)
    raises("contiguous", U, wide[:, 64:], uid, pid, nid, 1.0, None, None)
    raises("2-D", U[None], I[None], zero, zero, zero, 1.0, None, None)
    raises("2-D", U, I.reshape(-1), zero, zero, zero, 1.0, None, None)
    gU, gI = torch.zeros_like(U), torch.zeros_like(I)
    for bad in (torch.zeros(201, 64, device=DEV), torch.zeros(200, 64, dtype=torch.float64, device=DEV),
                torch.zeros(200, 128, device=DEV)[:, :64], torch.zeros(200 * 64, device=DEV)):
        raises("grad_user", U, I, uid, pid, nid, 1.0, bad, gI)
        assert not bad.any() and not gI.any()
    for bad in (torch.zeros(301, 64, device=DEV), torch.zeros(300, 64, dtype=torch.float64, device=DEV),
                torch.zeros(300, 128, device=DEV)[:, 64:], torch.zeros(64, 300, device=DEV).t()):
        raises("grad_item", U, I, uid, pid, nid, 1.0, gU, bad)
        assert not bad.any() and not gU.any()
    loss, hit = ops.bpr_fwd_bwd(U, I, uid, pid, nid, 1.0, gU, gI)  # the valid call still runs
    assert gU.any() and gI.any() and loss.numel() == 64


# --------------------------------------------------------------------------- dense Adam
@pytest.mark.parametrize("beta1,beta2,wd", ADAM_CASES)
@pytest.mark.parametrize("n", ADAM_SIZES)
def test_adam_dense_against_float64(n, beta1, beta2, wd):
    """Three chained steps from zero moments, then step 1000 from given
    moments; each step against oracle.adam_step (float64) of the state the
    kernel itself started the step from: param, exp_avg and exp_avg_sq of
    every element. beta1 = 0.3 takes the lerp's other branch; the largest n
    runs the grid-stride loop."""
    hp = dict(lr=1e-3, beta1=beta1, beta2=beta2, eps=1e-8, wd=wd)
    p0, grads, m_late, v_late = adam_inputs(n, n)
    p, m, v = dev(p0), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    for step, g in [(s, g) for s, g in enumerate(grads, 1)] + [(1000, grads[0])]:
        if step == 1000:
            m, v = dev(m_late), dev(v_late)
        before = host(p, m, v)
        gd = dev(g)
        ops.adam_dense(p, gd, m, v, 1e-3, beta1, beta2, 1e-8, wd, step)
        assert torch.equal(gd, dev(g))  # the gradient is an input only
        check_adam(host(p, m, v), adam_ref(before[0], g, before[1], before[2], step, **hp),
                   what=f"adam {beta1} {beta2} {wd} step {step}")


# --------------------------------------------------------------------------- row-sparse Adam
@pytest.mark.parametrize("n,d,n_rows", [(4200, 256, 4100), (500, 1, 137), (500, 100, 137)],
                         ids=["stride-loop", "d1", "d100"])
@pytest.mark.parametrize("zero_grad", [True, False])
def test_adam_rows_bit_exact(n, d, n_rows, zero_grad):
    """dr_adam_rows against oracle.sparse_adam_rows, bit for bit, over three
    steps with different row sets (int32 ids on the second step), with and
    without zeroing the touched gradient rows; rows not listed keep all four
    tables' values."""
    rng = np.random.default_rng(n + d)
    lr, betas, eps = 3e-3, (0.85, 0.995), 1e-7
    P0 = rng.standard_normal((n, d)).astype(F)
    oP, oM, oV = P0.copy(), np.zeros_like(P0), np.zeros_like(P0)
    P, M, V = dev(P0), torch.zeros(n, d, device=DEV), torch.zeros(n, d, device=DEV)
    for t in (1, 2, 3):
        rows = rng.choice(n, size=n_rows, replace=False).astype(np.int64)
        G0 = (rng.standard_normal((n, d)) * 0.1).astype(F)  # unlisted rows hold values too
        G = dev(G0)
        keep = np.setdiff1d(np.arange(n), rows)
        prev = host(P, M, V)
        oracle.sparse_adam_rows(oP, oM, oV, rows, G0[rows], t, lr, *betas, eps)
        ops.adam_rows(P, G, M, V, dev(rows, torch.int32 if t == 2 else None), lr, *betas, eps, t,
                      zero_grad=zero_grad)
        gP, gM, gV, gG = host(P, M, V, G)
        assert np.array_equal(gP, oP) and np.array_equal(gM, oM) and np.array_equal(gV, oV)
        for now, was in zip((gP, gM, gV, gG), prev + (G0,)):
            assert np.array_equal(now[keep], was[keep])
        assert not gG[rows].any() if zero_grad else np.array_equal(gG[rows], G0[rows])
        assert not np.array_equal(gP[rows], prev[0][rows])
    empty = torch.zeros(0, dtype=torch.int64, device=DEV)
    ops.adam_rows(P, G, M, V, empty, lr, *betas, eps, 4, zero_grad=zero_grad)
    assert all(np.array_equal(a, b) for a, b in zip(host(P, M, V, G), (gP, gM, gV, gG)))


# --------------------------------------------------------------------------- rank metrics
@functools.lru_cache(maxsize=None)
def _rank_reference(k, n_users):
    case = rank_case(k, n_users)
    return case, rank_metrics_f64(*case)


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64], ids=["int32", "int64"])
@pytest.mark.parametrize("n_users", [1, 5, 203])
@pytest.mark.parametrize("k", [1, 63, 64, 65, 128, 129, 200, 1000])
def test_rank_metrics_against_float64(k, n_users, dtype):
    """Lists of one block, exactly one and two blocks, and a partial last
    block (the carry of earlier hits, the second ballot, the p < k mask);
    user counts that leave waves of the last workgroup idle; positives rows of
    0, 1 and 5000 entries; all hits before or after position 64, everywhere,
    nowhere, and at positions 63, 64 and k - 1 alone."""
    (recs, rowptr, items), ref = _rank_reference(k, n_users)
    got = ops.rank_metrics(dev(recs, dtype), dev(rowptr), dev(items))
    check_rank(host(*got), ref, what=f"k={k} n={n_users} {dtype}")


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64], ids=["int32", "int64"])
def test_rank_metrics_duplicates_empty_slots_and_wide_ids(dtype):
    """An item listed twice hits twice; -1 never hits, nor does (int64 only)
    2^32 + p for a positive p; duplicate positives count in recall's
    denominator."""
    k = 130
    recs, rowptr, items = rank_case(k, 18, seed=1)
    rows = [items[rowptr[u]:rowptr[u + 1]].astype(np.int64) for u in range(18)]
    recs = recs.copy()
    for u in range(18):
        recs[u, [3, 70, 129]] = -1
        recs[u, [5, 64, 100]] = recs[u, 1]                   # one item four times
        rows[u] = np.concatenate([rows[u], recs[u, [1, 1, 2]]])  # ... a positive, listed twice
        if dtype == torch.int64:
            recs[u, [0, 63, 128]] = (1 << 32) + rows[u][:3]
    rowptr, items = csr(rows)
    ref = rank_metrics_f64(recs, rowptr, items)
    assert ref[0].min() >= 4 / k  # the repeated item's four hits
    got = ops.rank_metrics(dev(recs, dtype), dev(rowptr), dev(items))
    check_rank(host(*got), ref, what=f"special entries {dtype}")


def test_rank_metrics_without_any_positive():
    recs = rank_case(65, 5)[0]
    got = host(*ops.rank_metrics(dev(recs), torch.zeros(6, dtype=torch.int64, device=DEV),
                                 torch.zeros(0, dtype=torch.int32, device=DEV)))
    assert np.isnan(got[1]).all()
    assert not got[0].any() and not got[2].any() and not got[3].any()
    assert all(o.numel() == 0 for o in ops.rank_metrics(
        dev(recs[:0]), torch.zeros(1, dtype=torch.int64, device=DEV),
        torch.zeros(0, dtype=torch.int32, device=DEV)))


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64], ids=["int32", "int64"])
def test_rank_metrics_positive_rows_of_length_0_1_5(dtype):
    """3 users x 8 items, k = 4: the listed ids meet their user's sorted
    positives row at its first entry, at its last entry and nowhere, in an
    empty row, a row of one and a row of five."""
    recs = np.array([[0, 1, 2, 3], [3, 0, 5, 7], [1, 7, 5, 0]], dtype=np.int64)
    rowptr, items = csr([[], [3], [1, 2, 4, 6, 7]])
    ref = rank_metrics_f64(recs, rowptr, items)
    assert [round(4 * p) for p in ref[0]] == [0, 1, 2]
    got = ops.rank_metrics(dev(recs, dtype), dev(rowptr), dev(items))
    check_rank(host(*got), ref, what=f"short rows {dtype}")


# --------------------------------------------------------------------------- catalog histogram
def _hist_reference(recs, n_items):
    ok = (recs >= 0) & (recs < n_items)
    pos = np.broadcast_to(np.arange(recs.shape[1]), recs.shape)[ok]
    return (np.bincount(recs[ok], minlength=n_items),
            np.bincount(recs[ok], weights=pos, minlength=n_items).astype(np.int64))


@pytest.mark.parametrize("n,k", [((65536 * 256 + 300) // 4, 4), (70001, 1), (1, 1000)],
                         ids=["stride-loop", "k1", "one-row"])
def test_catalog_histogram_shapes_exact(n, k):
    """65536 * 256 + 300 entries: 300 lanes take a second turn of the
    grid-stride loop. Counts and position sums exact, ids -1, n_items and
    n_items + 1 skipped."""
    rng = np.random.default_rng(k)
    ni = 3000
    recs = rng.integers(-1, ni + 2, size=(n, k), dtype=np.int32)
    counts, pos = ops.catalog_histogram(dev(recs), ni)
    ref_c, ref_p = _hist_reference(recs, ni)
    assert np.array_equal(counts.cpu().numpy(), ref_c)
    assert np.array_equal(pos.cpu().numpy(), ref_p)


@pytest.mark.parametrize("dt", [torch.int32, torch.int64], ids=["int32", "int64"])
def test_catalog_histogram_position_sums_carry_past_32_bits(dt):
    """The C call adds into what the arrays hold: position sums that start
    just below 2^32 carry into the upper word; with pos_sum NULL the counts
    are the same."""
    rng = np.random.default_rng(19)
    n, k, ni = 300, 37, 50
    recs = rng.integers(-1, ni + 1, size=(n, k))
    ref_c, ref_p = _hist_reference(recs, ni)
    assert ref_p.min() > 10  # every item's sum crosses 2^32
    lib, r = _backend.lib(), dev(recs, dt)
    start = (1 << 32) - 5
    counts = torch.zeros(ni, dtype=torch.int32, device=DEV)
    pos = torch.full((ni,), start, dtype=torch.int64, device=DEV)
    for pos_sum in (pos, None):
        counts.zero_()
        rc = lib.dr_catalog_histogram(r.data_ptr(), _backend.dtype_code(dt), n, k, ni,
                                      counts.data_ptr(), _backend.ptr(pos_sum), _backend.stream(DEV))
        assert rc == 0
        assert np.array_equal(counts.cpu().numpy(), ref_c)
        assert np.array_equal(pos.cpu().numpy(), ref_p + start)  # the second call leaves it alone


# --------------------------------------------------------------------------- sampler
def _sampler_case(seed=40, nu=60, ni=500):
    rng = np.random.default_rng(seed)
    pos = [set(rng.integers(0, ni, 6).tolist()) for _ in range(nu)]
    frz = [set(rng.integers(0, ni, 15).tolist()) for _ in range(nu)]
    return pos, frz, [dev(a) for a in csr([sorted(s) for s in pos])], \
        [dev(a) for a in csr([sorted(s) for s in frz])]


@pytest.mark.parametrize("exclude", [False, True], ids=["no-exclusion", "exclusion"])
@pytest.mark.parametrize("m", [1, 3, 129])
def test_sample_pairwise_membership_and_layout(m, exclude):
    """60 users x 2m draws: less than one 256-thread block (m = 1), one block
    and a part (3), many (129). Positives are the user's, negatives outside
    its positives (and its frozen items, when given), triples the m x m
    product in positive-major order."""
    pos, frz, pos_csr, excl_csr = _sampler_case()
    users = torch.arange(60, device=DEV)
    ex = excl_csr if exclude else None
    p, n, trip = ops.sample_pairwise(users, *pos_csr, 500, m, 77, exclude=ex)
    p, n = host(p, n)
    uid, pid, nid = (t.reshape(60, m, m) for t in host(*trip))
    assert p.shape == (60, m) and n.shape == (60, m)
    for u in range(60):
        assert set(p[u].tolist()) <= pos[u]
        assert not (set(n[u].tolist()) & (pos[u] | frz[u] if exclude else pos[u]))
        assert n[u].min() >= 0 and n[u].max() < 500
        assert np.all(uid[u] == u)
        assert np.array_equal(pid[u], np.repeat(p[u][:, None], m, axis=1))
        assert np.array_equal(nid[u], np.repeat(n[u][None, :], m, axis=0))
    if m == 129 and not exclude:  # without exclusion, frozen items are drawn too
        assert any(set(n[u].tolist()) & frz[u] for u in range(60))
    p2, n2, none = ops.sample_pairwise(users, *pos_csr, 500, m, 77, exclude=ex, expand=False)
    assert none is None and np.array_equal(p2.cpu().numpy(), p) and np.array_equal(n2.cpu().numpy(), n)


@pytest.mark.parametrize("exclude", [False, True], ids=["no-exclusion", "exclusion"])
def test_sample_pairwise_draws_depend_on_seed_and_user_only(exclude):
    """The header's promise: a user's draws do not depend on where the user
    stands in the call or on what else the call holds."""
    _, _, pos_csr, excl_csr = _sampler_case()
    ex = excl_csr if exclude else None
    m = 5
    order = np.random.default_rng(3).permutation(60)[:41]
    users = dev(order)
    sample = lambda us: host(*ops.sample_pairwise(us, *pos_csr, 500, m, 9, exclude=ex)[:2])
    p, n = sample(users)
    pa, na = sample(users[:17])  # the same users in two calls
    pb, nb = sample(users[17:])
    assert np.array_equal(np.concatenate([pa, pb]), p) and np.array_equal(np.concatenate([na, nb]), n)
    perm = np.random.default_rng(4).permutation(41)
    pp, pn = sample(dev(order[perm]))
    assert np.array_equal(pp, p[perm]) and np.array_equal(pn, n[perm])
    twice = dev(np.concatenate([order[:3], order[:3], order[1:2]]))
    tp, tn = sample(twice)
    assert np.array_equal(tp, p[[0, 1, 2, 0, 1, 2, 1]]) and np.array_equal(tn, n[[0, 1, 2, 0, 1, 2, 1]])
    assert len({tuple(r) for r in n.tolist()}) > 30  # users differ from each other


def test_sample_pairwise_exclusion_rows_of_length_0_1_5():
    """3 users x 8 items, m = 4 over 40 seeds (160 draws per user: an allowed
    item is missed with probability (6/7)^160 < 1e-10): every item is looked
    up in its user's sorted rows, so the search meets a row's first entry,
    its last entry and ids around them, in an exclusion row that is empty, of
    one and of five. Negatives are exactly the allowed items."""
    pos, frz = [[4], [1], [1]], [[], [6], [0, 2, 3, 5, 7]]
    pos_csr, excl_csr = [dev(a) for a in csr(pos)], [dev(a) for a in csr(frz)]
    users = torch.arange(3, device=DEV)
    seen = [set(), set(), set()]
    for seed in range(40):
        p, n, _ = ops.sample_pairwise(users, *pos_csr, 8, 4, seed, exclude=excl_csr, expand=False)
        assert np.array_equal(p.cpu().numpy(), np.repeat([[4], [1], [1]], 4, axis=1))
        for u, row in enumerate(n.cpu().numpy()):
            seen[u] |= set(row.tolist())
    assert seen == [set(range(8)) - set(pos[u]) - set(frz[u]) for u in range(3)]


def test_sample_pairwise_one_or_no_allowed_negative():
    """64 items of which 63 are positive or frozen: every negative is the one
    left (4096 tries that all miss at 63/64 each have probability e^-64).
    With none left the call raises IndexError, as random.choices([]) does."""
    ni, free = 64, 37
    taken = [i for i in range(ni) if i != free]
    users = torch.zeros(1, dtype=torch.int64, device=DEV)
    split = ([dev(a) for a in csr([taken[:20]])], [dev(a) for a in csr([taken[20:]])])
    whole = [dev(a) for a in csr([taken])]
    for pos_csr, ex in ((split[0], split[1]), (whole, None)):
        p, n, _ = ops.sample_pairwise(users, *pos_csr, ni, 200, 11, exclude=ex)
        assert (n.cpu().numpy() == free).all()
        assert set(p.cpu().numpy().ravel().tolist()) <= set(taken)
    full = [dev(a) for a in csr([list(range(ni))])]
    with pytest.raises(IndexError):
        ops.sample_pairwise(users, *full, ni, 8, 11)
    with pytest.raises(IndexError):  # positives and frozen together cover the catalog
        ops.sample_pairwise(users, *split[0], ni, 8, 11,
                            exclude=[dev(a) for a in csr([taken[20:] + [free]])])
