"""Argument checks of the three re-rank entry points (dr_mmr_rerank,
dr_dpp_rerank, dr_calibrated_rerank) as one table of (return code, message):
every single bad argument, and the pairs of bad arguments that show in which
order an entry point looks at them. The entry points answer some of these
differently (code, message or order); the table pins each as it is, so a
change to the checks they share cannot move one by accident. Every case
returns before any HIP call. No GPU."""
import ctypes

import pytest

from divrec import _backend

OK, EINVAL, EUNSUPPORTED = 0, -1, -2
NAN = float("nan")
ONE = ctypes.c_void_p(8)  # a non-NULL pointer the checks never dereference


def _mmr(lib, n=4, C=100, n_items=10, d=128, k_out=10, lam=0.5, ptr=ONE):
    return lib.dr_mmr_rerank(ptr, ptr, n, C, ptr, n_items, d, k_out, lam, ptr, None, None)


def _dpp(lib, n=4, C=100, n_items=10, d=128, k_out=10, lam=0.5, ptr=ONE):
    return lib.dr_dpp_rerank(ptr, ptr, n, C, ptr, n_items, d, k_out, lam, ptr, None, None, None)


def _calibrated(lib, n=4, C=100, n_items=10, G=5, k_out=10, lam=0.5, ptr=ONE):
    return lib.dr_calibrated_rerank(ptr, ptr, n, C, ptr, n_items, G, ptr, k_out, lam, ptr, None,
                                    None, None)


CALLS = {"mmr": _mmr, "dpp": _dpp, "calibrated": _calibrated}

C_RANGE = b"C must be in [1, 1024]"
K_RANGE = b"k_out must be in [1, C]"
K_RANGE_DPP = b"k_out must be in [1, min(C, 128)]"
LAMBDA = b"lambda must be in [0, 1]"
N_ITEMS = b"n_items must be in [0, 2^31)"
G_N_ITEMS = b"G must be >= 1 and n_items in [0, 2^31)"
D_WIDTH = b"d must be 64 or 128"
N_USERS = b"n_users must be >= 0"
NULL = b"null pointer"

# (entry point, arguments away from the valid defaults, return code, message)
TABLE = [
    # ---- one bad argument
    ("mmr", dict(C=0), EINVAL, C_RANGE),
    ("dpp", dict(C=0), EINVAL, C_RANGE),
    ("calibrated", dict(C=0), EINVAL, b"C must be >= 1"),
    ("mmr", dict(C=1025), EINVAL, C_RANGE),
    ("dpp", dict(C=1025), EINVAL, C_RANGE),
    ("calibrated", dict(C=1025), EUNSUPPORTED, b"C must be <= 1024"),
    ("mmr", dict(C=2000), EINVAL, C_RANGE),
    ("dpp", dict(C=2000), EINVAL, C_RANGE),
    ("calibrated", dict(C=2000), EUNSUPPORTED, b"C must be <= 1024"),
    ("mmr", dict(k_out=0), EINVAL, K_RANGE),
    ("dpp", dict(k_out=0), EINVAL, K_RANGE_DPP),
    ("calibrated", dict(k_out=0), EINVAL, K_RANGE),
    ("mmr", dict(k_out=101), EINVAL, K_RANGE),  # C + 1
    ("dpp", dict(k_out=101), EINVAL, K_RANGE_DPP),
    ("calibrated", dict(k_out=101), EINVAL, K_RANGE),
    ("dpp", dict(C=200, k_out=129), EINVAL, K_RANGE_DPP),  # within C, past DPP's own 128
    ("mmr", dict(lam=-0.1), EINVAL, LAMBDA),
    ("dpp", dict(lam=-0.1), EINVAL, LAMBDA),
    ("calibrated", dict(lam=-0.1), EINVAL, LAMBDA),
    ("mmr", dict(lam=1.5), EINVAL, LAMBDA),
    ("dpp", dict(lam=1.5), EINVAL, LAMBDA),
    ("calibrated", dict(lam=1.5), EINVAL, LAMBDA),
    ("mmr", dict(lam=NAN), EINVAL, LAMBDA),
    ("dpp", dict(lam=NAN), EINVAL, LAMBDA),
    ("calibrated", dict(lam=NAN), EINVAL, LAMBDA),
    ("mmr", dict(n_items=-1), EINVAL, N_ITEMS),
    ("dpp", dict(n_items=-1), EINVAL, N_ITEMS),
    ("calibrated", dict(n_items=-1), EINVAL, G_N_ITEMS),
    ("mmr", dict(n_items=0), EINVAL, b"empty item table"),
    ("dpp", dict(n_items=0), EINVAL, b"empty item table"),
    ("calibrated", dict(n_items=0), EINVAL, b"empty label table"),
    ("mmr", dict(n_items=2**31 - 1), EINVAL, N_ITEMS),
    ("dpp", dict(n_items=2**31 - 1), EINVAL, N_ITEMS),
    ("calibrated", dict(n_items=2**31 - 1), EINVAL, G_N_ITEMS),
    ("mmr", dict(d=100), EUNSUPPORTED, D_WIDTH),
    ("dpp", dict(d=100), EUNSUPPORTED, D_WIDTH),
    ("calibrated", dict(G=0), EINVAL, G_N_ITEMS),
    ("calibrated", dict(G=65), EUNSUPPORTED, b"G must be <= 64"),
    ("mmr", dict(ptr=None), EINVAL, NULL),
    ("dpp", dict(ptr=None), EINVAL, NULL),
    ("calibrated", dict(ptr=None), EINVAL, NULL),
    ("dpp", dict(n=-1), EINVAL, N_USERS),
    ("calibrated", dict(n=-1), EINVAL, N_USERS),
    # dr_mmr_rerank has no check of n_users: n = -1 with everything else valid
    # would reach the launch, so it is shown with a second bad argument, which
    # is what gets reported
    ("mmr", dict(n=-1, ptr=None), EINVAL, NULL),
    ("mmr", dict(n=-1, d=100), EUNSUPPORTED, D_WIDTH),
    ("dpp", dict(n=-1, ptr=None), EINVAL, N_USERS),
    ("dpp", dict(n=-1, d=100), EINVAL, N_USERS),
    ("calibrated", dict(n=-1, ptr=None), EINVAL, N_USERS),
    ("calibrated", dict(n=-1, G=65), EINVAL, N_USERS),
    # no users: a no-op success, whatever the pointers
    ("mmr", dict(n=0), OK, b""),
    ("dpp", dict(n=0), OK, b""),
    ("calibrated", dict(n=0), OK, b""),
    ("mmr", dict(n=0, ptr=None), OK, b""),
    ("dpp", dict(n=0, ptr=None), OK, b""),
    ("calibrated", dict(n=0, ptr=None), OK, b""),
    # ---- two bad arguments: which one an entry point sees first
    ("mmr", dict(n=0, d=100), OK, b""),  # returns for n = 0 before it looks at d
    ("dpp", dict(n=0, d=100), EUNSUPPORTED, D_WIDTH),  # looks at d first
    ("mmr", dict(n=0, C=2000), EINVAL, C_RANGE),
    ("dpp", dict(n=0, C=2000), EINVAL, C_RANGE),
    ("calibrated", dict(n=0, C=2000), EUNSUPPORTED, b"C must be <= 1024"),
    ("mmr", dict(n=0, n_items=0), OK, b""),
    ("dpp", dict(n=0, n_items=0), OK, b""),
    ("calibrated", dict(n=0, n_items=0), EINVAL, b"empty label table"),  # table before n = 0
    ("calibrated", dict(n=0, G=65), EUNSUPPORTED, b"G must be <= 64"),
    ("mmr", dict(C=2000, lam=1.5), EINVAL, C_RANGE),
    ("dpp", dict(C=2000, lam=1.5), EINVAL, C_RANGE),
    ("calibrated", dict(C=2000, lam=1.5), EUNSUPPORTED, b"C must be <= 1024"),
]


def _case_id(case):
    entry, args, _, _ = case
    return entry + "-" + "-".join(f"{k}={v}" for k, v in args.items())


@pytest.mark.parametrize("case", TABLE, ids=_case_id)
def test_rerank_argument_table(case):
    entry, args, code, message = case
    lib = _backend.load_library()
    rc = CALLS[entry](lib, **args)
    last = lib.dr_last_error() if rc else b""
    assert rc == code, (rc, last)
    if code:
        assert last.startswith(b"dr_%s_rerank: " % entry.encode()) and message in last, last
