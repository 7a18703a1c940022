"""lhpc_spmv_plan_set_values / lhpc_spmm_plan_set_values on the GPU: "same
structure, new values".  The contract is that the updated plan is
indistinguishable from a fresh plan built from (row_ptr, col_idx, new val)
with the same flags and options, so every check is exact and needs no
tolerance: plan P is built from v0, plan F from v1, P.set_values(v1), then
P's layout digests (XTILE: they cover the val runs, padding included), plan
info (but device_bytes) and the bits of y must equal F's, for random
non-dyadic v1 and x.  Once per family dyadic values are also checked against
the CPU oracle.  Shapes are the small ones tests/test_gpu_spmv.py and
tests/test_gpu_sell.py use to reach each code path; the matrices are built
once per module."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import _support as S
from tests.test_gpu_spmv import _csr_from_lengths

pytestmark = pytest.mark.gpu

XTILE, XSLICE, SELL, ADAPTIVE, ROWGROUP = 1 << 9, 1 << 6, 1 << 10, 1 << 5, 1 << 4
# rows cut by chunk ends, chunk starts at odd element alignment, a partial last wave region
LONG = [20000] + [3] * 50 + [5000, 4096, 4095, 1, 0, 9000] + [15] * 3000 + [0, 0] + [30000]
# tests/test_gpu_spmv.py::test_xtile_empty_row_runs
EMPTY_RUNS = [0] * 3000 + [7] * 10 + [0] * 2500 + [1] + [0] * 1500 + [4096] + [0] * 2049
SHAPES = {"long": (LONG, 200_000, 0x5E70), "empty_runs": (EMPTY_RUNS, 150_000, 0x5E71)}
LAYOUTS = {"perm": {"xtile_reduce": 1, "xtile_align": 1}, "iperm": {"xtile_reduce": 2, "xtile_align": 1},
           "iperm_aligned": {"xtile_reduce": 2, "xtile_align": 2}}
_CSR, _VALS = {}, {}


def _structure(shape):
    """(row_ptr, col_idx, n_cols) of a named shape, built once"""
    if shape not in _CSR:
        lengths, n_cols, seed = SHAPES[shape]
        rp, col, _ = _csr_from_lengths(lengths, n_cols, seed, dyadic=True)
        _CSR[shape] = (rp, col, n_cols)
    return _CSR[shape]


def _values(nnz, n_cols, dt, seed, dyadic=False):
    """(v0, v1, x): two value sets for one structure and an x, random
    non-dyadic (or dyadic k/8: every summation order is then exact)"""
    key = (nnz, n_cols, np.dtype(dt).name, seed, dyadic)
    if key not in _VALS:
        rng = np.random.default_rng(seed)
        if dyadic:
            draw = lambda m: (rng.integers(-8, 9, size=m) / 8.0).astype(dt)  # noqa: E731
        else:
            draw = lambda m: rng.uniform(-1.0, 1.0, size=m).astype(dt)  # noqa: E731
        _VALS[key] = (draw(nnz), draw(nnz), draw(n_cols))
    return _VALS[key]


def _dev(gpu, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _bits(a):
    a = a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _same(a, b):
    """bit for bit (array_equal on the bit patterns: −0 ≠ +0, NaN = NaN)"""
    return np.array_equal(_bits(a), _bits(b))


def _info_but_bytes(plan):
    return {k: v for k, v in plan.info().items() if k != "device_bytes"}


def _check_update(lhpc, gpu, rp, col, n_cols, dt, flags, options=None, splits=None, on_device=True, seed=1,
                  digest=True, kernel=None):
    """The common scheme.  Returns (P, F, v0, v1, xd) with P updated to v1."""
    v0, v1, x = _values(int(col.size), n_cols, dt, seed)
    xd = _dev(gpu, x)
    P = lhpc.SpMVPlan(rp, col, v0, n_cols, flags=flags, options=options, splits=splits)
    F = lhpc.SpMVPlan(rp, col, v1, n_cols, flags=flags, options=options, splits=splits)
    if kernel is not None:
        assert P.info()["kernel"] == kernel
    y0 = P(xd)
    assert not _same(y0, F(xd)), "v0 and v1 give the same y: the test would show nothing"
    if digest:
        assert P.layout_digest() != F.layout_digest(), "the digests do not cover the values"
    P.set_values(_dev(gpu, v1) if on_device else v1)
    if digest:
        assert P.layout_digest() == F.layout_digest()
    assert _info_but_bytes(P) == _info_but_bytes(F)
    assert _same(P(xd), F(xd))
    return P, F, v0, v1, xd


# ------------------------------------------------------------------ XTILE
XTILE_CASES = {
    "plain": {},
    "ranges_ring": {"xtile_ranges": 2, "xtile_ring": 0},
    "ranges_no_ring": {"xtile_ranges": 2, "xtile_ring": 1},
    "pretable1": {"xtile_pretable": 1},
    "pretable2": {"xtile_pretable": 2},
    "host_build0": {"xtile_host_build": 0},
    "host_build1": {"xtile_host_build": 1},
    "row_parts": {"xtile_part_nnz": 40_000},
}


@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("case", list(XTILE_CASES))
def test_xtile_update_equals_fresh_plan(lhpc, gpu, case, layout, dt):
    rp, col, n_cols = _structure("long")
    opts = dict(LAYOUTS[layout], **XTILE_CASES[case])
    P, F, *_ = _check_update(lhpc, gpu, rp, col, n_cols, dt, XTILE, options=opts, kernel=lhpc.KERNEL_XTILE)
    P.close(), F.close()


@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_xtile_empty_row_runs(lhpc, gpu, layout, dt):
    rp, col, n_cols = _structure("empty_runs")
    P, F, *_ = _check_update(lhpc, gpu, rp, col, n_cols, dt, XTILE, options=LAYOUTS[layout],
                             kernel=lhpc.KERNEL_XTILE)
    P.close(), F.close()


@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_xtile_split_plan_stage_and_ranges(lhpc, gpu, layout, dt):
    """A create_split plan: after the update, stage + range give F's bits too."""
    import torch
    rp, col, n_cols = _structure("long")
    n = rp.size - 1
    splits = [1, 51, 57, 2000, n - 1]
    P, F, _, _, xd = _check_update(lhpc, gpu, rp, col, n_cols, dt, XTILE, options=LAYOUTS[layout], splits=splits,
                                   kernel=lhpc.KERNEL_XTILE)
    bounds = [0] + splits + [n]
    out = []
    for plan in (P, F):
        ys = [torch.full((bounds[k + 1] - bounds[k],), float("nan"), dtype=xd.dtype, device=gpu)
              for k in range(len(bounds) - 1)]
        plan.stage(xd)
        for k, yk in enumerate(ys):
            plan.range(k, yk)
        out.append(torch.cat(ys))
    assert _same(out[0], out[1]) and _same(out[0], F(xd))
    P.close(), F.close()


@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("case", ["plain", "row_parts"])
def test_xtile_host_and_device_values_same_digest(lhpc, gpu, case, dt):
    rp, col, n_cols = _structure("long")
    opts = dict(LAYOUTS["iperm"], **XTILE_CASES[case])
    Pd, F, *_ = _check_update(lhpc, gpu, rp, col, n_cols, dt, XTILE, options=opts, on_device=True)
    Ph, F2, *_ = _check_update(lhpc, gpu, rp, col, n_cols, dt, XTILE, options=opts, on_device=False)
    assert Pd.layout_digest() == Ph.layout_digest() == F.layout_digest()
    for p in (Pd, Ph, F, F2):
        p.close()


@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_xtile_nonfinite_old_values_leave_nothing(lhpc, gpu, layout, dt):
    """v0 is NaN / ±Inf everywhere, v1 finite: digest and y equal F's, so no
    stale value survives and the padding (val 0) was never touched — a NaN
    left in a padded position would also turn its row's y into NaN."""
    rp, col, n_cols = _structure("long")
    _, v1, x = _values(int(col.size), n_cols, dt, 2)
    v0 = np.resize(np.array([np.nan, np.inf, -np.inf], dtype=dt), col.size)
    xd = _dev(gpu, x)
    with lhpc.SpMVPlan(rp, col, v0, n_cols, flags=XTILE, options=LAYOUTS[layout]) as P, \
            lhpc.SpMVPlan(rp, col, v1, n_cols, flags=XTILE, options=LAYOUTS[layout]) as F:
        P.set_values(_dev(gpu, v1))
        assert P.layout_digest() == F.layout_digest()
        y = P(xd)
        assert np.isfinite(y.cpu().numpy()).all() and _same(y, F(xd))


@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["f32", "f64"])
def test_xtile_two_updates_return_to_the_original(lhpc, gpu, dt):
    rp, col, n_cols = _structure("long")
    P, F, v0, v1, xd = _check_update(lhpc, gpu, rp, col, n_cols, dt, XTILE, options=LAYOUTS["iperm"])
    with lhpc.SpMVPlan(rp, col, v0, n_cols, flags=XTILE, options=LAYOUTS["iperm"]) as orig:
        P.set_values(_dev(gpu, v0))
        assert P.layout_digest() == orig.layout_digest()
        assert _same(P(xd), orig(xd))
    P.close(), F.close()


@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["f32", "f64"])
def test_xtile_dyadic_against_oracle(lhpc, gpu, dt):
    rp, col, n_cols = _structure("long")
    v0, v1, x = _values(int(col.size), n_cols, dt, 3, dyadic=True)
    with lhpc.SpMVPlan(rp, col, v0, n_cols, flags=XTILE) as P:
        P.set_values(_dev(gpu, v1))
        assert np.array_equal(P(_dev(gpu, x)).cpu().numpy(), S.spmv_oracle(rp, col, v1, x)[1])


# ------------------------------------------------- SELL / ADAPTIVE / ROWGROUP
def _short_rows(n, seed):
    """row lengths drawn from 0 … 8 (n = 1: at least one nonzero)"""
    rng = np.random.default_rng(seed)
    lens = rng.integers(1 if n == 1 else 0, 9, size=n)
    rp = np.zeros(n + 1, dtype=np.int32)
    np.cumsum(lens, out=rp[1:])
    col = rng.integers(0, n, size=int(rp[-1])).astype(np.int32)
    return rp, col


SHORT_N = [1, 63, 64, 65, 1000, 4099]


@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("n", SHORT_N)
def test_sell_update_and_device_bytes(lhpc, gpu, n, dt):
    """SELL keeps no row_ptr: plan creation books what it always did (a second
    plan that is never updated holds the same bytes), the first update adds at
    most the n + 1 int64 row offsets, the second nothing."""
    rp, col = _short_rows(n, 0x5E11 + n)
    v0, v1, x = _values(int(col.size), n, dt, 4)
    xd = _dev(gpu, x)
    with lhpc.SpMVPlan(rp, col, v0, n, flags=SELL) as P, lhpc.SpMVPlan(rp, col, v0, n, flags=SELL) as Q, \
            lhpc.SpMVPlan(rp, col, v1, n, flags=SELL) as F:
        assert P.info()["kernel"] == lhpc.KERNEL_SELL
        b0 = P.info()["device_bytes"]
        assert b0 == Q.info()["device_bytes"] == F.info()["device_bytes"]
        P.set_values(_dev(gpu, v1))
        b1 = P.info()["device_bytes"]
        assert 0 <= b1 - b0 <= 8 * (n + 1), (b0, b1)
        assert _info_but_bytes(P) == _info_but_bytes(F)
        assert _same(P(xd), F(xd))
        P.set_values(v0)  # host values, second update
        assert P.info()["device_bytes"] == b1
        assert _same(P(xd), Q(xd))
        assert Q.info()["device_bytes"] == b0


@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("rp_dtype", [np.int32, np.int64], ids=["rp32", "rp64"])
@pytest.mark.parametrize("family", [ADAPTIVE, ROWGROUP], ids=["adaptive", "rowgroup"])
@pytest.mark.parametrize("n", SHORT_N)
def test_csr_families_update(lhpc, gpu, n, family, rp_dtype, dt):
    rp, col = _short_rows(n, 0x5E11 + n)
    for on_device in (True, False):
        P, F, *_ = _check_update(lhpc, gpu, rp.astype(rp_dtype), col, n, dt, family, on_device=on_device, seed=5,
                                 digest=False)
        b = P.info()["device_bytes"]
        assert b == F.info()["device_bytes"]
        P.close(), F.close()


@pytest.mark.parametrize("family", [SELL, ADAPTIVE, ROWGROUP], ids=["sell", "adaptive", "rowgroup"])
def test_short_row_families_dyadic_against_oracle(lhpc, gpu, family):
    n = 4099
    rp, col = _short_rows(n, 0x5E11 + n)
    v0, v1, x = _values(int(col.size), n, np.float64, 6, dyadic=True)
    with lhpc.SpMVPlan(rp, col, v0, n, flags=family) as P:
        P.set_values(_dev(gpu, v1))
        assert np.array_equal(P(_dev(gpu, x)).cpu().numpy(), S.spmv_oracle(rp, col, v1, x)[1])


def test_sell_nonfinite_old_values_leave_nothing(lhpc, gpu):
    n = 1000
    rp, col = _short_rows(n, 0x5E11 + n)
    _, v1, x = _values(int(col.size), n, np.float32, 7)
    v0 = np.resize(np.array([np.nan, np.inf, -np.inf], dtype=np.float32), col.size)
    xd = _dev(gpu, x)
    with lhpc.SpMVPlan(rp, col, v0, n, flags=SELL) as P, lhpc.SpMVPlan(rp, col, v1, n, flags=SELL) as F:
        P.set_values(_dev(gpu, v1))
        y = P(xd)
        assert np.isfinite(y.cpu().numpy()).all() and _same(y, F(xd))


# ------------------------------------------------------------------ SpMM
@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("k", [3, 33])
def test_spmm_plan_update(lhpc, gpu, k, dt):
    import torch
    n = 1000
    rp, col = _short_rows(n, 0x5E11 + n)
    v0, v1, _ = _values(int(col.size), n, dt, 8)
    rng = np.random.default_rng(k)
    X = _dev(gpu, rng.uniform(-1, 1, (n, k)).astype(dt))
    W = _dev(gpu, rng.uniform(-1, 1, (n, k)).astype(dt))
    with lhpc.SpMMPlan(rp, col, v0, n) as P, lhpc.SpMMPlan(rp, col, v1, n) as F:
        Y0 = P(X)
        for val in (_dev(gpu, v1), v1):  # device values, then (after going back to v0) host values
            P.set_values(val)
            assert P.info() == F.info()
            assert _same(P(X), F(X)) and not _same(P(X), Y0)
            Yp, dp = lhpc.spmm_dot(P, X, W)
            Yf, df = lhpc.spmm_dot(F, X, W)
            torch.cuda.synchronize()
            assert _same(Yp, Yf) and np.array_equal(dp.cpu().numpy().view(np.uint64), df.cpu().numpy().view(np.uint64))
            P.set_values(_dev(gpu, v0))
            assert _same(P(X), Y0)


# ------------------------------------------------------------------ CG
def _lap(shift):
    return S.laplacian_2d(64, 64, dtype=np.float64, shift=shift)


@pytest.mark.parametrize("flags,options", [(0, None), (SELL, None), (0, {"spmv_no_sell": 1})],
                         ids=["auto", "sell", "adaptive"])
def test_cg_after_update_matches_fresh_plan(lhpc, gpu, flags, options):
    """lhpc_cg_solve on a side stream with check_every = 4 (the captured-graph
    path): the graph kept with P stays valid across set_values (d_val keeps
    its address) and the next solve uses the new values — iterations, residual
    and x equal the same solve on a fresh plan of the shifted Laplacian."""
    import torch
    rp, col, v0 = _lap(0.0)
    _, _, v1 = _lap(0.5)
    n = rp.size - 1
    b = _dev(gpu, np.random.default_rng(31).uniform(-1, 1, n))
    s = torch.cuda.Stream(gpu)
    kw = dict(tol=1e-10, max_iter=400, check_every=4, stream=s)
    with lhpc.SpMVPlan(rp, col, v0, n, flags=flags, options=options) as P, \
            lhpc.SpMVPlan(rp, col, v1, n, flags=flags, options=options) as F:
        x0, it0, r0 = lhpc.cg(P, b, **kw)
        P.set_values(_dev(gpu, v1), stream=s)
        x1, it1, r1 = lhpc.cg(P, b, **kw)
        xf, itf, rf = lhpc.cg(F, b, **kw)
        s.synchronize()
        assert (it1, r1) == (itf, rf) and _same(x1, xf)
        assert it1 != it0 or not _same(x1, x0)  # the shift changed the solve
        assert P.info()["kernel"] == F.info()["kernel"]


def test_cg_multi_after_update_matches_fresh_plan(lhpc, gpu):
    import torch
    rp, col, v0 = _lap(0.0)
    _, _, v1 = _lap(0.5)
    n, k = rp.size - 1, 4
    B = _dev(gpu, np.random.default_rng(32).uniform(-1, 1, (n, k)))
    s = torch.cuda.Stream(gpu)
    kw = dict(tol=1e-10, max_iter=400, check_every=4, stream=s)
    with lhpc.SpMMPlan(rp, col, v0, n) as P, lhpc.SpMMPlan(rp, col, v1, n) as F:
        X0, it0, _ = lhpc.cg_multi(P, B, **kw)
        P.set_values(_dev(gpu, v1), stream=s)
        X1, it1, r1 = lhpc.cg_multi(P, B, **kw)
        Xf, itf, rf = lhpc.cg_multi(F, B, **kw)
        s.synchronize()
        assert np.array_equal(it1, itf) and np.array_equal(r1.view(np.uint64), rf.view(np.uint64)) and _same(X1, Xf)
        assert not _same(X1, X0)


# ------------------------------------------------------------------ graph capture
@pytest.mark.parametrize("family", [XTILE, SELL, ADAPTIVE], ids=["xtile", "sell", "adaptive"])
def test_update_and_spmv_captured_in_a_graph(lhpc, gpu, family):
    """A device-values update followed by lhpc_spmv, captured with
    torch.cuda.graph on a side stream and replayed, gives F's bits: the call
    is launches and asynchronous copies only.  The plan has had its first
    update before the capture (a SELL plan's first one allocates)."""
    import torch
    if family == XTILE:
        rp, col, n_cols = _structure("long")
    else:
        n_cols = 4099
        rp, col = _short_rows(n_cols, 0x5E11 + n_cols)
    v0, v1, x = _values(int(col.size), n_cols, np.float32, 9)
    xd, vbuf = _dev(gpu, x), _dev(gpu, v0)
    with lhpc.SpMVPlan(rp, col, v0, n_cols, flags=family) as P, lhpc.SpMVPlan(rp, col, v1, n_cols, flags=family) as F:
        P.set_values(vbuf)  # the first update
        y = torch.full((rp.size - 1,), float("nan"), dtype=xd.dtype, device=gpu)
        y0 = P(xd).clone()
        torch.cuda.synchronize()
        side, g = torch.cuda.Stream(gpu), torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            P.set_values(vbuf)
            P(xd, y)
        vbuf.copy_(_dev(gpu, v1))  # the graph reads the buffer's contents at replay
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert _same(y, F(xd)) and not _same(y, y0)
        if family == XTILE:
            assert P.layout_digest() == F.layout_digest()


# ------------------------------------------------------------------ refusals
@pytest.mark.parametrize("case", ["xslice", "col_blocks", "multi"])
def test_unsupported_plans_refuse_and_stay_as_they_were(lhpc, gpu, case):
    rp, col, n_cols = _structure("long")
    v0, v1, x = _values(int(col.size), n_cols, np.float32, 10)
    kw = {"xslice": dict(flags=XSLICE), "col_blocks": dict(flags=XTILE, options={"xtile_col_blocks": 2}),
          "multi": dict(devices=[0], options={"multi_force": 1})}[case]
    xd = _dev(gpu, x)
    with lhpc.SpMVPlan(rp, col, v0, n_cols, **kw) as P:
        y0 = P(xd).clone()
        if case == "xslice":
            assert P.info()["kernel"] == lhpc.KERNEL_XSLICE
        for val in (_dev(gpu, v1), v1):
            with pytest.raises(lhpc.LhpcError) as e:
                P.set_values(val)
            assert e.value.status == -5
        assert _same(P(xd), y0)


def test_wrong_nnz_and_empty_matrices(lhpc, gpu):
    rp, col, n_cols = _structure("long")
    v0, v1, x = _values(int(col.size), n_cols, np.float32, 10)
    xd, vd = _dev(gpu, x), _dev(gpu, v1)
    with lhpc.SpMVPlan(rp, col, v0, n_cols, flags=XTILE) as P:
        y0, d0 = P(xd).clone(), P.layout_digest()
        for nnz in (col.size - 1, col.size + 1, 0):
            for on_device, ptr in ((1, vd.data_ptr()), (0, v1.ctypes.data)):
                assert lhpc.lib.lhpc_spmv_plan_set_values(P._h, ptr, nnz, on_device, None) == -1
        assert lhpc.lib.lhpc_spmv_plan_set_values(P._h, None, col.size, 1, None) == -1
        assert P.layout_digest() == d0 and _same(P(xd), y0)
    with lhpc.SpMMPlan(rp, col, v0, n_cols) as M:
        assert lhpc.lib.lhpc_spmm_plan_set_values(M._h, vd.data_ptr(), col.size - 1, 1, None) == -1
        assert lhpc.lib.lhpc_spmm_plan_set_values(M._h, None, col.size, 0, None) == -1
    empty = np.zeros(0, dtype=np.float32)
    for n in (0, 5):  # no rows; rows without nonzeros
        rp0 = np.zeros(n + 1, dtype=np.int32)
        for flags in ((0, XTILE, SELL) if n else (0,)):
            with lhpc.SpMVPlan(rp0, np.zeros(0, np.int32), empty, 7, flags=flags) as P:
                P.set_values(empty)
                assert lhpc.lib.lhpc_spmv_plan_set_values(P._h, None, 0, 1, None) == 0
                import torch
                assert torch.count_nonzero(P(torch.ones(7, device=gpu))).item() == 0
        with lhpc.SpMMPlan(rp0, np.zeros(0, np.int32), empty, 7) as M:
            M.set_values(empty)


# ------------------------------------------------------------------ C++ and debug build
def test_cpp_set_values_on_gpu(gpu):
    """tests/cpp/test_set_values_api.cpp (built by tests/cpp/set_values.mk, as
    tests/test_layout.py builds test_cpp_api): both set_values overloads of
    sparse::SpMVPlan and sparse::SpMMPlan against fresh plans, bit for bit."""
    from tests.test_set_values_api import build_cpp
    r = subprocess.run([build_cpp()], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "set_values cpp api: ok" in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-2000:])


def test_debug_build_updates_trap_free(gpu):
    """XTILE and SELL updates and SpMV under the debug library (device bounds
    traps in the new kernels, a synchronous check after every launch), in a
    child process as tests/test_debug_build.py does; valid inputs only."""
    from tests.test_debug_build import DEBUG_SO
    env = dict(os.environ, LHPC_LIB_PATH=DEBUG_SO)
    r = subprocess.run([sys.executable, os.path.join(S.ROOT, "tests", "debug_set_values_check.py")], env=env,
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "DEBUG SET_VALUES OK" in r.stdout
