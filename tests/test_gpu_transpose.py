"""lhpc_csr_transpose and LHPC_PLAN_TRANSPOSE on the GPU.  Every comparison is
exact, bit patterns included; nothing here needs a tolerance.

* csr_transpose against the CPU oracle (tests/test_transpose_api.py
  transpose_oracle: a stable argsort of the positions by column) — t_row_ptr,
  t_col_idx, t_val and perm — for fp32, fp64 and pattern-only, 32- and 64-bit
  offsets, host arrays, device arrays and device arrays offset by one element,
  on shapes chosen where it can go wrong (one, two and three sort passes, the
  pair sort's sub-tile size, empty columns, a run longer than a sub-tile, …).
* A TRANSPOSE plan of A is indistinguishable from the plan of Aᵀ's arrays:
  layout digests, plan info but device_bytes, and the bits of y.  B is the
  structure the XTILE / SELL tests were written for, A its oracle transpose,
  so the operator Aᵀ = B has exactly that structure.
* set_values on TRANSPOSE plans takes A's CSR order and leaves a fresh
  TRANSPOSE plan of the new values.
* SpMM, spmv_dot, spmm_dot, cg and cg_multi on TRANSPOSE plans.
Matrices are built once per module; the "long" and "empty_runs" structures are
shared with tests/test_gpu_set_values.py."""
import subprocess

import numpy as np
import pytest

from tests import _support as S
from tests.test_gpu_set_values import LAYOUTS, _structure
from tests.test_gpu_spmv import _csr_from_lengths
from tests.test_transpose_api import transpose_oracle

pytestmark = pytest.mark.gpu

XTILE, XSLICE, SELL, ADAPTIVE, ROWGROUP = 1 << 9, 1 << 6, 1 << 10, 1 << 5, 1 << 4
TILE = 16384  # pairs per sub-tile of the 32-bit pair sort (lhpc_sort.hip: 1024 threads × 16; lhpc_sort.hpp kSortPairsTile)
_CASES, _MATS = {}, {}


def _dev(gpu, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _bits(a):
    a = a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
    if a.dtype.kind != "f":
        return a
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _same(a, b):
    """bit for bit (array_equal on the bit patterns: −0 ≠ +0, NaN = NaN)"""
    a, b = _bits(a), _bits(b)
    return a.shape == b.shape and np.array_equal(a, b)


def _info_but_bytes(plan):
    return {k: v for k, v in plan.info().items() if k != "device_bytes"}


# ------------------------------------------------------------------ csr_transpose against the oracle
def _rows_of_lengths(lens, n_cols, rng, lo=0, hi=None):
    """(rp, col): random columns in [lo, hi) per row, in no order, repeats allowed"""
    lens = np.asarray(lens, dtype=np.int64)
    rp = np.zeros(lens.size + 1, dtype=np.int32)
    np.cumsum(lens, out=rp[1:])
    col = rng.integers(lo, n_cols if hi is None else hi, size=int(rp[-1])).astype(np.int32)
    return rp, col


def _case(name):
    """(rp int32, col, n_cols) of a named shape, built once"""
    if name in _CASES:
        return _CASES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "nnz0":
        rp, col, n_cols = np.zeros(6, np.int32), np.zeros(0, np.int32), 7
    elif name == "n_rows0":
        rp, col, n_cols = np.zeros(1, np.int32), np.zeros(0, np.int32), 4
    elif name == "n_cols1":  # no key bits: the sort does nothing
        rp, col = _rows_of_lengths(rng.integers(0, 3, size=300), 1, rng)
        n_cols = 1
    elif name.startswith("n_cols"):  # 256: one pass, 257: two, 65536: two, 65537: three
        n_cols = int(name[6:])
        rp, col = _rows_of_lengths(rng.integers(0, 12, size=500), n_cols, rng)
        col[:4] = [n_cols - 1, 0, n_cols - 1, min(255, n_cols - 1)]  # the first and the last key, and digit 255
    elif name.startswith("nnz"):  # the sub-tile size − 1, + 0, + 1 and twice it + 1
        nnz, n_cols = int(name[3:]), 1000
        rp, col = _rows_of_lengths([7] * (nnz // 7) + [nnz % 7], n_cols, rng)
    elif name == "empty_columns":  # at both ends and runs inside
        n_cols = 5000
        rp, col = _rows_of_lengths(rng.integers(0, 9, size=400), n_cols, rng, 100, 200)
        col[::3] = rng.integers(3000, 3100, size=col[::3].size)
        col[5] = 4500
    elif name == "one_full_column":  # column 7 holds every row: a run of 40000 equal keys, longer than two sub-tiles
        n_rows, n_cols = 40000, 50
        rp, col = _rows_of_lengths([2] * n_rows, n_cols, rng)
        col[0::2] = 7
    elif name == "one_full_row":  # row 1 holds every column, in ascending order
        n_cols = 20000
        rp, col = _rows_of_lengths([3, n_cols, 0, 5], n_cols, rng)
        col[3:3 + n_cols] = np.arange(n_cols)
    elif name == "duplicates":  # the same coordinate several times (the values differ)
        n_cols = 37
        rp, col = _rows_of_lengths(rng.integers(0, 40, size=200), n_cols, rng, 0, 5)
    elif name == "descending_rows":
        n_cols = 3000
        rp, col = _rows_of_lengths(rng.integers(0, 30, size=300), n_cols, rng)
        for r in range(300):
            col[rp[r]:rp[r + 1]] = np.sort(col[rp[r]:rp[r + 1]])[::-1]
    else:
        raise KeyError(name)
    _CASES[name] = (rp, col, n_cols)
    return _CASES[name]


CASE_NAMES = ["nnz0", "n_rows0", "n_cols1", "n_cols256", "n_cols257", "n_cols65536", "n_cols65537",
              f"nnz{TILE - 1}", f"nnz{TILE}", f"nnz{TILE + 1}", f"nnz{2 * TILE + 1}", "empty_columns",
              "one_full_column", "one_full_row", "duplicates", "descending_rows"]


def _offset(gpu, a):
    """a device copy of `a` that starts one element into its allocation (4 or
    8 bytes past a 16-byte boundary)"""
    import torch
    buf = torch.empty(a.size + 1, dtype=torch.from_numpy(a[:0].copy()).dtype, device=gpu)
    buf[1:].copy_(torch.from_numpy(np.ascontiguousarray(a)))
    return buf[1:]


def _check_transpose(lhpc, gpu, rp, col, val, n_cols, where):
    want = transpose_oracle(rp, col, val, n_cols)
    if where == "host":
        got = lhpc.csr_transpose(rp, col, val, n_cols, return_perm=True)
        assert all(g is None or isinstance(g, np.ndarray) for g in got)
    else:
        put = _offset if where == "device_offset" else _dev
        args = [put(gpu, rp), put(gpu, col), None if val is None else put(gpu, val)]
        if where == "device_offset":
            assert all(a is None or a.numel() == 0 or a.data_ptr() % 16 != 0 for a in args)
        got = lhpc.csr_transpose(*args, n_cols, return_perm=True)
        assert all(g is None or g.is_cuda for g in got)
        # without perm the other arrays are the same
        short = lhpc.csr_transpose(*args, n_cols)
        assert len(short) == 3 and all(_same(s, w) if w is not None else s is None for s, w in zip(short, want))
    t_rp, t_col, t_val, perm = got
    assert _bits(t_rp).dtype == rp.dtype and _same(t_rp, want[0]), "t_row_ptr"
    assert _same(t_col, want[1]), "t_col_idx"
    assert (t_val is None and val is None) or _same(t_val, want[2]), "t_val"
    assert np.array_equal(_bits(perm).astype(np.int64), want[3].astype(np.int64)), "perm"


@pytest.mark.parametrize("where", ["host", "device", "device_offset"])
@pytest.mark.parametrize("name", CASE_NAMES)
def test_csr_transpose_against_the_oracle(lhpc, gpu, name, where):
    rp, col, n_cols = _case(name)
    rng = np.random.default_rng(col.size)
    for dt in (np.float32, np.float64, None):  # None: pattern only
        val = None if dt is None else rng.uniform(-1, 1, col.size).astype(dt)
        for rp_dtype in (np.int32, np.int64):
            _check_transpose(lhpc, gpu, rp.astype(rp_dtype), col, val, n_cols, where)


@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("name", [f"nnz{2 * TILE + 1}", "one_full_column", "empty_columns"])
def test_csr_transpose_into_unaligned_outputs(lhpc, gpu, name, dt):
    """The C entry point with every input and every output one element into
    its allocation: the scalar variants of both kernels (the Python wrapper
    allocates its outputs, which are always aligned)."""
    import torch
    rp, col, n_cols = _case(name)
    val = np.random.default_rng(9).uniform(-1, 1, col.size).astype(dt)
    for rp_dtype in (np.int32, np.int64):
        r = rp.astype(rp_dtype)
        want = transpose_oracle(r, col, val, n_cols)
        ins = [_offset(gpu, a) for a in (r, col, val)]
        outs = [_offset(gpu, np.zeros_like(w)) for w in (want[0], want[1], want[2], want[3].astype(np.int32))]
        assert all(t.data_ptr() % 16 != 0 for t in ins + outs)
        st = lhpc.lib.lhpc_csr_transpose(lhpc.F32 if dt == np.float32 else lhpc.F64, r.size - 1, n_cols, col.size,
                                         ins[0].data_ptr(), 8 * r.itemsize, ins[1].data_ptr(), ins[2].data_ptr(),
                                         outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(),
                                         outs[3].data_ptr(), 1, torch.cuda.current_stream(gpu).cuda_stream)
        assert st == 0
        assert _same(outs[0], want[0]) and _same(outs[1], want[1]) and _same(outs[2], want[2])
        assert np.array_equal(outs[3].cpu().numpy().astype(np.int64), want[3].astype(np.int64))


def test_csr_transpose_from_dirty_scratch(lhpc, gpu):
    """lhpc_scratch_poison: the next scratch allocations come back filled with
    0xFF; the transposition reads no scratch word it has not written."""
    import torch
    rp, col, n_cols = _case(f"nnz{2 * TILE + 1}")
    val = np.random.default_rng(5).uniform(-1, 1, col.size)
    s = torch.cuda.current_stream(gpu)
    assert lhpc.lib.lhpc_scratch_poison(64 << 20, 0xFF, s.cuda_stream) == 0
    _check_transpose(lhpc, gpu, rp, col, val, n_cols, "device")
    assert lhpc.lib.lhpc_scratch_poison(64 << 20, 0xFF, s.cuda_stream) == 0
    _check_transpose(lhpc, gpu, rp, col, val.astype(np.float32), n_cols, "host")


@pytest.mark.parametrize("where", ["host", "device"])
def test_csr_transpose_refuses_a_bad_matrix(lhpc, gpu, where):
    """Validated on the device either way: LHPC_ERR_BAD_CSR for a column out
    of range (high, negative), a decreasing row_ptr, row_ptr[0] ≠ 0 and
    row_ptr[n_rows] ≠ nnz."""
    rp, col, n_cols = _case("n_cols257")
    val = np.ones(col.size, np.float32)
    put = (lambda a: a) if where == "host" else (lambda a: _dev(gpu, a))
    bad = []
    for c in (n_cols, -1):
        cb = col.copy()
        cb[col.size // 2] = c
        bad.append((rp, cb))
    r = rp.copy()
    r[10], r[11] = max(r[10], r[11]) + 1, min(r[10], r[11])  # decreasing
    bad.append((r, col))
    r = rp.copy()
    r[0] = 1
    bad.append((r, col))
    r = rp.copy()
    r[-1] -= 1
    bad.append((r, col))
    for r, c in bad:
        with pytest.raises(lhpc.LhpcError) as e:
            lhpc.csr_transpose(put(r), put(c), put(val), n_cols)
        assert e.value.status == -2
    _check_transpose(lhpc, gpu, rp, col, val, n_cols, where)  # and the good one still passes


# ------------------------------------------------------------------ TRANSPOSE plan = plan of the transposed arrays
SHORT_LENS_SEED = 0x7A11


def _matrix(shape):
    """B = (rp, col, n_cols) of a named structure and A = its oracle transpose
    (a_rp, a_col, a_perm): Aᵀ = B.  a_perm[p] is the position in B of A's
    entry p, so A's values are B's through a_perm.  Built once."""
    if shape in _MATS:
        return _MATS[shape]
    if shape in ("long", "empty_runs"):
        rp, col, n_cols = _structure(shape)
    elif shape == "long_no_empty_rows":  # chunk records need a matrix without empty rows
        rp, col, n_cols = _structure("long")
        rp = np.unique(rp).astype(np.int32)
    elif shape == "short":  # ≤ 8 per row (SELL), rectangular
        lens = np.random.default_rng(SHORT_LENS_SEED).integers(0, 9, size=4099)
        rp, col, _ = _csr_from_lengths(lens, 3001, SHORT_LENS_SEED, dyadic=True)
        n_cols = 3001
    else:
        raise KeyError(shape)
    n_rows = rp.size - 1
    a_rp, a_col, _, a_perm = transpose_oracle(rp, col, None, n_cols)
    # the round trip on the CPU: transposing A gives B back (B's rows are sorted)
    b_rp, b_col, _, b_perm = transpose_oracle(a_rp, a_col, None, n_rows)
    assert np.array_equal(b_rp, rp) and np.array_equal(b_col, col)
    assert np.array_equal(a_perm[b_perm], np.arange(col.size))
    _MATS[shape] = (rp, col, n_cols, a_rp, a_col, a_perm.astype(np.int64))
    return _MATS[shape]


def _rand(n, dt, seed, dyadic=False):
    rng = np.random.default_rng(seed)
    if dyadic:
        return (rng.integers(-8, 9, size=n) / 8.0).astype(dt)
    return rng.uniform(-1.0, 1.0, size=n).astype(dt)


def _pair(lhpc, gpu, shape, dt, flags, options=None, device_input=False, seed=1, dyadic=False):
    """(T, F, xd, b_val): T the TRANSPOSE plan of A, F the plan of B = Aᵀ"""
    rp, col, n_cols, a_rp, a_col, a_perm = _matrix(shape)
    b_val = _rand(col.size, dt, seed, dyadic)
    a_val = b_val[a_perm]
    put = (lambda a: _dev(gpu, a)) if device_input else (lambda a: a)
    T = lhpc.SpMVPlan(put(a_rp), put(a_col), put(a_val), rp.size - 1, flags=flags, options=options, transpose=True)
    F = lhpc.SpMVPlan(rp, col, b_val, n_cols, flags=flags, options=options)
    return T, F, _dev(gpu, _rand(n_cols, dt, seed + 100, dyadic)), b_val


FAMILIES = {
    "xtile_perm": ("long", XTILE, LAYOUTS["perm"], "KERNEL_XTILE"),
    "xtile_iperm": ("long", XTILE, LAYOUTS["iperm"], "KERNEL_XTILE"),
    "xtile_iperm_aligned": ("long", XTILE, LAYOUTS["iperm_aligned"], "KERNEL_XTILE"),
    "xtile_empty_runs": ("empty_runs", XTILE, LAYOUTS["iperm"], "KERNEL_XTILE"),
    "xtile_chunkrec": ("long_no_empty_rows", XTILE, {"xtile_reduce": 2, "xtile_align": 1, "xtile_chunkrec": 2},
                       "KERNEL_XTILE"),
    "sell": ("short", SELL, None, "KERNEL_SELL"),
    "adaptive": ("short", ADAPTIVE, None, "KERNEL_ADAPTIVE"),
    "adaptive_long": ("long", ADAPTIVE, None, "KERNEL_ADAPTIVE"),
    "rowgroup": ("short", ROWGROUP, None, "KERNEL_ROWGROUP"),
    "xslice": ("short", XSLICE, None, "KERNEL_XSLICE"),
}


@pytest.mark.parametrize("device_input", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("family", list(FAMILIES))
def test_transpose_plan_equals_plan_of_the_transposed_arrays(lhpc, gpu, family, dt, device_input):
    shape, flags, options, kernel = FAMILIES[family]
    T, F, xd, _ = _pair(lhpc, gpu, shape, dt, flags, options, device_input)
    rp, col, n_cols = _matrix(shape)[:3]
    assert T.info()["kernel"] == getattr(lhpc, kernel)
    assert (T.n_rows, T.n_cols, T.nnz) == (rp.size - 1, n_cols, col.size)  # the operator's shape
    assert T.info()["n_rows"] == rp.size - 1 and T.info()["n_cols"] == n_cols
    assert _info_but_bytes(T) == _info_but_bytes(F)
    assert T.info()["device_bytes"] >= F.info()["device_bytes"] + 4 * col.size  # the permutation is counted
    if flags == XTILE:
        assert T.layout_digest() == F.layout_digest()
        assert T.chunkrec() == F.chunkrec()
        if family == "xtile_chunkrec":
            assert T.chunkrec()[0] == (1 if dt == np.float32 else 0)
    y = T(xd)
    assert y.shape[0] == rp.size - 1 and _same(y, F(xd))
    T.close(), F.close()


@pytest.mark.parametrize("family", ["xtile_iperm", "sell", "adaptive", "rowgroup", "xslice"])
def test_transposed_numerics_dyadic_and_adjoint_identity(lhpc, gpu, family):
    """Dyadic values (k/8): every summation order is exact, so Aᵀ·x equals the
    CPU oracle on the oracle-transposed matrix bit for bit, and the adjoint
    identity x·(A·y) = (Aᵀ·x)·y holds exactly: evaluated in integers on the
    host from the two device results (entries are multiples of 1/64)."""
    shape, flags, options, _ = FAMILIES[family]
    dt = np.float32 if flags == XTILE else np.float64
    T, F, xd, b_val = _pair(lhpc, gpu, shape, dt, flags, options, seed=3, dyadic=True)
    rp, col, n_cols, a_rp, a_col, a_perm = _matrix(shape)
    x = xd.cpu().numpy()  # n_cols of B = rows of A
    atx = T(xd).cpu().numpy()
    assert np.array_equal(atx, S.spmv_oracle(rp, col, b_val, x)[1].astype(dt))
    y = _rand(rp.size - 1, dt, 77, dyadic=True)  # A·y reads n_cols of A = rows of B
    with lhpc.SpMVPlan(a_rp, a_col, b_val[a_perm], rp.size - 1) as plain:
        ay = plain(_dev(gpu, y)).cpu().numpy()
    as_int = lambda v, scale: np.rint(v.astype(np.float64) * scale).astype(np.int64)  # noqa: E731
    assert np.array_equal(as_int(ay, 64) / 64.0, ay) and np.array_equal(as_int(atx, 64) / 64.0, atx)
    assert int(np.dot(as_int(x, 8), as_int(ay, 64))) == int(np.dot(as_int(atx, 64), as_int(y, 8)))
    T.close(), F.close()


# ------------------------------------------------------------------ set_values on TRANSPOSE plans
def _check_update(lhpc, gpu, shape, dt, flags, options, on_device, digest):
    """A TRANSPOSE plan built from v0 and updated to v1 (both in A's CSR
    order) equals a fresh TRANSPOSE plan from v1; the second update allocates
    nothing.  Returns (P, F, v0, v1, xd)."""
    rp, col, n_cols, a_rp, a_col, _ = _matrix(shape)
    n = rp.size - 1
    v0, v1, v2 = (_rand(col.size, dt, s) for s in (11, 12, 13))
    xd = _dev(gpu, _rand(n_cols, dt, 14))
    mk = lambda v: lhpc.SpMVPlan(a_rp, a_col, v, n, flags=flags, options=options, transpose=True)  # noqa: E731
    P, F, F2 = mk(v0), mk(v1), mk(v2)
    y0, b0 = P(xd).clone(), P.info()["device_bytes"]
    assert b0 == F.info()["device_bytes"] and not _same(y0, F(xd))
    P.set_values(_dev(gpu, v1) if on_device else v1)
    b1 = P.info()["device_bytes"]
    tsz = np.dtype(dt).itemsize
    # the staging buffer of nnz values (and a SELL plan's row offsets) came with the first update
    assert col.size * tsz <= b1 - b0 <= col.size * tsz + 8 * (n + 1) + 32, (b0, b1)
    if digest:
        assert P.layout_digest() == F.layout_digest()
    assert _info_but_bytes(P) == _info_but_bytes(F) and _same(P(xd), F(xd))
    P.set_values(_dev(gpu, v2) if on_device else v2)  # the second update: no allocation
    assert P.info()["device_bytes"] == b1
    if digest:
        assert P.layout_digest() == F2.layout_digest()
    assert _same(P(xd), F2(xd))
    P.set_values(v0 if on_device else _dev(gpu, v0))  # and back, the other way
    assert _same(P(xd), y0) and F.info()["device_bytes"] == b0
    F2.close()
    return P, F, v0, v1, xd


@pytest.mark.parametrize("on_device", [True, False], ids=["device_values", "host_values"])
@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("family", ["xtile_perm", "xtile_iperm_aligned", "xtile_chunkrec", "sell", "adaptive",
                                    "rowgroup"])
def test_set_values_on_a_transpose_plan(lhpc, gpu, family, dt, on_device):
    shape, flags, options, _ = FAMILIES[family]
    P, F, *_ = _check_update(lhpc, gpu, shape, dt, flags, options, on_device, digest=flags == XTILE)
    P.close(), F.close()


def test_set_values_on_a_transpose_plan_of_row_parts(lhpc, gpu):
    """XTILE row parts (xtile_part_nnz): the gathered values are cut at the parts of Aᵀ."""
    P, F, *_ = _check_update(lhpc, gpu, "long", np.float32, XTILE, dict(LAYOUTS["iperm"], xtile_part_nnz=40_000),
                             True, digest=True)
    P.close(), F.close()


@pytest.mark.parametrize("family", ["xtile_iperm", "sell", "adaptive"])
def test_transpose_update_and_spmv_captured_in_a_graph(lhpc, gpu, family):
    """After its first update (which allocates), a device-values update of a
    TRANSPOSE plan is launches and asynchronous copies only: captured with
    lhpc_spmv on a side stream and replayed, it gives the fresh plan's bits."""
    import torch
    shape, flags, options, _ = FAMILIES[family]
    rp, col, n_cols, a_rp, a_col, _ = _matrix(shape)
    n = rp.size - 1
    v0, v1 = _rand(col.size, np.float32, 21), _rand(col.size, np.float32, 22)
    xd, vbuf = _dev(gpu, _rand(n_cols, np.float32, 23)), _dev(gpu, v0)
    with lhpc.SpMVPlan(a_rp, a_col, v0, n, flags=flags, options=options, transpose=True) as P, \
            lhpc.SpMVPlan(a_rp, a_col, v1, n, flags=flags, options=options, transpose=True) as F:
        P.set_values(vbuf)  # the first update
        y = torch.full((n,), float("nan"), dtype=xd.dtype, device=gpu)
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
        if flags == XTILE:
            assert P.layout_digest() == F.layout_digest()


def test_set_values_refusals_are_unchanged(lhpc, gpu):
    """XSLICE and column-block plans refuse (and stay as they were), a wrong
    nnz is LHPC_ERR_INVALID_ARG, for TRANSPOSE plans as for any other."""
    rp, col, n_cols, a_rp, a_col, _ = _matrix("long")
    n = rp.size - 1
    v0, v1 = _rand(col.size, np.float32, 31), _rand(col.size, np.float32, 32)
    xd, vd = _dev(gpu, _rand(n_cols, np.float32, 33)), _dev(gpu, v1)
    for kw in (dict(flags=XSLICE), dict(flags=XTILE, options={"xtile_col_blocks": 2})):
        with lhpc.SpMVPlan(a_rp, a_col, v0, n, transpose=True, **kw) as P:
            y0, b0 = P(xd).clone(), P.info()["device_bytes"]
            for val in (vd, v1):
                with pytest.raises(lhpc.LhpcError) as e:
                    P.set_values(val)
                assert e.value.status == -5
            assert _same(P(xd), y0) and P.info()["device_bytes"] == b0  # refused before the buffer is allocated
    rp, col, n_cols, a_rp, a_col, _ = _matrix("short")
    n = rp.size - 1
    v0, v1 = _rand(col.size, np.float32, 31), _rand(col.size, np.float32, 32)
    xd, vd = _dev(gpu, _rand(n_cols, np.float32, 33)), _dev(gpu, v1)
    with lhpc.SpMVPlan(a_rp, a_col, v0, n, flags=ADAPTIVE, transpose=True) as P:
        y0 = P(xd).clone()
        for nnz in (col.size - 1, col.size + 1, 0):
            assert lhpc.lib.lhpc_spmv_plan_set_values(P._h, vd.data_ptr(), nnz, 1, None) == -1
        assert lhpc.lib.lhpc_spmv_plan_set_values(P._h, None, col.size, 1, None) == -1
        assert _same(P(xd), y0)
    with lhpc.SpMMPlan(a_rp, a_col, v0, n, transpose=True) as M:
        assert lhpc.lib.lhpc_spmm_plan_set_values(M._h, vd.data_ptr(), col.size - 1, 1, None) == -1
    # a matrix without entries: nothing to do, nothing launched
    with lhpc.SpMVPlan(np.zeros(6, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32), 7, transpose=True) as P:
        import torch
        assert (P.n_rows, P.n_cols) == (7, 5)
        P.set_values(np.zeros(0, np.float32))
        assert torch.count_nonzero(P(torch.ones(5, device=gpu))).item() == 0


# ------------------------------------------------------------------ SpMM, the fused dots and the solvers
@pytest.mark.parametrize("device_input", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["f32", "f64"])
def test_spmm_and_dots_on_a_transpose_plan(lhpc, gpu, dt, device_input):
    """The small rectangular, non-symmetric "short" matrix: the TRANSPOSE SpMM
    plan against the SpMM plan of the transposed arrays (info but
    device_bytes, the bits of Y and of spmm_dot's dots), set_values in A's
    order, and spmv_dot on the TRANSPOSE SpMV plans (SELL: fused; XTILE: SpMV
    then dot)."""
    import torch
    rp, col, n_cols, a_rp, a_col, a_perm = _matrix("short")
    n = rp.size - 1
    b_val, b_val1 = _rand(col.size, dt, 41), _rand(col.size, dt, 42)
    put = (lambda a: _dev(gpu, a)) if device_input else (lambda a: a)
    rng = np.random.default_rng(43)
    with lhpc.SpMMPlan(put(a_rp), put(a_col), put(b_val[a_perm]), n, transpose=True) as T, \
            lhpc.SpMMPlan(rp, col, b_val, n_cols) as F, lhpc.SpMMPlan(rp, col, b_val1, n_cols) as F1:
        assert (T.n_rows, T.n_cols) == (n, n_cols)
        but = lambda p: {k: v for k, v in p.info().items() if k != "device_bytes"}  # noqa: E731
        assert but(T) == but(F) and T.info()["device_bytes"] >= F.info()["device_bytes"] + 4 * col.size
        for k in (3, 33):
            X = _dev(gpu, rng.uniform(-1, 1, (n_cols, k)).astype(dt))
            W = _dev(gpu, rng.uniform(-1, 1, (n, k)).astype(dt))
            assert _same(T(X), F(X))
            Yt, dt_ = lhpc.spmm_dot(T, X, W)
            Yf, df = lhpc.spmm_dot(F, X, W)
            torch.cuda.synchronize()
            assert _same(Yt, Yf) and _same(dt_, df)
        b = T.info()["device_bytes"]
        for val in (_dev(gpu, b_val1[a_perm]), b_val1[a_perm]):  # device values, then host values
            T.set_values(val)
            assert _same(T(X), F1(X)) and but(T) == but(F1)
            assert T.info()["device_bytes"] == b + col.size * np.dtype(dt).itemsize
            T.set_values(_dev(gpu, b_val[a_perm]))
            assert _same(T(X), F(X))
    for flags in (SELL, XTILE):
        with lhpc.SpMVPlan(put(a_rp), put(a_col), put(b_val[a_perm]), n, flags=flags, transpose=True) as T, \
                lhpc.SpMVPlan(rp, col, b_val, n_cols, flags=flags) as F:
            x, w = _dev(gpu, _rand(n_cols, dt, 44)), _dev(gpu, _rand(n, dt, 45))
            outs = []
            for plan in (T, F):
                y = torch.empty(n, dtype=x.dtype, device=gpu)
                d = torch.zeros(1, dtype=torch.float64, device=gpu)
                lhpc.spmv_dot(plan, x, y, w, d)
                torch.cuda.synchronize()
                outs.append((y, d))
            assert _same(outs[0][0], outs[1][0]) and _same(outs[0][1], outs[1][1])


@pytest.mark.parametrize("flags,options", [(0, None), (SELL, None), (0, {"spmv_no_sell": 1})],
                         ids=["auto", "sell", "adaptive"])
def test_cg_on_a_transpose_plan(lhpc, gpu, flags, options):
    """The 64² Laplacian is symmetric with sorted rows, so Aᵀ's arrays are
    A's: the solve on the TRANSPOSE plan takes the same iterations and gives
    the same bits as on the plain plan — also after set_values (the shifted
    Laplacian) on the captured-graph path."""
    import torch
    rp, col, v0 = S.laplacian_2d(64, 64, dtype=np.float64, shift=0.0)
    _, _, v1 = S.laplacian_2d(64, 64, dtype=np.float64, shift=0.5)
    n = rp.size - 1
    b = _dev(gpu, np.random.default_rng(51).uniform(-1, 1, n))
    s = torch.cuda.Stream(gpu)
    kw = dict(tol=1e-10, max_iter=400, check_every=4, stream=s)
    # the initial guesses and the new values are made on torch's current stream and read on s, which does not
    # wait for it: they are complete before the first call that reads them
    x0 = [torch.zeros_like(b) for _ in range(4)]
    v1d = _dev(gpu, v1)
    torch.cuda.synchronize()
    with lhpc.SpMVPlan(rp, col, v0, n, flags=flags, options=options, transpose=True) as T, \
            lhpc.SpMVPlan(rp, col, v0, n, flags=flags, options=options) as F, \
            lhpc.SpMVPlan(rp, col, v1, n, flags=flags, options=options) as F1:
        assert _info_but_bytes(T) == _info_but_bytes(F)
        xt, itt, rt = lhpc.cg(T, b, x0[0], **kw)
        xf, itf, rf = lhpc.cg(F, b, x0[1], **kw)
        s.synchronize()
        assert (itt, rt) == (itf, rf) and itt > 4 and _same(xt, xf)
        T.set_values(v1d, stream=s)
        x1, it1, r1 = lhpc.cg(T, b, x0[2], **kw)
        xg, itg, rg = lhpc.cg(F1, b, x0[3], **kw)
        s.synchronize()
        assert (it1, r1) == (itg, rg) and _same(x1, xg) and not _same(x1, xt)


def test_cg_multi_on_a_transpose_plan(lhpc, gpu):
    import torch
    rp, col, v0 = S.laplacian_2d(64, 64, dtype=np.float64, shift=0.0)
    n, k = rp.size - 1, 4
    B = _dev(gpu, np.random.default_rng(52).uniform(-1, 1, (n, k)))
    s = torch.cuda.Stream(gpu)
    kw = dict(tol=1e-10, max_iter=400, check_every=4, stream=s)
    X0 = [torch.zeros_like(B) for _ in range(2)]  # made on torch's current stream, read on s
    torch.cuda.synchronize()
    with lhpc.SpMMPlan(rp, col, v0, n, transpose=True) as T, lhpc.SpMMPlan(rp, col, v0, n) as F:
        Xt, itt, rt = lhpc.cg_multi(T, B, X0[0], **kw)
        Xf, itf, rf = lhpc.cg_multi(F, B, X0[1], **kw)
        s.synchronize()
        assert np.array_equal(itt, itf) and np.array_equal(rt.view(np.uint64), rf.view(np.uint64)) and _same(Xt, Xf)
        assert itt.min() > 4


# ------------------------------------------------------------------ C++
def test_cpp_transpose_on_gpu(gpu):
    """tests/cpp/test_transpose_api.cpp (built by tests/cpp/transpose.mk):
    sparse::transpose against a host counting transposition, and transposed
    sparse::SpMVPlan / SpMMPlan against plans of the transposed matrix."""
    from tests.test_transpose_api import build_cpp
    r = subprocess.run([build_cpp()], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "transpose cpp api: ok" in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-2000:])
