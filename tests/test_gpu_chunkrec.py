"""XTILE fp32 reduce from per-chunk records (options.xtile_chunkrec = 2: the
plan's segment-start bitmap, segment bases and row-start bitmap copied to LDS
by LDS-DMA, instead of the segment scan and the row_ptr decode of every call)
against the same plan with the option off (1): y must be the same bytes.
Small forced-XTILE matrices only; every case builds its two plans once."""
import numpy as np
import pytest

from tests import _support as S

pytestmark = pytest.mark.gpu

XTILE = 1 << 9  # LHPC_PLAN_FORCE_XTILE
M = 8192        # nonzeros per fp32 reduce chunk
_CASES = {}


def _csr(lengths, n_cols, seed):
    """CSR with the given row lengths and sorted random columns (float32 U[-1, 1) values)."""
    rng = np.random.default_rng(seed)
    lengths = np.asarray(lengths, dtype=np.int64)
    rp = np.zeros(len(lengths) + 1, dtype=np.int32)
    np.cumsum(lengths, out=rp[1:])
    row = np.repeat(np.arange(len(lengths)), lengths)
    col = rng.integers(0, n_cols, size=int(rp[-1]))
    col = col[np.lexsort((col, row))].astype(np.int32)
    return rp, col, rng.uniform(-1.0, 1.0, size=col.size).astype(np.float32)


def _matrix(lhpc, shape, tiles):
    """(rp, col, val, n_cols, chunks or None) of a row shape; built once."""
    key = (shape, tiles)
    if key in _CASES:
        return _CASES[key]
    n_cols = 40960 * tiles - 7  # the last tile is partial
    chunks = None
    if shape == "uniform15":
        rp, col, val = lhpc.gen_uniform_csr(30000, n_cols, 15, dtype=lhpc.F32, dist=1, seed=0xC11 + tiles)
    elif shape == "powerlaw":
        rp, col, val = lhpc.gen_powerlaw_csr(20000, n_cols, lmax=3000, dtype=lhpc.F32, dist=1, seed=0xC12 + tiles)
    elif shape == "long_row":  # one row of more than 8192 nonzeros, crossing two chunk ends
        rp, col, val = _csr([15] * 40 + [20000] + [15] * 600 + [3] * 50, n_cols, 0xC13)
    elif shape == "nnz1":
        rp, col, val = _csr([1], n_cols, 0xC14)
        chunks = 1
    elif shape == "full_chunk_then_1":  # chunk 0: m = M, its row ends on the chunk end; last chunk: 1 nonzero
        rp, col, val = _csr([M, 1], n_cols, 0xC15)
        chunks = 2
    elif shape == "ends_on_chunk_end":  # no row start in the back M/32 of the window, a row end at M
        rp, col, val = _csr([7000, M - 7000] + [15] * 1000 + [M - 100, 100] + [16] * 1024 + [2 * M] + [7], n_cols, 0xC16)
    elif shape == "short_rows":  # chunks of the most rows a chunk owns (M/8), one with its last row running on
        rp, col, val = _csr([1] * 1023 + [9000] + [2] * 3000 + [1] * 500 + [3] * 700 + [1] * 2048, n_cols, 0xC1A)
    elif shape == "mixed":  # the pinned layouts' matrix without its empty rows
        rp, col, val = _csr([20000] + [3] * 50 + [5000, 4096, 4095, 1, 9000] + [15] * 30000 + [30000], n_cols, 0xC17)
    else:
        raise KeyError(shape)
    _CASES[key] = (rp, col, val.astype(np.float32), n_cols, chunks)
    return _CASES[key]


def _both(lhpc, gpu, rp, col, val, n_cols, x, opts=None, splits=None, want_on=True):
    """y (numpy) of the record plan and of the plan with the option off."""
    import torch
    xd = torch.from_numpy(x).to(gpu)
    ys, infos = [], []
    for rec in (2, 1):
        o = dict(opts or {}, xtile_chunkrec=rec)
        with lhpc.SpMVPlan(rp, col, val, n_cols, flags=XTILE, options=o, splits=splits) as plan:
            info = plan.info()
            assert info["kernel"] == lhpc.KERNEL_XTILE
            assert info.get("xtile_chunkrec", 0) == (1 if rec == 2 and want_on else 0)
            for _ in range(2):  # the second call reads what the first left in carry
                y = plan(xd)
            ys.append(y.cpu().numpy())
            infos.append(info)
    return ys, infos


def _x(n_cols, seed=0xC1F0):
    return np.random.default_rng(seed).uniform(-1, 1, n_cols).astype(np.float32)


@pytest.mark.parametrize("ranges", [1, 3])
@pytest.mark.parametrize("shape,tiles", [
    ("uniform15", 3), ("uniform15", 256), ("powerlaw", 3), ("powerlaw", 256), ("mixed", 3), ("mixed", 256),
    ("short_rows", 3), ("short_rows", 256), ("long_row", 3), ("nnz1", 3), ("full_chunk_then_1", 3), ("ends_on_chunk_end", 3)])
def test_chunkrec_matches_row_ptr_reduce(lhpc, gpu, shape, tiles, ranges):
    """Option 2 against option 1, same bytes of y: uniform 15 per row,
    power-law rows, rows of 4095 / 4096 / 5000 / 9000 / 20000 / 30000
    nonzeros, chunks of 1024 rows of 1–3 nonzeros (their y staged in LDS), a
    single nonzero, a full chunk followed by a last chunk of one nonzero, rows
    ending exactly on a chunk end — 3 and 256 tiles, one range and three ring
    ranges.  The base case is also held to the oracle."""
    rp, col, val, n_cols, chunks = _matrix(lhpc, shape, tiles)
    x = _x(n_cols)
    (y2, y1), (i2, i1) = _both(lhpc, gpu, rp, col, val, n_cols, x, {"xtile_reduce": 2, "xtile_ranges": ranges})
    assert y2.tobytes() == y1.tobytes()
    assert i2["n_blocks"] == i1["n_blocks"] and i2["device_bytes"] > i1["device_bytes"]
    if chunks is not None:
        assert i2["n_blocks"] == chunks
    if shape == "uniform15" and tiles == 3 and ranges == 1:
        _, yr, asum = S.spmv_oracle(rp, col, val, x)
        S.assert_spmv_close(y2, yr, asum)


@pytest.mark.parametrize("shape", ["uniform15", "mixed"])
def test_chunkrec_non_finite_x(lhpc, gpu, shape):
    """NaN and ±Inf entries of x reach the same rows with the same bits."""
    rp, col, val, n_cols, _ = _matrix(lhpc, shape, 3)
    x = _x(n_cols, 0xC1F1)
    x[::1009] = np.nan
    x[5::2003] = np.inf
    x[11::3001] = -np.inf
    (y2, y1), _ = _both(lhpc, gpu, rp, col, val, n_cols, x, {"xtile_reduce": 2})
    assert np.isnan(y1).any() and np.isinf(y1).any() and np.isfinite(y1).any()
    assert np.array_equal(y2, y1, equal_nan=True)


def test_chunkrec_empty_row_falls_back(lhpc, gpu):
    """A row without nonzeros has no bit in the record: the plan keeps the
    row_ptr reduce (info shows the variant off) and y is the same."""
    rp, col, val = _csr([15] * 700 + [0] + [15] * 700 + [9000, 0, 0, 3], 40960 * 3 - 7, 0xC18)
    n_cols = 40960 * 3 - 7
    x = _x(n_cols)
    (y2, y1), _ = _both(lhpc, gpu, rp, col, val, n_cols, x, {"xtile_reduce": 2}, want_on=False)
    assert y2.tobytes() == y1.tobytes()
    _, yr, asum = S.spmv_oracle(rp, col, val, x)
    S.assert_spmv_close(y2, yr, asum)


def test_chunkrec_column_blocks_fall_back(lhpc, gpu):
    """Column blocks (every block after the first adds into y): all blocks
    keep the row_ptr reduce, info shows the variant off, y is the same."""
    rp, col, val, n_cols, _ = _matrix(lhpc, "uniform15", 256)
    x = _x(n_cols)
    (y2, y1), (i2, i1) = _both(lhpc, gpu, rp, col, val, n_cols, x, {"xtile_reduce": 2, "xtile_col_blocks": 2},
                               want_on=False)
    assert y2.tobytes() == y1.tobytes() and i2 == i1


def test_chunkrec_excludes_phase_tables(lhpc, gpu):
    """xtile_pretable = 2 asked for together with the records: the phase-A
    tables win, the variant is off."""
    rp, col, val, n_cols, _ = _matrix(lhpc, "uniform15", 3)
    (y2, y1), _ = _both(lhpc, gpu, rp, col, val, n_cols, _x(n_cols), {"xtile_reduce": 2, "xtile_pretable": 2},
                        want_on=False)
    assert y2.tobytes() == y1.tobytes()


def test_chunkrec_set_values(lhpc, gpu):
    """lhpc_spmv_plan_set_values on a record plan (the values are not in the
    record): the next call gives the y of a plan built from the new values."""
    import torch
    rp, col, val, n_cols, _ = _matrix(lhpc, "mixed", 3)
    x = _x(n_cols)
    xd = torch.from_numpy(x).to(gpu)
    val2 = np.random.default_rng(0xC19).uniform(-1, 1, val.size).astype(np.float32)
    opts = {"xtile_reduce": 2, "xtile_chunkrec": 2}
    with lhpc.SpMVPlan(rp, col, val, n_cols, flags=XTILE, options=opts) as plan:
        assert plan.info()["xtile_chunkrec"] == 1
        plan(xd)
        plan.set_values(val2)
        y = plan(xd).cpu().numpy()
    with lhpc.SpMVPlan(rp, col, val2, n_cols, flags=XTILE, options=dict(opts, xtile_chunkrec=1)) as plan:
        want = plan(xd).cpu().numpy()
    assert y.tobytes() == want.tobytes()


def test_chunkrec_range_on_ring_split_plan(lhpc, gpu):
    """A row-range plan with xtile_ring = 2 (the per-rank plans' form): whole
    calls of the record plan with two ring ranges give the off plan's bytes;
    without cache ranges the same options leave lhpc_spmv_range usable, and
    each range is reduced from the records."""
    import torch
    rp, col, val, n_cols, _ = _matrix(lhpc, "mixed", 3)
    n = len(rp) - 1
    splits = [55, 56, 9000, n - 2]
    x = _x(n_cols)
    (y2, y1), _ = _both(lhpc, gpu, rp, col, val, n_cols, x,
                        {"xtile_reduce": 2, "xtile_ranges": 2, "xtile_ring": 2}, splits=splits)
    assert y2.tobytes() == y1.tobytes()
    xd = torch.from_numpy(x).to(gpu)
    with lhpc.SpMVPlan(rp, col, val, n_cols, flags=XTILE, splits=splits,
                       options={"xtile_reduce": 2, "xtile_ring": 2, "xtile_chunkrec": 2}) as plan:
        assert plan.info()["xtile_chunkrec"] == 1
        plan.stage(xd)
        out = torch.full((n,), 7.0, dtype=torch.float32, device=gpu)
        for k in reversed(range(len(splits) + 1)):
            plan.range(k, out[plan.splits[k]:plan.splits[k + 1]])
        assert out.cpu().numpy().tobytes() == y1.tobytes()


def test_chunkrec_device_input_records_match_host(lhpc, gpu):
    """A plan built from device-resident CSR holds the host build's records
    byte for byte (FNV-1a digest), the same layout digests as the plan with
    the option off, and gives the same y."""
    import torch
    rp, col, val, n_cols, _ = _matrix(lhpc, "powerlaw", 3)
    opts = {"xtile_reduce": 2, "xtile_ranges": 3, "xtile_chunkrec": 2}
    xd = torch.from_numpy(_x(n_cols)).to(gpu)
    with lhpc.SpMVPlan(rp, col, val, n_cols, flags=XTILE, options=dict(opts, xtile_host_build=1)) as ph:
        on_h, rec_h = ph.chunkrec()
        dig_h, y_h = ph.layout_digest(), ph(xd).cpu().numpy()
    drp, dcol, dval = (torch.from_numpy(np.ascontiguousarray(a)).to(gpu) for a in (rp, col, val))
    with lhpc.SpMVPlan(drp, dcol, dval, n_cols, flags=XTILE, options=opts) as pd:
        on_d, rec_d = pd.chunkrec()
        dig_d, y_d = pd.layout_digest(), pd(xd).cpu().numpy()
    with lhpc.SpMVPlan(rp, col, val, n_cols, flags=XTILE, options=dict(opts, xtile_chunkrec=1)) as p1:
        on_1, rec_1 = p1.chunkrec()
        dig_1 = p1.layout_digest()
    assert (on_h, on_d, on_1) == (1, 1, 0)
    assert rec_h == rec_d and rec_h != rec_1
    assert dig_h == dig_d == dig_1  # the records change none of the other layout arrays
    assert y_h.tobytes() == y_d.tobytes()
