"""lhpc_sptrsv against lhpc_spmv of the same triangle, and the chain_rows sweep.

The D + L triangle of the 4096² 5-point Laplacian (diagonal 4, off-diagonals
−1; 16.8M rows, 50.3M entries), fp64 and fp32, in two orderings:
  natural    cell (ix, iy) at row iy·4096 + ix: 8191 levels of ≤ 4096 rows
  red_black  the cells with even ix + iy first: 2 levels of 8.4M rows
Per dtype and ordering, in one run:
  sptrsv_ms        one lhpc_sptrsv call at the automatic chain_rows
  launches, padded_per_kept (padded_entries / kept off-diagonal entries)
  spmv_ms          one lhpc_spmv of an automatic SpMVPlan of the same
                   triangular matrix: the same bytes with no dependencies
  ratio            sptrsv_ms / spmv_ms
  us_per_launch    sptrsv_ms / launches
and on the natural order the sweep chain_rows ∈ {−1, 256, 1024, 4096, 16384}
(ms and launches each), which is what the automatic value is chosen from.
Method: b and x resident in HBM, 2 warm-up calls, 5 timed calls
with HIP events around each, median.  The solve is checked against the
residual b − T·x (computed with the SpMV plan) before it is timed.
Every dtype runs in a child process of its own under a time limit; after a
child that fails or runs out of time nothing more is started.  Prints one JSON
line and writes it to --out (default profiles/r14/sptrsv.json).

  python tools/bench_sptrsv.py [--dtypes f64,f32] [--n 4096] [--out PATH]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SWEEP = (-1, 256, 1024, 4096, 16384)
WARMUP, REPS = 2, 5
CHILD_LIMIT_S = 420


def _median_ms(torch, fn):
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(REPS)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return statistics.median(a.elapsed_time(b) for a, b in ev)


def lower_triangle(np, nx, ny, red_black, dtype):
    """(row_ptr int64, col_idx, val) of D + L of the 5-point Laplacian in the
    given ordering, columns ascending in every row (the diagonal last)."""
    n = nx * ny
    cell = np.arange(n, dtype=np.int64)
    if red_black:
        cell_of_row = np.argsort((cell % nx + cell // nx) % 2, kind="stable")
        index = np.empty(n, dtype=np.int64)
        index[cell_of_row] = cell
    else:
        cell_of_row = index = cell
    c = cell_of_row
    ix, iy = c % nx, c // nx
    # neighbours in ascending cell order (= ascending row index inside one colour), then the diagonal
    cand = np.stack([c - nx, c - 1, c + 1, c + nx, c], axis=1)
    ok = np.stack([iy > 0, ix > 0, ix < nx - 1, iy < ny - 1, np.ones(n, bool)], axis=1)
    cols = index[np.where(ok, cand, 0)]
    keep = ok & (cols <= np.arange(n)[:, None])
    rp = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(keep.sum(axis=1), out=rp[1:])
    val = np.where(cand == c[:, None], 4.0, -1.0).astype(dtype)
    return rp, cols[keep].astype(np.int32), val[keep]


def run_dtype(dtype, nx):
    import numpy as np
    import torch

    import libhpc_amd as L
    if L.device_count() < 1 or not torch.cuda.is_available():
        raise SystemExit("bench_sptrsv needs a gfx950 device (no CPU fallback)")
    dev = torch.device("cuda:0")
    npdt, tdt = (np.float32, torch.float32) if dtype == "f32" else (np.float64, torch.float64)
    n = nx * nx
    gen = torch.Generator(device=dev).manual_seed(0x5EED0014)
    b = torch.rand(n, dtype=tdt, device=dev, generator=gen) * 2 - 1
    x = torch.empty_like(b)
    out = dict(dtype=dtype, n=n, orderings={})
    for order in ("red_black", "natural"):
        rp, col, val = lower_triangle(np, nx, nx, order == "red_black", npdt)
        o = dict(nnz=int(col.size))
        with L.SpMVPlan(rp, col, val, n) as mv:
            o["spmv_kernel"] = mv.info()["kernel"]
            y = torch.empty_like(b)
            o["spmv_ms"] = _median_ms(torch, lambda: mv(b, y))
            for chain_rows in ((0,) + SWEEP if order == "natural" else (0,)):
                with L.SpTRSVPlan(rp, col, val, chain_rows=chain_rows) as plan:
                    inf = plan.info()
                    plan(b, x)
                    # the solve solves: ‖b − T·x‖∞ at rounding level of |b| ≤ 1 (rows of ≤ 5 entries)
                    resid = float((b - mv(x)).abs().max())
                    assert resid <= (1e-5 if dtype == "f32" else 1e-13), resid
                    ms = _median_ms(torch, lambda: plan(b, x))
                rec = dict(chain_rows=inf["chain_rows"], ms=ms, launches=inf["launches"])
                if chain_rows == 0:
                    o.update(sptrsv_ms=ms, launches=inf["launches"], n_levels=inf["n_levels"],
                             max_level_rows=inf["max_level_rows"], kept=inf["nnz"],
                             padded_per_kept=inf["padded_entries"] / max(inf["nnz"], 1),
                             ratio=ms / o["spmv_ms"], us_per_launch=1e3 * ms / max(inf["launches"], 1),
                             residual_max=resid)
                else:
                    o.setdefault("sweep", []).append(rec)
                print(f"bench_sptrsv: {dtype} {order} chain_rows {inf['chain_rows']}: {ms:.3f} ms, "
                      f"{inf['launches']} launches (spmv {o['spmv_ms']:.3f} ms)", file=sys.stderr, flush=True)
        out["orderings"][order] = o
        del rp, col, val
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--dtypes", default="f64,f32")
    ap.add_argument("--n", type=int, default=4096, help="grid side")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14", "sptrsv.json"))
    ap.add_argument("--child", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        print(json.dumps(run_dtype(a.child, a.n)), flush=True)
        return 0
    res = dict(tool="bench_sptrsv", matrix=f"D + L of laplacian_2d {a.n}x{a.n}",
               method=dict(warmup=WARMUP, reps=REPS, timer="hip events around one call, median",
                           sweep=list(SWEEP), yardstick="lhpc_spmv, automatic plan of the same triangle"), dtypes=[])
    status = 0
    for dtype in a.dtypes.split(","):
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", dtype, "--n", str(a.n)],
                               stdout=subprocess.PIPE, text=True, timeout=CHILD_LIMIT_S)  # progress on stderr
        except subprocess.TimeoutExpired:
            res["dtypes"].append(dict(dtype=dtype, error=f"time limit of {CHILD_LIMIT_S} s"))
            status = 1
            break  # nothing more on the GPU after a step that did not end
        if r.returncode != 0:
            res["dtypes"].append(dict(dtype=dtype, error=f"exit status {r.returncode}"))
            status = 1
            break
        res["dtypes"].append(json.loads(r.stdout.strip().splitlines()[-1]))
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line, flush=True)
    return status


if __name__ == "__main__":
    sys.exit(main())
