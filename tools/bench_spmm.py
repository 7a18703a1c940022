"""Y = A·X (lhpc_spmm) against k calls of lhpc_spmv, timed in the same run.

Method: A and X resident in HBM, 5 warm-ups, 50 timed repetitions
with HIP events around each repetition, median.  For every shape and
k in {1, 2, 4, 8, 16, 32, 64}:
  spmm_ms            one lhpc_spmm call on a row-major n_cols × k block
  spmv_auto_ms       k lhpc_spmv calls on the automatic plan — the only way to
                     compute A·X without lhpc_spmm
  spmv_adaptive_ms   k lhpc_spmv calls on a FORCE_ADAPTIVE plan (the CSR-keeping
                     kernel lhpc_spmm's block table comes from)
  gflops             2·nnz·k / spmm time
  bytes              algorithmic: A (col, val, row_ptr) once per 32-column panel,
                     X and Y once
Shapes: C2 (n = 10M, 15 per row) in fp32 and fp64, the 4096² Laplacian in fp64.

Every shape runs in a child process of its own under a time limit; after a
child that fails or runs out of time nothing more is started.  Prints one
JSON line and writes it to --out (default profiles/r07/spmm.json).

  python tools/bench_spmm.py [--shapes c2_f32,c2_f64,lap4096_f64] [--out PATH]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KS = (1, 2, 4, 8, 16, 32, 64)
WARMUP, REPS = 5, 50
SHAPES = ("c2_f32", "c2_f64", "lap4096_f64")
CHILD_LIMIT_S = 420


def _matrix(L, shape):
    if shape.startswith("c2_"):
        n = 10_000_000
        rp, col, val = L.gen_uniform_csr(n, n, 15, dtype=L.F32 if shape.endswith("f32") else L.F64)
        return rp, col, val, n
    if shape == "lap4096_f64":
        rp, col, val = L.gen_laplacian_2d(4096, 4096, L.F64)
        return rp, col, val, 4096 * 4096
    raise SystemExit(f"unknown shape {shape}")


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


def run_shape(shape):
    import torch

    import libhpc_amd as L
    if L.device_count() < 1 or not torch.cuda.is_available():
        raise SystemExit("bench_spmm needs a gfx950 device (no CPU fallback)")
    dev = torch.device("cuda:0")
    rp, col, val, n_cols = _matrix(L, shape)
    n_rows, nnz, tsz = rp.shape[0] - 1, int(col.shape[0]), val.dtype.itemsize
    tdt = torch.float32 if tsz == 4 else torch.float64
    a_bytes = nnz * (4 + tsz) + (n_rows + 1) * rp.dtype.itemsize
    out = dict(shape=shape, dtype="f32" if tsz == 4 else "f64", n_rows=n_rows, n_cols=n_cols, nnz=nnz, results=[])
    gen = torch.Generator(device=dev).manual_seed(0x5EED0002)
    with L.SpMMPlan(rp, col, val, n_cols) as mm, L.SpMVPlan(rp, col, val, n_cols) as auto, \
            L.SpMVPlan(rp, col, val, n_cols, flags=L.PLAN_FORCE_ADAPTIVE) as adaptive:
        out["spmv_auto_kernel"] = auto.info()["kernel"]
        out["spmm_blocks"] = mm.info()["n_blocks"]
        for k in KS:
            X = torch.rand((n_cols, k), dtype=tdt, device=dev, generator=gen) * 2 - 1
            Y = torch.empty((n_rows, k), dtype=tdt, device=dev)
            xs = X.t().contiguous()  # the same vectors, one contiguous x per lhpc_spmv call
            ys = torch.empty((k, n_rows), dtype=tdt, device=dev)

            def loop(plan):
                for j in range(k):
                    plan(xs[j], ys[j])

            t_mm = _median_ms(torch, lambda: mm(X, Y))
            t_auto = _median_ms(torch, lambda: loop(auto))
            # same seeded inputs, both ways: the results must agree to the SpMV bar's order
            err = float((Y.t() - ys).abs().max())
            t_ad = _median_ms(torch, lambda: loop(adaptive))
            panels = (k + 31) // 32
            nbytes = panels * a_bytes + (n_cols + n_rows) * k * tsz
            out["results"].append(dict(
                k=k, spmm_ms=t_mm, spmv_auto_ms=t_auto, spmv_adaptive_ms=t_ad, ratio_vs_auto=t_mm / t_auto,
                ratio_vs_adaptive=t_mm / t_ad, gflops=2.0 * nnz * k / (t_mm * 1e6), bytes=nbytes,
                gbytes_per_s=nbytes / (t_mm * 1e6), max_abs_diff_vs_auto=err))
            del X, Y, xs, ys
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07", "spmm.json"))
    ap.add_argument("--child", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        print(json.dumps(run_shape(a.child)), flush=True)
        return 0
    res = dict(tool="bench_spmm", method=dict(warmup=WARMUP, reps=REPS, timer="hip events, median"), shapes=[])
    status = 0
    for shape in a.shapes.split(","):
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", shape], capture_output=True,
                               text=True, timeout=CHILD_LIMIT_S)
        except subprocess.TimeoutExpired:
            res["shapes"].append(dict(shape=shape, error=f"time limit of {CHILD_LIMIT_S} s"))
            status = 1
            break  # nothing more on the GPU after a step that did not end
        if r.returncode != 0:
            res["shapes"].append(dict(shape=shape, error=f"exit status {r.returncode}", stderr=r.stderr[-1500:]))
            status = 1
            break
        res["shapes"].append(json.loads(r.stdout.strip().splitlines()[-1]))
        print(f"bench_spmm: {shape} done", file=sys.stderr, flush=True)
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line, flush=True)
    return status


if __name__ == "__main__":
    sys.exit(main())
