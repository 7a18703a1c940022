"""lhpc_cg_solve_multi against the loop it replaces: k calls of lhpc_cg_solve.

4096² 5-point Laplacian, fp64 and fp32, k in {1, 2, 4, 8, 16, 32}.  Both
solvers run a fixed number of iterations (tol = 0, max_iter = 100,
check_every = 10), so a solve's time divided by 100 is the time per
iteration (the set-up pass — A·x0, r, p, the first dots — is in it for both).
Method: B and X resident in HBM, 2 warm-up solves, 5 timed
solves with HIP events around each, median.  Per k:
  multi_ms_per_iter    lhpc_cg_solve_multi on the SpMM plan, k columns
  single_ms_per_iter   lhpc_cg_solve on the automatic SpMV plan (SELL on this
                       matrix, update fused into the SpMV), one column —
                       measured once per dtype in the same run
  ratio                multi / (k · single): below 1 the call pays
Every dtype runs in a child process of its own under a time limit; after a
child that fails or runs out of time nothing more is started.  Prints one
JSON line and writes it to --out (default profiles/r08/cg_multi.json).

  python tools/bench_cg_multi.py [--dtypes f64,f32] [--ks 1,2,4,8,16,32] [--out PATH]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KS = (1, 2, 4, 8, 16, 32)
NX = NY = 4096
ITERS, CHECK_EVERY = 100, 10
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


def run_dtype(dtype, ks):
    import numpy as np
    import torch

    import libhpc_amd as L
    if L.device_count() < 1 or not torch.cuda.is_available():
        raise SystemExit("bench_cg_multi needs a gfx950 device (no CPU fallback)")
    dev = torch.device("cuda:0")
    rp, col, val = L.gen_laplacian_2d(NX, NY, L.F32 if dtype == "f32" else L.F64)
    n = rp.shape[0] - 1
    tdt = torch.float32 if dtype == "f32" else torch.float64
    out = dict(dtype=dtype, n=n, nnz=int(col.shape[0]), iters=ITERS, check_every=CHECK_EVERY, results=[])
    gen = torch.Generator(device=dev).manual_seed(0x5EED0008)
    stream = torch.cuda.current_stream(dev)
    with L.SpMMPlan(rp, col, val, n) as mm, L.SpMVPlan(rp, col, val, n) as auto:
        out["spmv_auto_kernel"] = auto.info()["kernel"]
        b1 = torch.rand(n, dtype=tdt, device=dev, generator=gen) * 2 - 1
        x1 = torch.zeros(n, dtype=tdt, device=dev)

        def single():
            x1.zero_()
            _, it, _ = L.cg(auto, b1, x1, tol=0.0, max_iter=ITERS, check_every=CHECK_EVERY, stream=stream)
            assert it == ITERS, it

        t_single = _median_ms(torch, single) / ITERS
        out["single_ms_per_iter"] = t_single
        for k in ks:
            B = torch.rand((n, k), dtype=tdt, device=dev, generator=gen) * 2 - 1
            X = torch.zeros((n, k), dtype=tdt, device=dev)

            def multi():
                X.zero_()
                _, its, _ = L.cg_multi(mm, B, X, tol=0.0, max_iter=ITERS, check_every=CHECK_EVERY, stream=stream)
                assert (its == ITERS).all(), its

            t_multi = _median_ms(torch, multi) / ITERS
            # the same seeded column both ways: the two solvers must agree (different dot orders)
            B[:, 0] = b1
            multi()
            single()
            rel = float((X[:, 0] - x1).norm() / x1.norm())
            out["results"].append(dict(k=k, multi_ms_per_iter=t_multi, loop_ms_per_iter=k * t_single,
                                       ratio=t_multi / (k * t_single), rel_diff_column0_vs_single=rel,
                                       device_bytes=mm.info()["device_bytes"]))
            del B, X
            print(f"bench_cg_multi: {dtype} k={k} multi {t_multi:.3f} ms/iter, loop {k * t_single:.3f}",
                  file=sys.stderr, flush=True)
    assert np.isfinite([r["ratio"] for r in out["results"]]).all()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--dtypes", default="f64,f32")
    ap.add_argument("--ks", default=",".join(str(k) for k in KS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08", "cg_multi.json"))
    ap.add_argument("--child", help=argparse.SUPPRESS)
    a = ap.parse_args()
    ks = tuple(int(k) for k in a.ks.split(","))
    if a.child:
        print(json.dumps(run_dtype(a.child, ks)), flush=True)
        return 0
    res = dict(tool="bench_cg_multi", matrix=f"laplacian_2d {NX}x{NY}",
               method=dict(warmup=WARMUP, reps=REPS, timer="hip events around a whole solve, median",
                           iters=ITERS, check_every=CHECK_EVERY, tol=0.0), dtypes=[])
    status = 0
    for dtype in a.dtypes.split(","):
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", dtype, "--ks", a.ks],
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
