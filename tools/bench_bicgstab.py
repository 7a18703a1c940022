"""One lhpc_bicgstab_solve iteration against one lhpc_cg_solve iteration, and
against the HBM roofline.

4096² grid, fp64 and fp32.  BiCGStab runs on the 5-point upwind
convection–diffusion operator (diagonal 4.5, west −1.5, east −0.5, south −1.25,
north −0.75: not symmetric), CG on the same run's 5-point Laplacian (same
structure, so the same kernel family and bytes per SpMV).  Both solvers run a
fixed number of iterations (tol = 0, check_every = 8) twice, 8 and 24
iterations; the time of one iteration is the difference over 16, so the set-up
pass (A·x0, r, the first dots, the copies of x) cancels.  24 iterations end
before either solver has converged (BiCGStab needs 46 at 1e-10 in fp64, 22 at
1e-5 in fp32), so the device latch is still open and no iteration is a no-op;
the returned iteration count is asserted.
Method: b and x resident in HBM, 2 warm-up solves, 5 timed
solves with HIP events around each, median.  Per dtype:
  bicgstab_ms_per_iter, cg_ms_per_iter, ratio = bicgstab / cg
  bytes_per_iter   algorithmic: 2 SpMVs (nnz·(value + 4-B column) each) and 20
                   vector passes of n values (DESIGN.md §4.2 BiCGStab)
  gbps, of_8tbs    bytes_per_iter over the iteration's time, and over 8 TB/s
Every dtype runs in a child process of its own under a time limit; after a
child that fails or runs out of time nothing more is started.  Prints one JSON
line and writes it to --out (default profiles/r13/bicgstab.json).

  python tools/bench_bicgstab.py [--dtypes f64,f32] [--out PATH]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NX = NY = 4096
SHIFT = 0.5
LO, HI, CHECK_EVERY = 8, 24, 8
WARMUP, REPS = 2, 5
VECTOR_PASSES = 20  # p r̂ v | r v s | s t | t | x p s t r̂ x r | r p v p
PEAK_BYTES_PER_S = 8e12
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


def upwind_values(np, rp, col, dtype):
    """the Laplacian's structure with the convection–diffusion values, chosen by col − row"""
    row = np.repeat(np.arange(rp.shape[0] - 1, dtype=np.int32), np.diff(rp))
    d = col - row
    val = np.full(col.shape[0], 4.0 + SHIFT, dtype=dtype)
    for off, v in ((-1, -1.5), (1, -0.5), (-NX, -1.25), (NX, -0.75)):
        val[d == off] = v
    return val


def run_dtype(dtype):
    import numpy as np
    import torch

    import libhpc_amd as L
    if L.device_count() < 1 or not torch.cuda.is_available():
        raise SystemExit("bench_bicgstab needs a gfx950 device (no CPU fallback)")
    dev = torch.device("cuda:0")
    rp, col, lap = L.gen_laplacian_2d(NX, NY, L.F32 if dtype == "f32" else L.F64)
    n, nnz = rp.shape[0] - 1, int(col.shape[0])
    val = upwind_values(np, rp, col, lap.dtype)
    tdt, tsz = (torch.float32, 4) if dtype == "f32" else (torch.float64, 8)
    gen = torch.Generator(device=dev).manual_seed(0x5EED0013)
    b = torch.rand(n, dtype=tdt, device=dev, generator=gen) * 2 - 1
    x = torch.zeros(n, dtype=tdt, device=dev)
    stream = torch.cuda.current_stream(dev)
    out = dict(dtype=dtype, n=n, nnz=nnz, lo=LO, hi=HI, check_every=CHECK_EVERY)

    def per_iter(plan, solver):
        ms = {}
        for iters in (LO, HI):
            def solve():
                x.zero_()
                _, it, res = solver(plan, b, x, tol=0.0, max_iter=iters, check_every=CHECK_EVERY, stream=stream)
                assert it == iters and res > 0.0, (it, res)  # still iterating: no frozen iteration was timed
            ms[iters] = _median_ms(torch, solve)
        return (ms[HI] - ms[LO]) / (HI - LO), ms

    with L.SpMVPlan(rp, col, val, n) as plan:
        out["kernel"] = plan.info()["kernel"]
        t_bi, ms = per_iter(plan, L.bicgstab)
        out["bicgstab_solve_ms"] = {str(k): v for k, v in ms.items()}
    del val
    with L.SpMVPlan(rp, col, lap, n) as plan:
        out["cg_kernel"] = plan.info()["kernel"]
        t_cg, ms = per_iter(plan, L.cg)
        out["cg_solve_ms"] = {str(k): v for k, v in ms.items()}
    bytes_per_iter = 2 * nnz * (tsz + 4) + VECTOR_PASSES * n * tsz
    gbps = bytes_per_iter / (t_bi * 1e-3) / 1e9
    out.update(bicgstab_ms_per_iter=t_bi, cg_ms_per_iter=t_cg, ratio=t_bi / t_cg, bytes_per_iter=bytes_per_iter,
               gbps=gbps, of_8tbs=gbps * 1e9 / PEAK_BYTES_PER_S)
    assert np.isfinite([t_bi, t_cg]).all() and t_bi > 0 and t_cg > 0
    print(f"bench_bicgstab: {dtype} bicgstab {t_bi:.3f} ms/iter, cg {t_cg:.3f} ms/iter, {gbps:.0f} GB/s",
          file=sys.stderr, flush=True)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--dtypes", default="f64,f32")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13", "bicgstab.json"))
    ap.add_argument("--child", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        print(json.dumps(run_dtype(a.child)), flush=True)
        return 0
    res = dict(tool="bench_bicgstab", matrix=f"upwind convection-diffusion {NX}x{NY} shift {SHIFT}",
               cg_matrix=f"laplacian_2d {NX}x{NY}",
               method=dict(warmup=WARMUP, reps=REPS, timer="hip events around a whole solve, median",
                           per_iter=f"(solve of {HI} iterations - solve of {LO}) / {HI - LO}",
                           check_every=CHECK_EVERY, tol=0.0, vector_passes=VECTOR_PASSES,
                           peak_bytes_per_s=PEAK_BYTES_PER_S), dtypes=[])
    status = 0
    for dtype in a.dtypes.split(","):
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", dtype],
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
