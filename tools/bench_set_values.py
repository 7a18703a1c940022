"""lhpc_spmv_plan_set_values against the two things it stands between, timed in
the same run with the matrix and both value sets resident in HBM:
  set_values_ms   (a) plan.set_values(v1) with device values: HIP events around
                  each call, 5 warm-ups (the first also makes a SELL plan's row
                  offsets), median of 30
  create_ms       (b) a fresh lhpc_spmv_plan_create from the device-resident
                  CSR (LHPC_PLAN_DEVICE_INPUT) with the new values — what a
                  caller pays without set_values.  The call is synchronous host
                  and device work, so it is timed on the host clock between
                  device synchronisations: 1 warm-up, median of 5
  copy_ms         (c) a device-to-device hipMemcpyAsync of nnz·sizeof(T)
                  (torch's copy_ of a contiguous tensor): the floor for reading
                  and writing the values once; events, 5 warm-ups, median of 30
and the ratios (a)/(b), (a)/(c).  After the timed updates the plan's y must
equal the fresh plan's bit for bit (matches_fresh), and for XTILE its layout
digests too.
Shapes: C2 (n = 10M, 15 per row, fp32), C3 (the same in fp64) — XTILE — and
the 4096² Laplacian (fp64, SELL).

Every shape runs in a child process of its own under a time limit; after a
child that fails or runs out of time nothing more is started.  Prints one
JSON line and writes it to --out (default profiles/r10/set_values.json).

  python tools/bench_set_values.py [--shapes c2_f32,c3_f64,lap4096_f64] [--out PATH]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WARMUP, REPS, CREATE_REPS = 5, 30, 5
SHAPES = ("c2_f32", "c3_f64", "lap4096_f64")
CHILD_LIMIT_S = 420
KERNELS = {0: "ROWGROUP", 1: "ADAPTIVE", 2: "XSLICE", 3: "XTILE", 4: "SELL"}


def _matrix(L, shape):
    if shape in ("c2_f32", "c3_f64"):
        n = 10_000_000
        rp, col, val = L.gen_uniform_csr(n, n, 15, dtype=L.F32 if shape == "c2_f32" else L.F64)
        return rp, col, val, n
    if shape == "lap4096_f64":
        rp, col, val = L.gen_laplacian_2d(4096, 4096, L.F64)
        return rp, col, val, 4096 * 4096
    raise SystemExit(f"unknown shape {shape}")


def _median_ms(torch, fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return statistics.median(a.elapsed_time(b) for a, b in ev)


def run_shape(shape):
    import numpy as np
    import torch

    import libhpc_amd as L
    if L.device_count() < 1 or not torch.cuda.is_available():
        raise SystemExit("bench_set_values needs a gfx950 device (no CPU fallback)")
    dev = torch.device("cuda:0")
    rp, col, val, n_cols = _matrix(L, shape)
    n_rows, nnz, tsz = rp.shape[0] - 1, int(col.shape[0]), val.dtype.itemsize
    d_rp, d_col, d_v0 = (torch.from_numpy(a).to(dev) for a in (rp, col, val))
    gen = torch.Generator(device=dev).manual_seed(0x5EED0003)
    d_v1 = torch.rand(nnz, dtype=d_v0.dtype, device=dev, generator=gen) * 2 - 1
    x = torch.rand(n_cols, dtype=d_v0.dtype, device=dev, generator=gen) * 2 - 1
    del rp, col, val

    def create(v):
        return L.SpMVPlan(d_rp, d_col, v, n_cols)

    out = dict(shape=shape, dtype="f32" if tsz == 4 else "f64", n_rows=n_rows, n_cols=n_cols, nnz=nnz,
               value_bytes=nnz * tsz)
    with create(d_v0) as plan:
        info = plan.info()
        out["kernel"] = KERNELS[info["kernel"]]
        out["device_bytes_before"] = info["device_bytes"]
        out["set_values_ms"] = _median_ms(torch, lambda: plan.set_values(d_v1), WARMUP, REPS)
        out["device_bytes_after"] = plan.info()["device_bytes"]
        scratch = torch.empty_like(d_v1)
        out["copy_ms"] = _median_ms(torch, lambda: scratch.copy_(d_v1), WARMUP, REPS)
        del scratch
        times = []
        for i in range(CREATE_REPS + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fresh = create(d_v1)
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1e3)
            if i < CREATE_REPS:
                fresh.close()
        out["create_ms"] = statistics.median(times[1:])
        out["spmv_ms"] = _median_ms(torch, lambda: plan(x), WARMUP, REPS)
        yp, yf = plan(x), fresh(x)
        torch.cuda.synchronize()
        out["matches_fresh"] = bool(np.array_equal(yp.cpu().numpy().view(np.uint8), yf.cpu().numpy().view(np.uint8)))
        if info["kernel"] == L.KERNEL_XTILE:
            out["matches_fresh"] = out["matches_fresh"] and plan.layout_digest() == fresh.layout_digest()
        fresh.close()
    out["set_values_over_create"] = out["set_values_ms"] / out["create_ms"]
    out["set_values_over_copy"] = out["set_values_ms"] / out["copy_ms"]
    out["set_values_gbytes_per_s"] = 2.0 * nnz * tsz / (out["set_values_ms"] * 1e6)  # values read once, written once
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10", "set_values.json"))
    ap.add_argument("--child", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        print(json.dumps(run_shape(a.child)), flush=True)
        return 0
    res = dict(tool="bench_set_values",
               method=dict(warmup=WARMUP, reps=REPS, create_reps=CREATE_REPS,
                           timer="hip events, median (create: host clock between device synchronisations, median)"),
               shapes=[])
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
        one = json.loads(r.stdout.strip().splitlines()[-1])
        res["shapes"].append(one)
        if not one["matches_fresh"] or one["set_values_ms"] >= one["create_ms"]:
            status = 1  # the update must equal a rebuild and cost less than one
        print(f"bench_set_values: {shape} done", file=sys.stderr, flush=True)
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line, flush=True)
    return status


if __name__ == "__main__":
    sys.exit(main())
