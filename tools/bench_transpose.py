"""lhpc_csr_transpose and LHPC_PLAN_TRANSPOSE against what they replace and the
floor under them, timed in one run per shape with A resident in HBM:
  transpose_ms      (a) lhpc_csr_transpose on device arrays (with perm).  The
                    call is synchronous (it ends with the stream drained), so
                    it is timed on the host clock between device
                    synchronisations: 2 warm-ups, median of 7
  coo_route_ms      (b) the only device route to the same matrix without it:
                    row_ptr expanded into row indices (torch.repeat_interleave)
                    and the swapped triples through lhpc_coo_to_csr; host
                    clock, 1 warm-up, median of 5.  expand_ms is the expansion
                    alone, coo_to_csr_ms the rest.  same_matrix: (b)'s arrays
                    equal (a)'s (they do when A has no duplicate coordinates,
                    which (b) merges)
  copy_ms           (c) device-to-device copies of A's row_ptr, col_idx and val:
                    the floor for reading and writing the matrix once; HIP
                    events, 5 warm-ups, median of 30
  create_transpose_ms / create_pretransposed_ms
                    (d) plan create with LHPC_PLAN_TRANSPOSE from A on the
                    device against plan create from the device CSR of Aᵀ;
                    host clock, 1 warm-up, median of 3
  set_values_transpose_ms / set_values_plain_ms
                    (e) set_values with device values on the transposed plan
                    (gather through perm + the family's update) against the
                    plain plan of Aᵀ; HIP events, 5 warm-ups (the first
                    allocates the staging buffer), median of 30
and the ratios (b)/(a), (a)/(c), (d), (e).  matches: the transposed plan's y
equals the y of the plan of Aᵀ bit for bit, before and after the updates (and
for XTILE the layout digests).
Shapes: C2 (n = 10M, 15 per row, fp32), C3 (the same in fp64) and the 4096²
Laplacian (fp64).

Every shape runs in a child process of its own under a time limit; after a
child that fails or runs out of time nothing more is started.  Prints one
JSON line and writes it to --out (default profiles/r12/transpose.json).

  python tools/bench_transpose.py [--shapes c2_f32,c3_f64,lap4096_f64] [--out PATH]
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

WARMUP, REPS = 5, 30
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
    if shape == "tiny_f32":  # rehearsal only
        rp, col, val = L.gen_uniform_csr(20_000, 20_000, 15, dtype=L.F32)
        return rp, col, val, 20_000
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


def _host_ms(torch, fn, warmup, reps, keep=False):
    """median host-clock time of a synchronous call between device synchronisations"""
    times, last = [], None
    for i in range(warmup + reps):
        last = None
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
        if keep and i == warmup + reps - 1:
            last = r
        elif hasattr(r, "close"):
            r.close()
        del r
    return statistics.median(times[warmup:]), last


def run_shape(shape):
    import numpy as np
    import torch

    import libhpc_amd as L
    if L.device_count() < 1 or not torch.cuda.is_available():
        raise SystemExit("bench_transpose needs a gfx950 device (no CPU fallback)")
    dev = torch.device("cuda:0")
    rp, col, val, n_cols = _matrix(L, shape)
    n_rows, nnz, tsz = rp.shape[0] - 1, int(col.shape[0]), val.dtype.itemsize
    d_rp, d_col, d_val = (torch.from_numpy(a).to(dev) for a in (rp, col, val))
    del rp, col, val
    gen = torch.Generator(device=dev).manual_seed(0x5EED0004)
    d_v1 = torch.rand(nnz, dtype=d_val.dtype, device=dev, generator=gen) * 2 - 1
    x = torch.rand(n_rows, dtype=d_val.dtype, device=dev, generator=gen) * 2 - 1  # Aᵀ·x reads n_rows values
    same = lambda a, b: a.shape == b.shape and bool(torch.equal(a.view(torch.uint8), b.view(torch.uint8)))  # noqa: E731
    out = dict(shape=shape, dtype="f32" if tsz == 4 else "f64", n_rows=n_rows, n_cols=n_cols, nnz=nnz,
               matrix_bytes=d_rp.numel() * d_rp.element_size() + nnz * (4 + tsz), sort_bits=max(n_cols - 1, 0).bit_length())

    # (a) the transposition
    out["transpose_ms"], tr = _host_ms(torch, lambda: L.csr_transpose(d_rp, d_col, d_val, n_cols, return_perm=True), 2, 7,
                                       keep=True)
    t_rp, t_col, t_val, perm = tr

    # (b) row expansion + COO → CSR of the swapped triples
    lens = d_rp[1:] - d_rp[:-1]
    rows_of = lambda: torch.repeat_interleave(torch.arange(n_rows, dtype=torch.int32, device=dev), lens)  # noqa: E731
    out["expand_ms"], rows = _host_ms(torch, rows_of, 1, 5, keep=True)
    bits = 64 if d_rp.dtype == torch.int64 else 32
    out["coo_to_csr_ms"], coo = _host_ms(torch, lambda: L.coo_to_csr(n_cols, n_rows, d_col, rows, d_val, bits), 1, 5,
                                         keep=True)
    out["coo_route_ms"] = out["expand_ms"] + out["coo_to_csr_ms"]
    out["coo_route_nnz"] = int(coo[1].numel())
    out["same_matrix"] = same(coo[0], t_rp) and same(coo[1], t_col) and same(coo[2], t_val)
    del rows, coo, lens

    # (c) the floor: A copied once, device to device
    spare = [torch.empty_like(t) for t in (d_rp, d_col, d_val)]
    out["copy_ms"] = _median_ms(torch, lambda: [s.copy_(t) for s, t in zip(spare, (d_rp, d_col, d_val))], WARMUP, REPS)
    del spare

    # (d) plan create, (e) set_values
    out["create_transpose_ms"], T = _host_ms(torch, lambda: L.SpMVPlan(d_rp, d_col, d_val, n_cols, transpose=True), 1, 3,
                                             keep=True)
    out["create_pretransposed_ms"], F = _host_ms(torch, lambda: L.SpMVPlan(t_rp, t_col, t_val, n_rows), 1, 3, keep=True)
    info = T.info()
    out["kernel"] = KERNELS[info["kernel"]]
    out["device_bytes_transpose_plan"], out["device_bytes_plain_plan"] = info["device_bytes"], F.info()["device_bytes"]
    yt, yf = T(x), F(x)
    matches = same(yt, yf) and {k: v for k, v in info.items() if k != "device_bytes"} == \
        {k: v for k, v in F.info().items() if k != "device_bytes"}
    t_v1 = d_v1[perm.long()]  # the new values in Aᵀ's order, for the plain plan
    out["set_values_transpose_ms"] = _median_ms(torch, lambda: T.set_values(d_v1), WARMUP, REPS)
    out["set_values_plain_ms"] = _median_ms(torch, lambda: F.set_values(t_v1), WARMUP, REPS)
    out["device_bytes_transpose_plan_after_update"] = T.info()["device_bytes"]
    out["spmv_ms"] = _median_ms(torch, lambda: T(x), WARMUP, REPS)
    matches = matches and same(T(x), F(x)) and not same(T(x), yt)
    if info["kernel"] == L.KERNEL_XTILE:
        matches = matches and T.layout_digest() == F.layout_digest()
    torch.cuda.synchronize()
    out["matches"] = bool(matches)
    T.close(), F.close()
    out["coo_route_over_transpose"] = out["coo_route_ms"] / out["transpose_ms"]
    out["coo_to_csr_over_transpose"] = out["coo_to_csr_ms"] / out["transpose_ms"]
    out["transpose_over_copy"] = out["transpose_ms"] / out["copy_ms"]
    out["create_transpose_over_pretransposed"] = out["create_transpose_ms"] / out["create_pretransposed_ms"]
    out["set_values_transpose_over_plain"] = out["set_values_transpose_ms"] / out["set_values_plain_ms"]
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r12", "transpose.json"))
    ap.add_argument("--child", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        print(json.dumps(run_shape(a.child)), flush=True)
        return 0
    res = dict(tool="bench_transpose",
               method=dict(warmup=WARMUP, reps=REPS,
                           timer="hip events, median (transpose, coo route, create: host clock between device "
                                 "synchronisations, median of 7 / 5 / 3)"),
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
        if not one["matches"]:
            status = 1  # the transposed plan must equal the plan of the transposed arrays
        print(f"bench_transpose: {shape} done", file=sys.stderr, flush=True)
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line, flush=True)
    return status


if __name__ == "__main__":
    sys.exit(main())
