"""lhpc_bicgstab_solve on the GPU, on the upwind convection–diffusion operator
of tests/test_bicgstab_api.py (`convdiff_2d`: not symmetric, condition number
17 at 64 × 48) with b = default_rng(n).uniform(−1, 1, n).

Bounds.  The truth is a direct solve (scipy's sparse LU, fp64).  At tol 1e-10
the CPU restatement (`bicgstab_oracle`) converges in 44 / 44 / 46 / 7
iterations on 64×48 / 96×80 / 200×150 / 7×1, its recursive and true residuals
agree to two digits (4e-11 … 9e-11) and its error against the direct solve is
≤ 4e-10.  So: reported residual ≤ tol; true residual ≤ 2·tol (the factor
covers another dot order); ‖x − x*‖ ≤ 1e-8·‖x*‖ (the project's CG bound,
implied by κ·2·tol = 3.4e-9); iterations ≤ 2 × the oracle's (a cap that
catches a stalled solver).  fp32: residual ≤ 1e-5 and x within 1e-4 of the
fp64 solution (the CG test's bound; the restatement in fp32 reaches 2.7e-5).
Everything about check_every, streams, graphs and transposed plans is
compared bit for bit.  Matrices, right-hand sides, direct solutions and
oracle counts are computed once per module."""
import subprocess
import threading

import numpy as np
import pytest

from tests import _support as S
from tests.test_bicgstab_api import SKEW, bicgstab_oracle, build_cpp, convdiff_2d, csr_matvec

pytestmark = pytest.mark.gpu

TOL = 1e-10
_PROBLEMS = {}


def _dev(gpu, a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).to(gpu)  # a copy: the module's arrays are read-only


def _problem(shape):
    """(rp, col, val, b, x*, oracle iterations) of a shape, shift 0.5, fp64"""
    if shape not in _PROBLEMS:
        import scipy.sparse as sp
        from scipy.sparse.linalg import splu
        rp, col, val = convdiff_2d(*shape)
        n = rp.size - 1
        b = np.random.default_rng(n).uniform(-1, 1, n)
        want = splu(sp.csr_matrix((val, col, rp), shape=(n, n)).tocsc()).solve(b)
        _, it_o, res_o, broke = bicgstab_oracle(rp, col, val, b, tol=TOL, max_iter=5000)
        assert not broke and res_o <= TOL
        for a in (rp, col, val, b, want):
            a.setflags(write=False)
        _PROBLEMS[shape] = (rp, col, val, b, want, it_o)
    return _PROBLEMS[shape]


def _assert_solved(x, it, res, rp, col, val, b, want, it_o, scale=1.0):
    """test 1's bounds for the matrix (rp, col, val), whose solution is scale·x*"""
    x = x.cpu().numpy() if hasattr(x, "cpu") else x
    true_res = np.linalg.norm(b - csr_matvec(rp, col, val, x)) / np.linalg.norm(b)
    err = np.linalg.norm(x - scale * want) / np.linalg.norm(scale * want)
    print(f"bicgstab: iters {it} (oracle {it_o}) resid {res:.3e} true {true_res:.3e} error {err:.3e}")
    assert res <= TOL
    assert true_res <= 2 * TOL
    assert err <= 1e-8
    assert 0 < it <= 2 * it_o


# ------------------------------------------------------------------ 1. fp64 against the truth
@pytest.mark.parametrize("shape", [(64, 48), (200, 150), (7, 1)])
@pytest.mark.parametrize("flags", [0, 1 << 4, 1 << 5, 1 << 6])
def test_bicgstab_fp64_against_the_direct_solve(lhpc, gpu, shape, flags):
    rp, col, val, b, want, it_o = _problem(shape)
    with lhpc.SpMVPlan(rp, col, val, rp.size - 1, flags=flags) as plan:
        x, it, res = lhpc.bicgstab(plan, _dev(gpu, b), tol=TOL, max_iter=5000)
    _assert_solved(x, it, res, rp, col, val, b, want, it_o)


# ------------------------------------------------------------------ 2. fp32
def test_bicgstab_fp32(lhpc, gpu):
    import scipy.sparse as sp
    from scipy.sparse.linalg import splu
    rp, col, val = convdiff_2d(128, 128, dtype=np.float32)  # the values are exact in fp32
    n = rp.size - 1
    b = np.random.default_rng(n).uniform(-1, 1, n).astype(np.float32)
    want = splu(sp.csr_matrix((val.astype(np.float64), col, rp), shape=(n, n)).tocsc()).solve(b.astype(np.float64))
    with lhpc.SpMVPlan(rp, col, val, n) as plan:
        x, it, res = lhpc.bicgstab(plan, _dev(gpu, b), tol=1e-5, max_iter=5000, check_every=5)
    err = np.linalg.norm(x.cpu().numpy().astype(np.float64) - want) / np.linalg.norm(want)
    print(f"bicgstab fp32: iters {it} resid {res:.3e} error {err:.3e}")
    assert res <= 1e-5 and it > 0
    assert err <= 1e-4


# ------------------------------------------------------------------ 3. check_every, graph against loop
@pytest.mark.parametrize("max_iter", [5000, 20, 3])
def test_bicgstab_does_not_depend_on_check_every_or_stream(lhpc, gpu, max_iter):
    """On a non-null stream and check_every ≥ 4 the iterations between two
    reads of the latch are a replayed graph, on the null stream (and for
    check_every 1) the plain loop; the device latch ends the solve at the same
    iteration whenever the host looks.  x bit-identical, (iters, resid) equal
    over check_every ∈ {1, 4, 7, 50}, the null stream and a side stream
    (twice: the second solve replays the graph the first one captured), for a
    max_iter that is ample, one that ends in the middle of a block and one
    shorter than any block."""
    import torch
    rp, col, val, b, want, it_o = _problem((96, 80))
    bd = _dev(gpu, b)
    runs = []
    with lhpc.SpMVPlan(rp, col, val, rp.size - 1) as plan:
        assert plan.info()["kernel"] == lhpc.KERNEL_SELL  # ≤ 5 nonzeros per row
        side = torch.cuda.Stream(gpu)
        for ce in (1, 4, 7, 50):
            runs.append(lhpc.bicgstab(plan, bd, tol=TOL, max_iter=max_iter, check_every=ce,
                                      stream=torch.cuda.default_stream(gpu)))
            with torch.cuda.stream(side):
                for _ in range(2):
                    runs.append(lhpc.bicgstab(plan, bd, tol=TOL, max_iter=max_iter, check_every=ce, stream=side))
            side.synchronize()
    x0, it0, res0 = runs[0]
    for x, it, res in runs[1:]:
        assert (it, res) == (it0, res0)
        assert torch.equal(x, x0)
    if max_iter == 5000:
        assert it0 % 50 != 0  # the iteration at which rr ≤ stop first held, not the next check
        _assert_solved(x0, it0, res0, rp, col, val, b, want, it_o)
    else:
        assert it0 == max_iter and res0 > TOL and np.isfinite(res0)


# ------------------------------------------------------------------ 4. past convergence
def test_bicgstab_does_not_run_past_convergence(lhpc, gpu):
    """7 × 1 converges in 7 iterations (Krylov dimension); with check_every 50
    the host looks only at iteration 50.  Without the latch the iterations in
    between turn the solution into NaN (tests/test_bicgstab_api.py shows it on
    the CPU restatement); with it the solve has ended where it converged."""
    rp, col, val, b, want, it_o = _problem((7, 1))
    assert not np.isfinite(bicgstab_oracle(rp, col, val, b, tol=TOL, max_iter=200, check_every=50, latch=False)[0]).all()
    with lhpc.SpMVPlan(rp, col, val, 7) as plan:
        x, it, res = lhpc.bicgstab(plan, _dev(gpu, b), tol=TOL, max_iter=200, check_every=50)
    x = x.cpu().numpy()
    assert 0 < it <= 8 and res <= TOL
    assert np.isfinite(x).all() and np.linalg.norm(x - want) <= 1e-12 * np.linalg.norm(want)


# ------------------------------------------------------------------ 5. breakdown
@pytest.mark.parametrize("check_every", [1, 10])
def test_bicgstab_breakdown_is_reported_and_leaves_x0(lhpc, gpu, check_every):
    """[[0, 1], [−1, 0]], b = (1, 1), x0 = (0.25, −0.5): r = (1.5, 1.25),
    v = A·r = (1.25, −1.5), r̂·v = 1.875 − 1.875 = 0 exactly (every product and
    the sum are dyadic), so α = ρ/0: a numeric breakdown on valid input, found
    before x is written.  LHPC_ERR_INTERNAL, and the caller's x is x0 bit for
    bit.  (iters = 0 and the finite residual: the C++ program, test 9.)"""
    x0 = np.array([0.25, -0.5])
    x = _dev(gpu, x0)
    with lhpc.SpMVPlan(*SKEW, 2) as plan:
        with pytest.raises(lhpc.LhpcError) as e:
            lhpc.bicgstab(plan, _dev(gpu, np.array([1.0, 1.0])), x=x, max_iter=100, check_every=check_every)
    assert e.value.status == -6
    assert np.array_equal(x.cpu().numpy().view(np.uint64), x0.view(np.uint64))


# ------------------------------------------------------------------ 6. zero right-hand side, warm start
def test_bicgstab_zero_rhs_and_warm_start(lhpc, gpu):
    import torch
    rp, col, val, b, want, it_o = _problem((64, 48))
    n = rp.size - 1
    with lhpc.SpMVPlan(rp, col, val, n) as plan:
        x, it, res = lhpc.bicgstab(plan, torch.zeros(n, dtype=torch.float64, device=gpu))
        assert it == 0 and res == 0.0 and torch.count_nonzero(x) == 0
        x1, it1, _ = lhpc.bicgstab(plan, _dev(gpu, b), tol=1e-12, max_iter=5000)
        x2, it2, res2 = lhpc.bicgstab(plan, _dev(gpu, b), x=x1.clone(), tol=TOL, max_iter=5000)
        assert it1 > 1 and it2 <= 1 and res2 <= TOL
        assert torch.allclose(x2, x1, rtol=0, atol=1e-11)


# ------------------------------------------------------------------ 7. transposed plan
@pytest.mark.parametrize("flags", [0, 1 << 5])
def test_bicgstab_on_a_transposed_plan(lhpc, gpu, flags):
    """SpMVPlan(A, transpose=True) solves Aᵀ·x = b, bit-identical to a plan
    built from csr_transpose(A)."""
    import torch
    rp, col, val, b, _, _ = _problem((64, 48))
    n = rp.size - 1
    t_rp, t_col, t_val = lhpc.csr_transpose(rp, col, val, n)
    bd = _dev(gpu, b)
    with lhpc.SpMVPlan(rp, col, val, n, flags=flags, transpose=True) as tp, \
            lhpc.SpMVPlan(t_rp, t_col, t_val, n, flags=flags) as fresh:
        x, it, res = lhpc.bicgstab(tp, bd, tol=TOL, max_iter=5000, check_every=3)
        xf, itf, resf = lhpc.bicgstab(fresh, bd, tol=TOL, max_iter=5000, check_every=3)
    assert (it, res) == (itf, resf) and torch.equal(x, xf)
    assert res <= TOL and 0 < it < 5000
    true_res = np.linalg.norm(b - csr_matvec(t_rp, t_col, t_val, x.cpu().numpy())) / np.linalg.norm(b)
    assert true_res <= 2 * TOL


# ------------------------------------------------------------------ 8. busy, set_values
def test_bicgstab_and_cg_share_the_plan_one_at_a_time(lhpc, gpu):
    """The two solvers share the plan's busy flag: of a bicgstab and a cg call
    started together on one plan from two threads, the one that comes second
    gets LHPC_ERR_BUSY (−7) and the other runs to the end; afterwards the plan
    serves either again.  Both solves are long (tol 0: hundreds of iterations
    at ≈ 0.2 … 0.4 ms each on 1024²), the threads start within microseconds of
    each other (a barrier)."""
    ny = nx = 1024
    rp, col, val = S.laplacian_2d(ny, nx)  # SPD, so cg runs; bicgstab needs no more than A·x
    n = ny * nx
    bd = _dev(gpu, np.random.default_rng(0xB1C6).uniform(-1, 1, n))
    with lhpc.SpMVPlan(rp, col, val, n) as plan:
        ref = {"bicgstab": lhpc.bicgstab(plan, bd, tol=0.0, max_iter=400, check_every=10),
               "cg": lhpc.cg(plan, bd, tol=0.0, max_iter=800, check_every=10)}
        out, gate = {}, threading.Barrier(2)

        def run(name, fn):
            gate.wait()
            try:
                out[name] = fn(plan, bd, tol=0.0, max_iter=400 if name == "bicgstab" else 800, check_every=10)
            except lhpc.LhpcError as e:
                out[name] = e.status
        threads = [threading.Thread(target=run, args=(k, f)) for k, f in (("bicgstab", lhpc.bicgstab), ("cg", lhpc.cg))]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        refused = [k for k, v in out.items() if isinstance(v, int)]
        assert len(refused) == 1 and out[refused[0]] == -7, out
        (ran,) = [k for k in out if k not in refused]
        import torch
        assert out[ran][1:] == ref[ran][1:] and torch.equal(out[ran][0], ref[ran][0])
        again = lhpc.bicgstab(plan, bd, tol=0.0, max_iter=400, check_every=10)  # the plan is free again
        assert again[1:] == ref["bicgstab"][1:] and torch.equal(again[0], ref["bicgstab"][0])


@pytest.mark.parametrize("flags", [0, 1 << 5])
def test_bicgstab_after_set_values(lhpc, gpu, flags):
    """After plan.set_values(2·val) the next solve (same work, same graph: the
    plan's value array keeps its address) returns x*/2, within test 1's bounds."""
    import torch
    rp, col, val, b, want, it_o = _problem((64, 48))
    bd = _dev(gpu, b)
    side = torch.cuda.Stream(gpu)
    with lhpc.SpMVPlan(rp, col, val, rp.size - 1, flags=flags) as plan, torch.cuda.stream(side):
        x, it, res = lhpc.bicgstab(plan, bd, tol=TOL, max_iter=5000, check_every=4, stream=side)
        _assert_solved(x, it, res, rp, col, val, b, want, it_o)
        plan.set_values(2 * val)
        x, it, res = lhpc.bicgstab(plan, bd, tol=TOL, max_iter=5000, check_every=4, stream=side)
        _assert_solved(x, it, res, rp, col, 2 * val, b, want, it_o, scale=0.5)


# ------------------------------------------------------------------ 9. the C++ program
def test_cpp_program_on_the_gpu():
    """tests/cpp/test_bicgstab_api.cpp (built by tests/cpp/bicgstab.mk):
    sparse::bicgstab within test 1's bounds, fp32, and the breakdown through
    the C call — status LHPC_ERR_INTERNAL, iters 0, a finite residual."""
    r = subprocess.run([build_cpp()], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "bicgstab cpp api: ok" in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-2000:])
    line = [l for l in r.stdout.splitlines() if l.startswith("bicgstab breakdown:")]
    assert line and "status -6 iters 0 resid" in line[0] and np.isfinite(float(line[0].split()[-1]))
