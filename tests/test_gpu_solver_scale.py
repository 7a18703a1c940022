"""The solvers' reductions against the truth past their first lap: sizes at
which the two-stage sum of the fused dots (k_dpart_finish: a second stage past
2048 blocks), the one-block sums over block partials (part_sum, k_dot_finish,
k_coldot_finish: a second lap past 256 partials) and the grid-stride loops of
the vector kernels (grid capped at 1024 × 256 elements) all go round more
than once.  Every smaller test runs each of them exactly once, and the large
runs elsewhere compare a solver with itself.

Part 1 — exact dots.  tests/test_solver_scale_controls.py `band_dyadic`:
values and x in eighths, w in quarters, so y is exact in fp32 and fp64 and
Σ w·y is exact in fp64 in any order (|w·y| ≤ 6 < 10 in units of 1/256 over
≤ 2²¹ rows: below 2³³, of 53 bits).  The device dot must equal numpy's fp64
sum and y must equal the oracle's rounded result, bit for bit: no tolerance.

Part 2 — solves of a manufactured problem (`manufactured`: x* uniform in
[−1, 1], b = A·x* in fp64 on the CPU; convection–diffusion for BiCGStab, the
Laplacian for CG, both with shift 0.5, so κ ≤ 17 and the iteration counts stay
near 43 for every n) on the grids 256 × 257 (257 partials), 513 × 512 (the
capped grid with a partial second lap) and 700 × 750 (2051 blocks: a second
finish stage; two full laps and a tail of the grid-stride loops).  Bounds, the
project's own (tests/test_gpu_bicgstab.py, tests/test_gpu_cg.py): fp64 at tol
1e-10 — reported residual ≤ tol, true residual (on the CPU, from the returned
x) ≤ 2·tol, ‖x − x*‖ ≤ 1e-8·‖x*‖ (κ·2·tol = 3.4e-9), 0 < iterations ≤ 2 × the
CPU restatement's, and for CG the restatement's count ± 1, rounded up to the
check interval; fp32 at tol 1e-5 — residual ≤ 1e-5, error ≤ 1e-4.  The fp32
bound for BiCGStab: its restatement with fp32 vectors (`bicgstab_restatement`)
reaches tol 1e-5 at 700 × 750 in 19 iterations with error 4.3e-5 ≤ 5e-5 (CG:
2.4e-5), so 1e-4 stays.  The restatements alone are held to the same bounds
by the CPU module.

Part 3 — localised right-hand sides.  A solve is a forgiving judge of its own
dots: with every dot cut short alike (sums that stop after their first lap,
tried on a scratch build) CG and BiCGStab still converge to x* on the
spread-out b of part 2, a few iterations late and inside every bound, because
a fraction of each dot leaves the ratios α, β, ω nearly right.  So part 2 alone
catches a lost lap only where it makes the dots inconsistent with each other.
Part 3 puts x* (and with it b, within one grid row) where the first lap does
not read at all (tests/test_solver_scale_controls.py LOCAL_MID, LOCAL_TAIL):
a sum that loses the later laps is then 0, b·b = r·r = 0 ends the solve at
iteration 0 and p·A·p = 0 breaks it down, and the same bounds fail loudly.

Every case asserts the kernel family it means to run and the count that makes
it a second-lap case — from plan.info() where the plan reports it, else from n
with the kernels' block sizes (which the CPU module reads back from the
source) — so a change of block sizes fails here and does not quietly turn
these back into first-lap tests."""
import functools
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from tests import _support as S
from tests.test_bicgstab_api import csr_matvec
from tests.test_solver_scale_controls import (BLOCK_ROWS, FIN_TILE, GRIDS, LOCAL_MID, LOCAL_TAIL, TOL, TOL32,
                                              VEC_THREADS, band_dyadic, exact_dot, manufactured,
                                              restatement_iterations, solve_figures, transpose_csr, vec_laps,
                                              vec_partials)

pytestmark = pytest.mark.gpu

BIG = GRIDS[2]
CANARY = -1234.5
# (laps of the one-block sum over the vector partials, laps of the grid-stride loops) per grid
LAPS = {GRIDS[0]: (2, 1), GRIDS[1]: (4, 2), GRIDS[2]: (4, 3), LOCAL_TAIL[0]: (4, 3)}
# 256-row blocks of the grids whose fused dots finish in two stages
TWO_STAGE = {GRIDS[2]: 2051, LOCAL_TAIL[0]: 2400}


def _dev(gpu, a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).to(gpu)  # a copy: the shared inputs are read-only


def _blocks(n):
    return -(-n // BLOCK_ROWS)


def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


# ================================================================== 1. exact dots
@functools.lru_cache(maxsize=None)
def _band(n, dtype):
    """(rp, col, val, x, w, y as the oracle rounds it, Σ w·y) — once per size and type"""
    rp, col, val, x, w = band_dyadic(n, dtype, seed=n)
    y64, y, _ = S.spmv_oracle(rp, col, val, x)
    assert np.array_equal(y.astype(np.float64), y64)
    dot = float((w.astype(np.float64) * y64).sum())
    assert dot == exact_dot(w, y64)
    return _freeze(rp, col, val, x, w, y) + (dot,)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("n,blocks,stage1", [(524_288, 2048, 1), (524_289, 2049, 2), (1_048_577, 4097, 3)])
@pytest.mark.parametrize("family", ["sell", "adaptive"])
def test_spmv_dot_is_exact_at_the_finish_tile_edges(lhpc, gpu, family, n, blocks, stage1, dtype):
    """lhpc_spmv_dot on 2048 blocks (exactly one finish tile: one stage), 2049
    (a second stage whose last block holds a single partial, that of the last
    row) and 4097 (three stage-1 blocks), on SELL and ADAPTIVE, twice per plan
    (the second call reuses the plan's partials buffer)."""
    import torch
    rp, col, val, x, w, want_y, want_dot = _band(n, dtype)
    xd, wd = _dev(gpu, x), _dev(gpu, w)
    with lhpc.SpMVPlan(rp, col, val, n, options=None if family == "sell" else {"spmv_no_sell": 1}) as plan:
        info = plan.info()
        assert info["kernel"] == (lhpc.KERNEL_SELL if family == "sell" else lhpc.KERNEL_ADAPTIVE)
        assert info["n_blocks"] == blocks == _blocks(n) and -(-blocks // FIN_TILE) == stage1
        for call in range(2):
            y = torch.full((n,), float("nan"), dtype=xd.dtype, device=gpu)
            out = torch.full((1,), CANARY, dtype=torch.float64, device=gpu)
            lhpc.spmv_dot(plan, xd, y, wd, out)
            torch.cuda.synchronize()
            got = out.item()
            print(f"spmv_dot {family} n {n} call {call}: got {got!r} want {want_dot!r}")
            assert np.array_equal(y.cpu().numpy(), want_y), f"call {call}: y is not the exact product"
            assert got == want_dot, f"call {call}: dot {got!r}, exact {want_dot!r} (off by {got - want_dot!r})"


@functools.lru_cache(maxsize=None)
def _band_block(n, dtype):
    """the band matrix with 33 columns of X (eighths) and W (quarters), Y as the
    oracle rounds it and the exact column dots — once per size and type"""
    K = 33
    rp, col, val, _, _ = band_dyadic(n, dtype, seed=n + 7)
    rng = np.random.default_rng(n + 8)
    X = (rng.integers(-8, 9, size=(n, K)) / 8.0).astype(dtype)
    W = (rng.integers(-8, 9, size=(n, K)) / 4.0).astype(dtype)
    Y = np.stack([S.spmv_oracle(rp, col, val, np.ascontiguousarray(X[:, j]))[1] for j in range(K)], axis=1)
    prod = W.astype(np.float64) * Y.astype(np.float64)
    dots = prod.sum(axis=0)
    assert all(dots[j] == exact_dot(W[:, j], Y[:, j].astype(np.float64)) for j in range(K))
    # the blocks of each lap of the finish carry something in every column
    for lo in range(0, _blocks(n), VEC_THREADS):
        assert (prod[lo * BLOCK_ROWS:(lo + VEC_THREADS) * BLOCK_ROWS].sum(axis=0) != 0).all()
    return _freeze(rp, col, val, X, W, Y, dots)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("n,blocks", [(65_536, 256), (65_537 + 255, 257)])
def test_spmm_dot_is_exact_at_the_finish_lap_edge(lhpc, gpu, n, blocks, dtype):
    """lhpc_spmm_dot with 256 block partials per column (k_coldot_finish: one
    partial per thread) and 257 (thread 0 adds a second one), k ∈ {1, 5, 33},
    W ≠ X: every dot exact, Y the exact product, and column j of the k = 33
    call bit-identical to its k = 1 call."""
    import torch
    rp, col, val, X, W, want_y, want_dots = _band_block(n, dtype)
    xd, wd = _dev(gpu, X), _dev(gpu, W)
    with lhpc.SpMMPlan(rp, col, val, n) as plan:
        assert plan.info()["n_blocks"] == blocks == _blocks(n)
        assert -(-blocks // VEC_THREADS) == (1 if blocks == 256 else 2)
        y33, d33 = lhpc.spmm_dot(plan, xd, wd)
        got = d33.cpu().numpy()
        print(f"spmm_dot n {n} k 33: max |dot − exact| = {np.abs(got - want_dots).max()!r}")
        assert np.array_equal(y33.cpu().numpy(), want_y), "k = 33: Y is not the exact product"
        assert np.array_equal(got, want_dots), f"k = 33: columns {np.nonzero(got != want_dots)[0]} are not exact"
        for j0 in (0, 28):
            y5, d5 = lhpc.spmm_dot(plan, xd[:, j0:j0 + 5], wd[:, j0:j0 + 5])
            assert np.array_equal(d5.cpu().numpy(), want_dots[j0:j0 + 5]), f"k = 5 at column {j0}: not exact"
            assert torch.equal(y5, y33[:, j0:j0 + 5])
        for j in (0, 5, 31, 32):
            y1, d1 = lhpc.spmm_dot(plan, xd[:, j:j + 1], wd[:, j:j + 1])
            assert d1[0].item() == want_dots[j], f"k = 1, column {j}: dot {d1[0].item()!r}, exact {want_dots[j]!r}"
            assert d1[0] == d33[j] and torch.equal(y1[:, 0], y33[:, j]), f"column {j}: k = 1 differs from k = 33"


# ================================================================== 2. solves against a manufactured solution
@functools.lru_cache(maxsize=None)
def _problem(kind, shape, dtype=np.float64, transposed=False, support=None):
    """(rp, col, val, b, x*, iterations of the fp64 restatement); transposed:
    the arrays are A's, b = Aᵀ·x* and the count is Aᵀ's; support: a localised x*"""
    rp, col, val, b, want = manufactured(kind, shape, dtype, support)
    if transposed:
        b = csr_matvec(*transpose_csr(rp, col, val), want).astype(dtype)
    return _freeze(rp, col, val, b, want) + (restatement_iterations(kind, shape, transposed, support),)


def _assert_truth(name, x, it, res, rp, col, val, b, want, it_o, fp32=False, cg_every=0):
    """the module docstring's bounds; (rp, col, val) is the solved operator.
    cg_every > 0: CG's count, the restatement's ± 1 rounded up to the check interval"""
    x = x.cpu().numpy() if hasattr(x, "cpu") else x
    true_res, err = solve_figures(rp, col, val, b, x, want)
    print(f"{name}: iters {it} (restatement {it_o}) resid {res:.3e} true {true_res:.3e} error {err:.3e}")
    assert np.isfinite(x).all()
    if fp32:
        assert res <= TOL32 and err <= 1e-4 and 0 < it <= 2 * it_o
        return
    assert res <= TOL
    assert true_res <= 2 * TOL
    assert err <= 1e-8
    assert 0 < it <= 2 * it_o
    if cg_every:
        up = lambda k: -(-k // cg_every) * cg_every  # noqa: E731
        assert up(it_o - 1) <= it <= up(it_o + 1) and it % cg_every == 0


def _assert_second_lap(lhpc, info, kernel, n, shape, fused):
    """the plan runs the family meant, and n is past the first lap of the sums
    named in the module docstring"""
    assert info["kernel"] == kernel
    assert (info["n_rows"], info["n_cols"]) == (n, n)
    assert vec_laps(n) == LAPS[shape] and vec_partials(n) > VEC_THREADS
    if fused:  # the SpMV's epilogue dot: 256-row blocks, two stages past 2048 of them
        assert info["n_blocks"] == _blocks(n)
        if shape in TWO_STAGE:
            assert info["n_blocks"] == TWO_STAGE[shape] > FIN_TILE
        if shape == BIG:
            assert n % BLOCK_ROWS == 200


def _xtile_parts(lhpc, rp, col, val, n, single_launches):
    """a FORCE_XTILE plan cut into row parts of ≈ nnz / 3 nonzeros"""
    plan = lhpc.SpMVPlan(rp, col, val, n, flags=lhpc.PLAN_FORCE_XTILE, options={"xtile_part_nnz": col.size // 3 + 1})
    assert plan.info()["launches"] > single_launches, "the plan has no row parts"
    return plan


# ------------------------------------------------------------------ BiCGStab
@pytest.mark.parametrize("shape", GRIDS, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("family", ["sell", "rowgroup"])
def test_bicgstab_fp64_against_the_manufactured_solution(lhpc, gpu, family, shape):
    """the automatic plan (SELL: both SpMVs carry their dot) and FORCE_ROWGROUP
    (no fused dot: k_bi_dot and k_bi_ts_tt write the third partials array)"""
    rp, col, val, b, want, it_o = _problem("convdiff", shape)
    n = rp.size - 1
    flags, kernel = (0, lhpc.KERNEL_SELL) if family == "sell" else (lhpc.PLAN_FORCE_ROWGROUP, lhpc.KERNEL_ROWGROUP)
    with lhpc.SpMVPlan(rp, col, val, n, flags=flags) as plan:
        _assert_second_lap(lhpc, plan.info(), kernel, n, shape, fused=family == "sell")
        x, it, res = lhpc.bicgstab(plan, _dev(gpu, b), tol=TOL, max_iter=5000)
    _assert_truth(f"bicgstab {family} {shape}", x, it, res, rp, col, val, b, want, it_o)


@pytest.mark.parametrize("family", ["adaptive", "xtile", "xtile_parts"])
def test_bicgstab_fp64_on_the_other_families(lhpc, gpu, family):
    """700 × 750 on FORCE_ADAPTIVE (fused dots in ADAPTIVE's epilogue),
    FORCE_XTILE and an XTILE plan of row parts (both unfused; the parts run in
    turn, and graphs and fused dots are off for them)"""
    rp, col, val, b, want, it_o = _problem("convdiff", BIG)
    n = rp.size - 1
    if family == "adaptive":
        plan, kernel = lhpc.SpMVPlan(rp, col, val, n, flags=lhpc.PLAN_FORCE_ADAPTIVE), lhpc.KERNEL_ADAPTIVE
    else:
        plan, kernel = lhpc.SpMVPlan(rp, col, val, n, flags=lhpc.PLAN_FORCE_XTILE), lhpc.KERNEL_XTILE
        if family == "xtile_parts":
            with plan:
                single = plan.info()["launches"]
            plan = _xtile_parts(lhpc, rp, col, val, n, single)
    with plan:
        _assert_second_lap(lhpc, plan.info(), kernel, n, BIG, fused=family == "adaptive")
        x, it, res = lhpc.bicgstab(plan, _dev(gpu, b), tol=TOL, max_iter=5000, check_every=5)
    _assert_truth(f"bicgstab {family}", x, it, res, rp, col, val, b, want, it_o)


def test_bicgstab_fp64_on_a_transposed_plan(lhpc, gpu):
    """SpMVPlan(A, transpose=True) at 700 × 750 solves Aᵀ·x = Aᵀ·x*: held to the
    bounds with the CPU's transposed arrays"""
    rp, col, val, b, want, it_o = _problem("convdiff", BIG, transposed=True)
    n = rp.size - 1
    t_rp, t_col, t_val = transpose_csr(rp, col, val)
    with lhpc.SpMVPlan(rp, col, val, n, transpose=True) as plan:
        _assert_second_lap(lhpc, plan.info(), lhpc.KERNEL_SELL, n, BIG, fused=True)
        x, it, res = lhpc.bicgstab(plan, _dev(gpu, b), tol=TOL, max_iter=5000, check_every=3)
    _assert_truth("bicgstab transposed", x, it, res, t_rp, t_col, t_val, b, want, it_o)


@pytest.mark.parametrize("family", ["sell", "xtile"])
def test_bicgstab_fp32(lhpc, gpu, family):
    rp, col, val, b, want, it_o = _problem("convdiff", BIG, np.float32)
    n = rp.size - 1
    flags, kernel = (0, lhpc.KERNEL_SELL) if family == "sell" else (lhpc.PLAN_FORCE_XTILE, lhpc.KERNEL_XTILE)
    with lhpc.SpMVPlan(rp, col, val, n, flags=flags) as plan:
        assert plan.info()["dtype"] == lhpc.F32
        _assert_second_lap(lhpc, plan.info(), kernel, n, BIG, fused=family == "sell")
        x, it, res = lhpc.bicgstab(plan, _dev(gpu, b), tol=TOL32, max_iter=5000, check_every=5)
    _assert_truth(f"bicgstab fp32 {family}", x, it, res, rp, col, val, b, want, it_o, fp32=True)


def test_bicgstab_graph_replay_with_a_two_stage_dot(lhpc, gpu):
    """700 × 750 on the SELL plan, a side stream: check_every 1 is the plain
    loop, 7 and 50 replay captured blocks that hold the two-stage fused dot.
    x, iterations and residual are bit-identical, and meet the bounds."""
    import torch
    rp, col, val, b, want, it_o = _problem("convdiff", BIG)
    n = rp.size - 1
    bd = _dev(gpu, b)
    side = torch.cuda.Stream(gpu)
    runs = []
    with lhpc.SpMVPlan(rp, col, val, n) as plan:
        _assert_second_lap(lhpc, plan.info(), lhpc.KERNEL_SELL, n, BIG, fused=True)
        with torch.cuda.stream(side):
            for ce in (1, 7, 50):
                runs.append(lhpc.bicgstab(plan, bd, tol=TOL, max_iter=5000, check_every=ce, stream=side))
        side.synchronize()
    x0, it0, res0 = runs[0]
    for ce, (x, it, res) in zip((7, 50), runs[1:]):
        assert (it, res) == (it0, res0), f"check_every {ce}: {(it, res)} against the loop's {(it0, res0)}"
        assert torch.equal(x, x0), f"check_every {ce}: x differs from the loop's"
    assert it0 % 50 != 0  # the latch ended the solve inside a replayed block
    _assert_truth("bicgstab graphs", x0, it0, res0, rp, col, val, b, want, it_o)


# ------------------------------------------------------------------ CG
def test_cg_fp64_sell_and_adaptive(lhpc, gpu):
    """700 × 750 on a side stream with check_every 8 (captured blocks): the
    automatic plan (SELL: sell_cg_step with a two-stage dot) and spmv_no_sell
    (ADAPTIVE: lhpc_spmv_dot).  The two agree bit for bit, as they always had
    to — and both now meet the truth bounds."""
    import torch
    rp, col, val, b, want, it_o = _problem("laplacian", BIG)
    n = rp.size - 1
    bd = _dev(gpu, b)
    side = torch.cuda.Stream(gpu)
    out = []
    for opts, kernel in ((None, lhpc.KERNEL_SELL), ({"spmv_no_sell": 1}, lhpc.KERNEL_ADAPTIVE)):
        with lhpc.SpMVPlan(rp, col, val, n, options=opts) as plan:
            _assert_second_lap(lhpc, plan.info(), kernel, n, BIG, fused=True)
            with torch.cuda.stream(side):
                out.append(lhpc.cg(plan, bd, tol=TOL, max_iter=5000, check_every=8, stream=side))
            side.synchronize()
    for name, (x, it, res) in zip(("sell", "adaptive"), out):
        _assert_truth(f"cg {name}", x, it, res, rp, col, val, b, want, it_o, cg_every=8)
    assert out[0][1:] == out[1][1:] and torch.equal(out[0][0], out[1][0]), "SELL and ADAPTIVE differ"


@pytest.mark.parametrize("family", ["xtile", "xtile_parts"])
def test_cg_fp64_on_xtile(lhpc, gpu, family):
    """FORCE_XTILE and an XTILE plan of row parts: SpMV + k_dot_partial /
    k_dot_finish, 1024 partials of three laps each"""
    rp, col, val, b, want, it_o = _problem("laplacian", BIG)
    n = rp.size - 1
    plan = lhpc.SpMVPlan(rp, col, val, n, flags=lhpc.PLAN_FORCE_XTILE)
    if family == "xtile_parts":
        with plan:
            single = plan.info()["launches"]
        plan = _xtile_parts(lhpc, rp, col, val, n, single)
    with plan:
        _assert_second_lap(lhpc, plan.info(), lhpc.KERNEL_XTILE, n, BIG, fused=False)
        x, it, res = lhpc.cg(plan, _dev(gpu, b), tol=TOL, max_iter=5000)
    _assert_truth(f"cg {family}", x, it, res, rp, col, val, b, want, it_o, cg_every=1)


@pytest.mark.parametrize("family", ["sell", "xtile"])
def test_cg_fp32(lhpc, gpu, family):
    rp, col, val, b, want, it_o = _problem("laplacian", BIG, np.float32)
    n = rp.size - 1
    flags, kernel = (0, lhpc.KERNEL_SELL) if family == "sell" else (lhpc.PLAN_FORCE_XTILE, lhpc.KERNEL_XTILE)
    with lhpc.SpMVPlan(rp, col, val, n, flags=flags) as plan:
        assert plan.info()["dtype"] == lhpc.F32
        _assert_second_lap(lhpc, plan.info(), kernel, n, BIG, fused=family == "sell")
        x, it, res = lhpc.cg(plan, _dev(gpu, b), tol=TOL32, max_iter=5000, check_every=5)
    assert it % 5 == 0
    _assert_truth(f"cg fp32 {family}", x, it, res, rp, col, val, b, want, it_o, fp32=True)


# ------------------------------------------------------------------ multi-RHS CG
@functools.lru_cache(maxsize=None)
def _block_problem(shape, dtype=np.float64):
    """(rp, col, val, B, X*, per-column iterations of the C oracle) with 33
    columns, column j of B = A·X*_j; a k-column test takes the first k"""
    if dtype != np.float64:  # the same problem, val (quarters: exact) and B rounded
        rp, col, val, B, want, its = _block_problem(shape)
        return _freeze(rp, col, val.astype(dtype), B.astype(dtype), want) + (its,)
    K = 33
    rp, col, val = S.laplacian_2d(*shape, shift=0.5)
    n = rp.size - 1
    want = np.random.default_rng(n + 1).uniform(-1, 1, (n, K))
    B = np.stack([csr_matvec(rp, col, val, want[:, j]) for j in range(K)], axis=1)
    with ThreadPoolExecutor(8) as pool:  # the oracle is a C call: the columns run side by side
        ref = list(pool.map(lambda j: S.cg_oracle(rp, col, val, np.ascontiguousarray(B[:, j]), tol=TOL,
                                                  max_iter=5000), range(K)))
    assert all(r[2] <= TOL for r in ref)
    return _freeze(rp, col, val.astype(dtype), B.astype(dtype), want) + (tuple(r[1] for r in ref),)


def _assert_tiles(plan, n, shape):
    """256-row tiles: 257 (a second lap of k_coldot_finish) or 2051 (nine)"""
    assert plan.info()["n_blocks"] == _blocks(n) == {GRIDS[0]: 257, BIG: 2051}[shape]
    assert _blocks(n) > VEC_THREADS


@pytest.mark.parametrize("shape", [GRIDS[0], BIG], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("k", [3, 33])
def test_cg_multi_fp64_against_the_manufactured_solutions(lhpc, gpu, k, shape):
    """every column inside the bounds; at k = 33 the columns on both sides of
    the 32-column panel edge (and column 0) are bit-identical, in x,
    iterations and residual, to their one-column solves"""
    import torch
    rp, col, val, B, want, its = _block_problem(shape)
    n = rp.size - 1
    with lhpc.SpMMPlan(rp, col, val, n) as plan:
        _assert_tiles(plan, n, shape)
        X, iters, resid = lhpc.cg_multi(plan, _dev(gpu, B[:, :k]), tol=TOL, max_iter=5000)
        singles = {}
        if k == 33:
            for j in (0, 31, 32):
                x1, it1, res1 = lhpc.cg_multi(plan, _dev(gpu, B[:, j:j + 1]), tol=TOL, max_iter=5000)
                singles[j] = (x1[:, 0].clone(), int(it1[0]), float(res1[0]))
    Xh = X.cpu().numpy()
    for j in range(k):
        _assert_truth(f"cg_multi {shape} k {k} column {j}", Xh[:, j], int(iters[j]), float(resid[j]), rp, col, val,
                      B[:, j], want[:, j], its[j], cg_every=1)
    for j, (x1, it1, res1) in singles.items():
        assert (int(iters[j]), float(resid[j])) == (it1, res1), f"column {j}: k = 33 and k = 1 differ"
        assert torch.equal(X[:, j], x1), f"column {j}: x of k = 33 differs from its k = 1 solve"


def test_cg_multi_fp32(lhpc, gpu):
    rp, col, val, B, want, its = _block_problem(BIG, np.float32)
    n, k = rp.size - 1, 3
    with lhpc.SpMMPlan(rp, col, val, n) as plan:
        assert plan.info()["dtype"] == lhpc.F32
        _assert_tiles(plan, n, BIG)
        X, iters, resid = lhpc.cg_multi(plan, _dev(gpu, B[:, :k]), tol=TOL32, max_iter=5000, check_every=5)
    Xh = X.cpu().numpy()
    for j in range(k):
        _assert_truth(f"cg_multi fp32 column {j}", Xh[:, j], int(iters[j]), float(resid[j]), rp, col, val, B[:, j],
                      want[:, j], its[j], fp32=True)


# ================================================================== 3. right-hand sides the first lap does not see
LOCAL = {"mid": LOCAL_MID, "tail": LOCAL_TAIL}


@pytest.mark.parametrize("family,where", [("rowgroup", "mid"), ("sell", "mid"), ("sell", "tail")])
def test_bicgstab_on_a_localised_right_hand_side(lhpc, gpu, family, where):
    """b lies where only later laps read (the module docstring's last
    paragraph): FORCE_ROWGROUP and SELL with b in laps 2 – 4 of the one-block
    sums (bb, rr, ss, tt, ρ', and σ, ts where the dot is not fused), SELL with
    b in the second stage-1 sum of the fused dots (σ, ts)"""
    shape, support = LOCAL[where]
    rp, col, val, b, want, it_o = _problem("convdiff", shape, support=support)
    n = rp.size - 1
    flags, kernel = (0, lhpc.KERNEL_SELL) if family == "sell" else (lhpc.PLAN_FORCE_ROWGROUP, lhpc.KERNEL_ROWGROUP)
    with lhpc.SpMVPlan(rp, col, val, n, flags=flags) as plan:
        _assert_second_lap(lhpc, plan.info(), kernel, n, shape, fused=family == "sell")
        x, it, res = lhpc.bicgstab(plan, _dev(gpu, b), tol=TOL, max_iter=5000, check_every=4)
    _assert_truth(f"bicgstab {family} localised {where}", x, it, res, rp, col, val, b, want, it_o)


@pytest.mark.parametrize("family,where", [("xtile", "mid"), ("sell", "mid"), ("sell", "tail"), ("adaptive", "tail")])
def test_cg_on_a_localised_right_hand_side(lhpc, gpu, family, where):
    """CG likewise: k_dot_finish over 1024 partials (bb, rr; p·A·p on XTILE),
    and p·A·p in the second stage-1 sum of sell_cg_step's and lhpc_spmv_dot's
    finish; SELL and ADAPTIVE on a side stream with check_every 8 (graphs)"""
    import torch
    shape, support = LOCAL[where]
    rp, col, val, b, want, it_o = _problem("laplacian", shape, support=support)
    n = rp.size - 1
    flags, opts, kernel, ce = {"xtile": (lhpc.PLAN_FORCE_XTILE, None, lhpc.KERNEL_XTILE, 1),
                               "sell": (0, None, lhpc.KERNEL_SELL, 8),
                               "adaptive": (0, {"spmv_no_sell": 1}, lhpc.KERNEL_ADAPTIVE, 8)}[family]
    side = torch.cuda.Stream(gpu)
    with lhpc.SpMVPlan(rp, col, val, n, flags=flags, options=opts) as plan:
        _assert_second_lap(lhpc, plan.info(), kernel, n, shape, fused=family != "xtile")
        with torch.cuda.stream(side):
            x, it, res = lhpc.cg(plan, _dev(gpu, b), tol=TOL, max_iter=5000, check_every=ce, stream=side)
        side.synchronize()
    _assert_truth(f"cg {family} localised {where}", x, it, res, rp, col, val, b, want, it_o, cg_every=ce)


def test_cg_multi_on_localised_right_hand_sides(lhpc, gpu):
    """three columns whose B lies in tiles ≥ 256: every lap of k_coldot_finish
    but the first, for bb, rr and (lhpc_spmm_dot's blocks) p·A·p"""
    shape, support = LOCAL_MID
    rp, col, val = S.laplacian_2d(*shape, shift=0.5)
    n, k = rp.size - 1, 3
    want = np.random.default_rng(n + 2).uniform(-1, 1, (n, k))
    want[:support[0]] = 0.0
    want[support[1]:] = 0.0
    B = np.stack([csr_matvec(rp, col, val, want[:, j]) for j in range(k)], axis=1)
    assert np.nonzero(B.any(axis=1))[0].min() // BLOCK_ROWS >= VEC_THREADS
    its = [S.cg_oracle(rp, col, val, np.ascontiguousarray(B[:, j]), tol=TOL, max_iter=5000)[1] for j in range(k)]
    with lhpc.SpMMPlan(rp, col, val, n) as plan:
        _assert_tiles(plan, n, shape)
        X, iters, resid = lhpc.cg_multi(plan, _dev(gpu, B), tol=TOL, max_iter=5000)
    Xh = X.cpu().numpy()
    for j in range(k):
        _assert_truth(f"cg_multi localised column {j}", Xh[:, j], int(iters[j]), float(resid[j]), rp, col, val,
                      B[:, j], want[:, j], its[j], cg_every=1)
