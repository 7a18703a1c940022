"""GPU parity for the ghost-cell stencils through the C ABI.

blur_x / blur_y must be BIT-EXACT against (a) the golden fixtures produced by
the reference's own HPCHighDimensionFlatArray + BM_x_blur/BM_y_blur loop
(oracle/_ref/ref_probe, tests/golden/make_golden.py) and (b) the C oracle at
other shapes, up to the reference's 8192² grid.  stencil7 is bit-exact
against the oracle (both evaluate the same order without contraction).
"""
import glob
import os

import numpy as np
import pytest

from tests import _support as S

pytestmark = pytest.mark.gpu

GOLDEN_BLUR = sorted(glob.glob(os.path.join(S.GOLDEN, "blur_*.npz")))


def _dev(gpu, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


@pytest.mark.parametrize("buffers", ["device", "host"])
@pytest.mark.parametrize("path", GOLDEN_BLUR, ids=lambda p: os.path.basename(p)[:-4])
def test_blur_golden_bit_exact(lhpc, gpu, path, buffers):
    g = S.load_golden(os.path.basename(path))
    ny, nx, ghost, nb = (int(g[k]) for k in ("ny", "nx", "ghost", "nblur"))
    fn = lhpc.blur_y if os.path.basename(path).startswith("blur_y") else lhpc.blur_x
    if buffers == "device":
        import torch
        b = torch.empty(ny * nx, dtype=torch.float32, device=gpu)
        out = fn(_dev(gpu, g["a"]), b, ny, nx, ghost, nb).cpu().numpy()
    else:
        out = fn(g["a"].copy(), np.empty(ny * nx, dtype=np.float32), ny, nx, ghost, nb)
    assert np.array_equal(out, g["b"])


SHAPES = [(1, 1, 8), (3, 5, 8), (17, 33, 8), (64, 1000, 8), (257, 131, 12), (100, 96, 8),
          (33, 64, 3), (512, 1024, 8)]


@pytest.mark.parametrize("ny,nx,ghost", SHAPES)
@pytest.mark.parametrize("ydir", [False, True])
def test_blur_shapes_vs_oracle(lhpc, gpu, ny, nx, ghost, ydir):
    import torch
    nb = min(8, ghost)
    a = S.random_padded(((ny + 2 * ghost) * (nx + 2 * ghost),), seed=ny * 7919 + nx)
    want = S.blur_oracle(a, ny, nx, ghost, nb, ydir)
    b = torch.empty(ny * nx, dtype=torch.float32, device=gpu)
    fn = lhpc.blur_y if ydir else lhpc.blur_x
    got = fn(_dev(gpu, a), b, ny, nx, ghost, nb).cpu().numpy()
    assert np.array_equal(got, want)


@pytest.mark.slow
@pytest.mark.parametrize("ydir", [False, True])
def test_blur_reference_grid_8192(lhpc, gpu, ydir):
    """The reference benchmark's own size: 8192², ghost 8, nblur 8."""
    import torch
    n, g = 8192, 8
    a = S.random_padded(((n + 2 * g) ** 2,), seed=8192 + ydir)
    want = S.blur_oracle(a, n, n, g, 8, ydir)
    b = torch.empty(n * n, dtype=torch.float32, device=gpu)
    got = (lhpc.blur_y if ydir else lhpc.blur_x)(_dev(gpu, a), b, n, n, g, 8).cpu().numpy()
    assert np.array_equal(got, want)


def test_blur_rejects_narrow_ghost(lhpc):
    a = np.zeros((4 + 4) * (4 + 4), dtype=np.float32)
    with pytest.raises(lhpc.LhpcError):
        lhpc.blur_x(a, np.zeros(16, dtype=np.float32), 4, 4, 2, 8)


@pytest.mark.parametrize("nz,ny,nx", [(1, 1, 1), (2, 3, 5), (16, 17, 65), (33, 64, 64), (64, 96, 130),
                                      (4, 5, 512), (5, 9, 517), (3, 7, 1100)])  # ≥ 512: the 1 × 8 default tile
def test_stencil7_vs_oracle(lhpc, gpu, nz, ny, nx):
    g = 1
    shape = (nz + 2, ny + 2, nx + 2)
    u = S.random_padded(shape, seed=nz * 131 + nx, zero_ghost=False).reshape(-1)
    out0 = S.random_padded(shape, seed=99).reshape(-1)  # ghosts of `out` must survive
    want = S.stencil7_oracle(u, nz, ny, nx, g, -6.0, 1.0, out=out0.copy())
    got = lhpc.stencil7(_dev(gpu, u), _dev(gpu, out0), nz, ny, nx, g, -6.0, 1.0).cpu().numpy()
    assert np.array_equal(got, want)
    # host-buffer path
    got_h = lhpc.stencil7(u.copy(), out0.copy(), nz, ny, nx, g, -6.0, 1.0)
    assert np.array_equal(got_h, want)


def test_stencil7_planes_compose(lhpc, gpu):
    """Computing z-plane ranges separately (the halo-overlap schedule) gives
    exactly the full sweep."""
    nz, ny, nx = 40, 30, 70
    shape = (nz + 2, ny + 2, nx + 2)
    u = _dev(gpu, S.random_padded(shape, seed=5).reshape(-1))
    full = lhpc.stencil7(u, _dev(gpu, np.zeros(np.prod(shape), np.float32)), nz, ny, nx, 1, -6.0, 1.0)
    part = _dev(gpu, np.zeros(np.prod(shape), np.float32))
    for z0, z1 in ((0, 1), (1, 17), (17, 39), (39, 40)):
        lhpc.stencil7_planes(u, part, nz, ny, nx, 1, -6.0, 1.0, z0, z1)
    import torch
    assert torch.equal(full, part)


@pytest.mark.slow
def test_stencil7_c5_size(lhpc, gpu):
    """BASELINE configs[4] grid (512³, Dirichlet-0 ghosts, c0=-6, c1=1)."""
    n, g = 512, 1
    shape = (n + 2,) * 3
    u = S.random_padded(shape, seed=0x5EED0005, zero_ghost=True, ghost=1).reshape(-1)
    want = S.stencil7_oracle(u, n, n, n, g, -6.0, 1.0)
    got = lhpc.stencil7(_dev(gpu, u), _dev(gpu, np.zeros_like(u)), n, n, n, g, -6.0, 1.0).cpu().numpy()
    assert np.array_equal(got, want)


S7_IMPLS = ["buf", "buf:1,8,0,2", "buf:1,4,128,3", "buf:1,8,5,3", "buf:1,8,16", "buf:1,8,32", "buf:1,4,32",
            "buf:1,8,4", "simple",
            # tuning-build tiles (their kernels spill SGPRs): LHPC_ERR_UNSUPPORTED in the product library
            "buf:2,8,0,2", "buf:4,4,128,3", "buf:2,8,32", "buf:2,4,32", "buf:4,8,32"]


def _s7_in_product(name, cfg):
    """The tiles the product library compiles (lhpc_stencil.hip s7_launch):
    one row per wave, or the x4 ring's LDS-shared 2 rows × 4 blocks."""
    if name == "simple" or not cfg:
        return True
    ry, nj = (int(v) for v in cfg.split(",")[:2])
    return nj in (4, 8) and (ry == 1 or (name == "buf4lds" and ry == 2 and nj == 4))


def _s7_options(lhpc, name, cfg, store):
    """lhpc_options fields for a stencil7 variant: impl name, "RY,NJ,ZC[,PF]", store policy."""
    o = {"stencil7_impl": {"buf": lhpc.S7_RING, "buf4": lhpc.S7_RING_X4, "buf4lds": lhpc.S7_RING_X4_LDS,
                           "simple": lhpc.S7_SIMPLE}[name],
         "stencil7_store": {"nt": lhpc.STORE_NT, "plain": lhpc.STORE_PLAIN, "staged": lhpc.STORE_STAGED}[store]}
    if cfg:
        for k, v in zip(("stencil7_ry", "stencil7_nj", "stencil7_zc", "stencil7_pf"), cfg.split(",")):
            o[k] = int(v)
    return o


@pytest.mark.parametrize("impl", S7_IMPLS)
@pytest.mark.parametrize("store", ["nt", "plain", "staged"])
def test_stencil7_every_impl(lhpc, gpu, impl, store):
    """Every stencil7 implementation / tiling / store mode selectable through
    lhpc_options.stencil7_* ("simple": the thread-per-column kernel the launcher
    falls back to when a row's byte offset does not fit a buffer voffset) is
    bit-exact against the oracle on ragged shapes: nx
    spanning several 512-wide x tiles with a partial last one, ny and nz not
    multiples of the row / z-chunk tiles, ghost widths 1 and 2."""
    name, _, cfg = impl.partition(":")
    opts = _s7_options(lhpc, name, cfg, store)
    if not _s7_in_product(name, cfg):
        with pytest.raises(lhpc.LhpcError) as e:
            u = np.zeros(5 * 6 * 7, np.float32)
            lhpc.stencil7(_dev(gpu, u), _dev(gpu, u.copy()), 3, 4, 5, 1, -6.0, 1.0, options=opts)
        assert e.value.status == -5
        return
    for (nz, ny, nx, g) in ((37, 45, 1100, 1), (9, 19, 130, 2), (3, 2, 1, 1)):
        shape = (nz + 2 * g, ny + 2 * g, nx + 2 * g)
        u = S.random_padded(shape, seed=nz * 7 + nx + g, zero_ghost=False).reshape(-1)
        out0 = S.random_padded(shape, seed=1234 + g).reshape(-1)
        want = S.stencil7_oracle(u, nz, ny, nx, g, -6.0, 1.0, out=out0.copy())
        got = lhpc.stencil7(_dev(gpu, u), _dev(gpu, out0), nz, ny, nx, g, -6.0, 1.0, options=opts).cpu().numpy()
        assert np.array_equal(got, want), (impl, store, nz, ny, nx, g)


S7_BUF4 = ["1,8,16", "1,8,0", "1,4,0", "1,8,0,3", "1,4,7,1", "2,4,7", "2,4,0", "2,8,0", "4,8,32", "4,4,32"]


@pytest.mark.parametrize("cfg", S7_BUF4)
@pytest.mark.parametrize("store", ["nt", "plain"])
@pytest.mark.parametrize("impl", ["buf4", "buf4lds"])
def test_stencil7_buf4(lhpc, gpu, cfg, store, impl):
    """The x4 ring (stencil7_impl = S7_RING_X4, 4 consecutive x per lane,
    dwordx4 loads/stores at 4-B alignment) is bit-exact against the oracle on
    shapes whose nx is a multiple of its tile width — one and several x tiles,
    ny / nz ragged against the row and z-chunk tiles, ghost widths 1 to 3 (so
    rows start at every 4-B phase of a 16-B line) — and on ragged nx, where the
    last x tile is partial (dword loads and stores past nx, every lane phase
    of the last x4: nx % 4 = 0..3, nx < 4)."""
    opts = _s7_options(lhpc, impl, cfg, store)
    if not _s7_in_product(impl, cfg):  # tuning-build tile: refused by the product library
        with pytest.raises(lhpc.LhpcError) as e:
            u = np.zeros(5 * 6 * 7, np.float32)
            lhpc.stencil7(_dev(gpu, u), _dev(gpu, u.copy()), 3, 4, 5, 1, -6.0, 1.0, options=opts)
        assert e.value.status == -5
        return
    for (nz, ny, nx, g) in ((37, 45, 1024, 1), (9, 19, 512, 2), (3, 2, 1536, 3), (5, 9, 512, 1),
                            (37, 45, 1100, 1), (9, 19, 130, 2), (3, 2, 1, 1), (5, 7, 517, 3), (2, 3, 1541, 1),
                            (4, 5, 768, 2), (3, 4, 258, 1), (6, 3, 3, 2)):
        shape = (nz + 2 * g, ny + 2 * g, nx + 2 * g)
        u = S.random_padded(shape, seed=nz * 7 + nx + g, zero_ghost=False).reshape(-1)
        out0 = S.random_padded(shape, seed=1234 + g).reshape(-1)
        want = S.stencil7_oracle(u, nz, ny, nx, g, -6.0, 1.0, out=out0.copy())
        got = lhpc.stencil7(_dev(gpu, u), _dev(gpu, out0), nz, ny, nx, g, -6.0, 1.0, options=opts).cpu().numpy()
        assert np.array_equal(got, want), (cfg, store, nz, ny, nx, g)


@pytest.mark.parametrize("rows", [1, 2, 4, 8, 16, 32])
def test_blur_x_every_impl(lhpc, gpu, rows):
    """The wave-private blur_x at every rows-per-wave setting (options.blur_x_rows)
    is bit-exact against the oracle on vector-eligible ragged shapes: nx not a
    multiple of the 256-float segment, ny not a multiple of the row group.
    (Unaligned shapes take the block-LDS kernel: test_blur_shapes_vs_oracle.)"""
    import torch
    for ny, nx, ghost in ((37, 260, 8), (5, 1300, 8), (70, 2048, 12), (1, 4, 8)):
        a = S.random_padded(((ny + 2 * ghost) * (nx + 2 * ghost),), seed=ny * 31 + nx)
        want = S.blur_oracle(a, ny, nx, ghost, 8, False)
        b = torch.empty(ny * nx, dtype=torch.float32, device=gpu)
        got = lhpc.blur_x(_dev(gpu, a), b, ny, nx, ghost, 8, options={"blur_x_rows": rows}).cpu().numpy()
        assert np.array_equal(got, want), (rows, ny, nx, ghost)


# ------------------------------------------------- variants no other test launches
BLUR_Y_TILES = [(4, 16), (4, 32), (2, 32), (2, 48), (1, 64), (1, 48), (1, 16)]
# (ny, nx, ghost): one cell row; a second column strip with two live threads at
# V = 4; a last y-tile of one row at TY = 32; nx % 4 == 2 with an even ghost
# (vec2 only); odd ghost (no vector path: every request falls back to 1 × 16);
# three strips × 7 y-tiles = 21 workgroups (not a multiple of the 8 XCDs) with
# ghost > nblur
BLUR_Y_SHAPES = [(1, 4, 8), (15, 1032, 8), (33, 1032, 8), (49, 518, 8), (65, 515, 9), (100, 2052, 12)]
_BLUR_CASES = {}


def _blur_case(ny, nx, ghost, nb, ydir):
    """(padded input with random ghost cells, oracle output), built once per shape."""
    key = (ny, nx, ghost, nb, ydir)
    if key not in _BLUR_CASES:
        a = S.random_padded(((ny + 2 * ghost) * (nx + 2 * ghost),), seed=ny * 7919 + nx + ghost, zero_ghost=False)
        want = S.blur_oracle(a, ny, nx, ghost, nb, ydir)
        want.setflags(write=False)
        _BLUR_CASES[key] = (a, want)
    return _BLUR_CASES[key]


def _nan_out(gpu, n):
    """An output buffer no stencil result equals: a cell the kernel skips fails the comparison."""
    import torch
    return torch.full((n,), float("nan"), dtype=torch.float32, device=gpu)


@pytest.mark.parametrize("vec,rows", BLUR_Y_TILES)
def test_blur_y_every_tile(lhpc, gpu, vec, rows):
    """Every register-window shape of k_blur_y<8, V, TY> the product library
    compiles (options.blur_y_vec / blur_y_rows; the selection is not visible
    through the ABI — read from blur_launch: a request the shape's alignment
    does not allow falls back to 4 × 16, then 1 × 16) is bit-exact against the
    oracle on BLUR_Y_SHAPES, random ghost cells, every cell stored."""
    for ny, nx, ghost in BLUR_Y_SHAPES:
        a, want = _blur_case(ny, nx, ghost, 8, True)
        got = lhpc.blur_y(_dev(gpu, a), _nan_out(gpu, ny * nx), ny, nx, ghost, 8,
                          options={"blur_y_vec": vec, "blur_y_rows": rows}).cpu().numpy()
        assert np.array_equal(got, want), (vec, rows, ny, nx, ghost)


@pytest.mark.parametrize("ny,nx,ghost", [(3, 1025, 8), (5, 2051, 9), (2, 4099, 8), (4, 2048, 10)])
def test_blur_x_block_lds_past_one_segment(lhpc, gpu, ny, nx, ghost):
    """The block-LDS k_blur_x<8, false, 2> (rows that are not 16-B aligned)
    with more than one 1024-wide segment (x0 > 0), a partial last segment and
    an odd row count; (4, 2048, 10): nx aligned but (ghost − 8) % 4 != 0."""
    a, want = _blur_case(ny, nx, ghost, 8, False)
    got = lhpc.blur_x(_dev(gpu, a), _nan_out(gpu, ny * nx), ny, nx, ghost, 8).cpu().numpy()
    assert np.array_equal(got, want)


GUARD = 8  # floats kept around an offset slice


def _offset_slice(gpu, host, off, fill=None):
    """(whole tensor, slice) — the slice holds `host` (or `fill`) and starts
    `off` floats into a larger device tensor: 4-B but, for off = 1..3, not 16-B aligned."""
    import torch
    n = host.size
    whole = torch.full((n + 2 * GUARD,), -4321.5, dtype=torch.float32, device=gpu)
    assert whole.data_ptr() % 16 == 0
    sl = whole[4 + off:4 + off + n]
    if fill is None:
        sl.copy_(torch.from_numpy(host))
    else:
        sl.fill_(fill)
    assert (off % 4 == 0) == (sl.data_ptr() % 16 == 0)
    return whole, sl


def _guards_intact(whole, off, n):
    w = whole.cpu().numpy()
    return (w[:4 + off] == -4321.5).all() and (w[4 + off + n:] == -4321.5).all()


@pytest.mark.parametrize("which", ["in", "out"])
@pytest.mark.parametrize("off", [1, 2, 3])
@pytest.mark.parametrize("ydir", [False, True])
def test_blur_unaligned_pointers(lhpc, gpu, ydir, off, which):
    """blur_launch's aligned16(a) && aligned16(b) fallbacks: a vector-eligible
    shape whose input or output starts 1, 2 or 3 floats into a larger device
    tensor gives the aligned run's bits (= the oracle's) and leaves the floats
    around the output slice alone."""
    ny, nx, ghost = 37, 1028, 8
    a, want = _blur_case(ny, nx, ghost, 8, ydir)
    fn = lhpc.blur_y if ydir else lhpc.blur_x
    aligned = fn(_dev(gpu, a), _nan_out(gpu, ny * nx), ny, nx, ghost, 8).cpu().numpy()
    assert np.array_equal(aligned, want)
    _, ad = _offset_slice(gpu, a, off if which == "in" else 0)
    whole, bd = _offset_slice(gpu, want, off if which == "out" else 0, fill=float("nan"))
    assert (ad if which == "in" else bd).data_ptr() % 16 != 0
    fn(ad, bd, ny, nx, ghost, 8)
    assert np.array_equal(bd.cpu().numpy(), want)
    assert _guards_intact(whole, off if which == "out" else 0, ny * nx)


@pytest.mark.parametrize("which", ["in", "out"])
@pytest.mark.parametrize("off", [1, 2, 3])
@pytest.mark.parametrize("impl", ["default", "buf4"])
def test_stencil7_unaligned_pointers(lhpc, gpu, impl, off, which):
    """stencil7 (the default entry point and S7_RING_X4) with `u` or `out`
    starting 1, 2 or 3 floats into a larger device tensor: the aligned run's
    bits (= the oracle's, ghost cells of `out` kept) and nothing written
    around the output slice."""
    nz, ny, nx, g = 9, 19, 516, 1
    shape = (nz + 2 * g, ny + 2 * g, nx + 2 * g)
    u = S.random_padded(shape, seed=516, zero_ghost=False).reshape(-1)
    out0 = S.random_padded(shape, seed=517).reshape(-1)
    want = S.stencil7_oracle(u, nz, ny, nx, g, -6.0, 1.0, out=out0.copy())
    opts = None if impl == "default" else {"stencil7_impl": lhpc.S7_RING_X4}
    aligned = lhpc.stencil7(_dev(gpu, u), _dev(gpu, out0), nz, ny, nx, g, -6.0, 1.0, options=opts).cpu().numpy()
    assert np.array_equal(aligned, want)
    _, ud = _offset_slice(gpu, u, off if which == "in" else 0)
    whole, od = _offset_slice(gpu, out0, off if which == "out" else 0)
    assert (ud if which == "in" else od).data_ptr() % 16 != 0
    lhpc.stencil7(ud, od, nz, ny, nx, g, -6.0, 1.0, options=opts)
    assert np.array_equal(od.cpu().numpy(), want)
    assert _guards_intact(whole, off if which == "out" else 0, u.size)


@pytest.mark.parametrize("buffers", ["device", "host"])
@pytest.mark.parametrize("ydir", [False, True])
@pytest.mark.parametrize("nblur", [0, 1, 5, 12])
def test_blur_generic_nblur(lhpc, gpu, nblur, ydir, buffers):
    """k_blur_x_generic / k_blur_y_generic (any nblur != 8): the identity
    (nblur = 0), 3, 11 and 25 taps (nblur = ghost = 12), one cell, one block
    and several blocks, device and host buffers."""
    ghost = 12
    fn = lhpc.blur_y if ydir else lhpc.blur_x
    for ny, nx in ((1, 1), (17, 33), (70, 300)):
        a, want = _blur_case(ny, nx, ghost, nblur, ydir)
        if buffers == "device":
            got = fn(_dev(gpu, a), _nan_out(gpu, ny * nx), ny, nx, ghost, nblur).cpu().numpy()
        else:
            got = fn(a.copy(), np.full(ny * nx, np.nan, dtype=np.float32), ny, nx, ghost, nblur)
        assert np.array_equal(got, want), (ny, nx)


def _s7_product_variants(lhpc):
    """(label, options) of every stencil7 variant the product library runs
    among those test_stencil7_every_impl and test_stencil7_buf4 accept; None:
    the default entry point."""
    out = [("default", None)]
    for impl in S7_IMPLS:
        name, _, cfg = impl.partition(":")
        if _s7_in_product(name, cfg):
            out += [(f"{impl}/{st}", _s7_options(lhpc, name, cfg, st)) for st in ("nt", "plain", "staged")]
    for name in ("buf4", "buf4lds"):
        for cfg in S7_BUF4:
            if _s7_in_product(name, cfg):
                out += [(f"{name}:{cfg}/{st}", _s7_options(lhpc, name, cfg, st)) for st in ("nt", "plain")]
    return out


# (c0, c1, a contracted kernel would differ from the oracle).  c0 = 0 makes
# c0·u an exact zero, so fma(c1, s, c0·u) = round(c1·s) whatever the kernel
# does: that pair checks a c1 that is no power of two, not the contraction;
# (0.7, 1/3) is there to check it with c1 = 1/3.
S7_COEFFS = [(0.3, -1.7, True), (0.0, 1.0 / 3.0, False), (0.7, 1.0 / 3.0, True)]


@pytest.mark.parametrize("c0,c1,distinguishes", S7_COEFFS)
def test_stencil7_coefficients_round_separately(lhpc, gpu, c0, c1, distinguishes):
    """lhpc.h: stencil7 rounds c0·u and c1·(…) separately, no contraction.
    With c1 = 1.0 (every other test) c1·(…) is exact and a fused kernel would
    pass; here c1·s is inexact.  The oracle itself tells the forms apart on
    these inputs: c1·s + c0·u rounded once, and either product fused into the
    add (fma(c1, s, round(c0·u)), fma(c0, u, round(c1·s))), each computed in
    fp64 from the exact products of fp32 numbers, differ from it on ≥ 1 % of
    the cells (measured: 8 – 38 %).  Every product implementation, tile and
    store mode, and the default entry point."""
    c0f, c1f = np.float32(c0), np.float32(c1)
    variants = _s7_product_variants(lhpc)
    assert len(variants) > 40
    for (nz, ny, nx, g) in ((9, 19, 130, 2), (5, 7, 517, 3)):
        shape = (nz + 2 * g, ny + 2 * g, nx + 2 * g)
        u = S.random_padded(shape, seed=nz * 7 + nx + g, zero_ghost=False).reshape(-1)
        out0 = S.random_padded(shape, seed=1234 + g).reshape(-1)
        want = S.stencil7_oracle(u, nz, ny, nx, g, float(c0f), float(c1f), out=out0.copy())
        u3 = u.reshape(shape)
        c = u3[g:-g, g:-g, g:-g]
        s = u3[g - 1:-g - 1, g:-g, g:-g] + u3[g + 1:shape[0] - g + 1, g:-g, g:-g]
        s = s + u3[g:-g, g - 1:-g - 1, g:-g]
        s = s + u3[g:-g, g + 1:shape[1] - g + 1, g:-g]
        s = s + u3[g:-g, g:-g, g - 1:-g - 1]
        s = s + u3[g:-g, g:-g, g + 1:shape[2] - g + 1]
        assert s.dtype == np.float32
        inner = want.reshape(shape)[g:-g, g:-g, g:-g]
        split = c0f * c + c1f * s  # fp32 throughout: the documented order
        assert split.dtype == np.float32 and np.array_equal(split, inner)
        p0, p1 = np.float64(c0f) * c.astype(np.float64), np.float64(c1f) * s.astype(np.float64)  # exact products
        for form, fused in (("c1*s + c0*u rounded once", p1 + p0),
                            ("fma(c1, s, round(c0*u))", p1 + (c0f * c).astype(np.float64)),
                            ("fma(c0, u, round(c1*s))", p0 + (c1f * s).astype(np.float64))):
            frac = np.mean(fused.astype(np.float32) != inner)
            assert (frac >= 0.01) == distinguishes, (form, frac)
        ud = _dev(gpu, u)
        for label, opts in variants:
            got = lhpc.stencil7(ud, _dev(gpu, out0), nz, ny, nx, g, float(c0f), float(c1f), options=opts).cpu().numpy()
            assert np.array_equal(got, want), (label, nz, ny, nx, g)


@pytest.mark.parametrize("blocks", [1, 7, 1000])
def test_stencil7_blocks_option(lhpc, gpu, blocks):
    """options.stencil7_blocks (the grid the z chunk is sized for): one z
    chunk, a few, and more chunks than planes allow (the chunk floor of 4
    planes) give the oracle's bits."""
    nz, ny, nx, g = 37, 45, 130, 1
    shape = (nz + 2 * g, ny + 2 * g, nx + 2 * g)
    u = S.random_padded(shape, seed=3745, zero_ghost=False).reshape(-1)
    out0 = S.random_padded(shape, seed=3746).reshape(-1)
    want = S.stencil7_oracle(u, nz, ny, nx, g, -6.0, 1.0, out=out0.copy())
    got = lhpc.stencil7(_dev(gpu, u), _dev(gpu, out0), nz, ny, nx, g, -6.0, 1.0,
                        options={"stencil7_blocks": blocks}).cpu().numpy()
    assert np.array_equal(got, want)
