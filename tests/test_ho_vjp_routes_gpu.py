"""GPU parity of the higher-order Gram VJP (gpsig_sig_gram_vjp_ho; csrc/sig_ho_bwd.h REG, sig_ho_bwd_lds.h LDS at
W = 4 / 8 in its unpinned, pinned and fenced variants, sig_ho_bwd_split.h SPLIT4 and SPLIT8) with fp64 autodiff of
the project's restatement of signature_kern_higher_order (oracle/autodiff_ref.py k_seq / k_seq_diag), at every route
and seam.  Every case first asks gpsig_sig_vjp_ho_route (ops.ho_vjp_route: host only, the launch path's own plan)
which kernel its shape takes and asserts it, so a case that moves to another route fails instead of passing for the
wrong reason.  Criterion: norm_rel_err < GTOL = 1e-5, as tests/test_grad_gpu.py and tests/test_ho_grad_gpu.py.

Data: random walks cumsum(randn) / sqrt(l d) unless a case says otherwise.  RECT cases take l1 != l2 (the route
follows l2 alone); the x side is short where the case is about the columns, so that the fp64 reference stays cheap.

Sections: a every code variant at a short and a full geometry; b the l2 seams from both sides on shared data; c
asymmetric lengths; d row windows and += accumulation; e the fused epilogue by direct call; f SPLIT8 past one launch;
g data and channel regimes on the split kernels.  Each comparison prints its error with the route it ran on."""
import numpy as np
import pytest
import torch

from conftest import norm_rel_err
from oracle import autodiff_ref as ar

pytestmark = pytest.mark.gpu
GTOL = 1e-5
DEV = "cuda"


def t(x):
    return torch.as_tensor(np.asarray(x, dtype=np.float32), device=DEV)


def walks(n, l, d, seed, scale=1.0, norm_l=None):
    inc = np.random.default_rng(seed).standard_normal((n, l, d)) / np.sqrt((norm_l or l) * d)
    return np.cumsum(inc, 1) * scale


def jumpy_walks(n, l, d, seed):
    """5 % of the steps 20 times larger."""
    rng = np.random.default_rng(seed)
    inc = rng.standard_normal((n, l, d)) / np.sqrt(l * d)
    inc[rng.random((n, l)) < 0.05] *= 20.0
    return np.cumsum(inc, 1)


def route_is(r, kernel, **want):
    got = {k: r[k] for k in want}
    assert r["kernel"] == kernel and got == want, (kernel, want, r)
    return f"{kernel} W{r['W']} v{r['variant']} slots {r['slots']}"


def check(got, ref, tag, what):
    err = norm_rel_err(got.detach().cpu().numpy() if torch.is_tensor(got) else got, ref)
    print(f"HOVJP [{tag}] {what}: err {err:.3e}")
    assert err < GTOL, (tag, what, err)


def ref_grads(X, Y, M, order, base, G, mode, weight=None):
    """fp64 autodiff of sum(G * K): (dX, dY) for mode 'rect', (dX, None) for 'upper' (K(X, X), all n x n entries)
    and 'diag'.  One backward per x-sequence, so the (l1, n2, l2) blocks of one row are all that is alive."""
    Xr = torch.tensor(X, requires_grad=True)
    Yr = torch.tensor(Y, requires_grad=True) if mode == "rect" else None
    Gt = torch.tensor(np.asarray(G, dtype=np.float64))
    if mode == "diag":
        (ar.k_seq_diag(Xr, M, base, order=order) * Gt).sum().backward()
        return Xr.grad.numpy(), None
    for a in range(X.shape[0]):
        if not bool((Gt[:, a] != 0).any()):
            continue
        cols = torch.nonzero((Gt[:, a] != 0).any(0)).flatten()
        other = Yr if mode == "rect" else Xr
        K = ar.k_seq(Xr[a:a + 1], other[cols], M, base, order=order)
        (K * Gt[:, a:a + 1][:, :, cols]).sum().backward()
    return Xr.grad.numpy(), None if Yr is None else Yr.grad.numpy()


def run_rect(l1, l2, d, M, order, base, n1, n2, seed, tag, X=None, Y=None):
    from gpsig_amd import ops
    X = walks(n1, l1, d, seed) if X is None else X
    Y = walks(n2, l2, d, seed + 1) if Y is None else Y
    G = np.random.default_rng(seed + 2).standard_normal((M + 1, n1, n2))
    gX, gY = ops.sig_gram_vjp(t(X), t(Y), M, t(G), base=base, gout_levels=True, order=order)
    rX, rY = ref_grads(X, Y, M, order, base, G, "rect")
    check(gX, rX, tag, f"rect {n1}x{n2} l1 {l1} l2 {l2} d {d} ({order},{M}) {base} dX")
    check(gY, rY, tag, f"rect {n1}x{n2} l1 {l1} l2 {l2} d {d} ({order},{M}) {base} dY")


def run_same(l, d, M, order, base, n, seed, tag, diag, X=None):
    from gpsig_amd import ops
    X = walks(n, l, d, seed) if X is None else X
    G = np.random.default_rng(seed + 3 + diag).standard_normal((M + 1, n) if diag else (M + 1, n, n))
    gX, _ = ops.sig_gram_vjp(t(X), None, M, t(G), base=base, gout_levels=True, diag=diag, order=order)
    rX, _ = ref_grads(X, None, M, order, base, G, "diag" if diag else "upper")
    check(gX, rX, tag, f"{'diag' if diag else 'upper'} n {n} l {l} d {d} ({order},{M}) {base} dX")


# ------------------------------------------------------------------ a. every code variant, short and full geometry
@pytest.mark.parametrize("l2", [2, 3, 5, 6, 256])
@pytest.mark.parametrize("order,M,base", [(2, 2, "rbf"), (2, 6, "rbf"), (2, 7, "linear"), (3, 5, "linear")])
def test_reg_kernel(order, M, base, l2):
    """The register kernel: a one-lane row (2 .. 5 points: lane 0's four columns), the first second lane (6 points)
    and the last column of lane 63 (256 points)."""
    from gpsig_amd import ops
    tag = route_is(ops.ho_vjp_route(2, l2 + 3, 2, l2, 2, M, order, base), "REG", W=4, waves=1, variant=0)
    run_rect(l2 + 3, l2, 2, M, order, base, 2, 2, 100 + l2 + M, tag)


LDS4 = [  # (order, M, variant, slots)
    (3, 6, 0, 55), (3, 7, 1, 67), (4, 6, 1, 79), (5, 6, 1, 99), (4, 7, 1, 99), (4, 8, 2, 119), (6, 6, 2, 111),
    (5, 7, 2, 129)]


@pytest.mark.parametrize("l2", [10, 256])
@pytest.mark.parametrize("order,M,variant,slots", LDS4)
def test_lds_w4_variants(order, M, variant, slots, l2):
    """The one-wave LDS kernel at W = 4: unpinned, pinned (to the 99 slots at the edge of the unfenced code) and
    fenced, at 10 and at 256 points."""
    from gpsig_amd import ops
    base = "rbf" if (order + M + l2) % 2 else "linear"
    tag = route_is(ops.ho_vjp_route(2, l2 + 3, 2, l2, 3, M, order, base), "LDS", W=4, waves=1, variant=variant,
                   slots=slots, lds_bytes=slots * 64 * 4 * 4)
    run_rect(l2 + 3, l2, 3, M, order, base, 2, 2, 200 + l2 + slots, tag)


@pytest.mark.parametrize("base", ["rbf", "linear"])
@pytest.mark.parametrize("order,M,variant,slots", [(5, 6, 1, 99), (4, 7, 1, 99), (4, 8, 2, 119)])
def test_lds_w4_edge_of_unfenced_both_bases(order, M, variant, slots, base):
    """99 slots, the last unfenced shapes, and the first fenced one of order 4, at the full 256 points, both seeds,
    cross and symmetric pairs."""
    from gpsig_amd import ops
    tag = route_is(ops.ho_vjp_route(2, 250, 2, 256, 2, M, order, base), "LDS", W=4, variant=variant, slots=slots)
    run_rect(250, 256, 2, M, order, base, 2, 2, 300 + slots, tag)
    route_is(ops.ho_vjp_route(2, 256, None, None, 2, M, order, base), "LDS", W=4, variant=variant)
    run_same(256, 2, M, order, base, 2, 310 + slots, tag, diag=False)


@pytest.mark.parametrize("l2,order,M,base,split_off", [
    (512, 2, 8, "rbf", False), (510, 3, 7, "linear", False), (257, 2, 3, "rbf", True), (509, 2, 3, "linear", True)])
def test_lds_w8(l2, order, M, base, split_off, monkeypatch):
    """The one-wave W = 8 kernel against the oracle: where the 8-wave form does not hold (2, 8) and (3, 7) at
    510 .. 512 points, and in place of SPLIT4 under GPSIG_HO_SPLIT=0."""
    from gpsig_amd import ops
    if split_off:
        assert ops.ho_vjp_route(1, l2 - 5, 2, l2, 2, M, order, base)["kernel"] == "SPLIT4"
        monkeypatch.setenv("GPSIG_HO_SPLIT", "0")
    slots = ops.ho_vjp_route(1, l2 - 5, 2, l2, 2, M, order, base)["slots"]
    tag = route_is(ops.ho_vjp_route(1, l2 - 5, 2, l2, 2, M, order, base), "LDS", W=8, waves=1, variant=2,
                   lds_bytes=slots * 64 * 8 * 4, slab_bytes=0)
    run_rect(l2 - 5, l2, 2, M, order, base, 1, 2, 400 + l2, tag)


@pytest.mark.parametrize("l2,order,M,base", [
    (257, 2, 3, "rbf"), (382, 2, 3, "linear"), (383, 2, 3, "rbf"), (509, 2, 3, "linear"),
    (257, 5, 5, "rbf"), (257, 3, 7, "linear"), (257, 2, 8, "rbf")])
def test_split4(l2, order, M, base):
    """Four waves per pair: 257 points (block 2 holds two cells, block 3 none), three exactly full blocks (382), a
    one-cell last block (383), four full blocks (509); the largest slabs (5, 5), (3, 7) and (2, 8) at 257."""
    from gpsig_amd import ops
    n1 = 1 if order >= 3 else 2
    tag = route_is(ops.ho_vjp_route(n1, l2 - 5, 2, l2, 2, M, order, base), "SPLIT4", W=2, waves=4, variant=0,
                   slab_bytes=0)
    run_rect(l2 - 5, l2, 2, M, order, base, n1, 2, 500 + l2 + M, tag)


@pytest.mark.parametrize("l2,order,M,base", [
    (510, 2, 3, "rbf"), (636, 2, 3, "linear"), (637, 2, 3, "rbf"), (1016, 2, 3, "linear"), (1017, 2, 3, "rbf"),
    (510, 2, 7, "linear"), (510, 3, 6, "linear"), (510, 5, 5, "rbf")])
def test_split8(l2, order, M, base):
    """Eight waves per pair with the slab in the workspace: 510 points (a two-cell fifth block), an exact block
    (636), a one-cell last block (637), 1016 and the full 1017; the edges of the (order, levels) it holds."""
    from gpsig_amd import ops
    n2 = 1 if order >= 3 else 2
    r = ops.ho_vjp_route(1, l2 - 5, n2, l2, 2, M, order, base)
    tag = route_is(r, "SPLIT8", W=2, waves=8, variant=0, lds_bytes=0, launches=1,
                   slab_bytes=1024 * 8 * r["slots"] * 128 * 4)
    run_rect(l2 - 5, l2, 2, M, order, base, 1, n2, 600 + l2 + M, tag)


@pytest.mark.parametrize("l2,order,M", [(1018, 2, 3), (257, 3, 8), (513, 2, 8)])
def test_refusals_leave_outputs_untouched(l2, order, M):
    """Past 1017 points, (3, 8) past 256 and (2, 8) past 512 nothing runs: GpsigError before any launch."""
    import gpsig_amd
    from gpsig_amd import ops
    with pytest.raises(gpsig_amd.GpsigError):
        ops.ho_vjp_route(1, 9, 1, l2, 2, M, order)
    assert not ops.ho_vjp_supported(l2, M, order)
    X, Y = t(walks(1, 9, 2, 1)), t(walks(1, l2, 2, 2))
    gX, gY = torch.full((1, 9, 2), 3.5, device=DEV), torch.full((1, l2, 2), -1.25, device=DEV)
    with pytest.raises(gpsig_amd.GpsigError):
        ops.sig_gram_vjp(X, Y, M, torch.ones((M + 1, 1, 1), device=DEV), gout_levels=True, order=order, gX=gX, gY=gY)
    torch.cuda.synchronize()
    assert bool((gX == 3.5).all()) and bool((gY == -1.25).all())


# ------------------------------------------------------------------ b. the seams from both sides, same data
@pytest.mark.parametrize("order,M,base", [(2, 3, "rbf"), (3, 4, "linear")])
@pytest.mark.parametrize("lo,hi,k_lo,k_hi", [(256, 257, "REG", "SPLIT4"), (509, 510, "SPLIT4", "SPLIT8")])
def test_length_seams_both_sides(lo, hi, k_lo, k_hi, order, M, base):
    """256 | 257 (REG -> SPLIT4) and 509 | 510 (SPLIT4 -> SPLIT8): the shorter walks are prefixes of the longer,
    each side against its own oracle, RECT (l1 != l2), UPPER and DIAG."""
    from gpsig_amd import ops
    n = 2 if hi < 510 else 1
    Yhi = walks(2, hi, 2, 700 + hi, norm_l=hi)
    Xs = walks(n, 40, 2, 701 + hi)
    for l2, kern in ((lo, k_lo), (hi, k_hi)):
        Y = np.ascontiguousarray(Yhi[:, :l2])
        tag = route_is(ops.ho_vjp_route(n, 40, 2, l2, 2, M, order, base), kern)
        run_rect(40, l2, 2, M, order, base, n, 2, 710 + l2, tag, X=Xs, Y=Y)
        m = 2 if l2 < 510 and order == 2 else 1
        route_is(ops.ho_vjp_route(m, l2, None, None, 2, M, order, base), kern)
        run_same(l2, 2, M, order, base, m, 720 + l2, tag, diag=False, X=Y[:m])
        route_is(ops.ho_vjp_route(m, l2, None, None, 2, M, order, base, diag=True), kern)
        run_same(l2, 2, M, order, base, m, 730 + l2, tag, diag=True, X=Y[:m])


# ------------------------------------------------------------------ c. asymmetric lengths
@pytest.mark.parametrize("l1,l2,kernel", [(2, 300, "SPLIT4"), (300, 2, "REG"), (3, 600, "SPLIT8"), (600, 5, "REG"),
                                          (700, 20, "REG"), (1100, 12, "REG")])
def test_asymmetric_lengths(l1, l2, kernel):
    """The route follows l2 alone.  l1 is the number of streamed rows and has no bound of its own (the records are
    padded per sequence to any length, wide.h wide_lw; the kernels index rows by l1 - 1 alone and the tile chunk
    takes fewer x-rows as they grow): 1100 rows against 12 columns."""
    from gpsig_amd import ops
    base = "rbf" if l1 < l2 else "linear"
    tag = route_is(ops.ho_vjp_route(2, l1, 2, l2, 3, 3, 2, base), kernel)
    run_rect(l1, l2, 3, 3, 2, base, 2, 2, 800 + l1 + l2, tag)
    if l1 > l2:  # and the LDS kernel's own grid on a long x side
        tag = route_is(ops.ho_vjp_route(1, l1, 2, l2, 3, 4, 4, base), "LDS", W=4)
        run_rect(l1, l2, 3, 4, 4, base, 1, 2, 810 + l1 + l2, tag)


# ------------------------------------------------------------------ d. row windows and accumulation
KERNEL_SHAPES = [("REG", 10, 2, 3), ("LDS", 10, 4, 4), ("SPLIT4", 257, 2, 2), ("SPLIT8", 510, 2, 2)]
WINDOWS = ((0, 3), (3, 5), (5, 7))


@pytest.mark.parametrize("mode", ["rect", "upper", "diag"])
@pytest.mark.parametrize("kernel,l,order,M", KERNEL_SHAPES)
def test_row_windows_accumulate(kernel, l, order, M, mode):
    """rows = (0, 3), (3, 5), (5, 7) into the same pre-filled gX / gY: the chunk loop starts its tiles at the
    4-aligned row below the window and zeroes the rows before it, the LDS and split launchers build their own grid
    from row_begin.  Result minus pre-fill = the full gradient; an empty window launches nothing, changes nothing."""
    from gpsig_amd import ops
    n1, n2, d, base = 7, 3, 2, "rbf" if kernel in ("REG", "SPLIT8") else "linear"
    l1 = l + 3 if l < 100 else 31
    rng = np.random.default_rng(900 + l + M)
    if mode == "rect":
        X, Y = walks(n1, l1, d, 901 + l), walks(n2, l, d, 902 + l)
        G = rng.standard_normal((M + 1, n1, n2))
        geo = (n1, l1, n2, l)
    else:
        X, Y = walks(n1, l, d, 903 + l), None
        G = rng.standard_normal((M + 1, n1) if mode == "diag" else (M + 1, n1, n1))
        geo = (n1, l, None, None)
    diag = mode == "diag"
    fillX = rng.standard_normal(X.shape).astype(np.float32)
    gX = t(fillX)
    gY = fillY = None
    if mode == "rect":
        fillY = rng.standard_normal(Y.shape).astype(np.float32)
        gY = t(fillY)
    kw = dict(base=base, gout_levels=True, diag=diag, order=order, gX=gX, gY=gY)
    r = ops.ho_vjp_route(*geo, d, M, order, base, diag=diag, rows=(2, 2))
    tag = route_is(r, kernel, chunks=0, launches=0)
    ops.sig_gram_vjp(t(X), None if Y is None else t(Y), M, t(G), rows=(2, 2), **kw)
    assert np.array_equal(gX.cpu().numpy(), fillX) and (gY is None or np.array_equal(gY.cpu().numpy(), fillY))
    for w in WINDOWS:
        route_is(ops.ho_vjp_route(*geo, d, M, order, base, diag=diag, rows=w), kernel, chunks=1, launches=1)
        ops.sig_gram_vjp(t(X), None if Y is None else t(Y), M, t(G), rows=w, **kw)
    rX, rY = ref_grads(X, Y, M, order, base, G, mode)
    check(gX.cpu().numpy().astype(np.float64) - fillX, rX, tag, f"windows {mode} l {l} ({order},{M}) dX")
    if mode == "rect":
        check(gY.cpu().numpy().astype(np.float64) - fillY, rY, tag, f"windows {mode} l {l} ({order},{M}) dY")


# ------------------------------------------------------------------ e. the fused epilogue by direct call
@pytest.mark.parametrize("upper", [False, True])
@pytest.mark.parametrize("base", ["rbf", "linear"])
@pytest.mark.parametrize("kernel,l,order,M", KERNEL_SHAPES)
def test_fused_epilogue_direct(kernel, l, order, M, base, upper):
    """rs1, rs2, scale, jitter, grs1, grs2, gscale with per-level and with summed gout, against fp64 autodiff of
        out_m(a, b) = scale_m rs1_m(a) rs2_m(b) (K_m(a, b) + jitter [a == b, UPPER]),   Loss = sum gout out
    with respect to X, Y, rs1, rs2 and scale.  rs are random in [0.5, 2], not the true diagonals: the VJP treats them
    as independent inputs.  UPPER passes rs2 = rs1 and grs2 = grs1 as autograd.SigGram.backward does, and the one
    buffer holds both sides' sum; the level sums K_m the split kernels need here are combined across their waves."""
    from gpsig_amd import ops
    d = 2
    n1, n2 = (2, 2) if upper else (2, 3)
    l1 = l if upper else (l + 3 if l < 100 else 29)
    rng = np.random.default_rng(1000 + l + M + upper)
    X = walks(n1, l1, d, 1001 + l + upper)
    Y = None if upper else walks(n2, l, d, 1002 + l)
    rs1 = rng.uniform(0.5, 2.0, (M + 1, n1))
    rs2 = rs1 if upper else rng.uniform(0.5, 2.0, (M + 1, n2))
    scale = rng.uniform(0.5, 2.0, M + 1)
    jitter = 1e-3 if upper else 0.0
    geo = (n1, l1, None, None) if upper else (n1, l1, n2, l)
    tag = route_is(ops.ho_vjp_route(*geo, d, M, order, base), kernel)
    for levels in (True, False):
        G = rng.standard_normal((M + 1, n1, n2) if levels else (n1, n2))
        grs1 = torch.zeros((M + 1, n1), device=DEV)
        grs2 = grs1 if upper else torch.zeros((M + 1, n2), device=DEV)
        gscale = torch.zeros(M + 1, device=DEV)
        gX, gY = ops.sig_gram_vjp(t(X), None if upper else t(Y), M, t(G), base=base, gout_levels=levels, order=order,
                                  rs1=t(rs1), rs2=t(rs2), scale=t(scale), jitter=jitter, grs1=grs1, grs2=grs2,
                                  gscale=gscale)
        Xr = torch.tensor(X, requires_grad=True)
        Yr = Xr if upper else torch.tensor(Y, requires_grad=True)
        r1 = torch.tensor(rs1, requires_grad=True)
        r2 = r1 if upper else torch.tensor(rs2, requires_grad=True)
        sc = torch.tensor(scale, requires_grad=True)
        K = ar.k_seq(Xr, Yr, M, base, order=order)
        if upper:
            K = K + jitter * torch.eye(n1, dtype=torch.float64)
        out = sc[:, None, None] * r1[:, :, None] * r2[:, None, :] * K
        ((out if levels else out.sum(0)) * torch.tensor(G)).sum().backward()
        what = f"epilogue {'upper' if upper else 'rect'} l {l} ({order},{M}) {base} levels {int(levels)}"
        check(gX, Xr.grad.numpy(), tag, what + " dX")
        if not upper:
            check(gY, Yr.grad.numpy(), tag, what + " dY")
            check(grs2, r2.grad.numpy(), tag, what + " drs2")
        check(grs1, r1.grad.numpy(), tag, what + " drs1")
        check(gscale, sc.grad.numpy(), tag, what + " dscale")


# ------------------------------------------------------------------ f. SPLIT8 past one launch
@pytest.mark.parametrize("l1,chunks", [(12, 1), (510, 2)])
def test_split8_more_than_1024_pairs(l1, chunks):
    """33 x 33 = 1089 pairs of 510 columns.  With a short x side they are one chunk, which SPLIT8 runs as two
    launches of at most 1024 workgroups, the second offset by blk0; with 510 rows the 1 GiB point-weight tile holds
    28 x-rows, so the pairs go as two chunks of one launch each.  gout is zero but for six pairs at the corners of
    both launches / chunks, so the oracle evaluates six pairs."""
    from gpsig_amd import _lib as Lb
    from gpsig_amd import ops
    n, l2, d, M, order, base = 33, 510, 2, 2, 2, "linear"
    r = ops.ho_vjp_route(n, l1, n, l2, d, M, order, base)
    tag = route_is(r, "SPLIT8", chunks=chunks, launches=2, slab_bytes=1024 * 8 * 7 * 128 * 4)
    # the slab region is the workspace's growth over a shape with the same tiles and no slab ((2, 8): LDS W = 8)
    lib = Lb.load()
    assert ops.ho_vjp_route(n, l1, n, l2, d, 8, order, base)["slab_bytes"] == 0
    grow = lib.gpsig_sig_vjp_ho_workspace_bytes(n, l1, n, l2, d, M, order, ops.base_kind(base)) - \
        lib.gpsig_sig_vjp_ho_workspace_bytes(n, l1, n, l2, d, 8, order, ops.base_kind(base))
    assert grow == r["slab_bytes"]
    X, Y = walks(n, l1, d, 1100 + l1), walks(n, l2, d, 1101)
    G = np.zeros((M + 1, n, n))
    for a in (0, 32):
        for b in (0, 31, 32):
            G[:, a, b] = np.random.default_rng(1102 + a + b).standard_normal(M + 1)
    gX, gY = ops.sig_gram_vjp(t(X), t(Y), M, t(G), base=base, gout_levels=True, order=order)
    rX, rY = ref_grads(X, Y, M, order, base, G, "rect")
    check(gX, rX, tag, f"1089 pairs l1 {l1} dX")
    check(gY, rY, tag, f"1089 pairs l1 {l1} dY")


# ------------------------------------------------------------------ g. data and channel regimes on the split kernels
@pytest.mark.parametrize("regime", ["jumpy-rbf", "jumpy-linear", "rbf-0.1x", "rbf-3x", "d1", "d9", "d33"])
@pytest.mark.parametrize("kernel,l2", [("SPLIT4", 257), ("SPLIT8", 510)])
def test_split_kernels_data_and_channel_regimes(kernel, l2, regime):
    """One pair at (2, 3): walks with 5 % of the steps 20 times larger, RBF walks at 0.1 and 3 times the usual
    scale, and 1, 9 and 33 channels (the wide-channel seed's channel loop)."""
    from gpsig_amd import ops
    M, order, l1 = 3, 2, l2 - 5
    d = int(regime[1:]) if regime[0] == "d" else 2
    base = "linear" if regime == "jumpy-linear" else "rbf"
    seed = 1200 + l2 + len(regime)
    if regime.startswith("jumpy"):
        X, Y = jumpy_walks(1, l1, d, seed), jumpy_walks(1, l2, d, seed + 1)
    else:
        s = {"rbf-0.1x": 0.1, "rbf-3x": 3.0}.get(regime, 1.0)
        X, Y = walks(1, l1, d, seed, s), walks(1, l2, d, seed + 1, s)
    tag = route_is(ops.ho_vjp_route(1, l1, 1, l2, d, M, order, base), kernel)
    run_rect(l1, l2, d, M, order, base, 1, 1, seed, tag + " " + regime, X=X, Y=Y)
