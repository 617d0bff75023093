"""GPU parity of the first-order fp32 Gram and diagonal (csrc/sig_fo.h: the fixed-channel kernels, the 10-lane
groups, the column blocks; csrc/wide.h: the runtime channel loop and the diagonal's seed tiles; csrc/sig_fo_mf.h: the
matrix-core Gram) with the float64 oracle (oracle/kernels_ref.py, signature_algs.py:8-35) on the fp32-rounded inputs
the kernels receive, at every route and geometry seam.  Every case asks gpsig_sig_fo_route (ops.fo_route: host
only, the launch path's own helpers; its table is pinned in tests/test_fo_routes.py) which route its shape takes and
asserts it before it compares, so a case that a retuned seam moves to another kernel fails instead of passing for
the wrong reason.

Bar: norm_rel_err < TOL = 1e-5 per level on the raw levels of ops.sig_gram / ops.sig_diag.  Data: the benchmark's
walks cumsum(N(0,1)) / sqrt(L D).  In K(X, Y) X is three points longer than Y; the lengths named are Y's (the columns
decide the route), and K(Y) and the diagonal of Y sit on the same seam.

Largest per-level errors per route group on an MI355X (the MAXERR lines this module prints), bar 1e-5:
  a  fixed geometries      rbf 3.0e-6, linear 1.1e-6, matern32 7.5e-7, the three point seeds <= 1.5e-7
  b  column blocks         rbf 1.1e-6 (4 columns per lane 1.4e-6), linear 2.4e-6, matern12 3.8e-7, rbf-point 1.1e-7;
                           the largest carry (1463 x 513, M = 8) 3.7e-6
  c  fixed-path tiles      2.0e-6
  d  channel loop          rbf 1.1e-6, linear 1.1e-6 (difference seeds, RECT and UPPER)
  e  matrix cores          W and block seams rbf 7.0e-6, linear 8.6e-6: both level 2 of K(X, Y) at 255 points, whose
                           largest entry on this data is a quarter of its neighbours' (1.6e-2 against 6.1e-2 at 256
                           points; the same absolute error), every other case <= 3.6e-6; waves seams 9.0e-7; 8-float
                           carries 3.3e-6; tile rows 6.2e-7; 257 workgroups in two launches 4.0e-6
  f  wide diagonal         tile seams 3.8e-7, second chunk 2.9e-7
  g  fused epilogue        10-lane groups 1.1e-6, channel loop 6.8e-7, matrix cores 1.6e-6
"""
import numpy as np
import pytest
import torch

from conftest import norm_rel_err
from oracle import kernels_ref as kr

pytestmark = pytest.mark.gpu
TOL = 1e-5
DEV = "cuda"
SEEDS = {"rbf": ("rbf", True), "linear": ("linear", True), "rbf-point": ("rbf", False),
         "linear-point": ("linear", False), "matern12": ("matern12", True), "matern32": ("matern32", True),
         "matern32-point": ("matern32", False)}
MAXERR = {}


@pytest.fixture(scope="module", autouse=True)
def report_max_errors():
    yield
    for group, e in sorted(MAXERR.items()):
        print(f"MAXERR {group}: {e:.2e}")


def t(x):
    return torch.as_tensor(np.asarray(x, dtype=np.float32), device=DEV)


def r32(x):
    """The fp32-rounded inputs the kernels receive, as the oracle's float64."""
    return np.asarray(x).astype(np.float32).astype(np.float64)


def walks(n, l, d, seed):
    rng = np.random.default_rng(seed)
    return r32(np.cumsum(rng.standard_normal((n, l, d)), 1) / np.sqrt(l * d))


def assert_levels(got, exp, group, what, tol=TOL):
    err = norm_rel_err(got, exp, axis_levels=True)
    print(f"{group} {what}: per-level err {np.array2string(err, precision=2)}")
    MAXERR[group] = max(MAXERR.get(group, 0.0), float(err.max()))
    assert (err < tol).all(), (group, what, err)


def assert_route(r, want, what):
    got = {k: r[k] for k in want}
    assert got == want, (what, r)


def reference(M, seed):
    base, diff = SEEDS[seed]
    return kr.SignatureKernelRef(1, 1, M, normalization=False, base=base, difference=diff)


def oracle_gram(ref, X, Y=None, chunk=4):
    """ref.K_seq in chunks of x-sequences (the 4-D base-kernel grid of a whole Gram is large at many sequences)."""
    Z = X if Y is None else Y
    return np.concatenate([ref.K_seq(X[a:a + chunk], Z) for a in range(0, len(X), chunk)], axis=1)


def check_case(group, l2, D, M, seed, want, want_sym=None, want_diag=None, n1=5, n2=4, modes=("xy", "sym", "diag"),
               l1=None, data_seed=0):
    """K(X, Y), K(Y) and diag(Y) against the oracle, routes first.  want: the route keys of K(X, Y) that are compared;
    want_sym / want_diag: those of K(Y) / the diagonal (default: want without the per-mode keys)."""
    from gpsig_amd import ops
    base, diff = SEEDS[seed]
    l1 = l2 + 3 if l1 is None else l1
    X = walks(n1, l1, D, 7919 * l2 + 31 * D + M + data_seed)
    Y = walks(n2, l2, D, 7919 * l2 + 31 * D + M + data_seed + 1)
    ref = reference(M, seed)
    strip = lambda w: {k: v for k, v in w.items() if k not in ("pairs_per_wave", "workgroups", "launches")}  # noqa: E731
    if "xy" in modes:
        assert_route(ops.fo_route(n1, l1, n2, l2, D, M, base, diff), want, "K(X, Y)")
    if "sym" in modes:
        assert_route(ops.fo_route(n2, l2, None, None, D, M, base, diff), strip(want) if want_sym is None else want_sym,
                     "K(Y)")
    if "diag" in modes:
        assert_route(ops.fo_route(n2, l2, None, None, D, M, base, diff, diag=True),
                     strip(want) if want_diag is None else want_diag, "diag(Y)")
    Xt, Yt = t(X), t(Y)
    out = {}
    if "xy" in modes:
        out["xy"] = ops.sig_gram(Xt, Yt, M, base=base, difference=diff).cpu().numpy()
        assert_levels(out["xy"], ref.K_seq(X, Y), group, f"K(X, Y) {seed} l2={l2} D={D} M={M}")
    if "sym" in modes:
        out["sym"] = ops.sig_gram(Yt, None, M, base=base, difference=diff).cpu().numpy()
        assert_levels(out["sym"], ref.K_seq(Y), group, f"K(Y) {seed} l2={l2} D={D} M={M}")
        np.testing.assert_array_equal(out["sym"], out["sym"].transpose(0, 2, 1))
    if "diag" in modes:
        out["diag"] = ops.sig_diag(Yt, M, base=base, difference=diff).cpu().numpy()
        assert_levels(out["diag"], ref.K_seq_diag(Y), group, f"diag(Y) {seed} l2={l2} D={D} M={M}")
    return out


# ------------------------------------------------------------------------------------------ a. fixed geometries
# (W, LP, nblk) by fo_wmax (tests/test_fo_routes.py): 8 columns per lane, 4 at D = 8 with M = 7, and the 10-lane groups
G8 = {32: (2, 16, 1), 33: (4, 16, 1), 64: (4, 16, 1), 65: (8, 16, 1), 100: (8, 16, 1), 101: (8, 16, 1),
      128: (8, 16, 1), 129: (8, 32, 1), 256: (8, 32, 1), 257: (8, 64, 1), 512: (8, 64, 1), 513: (8, 64, 2)}
G10 = {**G8, 65: (10, 10, 1), 100: (10, 10, 1)}
G4 = {32: (2, 16, 1), 33: (4, 16, 1), 64: (4, 16, 1), 65: (4, 32, 1), 100: (4, 32, 1), 101: (4, 32, 1),
      128: (4, 32, 1), 129: (4, 64, 1), 256: (4, 64, 1), 257: (4, 64, 2), 512: (4, 64, 3), 513: (4, 64, 3)}
CLASSES = {(5, 5): (5, G10), (6, 5): (6, G8), (5, 6): (5, G8), (7, 6): (8, G8), (8, 7): (8, G4)}


@pytest.mark.parametrize("l2", sorted(G8))
@pytest.mark.parametrize("D,M", sorted(CLASSES))
def test_fixed_geometry_seams_rbf(D, M, l2):
    DP, table = CLASSES[D, M]
    W, LP, nblk = table[l2]
    check_case("a fixed rbf", l2, D, M, "rbf", dict(path=0, DP=DP, W=W, LP=LP, nblk=nblk, pairs_per_wave=64 // LP))


@pytest.mark.parametrize("l2", [33, 65, 129, 257, 513])
@pytest.mark.parametrize("seed", ["linear", "rbf-point", "linear-point", "matern32", "matern32-point"])
def test_fixed_geometry_other_seeds(seed, l2):
    W, LP, nblk = G8[l2]
    check_case("a fixed " + seed, l2, 3, 4, seed, dict(path=0, DP=3, W=W, LP=LP, nblk=nblk, pairs_per_wave=64 // LP))


# ------------------------------------------------------------------------------------------ b. column blocks
@pytest.mark.parametrize("seed,l2,nblk", [("rbf", 1023, 2), ("rbf", 1024, 3), ("linear", 1023, 2), ("linear", 1024, 3),
                                          ("rbf-point", 1022, 2), ("rbf-point", 1023, 3), ("matern12", 1023, 2),
                                          ("matern12", 1024, 3)])
def test_block_count_seams(seed, l2, nblk):
    """Blocks of 511 cells: l2 - 1 cells with difference, l2 without.  The walk's step is the benchmark's,
    1 / sqrt(L D); the errors of these cases are in the header."""
    check_case("b blocks " + seed, l2, 2, 3, seed, dict(path=0, DP=2, W=8, LP=64, nblk=nblk, pairs_per_wave=1),
               n1=3, n2=2)


@pytest.mark.parametrize("l2,nblk", [(511, 2), (512, 3)])
def test_block_count_seam_four_columns(l2, nblk):
    """Blocks of 255 cells at 4 columns per lane (D = 8, M = 7)."""
    check_case("b blocks rbf W4", l2, 8, 7, "rbf", dict(path=0, DP=8, W=4, LP=64, nblk=nblk, pairs_per_wave=1),
               n1=3, n2=2)


def test_largest_carry():
    """4 waves x 1462 rows x 7 levels x 4 B = 163744 B of carries, the most the 160 KiB of LDS take; one more row is
    refused by the route and by the call."""
    import gpsig_amd
    from gpsig_amd import ops
    check_case("b largest carry", 513, 2, 8, "rbf", dict(path=0, W=8, LP=64, nblk=2, carry_bytes=163744, launches=1),
               n1=3, n2=2, l1=1463, modes=("xy",))
    with pytest.raises(gpsig_amd.GpsigError):
        ops.fo_route(3, 1464, 2, 513, 2, 8)
    with pytest.raises(gpsig_amd.GpsigError):
        ops.sig_gram(t(walks(3, 1464, 2, 1)), t(walks(2, 513, 2, 2)), 8)


# ------------------------------------------------------------------------------------------ c. tiles of the fixed paths
def windows_match(full, X, M, windows, rect=True):
    """Row windows of the symmetric call (and of K(X, X)) against the full symmetric one, with the tolerance of
    test_gram_gpu.test_row_windows_and_rect_tiles."""
    from gpsig_amd import ops
    n = len(X)
    for r0, r1 in windows:
        up = torch.zeros(M + 1, r1 - r0, n, device=DEV)
        ops.sig_gram(X, None, M, rows=(r0, r1), out=up)
        mask = torch.arange(n, device=DEV)[None, :] >= torch.arange(r0, r1, device=DEV)[:, None]
        torch.testing.assert_close(up[:, mask], full[:, r0:r1][:, mask], rtol=1e-5, atol=1e-6)
        if rect:
            part = ops.sig_gram(X, X, M, rows=(r0, r1))
            torch.testing.assert_close(part, full[:, r0:r1], rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("L,LP", [(200, 32), (300, 64)])
def test_fixed_path_tiles(L, LP):
    """UPPER, RECT and DIAG tiles of 4 x-sequences x G = 64 / LP y-sequences around the tile sizes, and row windows
    (one row, mid-tile, across tiles) of the largest batch."""
    from gpsig_amd import ops
    D, M, G = 3, 3, 64 // LP
    ref = reference(M, "rbf")
    Xall = walks(3 * 4 * G + 2, L, D, L)
    Y = walks(3, L, D, L + 1)
    for n in (1, 4 * G - 1, 4 * G, 4 * G + 1, 3 * 4 * G + 2):
        X = Xall[:n]
        want = dict(path=0, DP=3, W=8, LP=LP, nblk=1)
        ta, tb = (n + 3) // 4, (n + G - 1) // G
        assert_route(ops.fo_route(n, L, None, None, D, M), dict(want, pairs_per_wave=G, launches=1,
                                                                workgroups=sum(tb - 4 * r // G for r in range(ta))), n)
        assert_route(ops.fo_route(n, L, 3, L, D, M), dict(want, workgroups=ta * ((3 + G - 1) // G)), n)
        assert_route(ops.fo_route(n, L, None, None, D, M, diag=True), dict(want, pairs_per_wave=1, workgroups=ta), n)
        sym = ops.sig_gram(t(X), None, M)
        exp = oracle_gram(ref, X)
        assert_levels(sym.cpu().numpy(), exp, "c fixed tiles", f"K(X) L={L} n={n}")
        assert torch.equal(sym, sym.transpose(1, 2))
        assert_levels(ops.sig_gram(t(X), t(Y), M).cpu().numpy(), oracle_gram(ref, X, Y), "c fixed tiles",
                      f"K(X, Y) L={L} n={n}")
        assert_levels(ops.sig_diag(t(X), M).cpu().numpy(), np.stack([np.diagonal(e) for e in exp]), "c fixed tiles",
                      f"diag(X) L={L} n={n}")
    n = len(Xall)
    assert ops.fo_route(n, L, None, None, D, M, rows=(5, 5))["launches"] == 0
    windows_match(sym, t(Xall), M, [(0, 3), (5, 6), (2, 7), (4 * G + 1, n), (n - 1, n)])


# ------------------------------------------------------------------------------------------ d. channel loop, difference seeds
@pytest.mark.parametrize("seed,D,l2,W,LP,nblk", [("rbf", 545, 20, 4, 16, 1), ("rbf", 225, 70, 8, 16, 1),
                                                 ("rbf", 161, 140, 8, 32, 1), ("rbf", 225, 300, 8, 64, 1),
                                                 ("rbf", 225, 520, 8, 64, 2), ("linear", 545, 20, 8, 16, 1),
                                                 ("linear", 225, 70, 8, 16, 1)])
def test_channel_loop_difference_seeds(seed, D, l2, W, LP, nblk):
    """Past the matrix cores' LDS bound the RBF / linear difference seeds run the channel loop in RECT and UPPER:
    sig_fo_kernel<0, W, LP, M, SEED_RBF_DIFF / SEED_LIN_DIFF>."""
    want = dict(path=1, DP=0, W=W, LP=LP, nblk=nblk, pairs_per_wave=64 // LP, nw=0, xb=0)
    wd = dict(path=1, DP=0, W=W, LP=LP, nblk=nblk, dtiles=1 if seed == "rbf" and nblk == 1 else 0)
    check_case("d channel loop " + seed, l2, D, 4, seed, want, want_diag=wd)


@pytest.mark.parametrize("seed", ["rbf", "linear"])
def test_channel_loop_saved_state(seed):
    """The saved-state launch of the channel loop writes the plain launch's Gram bit for bit (as
    test_fo_rowloop_gpu.test_saved_state_launch_writes_the_same_gram on the fixed path)."""
    from gpsig_amd import ops
    D, L, M, n1, n2 = 225, 70, 4, 5, 4
    X, Y = t(walks(n1, L + 3, D, 1)), t(walks(n2, L, D, 2))
    want = dict(path=1, DP=0, W=8, LP=16, nblk=1)
    assert_route(ops.fo_route(n1, L + 3, n2, L, D, M, seed, state=True), want, "K(X, Y), state")
    assert_route(ops.fo_route(n2, L, None, None, D, M, seed, state=True), want, "K(Y), state")
    state = torch.empty(ops.sig_state_numel(n1, n2, L, M), dtype=torch.float32, device=DEV)
    assert torch.equal(ops.sig_gram(X, Y, M, base=seed, state=state), ops.sig_gram(X, Y, M, base=seed))
    state = torch.empty(ops.sig_state_numel(n2, None, L, M), dtype=torch.float32, device=DEV)
    assert torch.equal(ops.sig_gram(Y, None, M, base=seed, state=state), ops.sig_gram(Y, None, M, base=seed))


# ------------------------------------------------------------------------------------------ e. matrix cores
def wide_geo(l, seed):
    """The channel loop's (W, LP, nblk) (the diagonal past 8 channels)."""
    if l <= 64 and seed == "rbf":
        return 4, 16, 1
    return (8, 16, 1) if l <= 128 else (8, 32, 1) if l <= 256 else (8, 64, 1 if l <= 512 else 2)


def mf_case(group, l2, D, M, seed, W, nblk, nw, **kw):
    want = dict(path=2, DP=0, W=W, LP=16, nblk=nblk, nw=nw, xb=4 * nw, np=2, cw=4 if M <= 5 else 8, pairs_per_wave=0)
    gw = wide_geo(l2, seed)
    wd = dict(path=1, DP=0, W=gw[0], LP=gw[1], nblk=gw[2], nw=0, xb=0, dtiles=1 if seed == "rbf" and gw[2] == 1 else 0)
    return check_case(group, l2, D, M, seed, want, want_diag=wd, **kw)


@pytest.mark.parametrize("l2,W,nblk", [(64, 4, 1), (65, 8, 1), (128, 8, 1), (129, 10, 1), (160, 10, 1), (161, 8, 2),
                                       (255, 8, 2), (256, 8, 3)])
@pytest.mark.parametrize("seed", ["rbf", "linear"])
def test_matrix_core_w_and_block_seams(seed, l2, W, nblk):
    mf_case("e matrix cores W " + seed, l2, 9, 4, seed, W, nblk, 8)


@pytest.mark.parametrize("l2,D,nw", [(40, 480, 8), (40, 481, 4), (40, 544, 4), (100, 160, 8), (100, 161, 4),
                                     (100, 224, 4), (140, 96, 8), (140, 97, 4), (140, 160, 4), (170, 160, 8),
                                     (170, 161, 4), (170, 224, 4)])
def test_matrix_core_wave_seams(l2, D, nw):
    """8 waves per workgroup while the B image and 8 tiles fit 160 KiB, then 4; one channel more than the last of
    these is the channel loop's (test_channel_loop_difference_seeds)."""
    W, nblk = (4, 1) if l2 <= 64 else (8, 1) if l2 <= 128 else (10, 1) if l2 <= 160 else (8, 2)
    mf_case("e matrix cores nw", l2, D, 3, "rbf", W, nblk, nw, n2=5, modes=("xy", "sym"))


@pytest.mark.parametrize("seed,M", [("linear", 6), ("rbf", 6)])
def test_matrix_core_eight_float_carries(seed, M):
    """cw = 8: the carry rows of a blocked launch past 5 levels."""
    mf_case("e matrix cores cw8 " + seed, 161, 9, M, seed, 8, 2, 8, modes=("xy", "sym"))


@pytest.mark.parametrize("D,L,xb,sizes", [(9, 20, 32, (31, 32, 33, 65)), (97, 130, 16, (15, 16, 17, 33))])
def test_matrix_core_tile_rows(D, L, xb, sizes):
    """More than one tile row of xb x-sequences: UPPER's tile prefix, a partial last tile, RECT against 3 sequences,
    and row windows that start inside a tile, against the oracle and the full call."""
    from gpsig_amd import ops
    M = 3
    ref = reference(M, "rbf")
    Xall = walks(max(sizes), L, D, D + L)
    Y = walks(3, L, D, D + L + 1)
    W = 4 if L <= 64 else 10
    for n in sizes:
        X = Xall[:n]
        want = dict(path=2, W=W, LP=16, nblk=1, nw=xb // 4, xb=xb, launches=1)
        tr = (n + xb - 1) // xb
        assert_route(ops.fo_route(n, L, None, None, D, M), dict(want, workgroups=sum(n - xb * r for r in range(tr))), n)
        assert_route(ops.fo_route(n, L, 3, L, D, M), dict(want, workgroups=3 * tr), n)
        sym = ops.sig_gram(t(X), None, M)
        assert_levels(sym.cpu().numpy(), oracle_gram(ref, X), "e matrix cores tiles", f"K(X) D={D} L={L} n={n}")
        assert torch.equal(sym, sym.transpose(1, 2))
        assert_levels(ops.sig_gram(t(X), t(Y), M).cpu().numpy(), oracle_gram(ref, X, Y), "e matrix cores tiles",
                      f"K(X, Y) D={D} L={L} n={n}")
    n = max(sizes)
    wins = [(9, 21), (30, 34), (32, 65), (33, 34)] if xb == 32 else [(5, 11), (14, 18), (16, 33), (17, 18)]
    tiles = [n, n + (n - xb), (n - xb) + (n - 2 * xb), n - xb]   # tile rows 0 | 0, 1 | 1, 2 | 1
    for w, wg in zip(wins, tiles):
        assert_route(ops.fo_route(n, L, None, None, D, M, rows=w), dict(path=2, xb=xb, workgroups=wg, launches=1), w)
    windows_match(sym, t(Xall), M, wins, rect=False)


@pytest.mark.parametrize("M", [2, 6])
def test_matrix_core_second_launch_chunk(M):
    """A column-blocked launch of 257 workgroups: the second chunk of MF_BLK_CHUNK = 256 runs one workgroup with
    blk0 = 256 on the first chunk's carry scratch.  Y repeats three sequences, so the oracle evaluates nine pairs
    and every column of a repeat equals its original's bit for bit."""
    from gpsig_amd import ops
    n1, n2, l2, D = 3, 257, 161, 9
    assert_route(ops.fo_route(n1, l2 + 3, n2, l2, D, M),
                 dict(path=2, W=8, LP=16, nblk=2, nw=8, xb=32, cw=4 if M <= 5 else 8, workgroups=257, launches=2,
                      carry_bytes=256 * 32 * (l2 + 2) * 8 * 4), M)
    X, Y3 = walks(n1, l2 + 3, D, 50 + M), walks(3, l2, D, 60 + M)
    Y = Y3[np.arange(n2) % 3]
    got = ops.sig_gram(t(X), t(Y), M)
    for b in range(3, n2):
        assert torch.equal(got[:, :, b], got[:, :, b % 3]), b
    assert_levels(got[:, :, :3].cpu().numpy(), reference(M, "rbf").K_seq(X, Y3), "e matrix cores chunks", f"M={M}")


# ------------------------------------------------------------------------------------------ f. wide diagonal
@pytest.mark.parametrize("l,D,dtiles", [(2, 9, 1), (64, 9, 1), (65, 9, 1), (512, 9, 1), (513, 9, 0), (300, 8, 0)])
def test_wide_diagonal_tile_seams(l, D, dtiles):
    """diag_tiles_apply and diag_tiled: the RBF difference seed's diagonal past 8 channels in one column block."""
    from gpsig_amd import ops
    M, n = 4, 5
    W, LP, nblk = wide_geo(l, "rbf") if D > 8 else (8, 64, 1)
    assert_route(ops.fo_route(n, l, None, None, D, M, diag=True),
                 dict(path=1 if D > 8 else 0, W=W, LP=LP, nblk=nblk, dtiles=dtiles, pairs_per_chunk=n * dtiles,
                      launches=1), (l, D))
    X = walks(n, l, D, 11 * l + D)
    assert_levels(ops.sig_diag(t(X), M).cpu().numpy(), reference(M, "rbf").K_seq_diag(X), "f wide diagonal",
                  f"l={l} D={D}")
    # the other seeds' diagonals never take tiles
    assert ops.fo_route(n, l, None, None, D, M, "linear", diag=True)["dtiles"] == 0


@pytest.mark.parametrize("l,cp", [(300, 344), (297, 354), (512, 204)])
def test_wide_diagonal_second_chunk(l, cp):
    """n = pairs_per_chunk + 1: the second chunk of seed tiles holds one pair and starts at row cp, mid-workgroup of
    the 4-pair diagonal launch at l = 297 (cp = 354).  The sequences repeat three: every row equals its original's
    bit for bit, and the originals are compared with the oracle."""
    from gpsig_amd import ops
    D, M = 9, 4
    n = cp + 1
    assert_route(ops.fo_route(n, l, None, None, D, M, diag=True),
                 dict(path=1, W=8, LP=64, nblk=1, dtiles=1, pairs_per_chunk=cp, launches=2,
                      workgroups=(cp + 3) // 4 + 1), l)
    X3 = walks(3, l, D, l)
    X = X3[np.arange(n) % 3]
    got = ops.sig_diag(t(X), M)
    for a in range(3):
        assert torch.equal(got[:, a::3], got[:, a:a + 1].expand(-1, len(range(a, n, 3)))), a
    assert_levels(got[:, :3].cpu().numpy(), reference(M, "rbf").K_seq_diag(X3), "f wide diagonal chunks", f"l={l}")


# ------------------------------------------------------------------------------------------ g. fused epilogue
@pytest.mark.parametrize("name,L,D,M,want", [("ten-lane", 100, 5, 5, dict(path=0, W=10, LP=10)),
                                             ("channel-loop", 70, 225, 4, dict(path=1, W=8, LP=16)),
                                             ("matrix-cores", 70, 9, 4, dict(path=2, W=8, LP=16, nw=8))])
def test_fused_epilogue(name, L, D, M, want):
    """The class-level kernel with lengthscales and variances: normalised K(X), K(X, X2) with return_levels and Kdiag
    (the fused normalisation and scaling of the launch's epilogue) against SignatureKernelRef."""
    import gpsig_amd
    from gpsig_amd import ops
    n1, n2 = 5, 4
    assert_route(ops.fo_route(n1, L, None, None, D, M), want, "K(X)")
    assert_route(ops.fo_route(n1, L, n2, L, D, M), want, "K(X, X2)")
    rng = np.random.default_rng(L + D)
    ls = r32(0.8 + 0.4 * rng.random(D))
    var = r32(0.5 + rng.random(M + 1))
    X = walks(n1, L, D, 3 * L + D).reshape(n1, -1)
    X2 = walks(n2, L, D, 3 * L + D + 1).reshape(n2, -1)
    ref = kr.SignatureKernelRef(L * D, D, M, lengthscales=ls, variances=var)
    k = gpsig_amd.SignatureRBF(L * D, D, M, lengthscales=ls, variances=var)
    Xt, X2t = torch.as_tensor(X, device=DEV), torch.as_tensor(X2, device=DEV)
    group = "g epilogue " + name
    assert_levels(k.K(Xt, return_levels=True).cpu().numpy(), ref.K(X, return_levels=True), group, "K(X) levels")
    assert_levels(k.K(Xt)[None].cpu().numpy(), ref.K(X)[None], group, "K(X)")
    assert_levels(k.K(Xt, X2t, return_levels=True).cpu().numpy(), ref.K(X, X2, return_levels=True), group, "K(X, X2)")
    assert_levels(k.Kdiag(Xt, return_levels=True).cpu().numpy(), ref.Kdiag(X, return_levels=True), group, "Kdiag")
    ku = gpsig_amd.SignatureRBF(L * D, D, M, lengthscales=ls, variances=var, normalization=False)
    ru = kr.SignatureKernelRef(L * D, D, M, lengthscales=ls, variances=var, normalization=False)
    assert_levels(ku.Kdiag(Xt, return_levels=True).cpu().numpy(), ru.Kdiag(X, return_levels=True), group,
                  "Kdiag, unnormalised")
