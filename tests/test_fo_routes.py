"""CPU: the route table of the first-order fp32 Gram and diagonal (gpsig_sig_fo_route / ops.fo_route: host only, built
from the helpers gpsig_sig_gram's launch path calls) as literal values on both sides of every seam.  A retuned
fo_wmax, fo_geometry, mf_w, mf_geo, MF_LDS_MAX or MF_BLK_CHUNK moves a shape to another kernel instantiation and
fails here; tests/test_fo_routes_gpu.py then runs one case on each side with the route asserted first.

Every expected value follows from the helpers, not from the query's output:

fixed channels (D <= 8; csrc/sig_fo.h fo_wmax, fo_geometry, fo_blocks, fo_carry_bytes)
  DP = D up to 6, 8 for D = 7, 8.  fo_wmax(DP, M) = 8, except 4 at DP = 8 with M >= 7.  The geometry is the smallest
  LP of 16, 32, 64 and then the smallest W of 2, 4, .., fo_wmax with LP W >= l2: at fo_wmax 8 (2,16) up to 32 points,
  (4,16) to 64, (8,16) to 128, (8,32) to 256, (8,64) past it; at fo_wmax 4 (2,16), (4,16), (4,32) to 128, (4,64) past
  it.  The RBF difference seed with DP <= 5 and M <= 5 takes 10 lanes x 10 columns at 65..100 points.  Past LP W
  points the columns run in blocks of LP W - 1 cells, l2 - 1 cells with difference and l2 without, and a blocked
  launch keeps 4 waves x rows x (M - 1) floats of carries in LDS, rows = l1 - 1 with difference: 160 KiB at most.

wide channels (D >= 9; csrc/abi.hip gram_plan, csrc/sig_fo.h fo_geometry_wide)
  The channel loop runs (4,16) up to 64 points for the RBF difference seed, else (8,16) to 128, (8,32) to 256, (8,64)
  past it, blocked from 513 points.  The RBF and linear difference seeds in RECT and UPPER run the matrix-core Gram
  (csrc/sig_fo_mf.h) where mf_geo finds a geometry: LP = 16, W = mf_w(l2) = 4 to 64 points, 8 to 128, 10 to 160, 8 in
  blocks of 127 cells past it (mf_nblk = (l2 - 2) / 127 + 1); LDS = LPW (2 KH + 8) 2 B for the two-part B image
  (KH = D rounded up to 32) + nw 16 (LPW + 4) 4 B of tiles <= 160 KiB at nw = 8 waves, else at nw = 4, else the
  channel loop.  With LPW = 64: 256 KH + 1024 + 4352 nw, so KH <= 480 at nw = 8 and <= 544 at nw = 4; LPW = 128:
  512 KH + 2048 + 8448 nw, KH <= 160 and <= 224; LPW = 160: 640 KH + 2560 + 10496 nw, KH <= 96 and <= 160.
  xb = 4 nw x-sequences per workgroup against one y-sequence; carries of cw = 4 floats per row up to 5 levels, 8 past;
  a blocked launch goes out in chunks of MF_BLK_CHUNK = 256 workgroups whose carries (256 x xb x (l1 - 1) x 8
  floats) are a workspace region.

wide diagonal (csrc/abi.hip diag_tiled, csrc/wide.h diag_tile_pairs)
  The RBF difference seed's diagonal in one column block (l <= 512) runs on seed tiles of 2.5 RP NC floats per pair,
  RP = l - 1 rounded up to 8, NC = LP W of the channel loop, in chunks of 512 MiB of tiles: min(n, 2^29 / (10 RP NC)).
"""
import ctypes
import os

import pytest

SWITCHES = ("GPSIG_FO_FIXED_MAX", "GPSIG_WIDE_MF", "GPSIG_MF_PARTS", "GPSIG_MF_NW")
KIB160 = 160 * 1024


@pytest.fixture(autouse=True)
def default_switches():
    """The table is the default build's: the library reads the switches once per process, so a set one fails the
    module instead of moving its seams."""
    for v in SWITCHES:
        if v in os.environ:
            pytest.fail(f"{v} is set in the environment: the first-order route table is pinned for the defaults")


def geo(l2, d, M, base="rbf", difference=True, **kw):
    """(path, DP, W, LP, nblk, pairs_per_wave) of K(X, Y) with Y of l2 points."""
    from gpsig_amd import ops
    r = ops.fo_route(5, l2 + 3, 4, l2, d, M, base, difference, **kw)
    return tuple(r[k] for k in ("path", "DP", "W", "LP", "nblk", "pairs_per_wave"))


def modes(l, d, M, base="rbf", difference=True):
    """The same for K(X, Y), K(X) and the diagonal at one length."""
    from gpsig_amd import ops
    keys = ("path", "DP", "W", "LP", "nblk")
    return [tuple(r[k] for k in keys) for r in (ops.fo_route(5, l, 4, l, d, M, base, difference),
                                                ops.fo_route(5, l, None, None, d, M, base, difference),
                                                ops.fo_route(5, l, None, None, d, M, base, difference, diag=True))]


# fo_wmax = 8: (W, LP, nblk, pairs per wave) on the two sides of each seam
WMAX8 = {32: (2, 16, 1, 4), 33: (4, 16, 1, 4), 64: (4, 16, 1, 4), 65: (8, 16, 1, 4), 100: (8, 16, 1, 4),
         101: (8, 16, 1, 4), 128: (8, 16, 1, 4), 129: (8, 32, 1, 2), 256: (8, 32, 1, 2), 257: (8, 64, 1, 1),
         512: (8, 64, 1, 1), 513: (8, 64, 2, 1)}
# the 10-lane groups at 65..100 points (6 pairs per wave)
SEG = {**WMAX8, 65: (10, 10, 1, 6), 100: (10, 10, 1, 6)}
# fo_wmax = 4: (4,32) at 65..128, (4,64) past it, blocks of 255 cells from 257 points (256, 511 and 512 cells)
WMAX4 = {32: (2, 16, 1, 4), 33: (4, 16, 1, 4), 64: (4, 16, 1, 4), 65: (4, 32, 1, 2), 100: (4, 32, 1, 2),
         101: (4, 32, 1, 2), 128: (4, 32, 1, 2), 129: (4, 64, 1, 1), 256: (4, 64, 1, 1), 257: (4, 64, 2, 1),
         512: (4, 64, 3, 1), 513: (4, 64, 3, 1)}


@pytest.mark.parametrize("d,M,DP,table", [(5, 5, 5, SEG), (6, 5, 6, WMAX8), (5, 6, 5, WMAX8), (7, 6, 8, WMAX8),
                                          (8, 7, 8, WMAX4)], ids=["D5M5", "D6M5", "D5M6", "D7M6", "D8M7"])
def test_fixed_geometry_seams(d, M, DP, table):
    for l2, want in table.items():
        assert geo(l2, d, M) == (0, DP) + want, (l2, d, M)
        # K(X) and the diagonal take the geometry of their own length (one pair per wave on the diagonal)
        assert modes(l2, d, M) == [(0, DP) + want[:3]] * 3, (l2, d, M)


def test_ten_lane_groups_are_the_rbf_difference_seeds():
    """fo_seg_ok: RBF with difference, DP <= 5, M <= 5; every other seed takes (8,16) at 65..100 points."""
    from gpsig_amd import ops
    for base, diff in (("linear", True), ("rbf", False), ("linear", False), ("matern32", True), ("matern12", False)):
        for l2 in (65, 100):
            assert geo(l2, 5, 5, base, diff) == (0, 5, 8, 16, 1, 4), (base, diff, l2)
    assert geo(100, 1, 1) == (0, 1, 10, 10, 1, 6)
    assert ops.fo_route(7, 100, None, None, 5, 5, diag=True)["pairs_per_wave"] == 1
    assert ops.fo_route(7, 100, None, None, 5, 5, state=True)["LP"] == 10  # the saved-state launch: the same geometry


@pytest.mark.parametrize("base,difference", [("linear", True), ("rbf", False), ("linear", False), ("matern32", True),
                                             ("matern32", False)])
def test_other_seeds_fixed_geometry(base, difference):
    """D = 3, M = 4: the fo_wmax = 8 table; a point seed's 513 columns are 513 cells, two blocks as well."""
    for l2, want in WMAX8.items():
        assert geo(l2, 3, 4, base, difference) == (0, 3) + want, (base, difference, l2)


def test_block_count_seams():
    """Blocks of LP W - 1 = 511 cells (255 at W = 4): l2 - 1 cells with difference, l2 without."""
    for base in ("rbf", "linear", "matern12"):
        assert [geo(l2, 2, 3, base)[2:5] for l2 in (1023, 1024)] == [(8, 64, 2), (8, 64, 3)], base
        assert [geo(l2, 2, 3, base, False)[2:5] for l2 in (512, 513, 1022, 1023)] == \
            [(8, 64, 1), (8, 64, 2), (8, 64, 2), (8, 64, 3)], base
    assert [geo(l2, 8, 7)[2:5] for l2 in (511, 512)] == [(4, 64, 2), (4, 64, 3)]
    # the channel loop's blocks are the same 511 cells
    assert [geo(l2, 9, 3, "matern12")[2:5] for l2 in (512, 513, 1023, 1024)] == \
        [(8, 64, 1), (8, 64, 2), (8, 64, 2), (8, 64, 3)]


def test_carry_cap():
    """fo_carry_bytes = 4 waves x rows x (M - 1) x 4 B in a blocked launch, 160 KiB at most: at M = 8 with difference
    4 x 1462 x 7 x 4 = 163744 B fit and 4 x 1463 x 7 x 4 = 163856 B do not; the code is the call's, with the size."""
    import gpsig_amd
    import gpsig_amd._lib as L
    from gpsig_amd import ops
    assert 4 * 1462 * 7 * 4 <= KIB160 < 4 * 1463 * 7 * 4
    r = ops.fo_route(5, 1463, 4, 513, 2, 8)
    assert (r["nblk"], r["carry_bytes"], r["launches"]) == (2, 163744, 1)
    out = (ctypes.c_int * 15)()
    rc = L.load().gpsig_sig_fo_route(5, 1464, 4, 513, 2, 8, L.BASE_RBF, 1, L.PAIRS_RECT, 0, 5, 0, out)
    assert rc == L.GPSIG_EUNSUPPORTED and out[5] == 163856 and out[4] == 2 and out[14] == 0
    with pytest.raises(gpsig_amd.GpsigError):
        ops.fo_route(5, 1464, 4, 513, 2, 8)
    # no carries in one block, whatever the rows; a point seed carries l1 rows: 1462 fit, 1463 do not
    assert ops.fo_route(5, 5000, 4, 512, 2, 8)["carry_bytes"] == 0
    assert ops.fo_route(5, 1462, 4, 513, 2, 8, difference=False)["carry_bytes"] == 163744
    with pytest.raises(gpsig_amd.GpsigError):
        ops.fo_route(5, 1463, 4, 513, 2, 8, difference=False)
    # the channel loop's blocked launch keeps the same carries
    assert ops.fo_route(5, 1463, 4, 513, 9, 8, "matern12")["carry_bytes"] == 163744
    with pytest.raises(gpsig_amd.GpsigError):
        ops.fo_route(5, 1464, 4, 513, 9, 8, "matern12")
    assert ops.fo_route(5, 1464, 4, 513, 9, 8, "matern12", rows=(2, 2))["launches"] == 0


def test_path_by_channels_seed_and_mode():
    """0 up to 8 channels; past 8 the matrix cores for the RBF / linear difference seeds in RECT and UPPER, the
    channel loop for the diagonal, the point seeds and the Matern seeds."""
    from gpsig_amd import ops
    for base in ("rbf", "linear"):
        assert [m[0] for m in modes(40, 8, 4, base)] == [0, 0, 0]
        assert [m[0] for m in modes(40, 9, 4, base)] == [2, 2, 1]
        assert [m[0] for m in modes(40, 9, 4, base, False)] == [1, 1, 1]
    assert [m[0] for m in modes(40, 8, 4, "matern52")] == [0, 0, 0]
    for base in ("matern12", "matern32", "matern52"):
        for diff in (True, False):
            assert [m[0] for m in modes(40, 9, 4, base, diff)] == [1, 1, 1]
    # the channel loop's geometry: (4,16) to 64 points for the RBF difference seed only, then 8 columns per lane
    assert [geo(l2, 9, 4, "rbf", diag=False)[1:5] for l2 in (64, 65)] == [(0, 4, 16, 1), (0, 8, 16, 1)]  # matrix cores
    for l2, want in {64: (4, 16, 1), 65: (8, 16, 1), 128: (8, 16, 1), 129: (8, 32, 1), 256: (8, 32, 1), 257: (8, 64, 1),
                     512: (8, 64, 1), 513: (8, 64, 2)}.items():
        r = ops.fo_route(5, l2, None, None, 9, 4, diag=True)
        assert (r["path"], r["DP"], r["W"], r["LP"], r["nblk"]) == (1, 0) + want, l2
        want_other = (8, 16, 1) if l2 <= 64 else want
        for base, diff in (("linear", True), ("rbf", False), ("matern32", True)):
            r = ops.fo_route(5, l2, None, None, 9, 4, base, diff, diag=True)
            assert (r["path"], r["DP"], r["W"], r["LP"], r["nblk"]) == (1, 0) + want_other, (base, diff, l2)
        assert ops.fo_route(5, l2, None, None, 9, 4, "matern12")["pairs_per_wave"] == 64 // want_other[1]


def mf(l2, d, M=4, base="rbf", n1=5, n2=4, **kw):
    from gpsig_amd import ops
    r = ops.fo_route(n1, l2 + 3, n2, l2, d, M, base, **kw)
    return tuple(r[k] for k in ("path", "W", "LP", "nblk", "nw", "xb", "np", "cw"))


def test_matrix_core_geometry_seams():
    for base in ("rbf", "linear"):
        # mf_w / mf_nblk by length, at 9 channels (8 waves everywhere)
        for l2, (W, nblk) in {64: (4, 1), 65: (8, 1), 128: (8, 1), 129: (10, 1), 160: (10, 1), 161: (8, 2),
                              255: (8, 2), 256: (8, 3)}.items():
            assert mf(l2, 9, 4, base) == (2, W, 16, nblk, 8, 32, 2, 4), (base, l2)
        # carry rows of 4 floats up to 5 levels, 8 past
        assert [mf(161, 9, M, base)[-1] for M in (1, 5, 6, 8)] == [4, 4, 8, 8]
        # waves by LDS: 8 | 4 | the channel loop
        for l2, (d8, d4) in {20: (480, 544), 64: (480, 544), 65: (160, 224), 128: (160, 224), 129: (96, 160),
                             160: (96, 160), 161: (160, 224), 300: (160, 224)}.items():
            assert mf(l2, d8, 4, base)[4:6] == (8, 32), (base, l2)
            assert mf(l2, d8 + 1, 4, base)[4:6] == (4, 16), (base, l2)
            assert mf(l2, d4, 4, base)[4:6] == (4, 16), (base, l2)
            assert mf(l2, d4 + 1, 4, base)[0] == 1 and mf(l2, d4 + 1, 4, base)[4:] == (0, 0, 0, 0), (base, l2)
    # the channel loop behind the LDS bound, difference seeds in RECT / UPPER
    assert geo(20, 545, 3) == (1, 0, 4, 16, 1, 4)
    assert geo(20, 545, 3, "linear") == (1, 0, 8, 16, 1, 4)
    assert geo(70, 225, 3) == geo(70, 225, 3, "linear") == (1, 0, 8, 16, 1, 4)
    assert geo(140, 161, 3) == (1, 0, 8, 32, 1, 2)
    assert geo(300, 225, 3) == (1, 0, 8, 64, 1, 1)
    assert geo(520, 225, 3) == (1, 0, 8, 64, 2, 1)
    assert geo(70, 225, 3, state=True) == (1, 0, 8, 16, 1, 4)
    assert mf(70, 224, 3, state=True)[0] == 2


def test_matrix_core_tiles_and_launches():
    """One workgroup per (tile row of xb x-sequences, y-sequence): RECT ceil(rows / xb) n2; UPPER tile row r holds
    the y-sequences from xb r on, P(r) = r n - xb r (r - 1) / 2 before it; a row window runs the tile rows it touches."""
    from gpsig_amd import ops

    def wl(n1, n2, l, d, **kw):
        r = ops.fo_route(n1, l if n2 is None else l + 3, n2, None if n2 is None else l, d, 3, **kw)
        return r["workgroups"], r["launches"]
    for n, want in {31: 31, 32: 32, 33: 33 + 1, 65: 65 + 33 + 1}.items():   # xb = 32
        assert wl(n, None, 20, 9) == (want, 1), n
        assert wl(n, 3, 20, 9) == (3 * ((n + 31) // 32), 1), n
    for n, want in {15: 15, 16: 16, 17: 17 + 1, 33: 33 + 17 + 1}.items():   # four waves: xb = 16
        assert wl(n, None, 130, 97) == (want, 1), n
        assert wl(n, 3, 130, 97) == (3 * ((n + 15) // 16), 1), n
    # UPPER windows of K(X), n = 65: tile rows 0 | 0, 1 | 1, 2 | 1
    assert [wl(65, None, 20, 9, rows=w)[0] for w in ((9, 21), (30, 34), (32, 65), (33, 34), (7, 7))] == \
        [65, 65 + 33, 33 + 1, 33, 0]
    assert wl(65, None, 20, 9, rows=(7, 7)) == (0, 0)
    # column blocks: chunks of 256 workgroups; the carries of one chunk in the workspace, 256 xb (l1 - 1) 8 floats
    assert wl(3, 256, 161, 9) == (256, 1)
    assert wl(3, 257, 161, 9) == (257, 2)
    assert wl(33, 256, 161, 9) == (512, 2)
    assert wl(3, 257, 160, 9) == (257, 1)     # 160 points: one block, one launch
    assert ops.fo_route(3, 164, 257, 161, 9, 3)["carry_bytes"] == 256 * 32 * 163 * 8 * 4
    assert ops.fo_route(3, 164, 257, 161, 161, 3)["carry_bytes"] == 256 * 16 * 163 * 8 * 4
    assert ops.fo_route(3, 163, 257, 160, 9, 3)["carry_bytes"] == 0


def test_fixed_tiles():
    """Fixed paths and channel loop: 4 x-sequences (one per wave) against G = 64 / LP y-sequences per workgroup, the
    diagonal 4 pairs per workgroup."""
    from gpsig_amd import ops

    def wg(n1, n2, l, **kw):
        r = ops.fo_route(n1, l, n2, l, 3, 3, **kw)
        return r["workgroups"], r["launches"]
    assert ops.fo_route(5, 200, None, None, 3, 3)["pairs_per_wave"] == 2      # (8,32)
    assert ops.fo_route(5, 300, None, None, 3, 3)["pairs_per_wave"] == 1      # (8,64)
    for l, G in ((200, 2), (300, 1)):
        for n in (1, 4 * G - 1, 4 * G, 4 * G + 1, 3 * 4 * G + 2):
            ta, tb = (n + 3) // 4, (n + G - 1) // G
            assert wg(n, n, l) == (ta * tb, 1), (l, n)
            assert wg(n, None, l, diag=True) == (ta, 1), (l, n)
            # UPPER: tile row r starts at y tile floor(4 r / G)
            assert wg(n, None, l) == (sum(tb - 4 * r // G for r in range(ta)), 1), (l, n)
        assert wg(9, 9, l, rows=(5, 6)) == ((9 + G - 1) // G, 1)
        assert wg(9, 9, l, rows=(3, 5)) == (2 * ((9 + G - 1) // G), 1)
        assert wg(9, 9, l, rows=(4, 4)) == (0, 0)


def test_wide_diagonal_tiles():
    """Seed tiles for the RBF difference seed's diagonal past 8 channels, up to 512 points (one column block of the
    channel loop), not for the other seeds, K(X), or the fixed channels; pairs per chunk 2^29 / (10 RP NC)."""
    from gpsig_amd import ops

    def dt(n, l, d=9, base="rbf", difference=True, **kw):
        r = ops.fo_route(n, l, None, None, d, 3, base, difference, diag=True, **kw)
        return r["dtiles"], r["pairs_per_chunk"], r["workgroups"], r["launches"]
    assert dt(5, 512) == (1, 5, 2, 1)
    assert dt(5, 513) == (0, 0, 2, 1)
    assert dt(5, 512, d=8) == (0, 0, 2, 1)
    assert dt(5, 2) == (1, 5, 2, 1)
    for base, diff in (("linear", True), ("rbf", False), ("matern12", True)):
        assert dt(5, 300, base=base, difference=diff)[:2] == (0, 0)
    assert ops.fo_route(5, 300, None, None, 9, 3)["dtiles"] == 0
    # RP = 304, NC = 512: 2^29 / (10 x 304 x 512) = 344.9; RP = 296: 354.2; RP = NC = 512: 204.8
    assert (1 << 29) // (10 * 304 * 512) == 344 and (1 << 29) // (10 * 296 * 512) == 354
    assert (1 << 29) // (10 * 512 * 512) == 204
    assert dt(344, 300) == (1, 344, 86, 1)
    assert dt(345, 300) == (1, 344, 86 + 1, 2)
    assert dt(355, 297) == (1, 354, 89 + 1, 2)       # 354 = 4 x 88 + 2: the second chunk starts mid-workgroup
    assert dt(205, 512) == (1, 204, 51 + 1, 2)
    assert dt(355, 297, rows=(353, 355)) == (1, 354, 1, 1)       # chunks count from the window's first row
    assert dt(355, 297, rows=(9, 9)) == (1, 354, 0, 0)
    # short sequences: 65535 pairs at most (the anchor launch's grid)
    assert (1 << 29) // (10 * 8 * 64) > 65535
    assert dt(70000, 9)[1:] == (65535, (65535 + 3) // 4 + (70000 - 65535 + 3) // 4, 2)
