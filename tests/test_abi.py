"""CPU: the C-ABI library loads, exports every symbol include/gpsig_amd.h declares, and validates
arguments without touching a GPU."""
import ctypes
import os
import re

import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "gpsig_amd.h")


def header_symbols():
    txt = open(HEADER).read()
    return sorted(set(re.findall(r"\b(gpsig_[a-z_]+)\s*\(", txt)))


def test_header_declares_expected_entry_points():
    syms = header_symbols()
    for s in ["gpsig_sig_gram", "gpsig_sig_diag", "gpsig_pde_gram", "gpsig_pde_diag", "gpsig_pde_route",
              "gpsig_sig_ho_route", "gpsig_sig_fo_route", "gpsig_tens_vs_seq",
              "gpsig_tens_gram", "gpsig_rescaled", "gpsig_sym_assemble", "gpsig_version"]:
        assert s in syms, s


def test_library_exports_every_header_symbol():
    import gpsig_amd._lib as L
    lib = L.load()
    for s in header_symbols():
        assert hasattr(lib, s), s
    assert b"gfx950" in lib.gpsig_version()


def test_python_signatures_cover_header():
    import gpsig_amd._lib as L
    assert set(header_symbols()) <= set(L.SIGNATURES)


def test_argument_validation_without_gpu():
    import gpsig_amd._lib as L
    lib = L.load()
    # null pointers / bad shapes are rejected before any HIP call
    rc = lib.gpsig_sig_gram(None, 4, 10, None, 4, 10, 3, 4, 1, 0, 1, 0, 0, 4, None, None, None, 0.0, 0,
                            None, 0, 4, None, 0, None)
    assert rc == L.GPSIG_EINVAL
    rc = lib.gpsig_pde_gram(None, 4, 10, None, 4, 10, 3, 9, 1, 0, 0, 4, None, 0, 4, None)
    assert rc == L.GPSIG_EINVAL
    assert lib.gpsig_sig_workspace_bytes(10, 20, 10, 20, 5) > 0


def test_library_binary_targets_gfx950():
    import gpsig_amd._lib as L
    data = open(L.LIB_PATH, "rb").read()
    assert b"gfx950" in data


def test_product_path_refuses_cpu_tensors():
    import torch
    import gpsig_amd
    from gpsig_amd import ops
    X = torch.zeros(2, 5, 3)
    with pytest.raises(gpsig_amd.GpsigError):
        ops.sig_diag(X, 3)


def test_vjp_and_feature_entry_points_validate_arguments():
    """The gradient / signature entry points reject null pointers and bad shapes before any HIP call."""
    import gpsig_amd._lib as L
    lib = L.load()
    assert lib.gpsig_sig_gram_vjp(None, 4, 10, None, 4, 10, 3, 4, 0, 1, 0, 0, 4, None, 0, None, None, None, 0.0,
                                  None, None, None, None, None, None, None, 0, None) == L.GPSIG_EINVAL
    assert lib.gpsig_sig_gram_state(None, 4, 10, None, 4, 10, 3, 4, 0, 0, 0, 4, None, None, None, 0.0, 0, None,
                                    0, 4, None, 0, None, 0, None) == L.GPSIG_EINVAL
    # saved VJP state: (M-1)(l2-1) + M floats per pair; upper triangle for K(X); DIAG has none
    assert lib.gpsig_sig_state_bytes(4, 6, 10, 5, L.PAIRS_RECT) == 4 * 6 * (4 * 9 + 5) * 4
    assert lib.gpsig_sig_state_bytes(6, 6, 10, 5, L.PAIRS_UPPER) == 21 * (4 * 9 + 5) * 4
    assert lib.gpsig_sig_state_bytes(6, 6, 10, 5, L.PAIRS_DIAG) == 0
    assert lib.gpsig_tens_vs_seq_vjp(None, 6, 2, 0, 3, None, 4, 10, 3, 0, 1, None, None, None, None, None, 0,
                                     None) == L.GPSIG_EINVAL
    assert lib.gpsig_tens_vs_seq_state(None, 6, 2, 0, 3, None, 4, 10, 3, 0, None, None, None, 0,
                                       None) == L.GPSIG_EINVAL
    assert lib.gpsig_tens_gram_vjp(None, 6, 2, 0, 3, 3, 0, None, None, None, 0, None) == L.GPSIG_EINVAL
    # the pair-tile + GEMM path past 32 channels: m (LT T^2), kv (4 LT T^2), [Z_h | 1] and G (LT 2 T (d + 1))
    assert lib.gpsig_tens_gram_vjp_workspace_bytes(10, 64, 1, 3, 4, L.BASE_RBF) == 0
    assert lib.gpsig_tens_gram_vjp_workspace_bytes(10, 64, 1, 46, 4, L.BASE_RBF) == \
        (10 * 64 * 64 + 40 * 64 * 64 + 2 * 20 * 64 * 47) * 4
    assert lib.gpsig_pde_vjp(None, 4, 10, None, 4, 10, 3, 0, 1, 0, 0, 4, None, None, None, None, 0,
                             None) == L.GPSIG_EINVAL
    assert lib.gpsig_signature(None, 4, 10, 3, 3, None, None) == L.GPSIG_EINVAL
    assert lib.gpsig_signature_vjp(None, 4, 10, 3, 3, None, None, None) == L.GPSIG_EINVAL
    assert lib.gpsig_signature_channels(5, 3) == 5 + 25 + 125
    # past the 160 KiB of LDS the levels take per-path workspace slabs (256-byte aligned, <= 1 GiB per launch)
    assert lib.gpsig_signature_workspace_bytes(4, 5, 5, 0) == 0 and lib.gpsig_signature_workspace_bytes(4, 5, 5, 1) == 0
    tot = lib.gpsig_signature_channels(6, 6)  # 55 986 coordinates
    assert lib.gpsig_signature_workspace_bytes(4, 6, 6, 0) == 4 * ((tot + 6 + 63) // 64 * 64) * 4
    assert lib.gpsig_signature_workspace_bytes(4, 6, 6, 1) == 4 * ((4 * tot + 12 + 63) // 64 * 64) * 4
    fake = ctypes.c_void_p(256)  # never dereferenced: the workspace check comes before any launch
    assert lib.gpsig_signature(fake, 4, 10, 6, 6, fake, None) == L.GPSIG_EWORKSPACE
    assert lib.gpsig_signature_vjp(fake, 4, 10, 6, 6, fake, fake, None) == L.GPSIG_EWORKSPACE
    # J = 18 fine columns at dyadic 1: W = 2 per lane, U = 9 lanes, 9 + 9 - 1 = 17 coarse steps, a front every
    # 32 / (2 * 2) = 8 steps -> 3 fronts of (W + REP) x 64 floats per pair
    assert lib.gpsig_pde_vjp_workspace_bytes(2, 10, 10, 1) == 2 * 3 * (2 + 2) * 64 * 4
    # J = 1099 > 64 x 16: two column blocks of 1024 (W = 16, H = 2, 36 fronts each) + fp64 boundary columns
    assert lib.gpsig_pde_vjp_workspace_bytes(2, 10, 1100, 0) == 2 * (2 * 36 * 17 * 64 + 2 * 2 * 10) * 4
    # dyadic > 3: the order-3 layout of the grid whose cells are split 2^(dyadic-3) (tile sub-refinement)
    assert lib.gpsig_pde_vjp_workspace_bytes(2, 10, 10, 4) == lib.gpsig_pde_vjp_workspace_bytes(2, 19, 19, 3)
    assert lib.gpsig_pde_vjp_workspace_bytes(2, 10, 10, 7) == lib.gpsig_pde_vjp_workspace_bytes(2, 145, 145, 3)
    assert lib.gpsig_pde_vjp_workspace_bytes(2, 10, 10, 9) == 0


@pytest.mark.skipif("GPSIG_PDE_LP" in os.environ, reason="GPSIG_PDE_LP pins the lane group the query reports")
def test_pde_route_query_without_gpu():
    """gpsig_pde_route is host only: the launch path's choices for a shape, no device touched."""
    import gpsig_amd._lib as L
    from gpsig_amd import ops
    lib = L.load()
    out = (ctypes.c_int * 9)()
    assert lib.gpsig_pde_route(1, 9, 3, 0, 1, 0, 0, out) == L.GPSIG_EINVAL       # l1 < 2
    assert lib.gpsig_pde_route(9, 9, 3, 9, 1, 0, 0, out) == L.GPSIG_EINVAL       # dyadic > 8
    assert lib.gpsig_pde_route(9, 9, 3, 0, 1, 1, 1, out) == L.GPSIG_EINVAL       # the adjoint has no UPPER mode
    assert lib.gpsig_pde_route(9, 9, 3, 0, 1, 0, 0, None) == L.GPSIG_EINVAL
    # solver-1 Gram pairs, d <= 8: lane groups; 128 columns fill (16, 8), one more goes to (16, 14)
    assert ops.pde_route(9, 129, 3, 0, 1, L.PAIRS_RECT) == dict(family="lane_group", DP=3, REP=1, W=8, LP=16, nblk=1, sub=0)
    assert ops.pde_route(9, 130, 3, 0, 1, L.PAIRS_RECT)["W"] == 14
    # k(x, x), solver 0, d > 8: one pair per wave; W = 3 REP at 129 .. 192 coarse columns, blocks past 256
    assert ops.pde_route(9, 194, 3, 1, 1, L.PAIRS_DIAG) == dict(family="pair", DP=3, REP=2, W=8, LP=64, nblk=1, sub=0)
    assert ops.pde_route(9, 193, 12, 1, 0, L.PAIRS_RECT) == dict(family="pair", DP=16, REP=2, W=6, LP=64, nblk=1, sub=0)
    assert ops.pde_route(9, 258, 12, 2, 1, L.PAIRS_RECT)["nblk"] == 2
    assert ops.pde_route(9, 66, 5, 3, 1, L.PAIRS_RECT) == dict(family="pair", DP=5, REP=8, W=16, LP=64, nblk=1, sub=0)
    # increment tiles: d > 16, or dyadic > 4 with the tile cells split 2^sub ways
    assert ops.pde_route(9, 9, 17, 0, 1, L.PAIRS_UPPER) == dict(family="tile", DP=0, REP=1, W=1, LP=64, nblk=1, sub=0)
    assert ops.pde_route(9, 9, 3, 6, 1, L.PAIRS_RECT) == dict(family="tile", DP=0, REP=16, W=16, LP=64, nblk=1, sub=2)
    # adjoint: W, H, blocks as gpsig_pde_vjp_workspace_bytes' layouts above; tiles past d = 16 and dyadic 3
    assert ops.pde_route(10, 10, 3, 1, 1, L.PAIRS_RECT, True) == dict(tiled=0, DP=3, REP=2, W=2, H=8, nblk=1, sub=0, wpb=4,
                                                                      wpb_fronts=4)
    assert ops.pde_route(10, 1100, 3, 0, 1, L.PAIRS_DIAG, True) == dict(tiled=0, DP=3, REP=1, W=16, H=2, nblk=2, sub=0,
                                                                        wpb=4, wpb_fronts=4)
    assert ops.pde_route(10, 10, 3, 4, 1, L.PAIRS_RECT, True) == dict(tiled=1, DP=0, REP=8, W=8, H=1, nblk=1, sub=1, wpb=4,
                                                                      wpb_fronts=4)
    # long x at DP 16: the per-wave LDS leaves 2 pairs, then 1 pair per workgroup
    assert ops.pde_route(200, 7, 16, 0, 1, L.PAIRS_RECT, True)["wpb"] == 2
    assert ops.pde_route(200, 7, 16, 0, 1, L.PAIRS_RECT, True)["wpb_fronts"] == 4
    assert ops.pde_route(450, 7, 16, 0, 1, L.PAIRS_RECT, True)["wpb"] == 1


@pytest.mark.skipif("GPSIG_HO_SPLIT" in os.environ, reason="GPSIG_HO_SPLIT pins the kernel form the query reports")
def test_sig_ho_route_query_without_gpu(monkeypatch):
    """gpsig_sig_ho_route is host only: what gpsig_sig_gram / gpsig_sig_diag at order >= 2 would run for a shape."""
    import gpsig_amd
    import gpsig_amd._lib as L
    from gpsig_amd import ops
    lib = L.load()
    out = (ctypes.c_int * 7)()

    def rc(n1=4, l1=45, n2=2, l2=40, d=3, M=4, order=3, base=L.BASE_RBF, diff=1, pm=L.PAIRS_RECT, r0=0, r1=4, o=out):
        return lib.gpsig_sig_ho_route(n1, l1, n2, l2, d, M, order, base, diff, pm, r0, r1, o)
    assert rc() == L.GPSIG_OK
    assert rc(o=None) == L.GPSIG_EINVAL
    assert rc(l2=1) == L.GPSIG_EINVAL                       # difference needs two points
    assert rc(order=1) == L.GPSIG_EINVAL                    # the first-order kernels are not this query's
    assert rc(r1=5) == L.GPSIG_EINVAL                       # row window past n1
    assert rc(pm=L.PAIRS_UPPER) == L.GPSIG_EINVAL           # UPPER pairs X with itself: equal shapes
    assert rc(pm=3) == L.GPSIG_EINVAL
    assert rc(diff=0) == L.GPSIG_EUNSUPPORTED               # the higher-order seeds are the difference seeds
    assert rc(M=9, order=9) == L.GPSIG_EUNSUPPORTED
    assert rc(d=33, base=L.BASE_MATERN32) == L.GPSIG_EUNSUPPORTED  # tile cells: linear and RBF only
    assert rc(base=L.BASE_RBF | L.BASE_SEED_MFMA) == L.GPSIG_EUNSUPPORTED

    def route(n1, l1, n2, l2, d, M, order, base="rbf", **kw):
        r = ops.ho_route(n1, l1, n2, l2, d, M, order, base, **kw)
        return tuple(r[k] for k in ("tiled", "DP", "W", "nblk", "split", "carry_bytes", "features"))
    # W: the fewest columns per lane that cover l2, up to 4 (order <= 4), 2 (order 5), 1 (orders 6..8)
    assert route(4, 45, 2, 40, 3, 8, 8) == (0, 4, 1, 1, 0, 0, False)
    assert route(4, 70, 2, 65, 3, 8, 8) == (0, 4, 1, 2, 1, 0, False)       # blocks of 63 cells from 65 points
    assert route(4, 133, 2, 128, 3, 5, 3, "linear") == (0, 4, 2, 1, 0, 0, False)
    assert route(4, 262, 2, 257, 3, 5, 4) == (0, 4, 4, 2, 1, 0, False)     # 255 cells + a last block of one
    assert route(4, 261, 2, 256, 7, 5, 5, "linear") == (0, 8, 2, 3, 1, 0, False)  # 19607 coordinates: recursion
    # five blocks are past SPLIT: the plain kernel, 4 waves x 258 rows x (2 + 3 + 4 + 5 + 6) scans x 4 B of carries
    assert route(3, 259, 2, 254, 3, 6, 6) == (0, 4, 1, 5, 0, 4 * 258 * 20 * 4, False)
    # SPLIT up to 2048 workgroups: 12 row groups x 42 sequences x 4, not x 43; GPSIG_HO_SPLIT=0 keeps the plain kernel
    assert route(48, 68, 42, 65, 2, 6, 6) == (0, 4, 1, 2, 1, 0, False)
    assert route(48, 68, 43, 65, 2, 6, 6) == (0, 4, 1, 2, 0, 4 * 67 * 20 * 4, False)
    monkeypatch.setenv("GPSIG_HO_SPLIT", "0")
    assert route(4, 70, 2, 65, 3, 8, 8) == (0, 4, 1, 2, 0, 4 * 69 * 35 * 4, False)
    monkeypatch.delenv("GPSIG_HO_SPLIT")
    # channel paddings 4 / 8 / 16 / 32, increment tiles from 33
    assert [route(4, 45, 2, 40, d, 4, 3)[:2] for d in (4, 5, 8, 9, 16, 17, 32, 33)] == \
        [(0, 4), (0, 8), (0, 8), (0, 16), (0, 16), (0, 32), (0, 32), (1, 0)]
    assert ops.ho_route(13, 30, None, None, 40, 4, 2, "linear", rows=(3, 11))["launches"] == 1
    assert ops.ho_route(13, 30, None, None, 40, 4, 2, "linear", rows=(3, 3))["launches"] == 0
    # the carries' 160 KiB: 4 x 292 x 35 x 4 = 163520 B fit, one more row does not
    assert route(3, 293, 2, 254, 2, 8, 8)[3:6] == (5, 0, 163520)
    assert rc(n1=3, l1=294, l2=254, d=2, M=8, order=8, r1=3) == L.GPSIG_EUNSUPPORTED and out[5] == 4 * 293 * 35 * 4
    with pytest.raises(gpsig_amd.GpsigError):
        ops.ho_route(3, 294, 2, 254, 2, 8, 8)
    # linear, order >= num_levels, at most 16000 signature coordinates: Python computes signature features
    assert route(4, 74, 2, 70, 3, 8, 8, "linear") == (0, 4, 1, 2, 1, 0, True)
    assert route(4, 45, 2, 40, 4, 8, 8, "linear")[-1] is False             # 87380 coordinates
    monkeypatch.setattr(ops, "SIG_FEATURE_MAX", 0)
    assert route(4, 74, 2, 70, 3, 8, 8, "linear")[-1] is False


def test_sig_fo_route_argument_checks_without_gpu():
    """gpsig_sig_fo_route is host only and returns what gpsig_sig_gram / gpsig_sig_diag / gpsig_sig_gram_state return
    for the same arguments (the route table itself: tests/test_fo_routes.py)."""
    import gpsig_amd._lib as L
    lib = L.load()
    out = (ctypes.c_int * 15)()

    def rc(n1=4, l1=45, n2=2, l2=40, d=3, M=4, base=L.BASE_RBF, diff=1, pm=L.PAIRS_RECT, r0=0, r1=4, state=0, o=out):
        return lib.gpsig_sig_fo_route(n1, l1, n2, l2, d, M, base, diff, pm, r0, r1, state, o)
    assert rc() == L.GPSIG_OK and out[13] == 1 and out[14] == 1   # one workgroup: 4 x-sequences x 4 pairs per wave
    assert rc(o=None) == L.GPSIG_EINVAL
    assert rc(M=0) == L.GPSIG_EINVAL
    assert rc(l2=1) == L.GPSIG_EINVAL                       # difference needs two points
    assert rc(l2=1, diff=0) == L.GPSIG_OK                   # the point seeds take one
    assert rc(d=0) == L.GPSIG_EINVAL
    assert rc(r1=5) == L.GPSIG_EINVAL                       # row window past n1
    assert rc(r0=3, r1=2) == L.GPSIG_EINVAL
    assert rc(pm=L.PAIRS_UPPER) == L.GPSIG_EINVAL           # UPPER pairs X with itself: equal shapes
    assert rc(pm=3) == L.GPSIG_EINVAL
    assert rc(state=1, diff=0) == L.GPSIG_EINVAL            # gpsig_sig_gram_state: difference seeds, RECT / UPPER
    assert rc(n2=4, l2=45, pm=L.PAIRS_DIAG, state=1) == L.GPSIG_EINVAL
    assert rc(state=1) == L.GPSIG_OK
    assert rc(base=7) == L.GPSIG_EUNSUPPORTED
    assert rc(M=9) == L.GPSIG_EUNSUPPORTED
    assert rc(M=9, r1=0) == L.GPSIG_OK                      # no rows: the call returns before it meets the level count
    assert rc(base=L.BASE_MATERN32, state=1) == L.GPSIG_EUNSUPPORTED
    assert rc(base=L.BASE_RBF | L.BASE_SEED_MFMA) == L.GPSIG_EUNSUPPORTED
    assert rc(base=L.BASE_RBF | L.GRAM_SPLIT) == L.GPSIG_EUNSUPPORTED


def _ho_vjp_slots(o, M):
    """include/gpsig_amd.h: column sums d_k of levels 1..M plus multipliers d_k^2 of levels 2..M, d_k = min(k, o)."""
    return sum(min(k, o) + (min(k, o) ** 2 if k >= 2 else 0) for k in range(1, M + 1))


def _ho_vjp_expected(l2, o, M, split_on):
    """The route table from the rules of include/gpsig_amd.h (gpsig_sig_vjp_ho_route), not from the library:
    (kernel, W, waves, slots, variant, lds_bytes, slab_bytes of one call), or None where nothing covers the shape."""
    budget = 160 * 1024
    slots = _ho_vjp_slots(o, M)

    def cbuf(W):
        return 4 * 64 * 2 * W * 4

    def lds_ok(W):
        return o <= 6 and slots * 64 * W * 4 + cbuf(W) <= budget

    def lds(W):
        variant = 2 if (W == 8 or slots > 100) else (1 if slots > 60 else 0)
        return ("LDS", W, 1, slots, variant, slots * 64 * W * 4, 0)
    split8_ok = (o == 2 and M <= 7) or (o == 3 and M <= 6) or (o in (4, 5) and M <= 5)
    if l2 < 2 or M > 8:
        return None
    if 510 <= l2 <= 1017 and split8_ok:
        return ("SPLIT8", 2, 8, slots, 0, 0, 1024 * 8 * slots * 64 * 2 * 4)
    if l2 > 512:
        return None
    if l2 <= 256:
        if o == 2 or (o == 3 and M <= 5):
            np_ = slots - sum(min(k, o) for k in range(1, M + 1))  # the multipliers alone, 4 pairs x 64 x 4 columns
            return ("REG", 4, 1, slots, 0, 4 * np_ * 64 * 4 * 4, 0)
        return lds(4) if lds_ok(4) else None
    if split_on and l2 <= 509 and o <= 6 and slots * 64 * 8 * 4 + cbuf(8) + 256 <= budget:
        return ("SPLIT4", 2, 4, slots, 0, 4 * slots * 64 * 2 * 4, 0)
    return lds(8) if lds_ok(8) else None


@pytest.mark.skipif("GPSIG_HO_SPLIT" in os.environ, reason="GPSIG_HO_SPLIT pins the kernel form the query reports")
def test_sig_vjp_ho_route_query_without_gpu(monkeypatch):
    """gpsig_sig_vjp_ho_route is host only: what gpsig_sig_gram_vjp_ho would run for a shape.  Argument errors,
    the whole support table 2 <= o <= M <= 8 at every length seam with the split on and off against the header's
    rules, the slot counts and code variants, chunks and launches, and agreement with the support and workspace
    queries."""
    import gpsig_amd
    import gpsig_amd._lib as L
    from gpsig_amd import ops
    lib = L.load()
    out = (ctypes.c_int * 9)()

    def rc(n1=4, l1=45, n2=2, l2=40, d=3, M=4, order=3, base=L.BASE_RBF, pm=L.PAIRS_RECT, r0=0, r1=4, o=out):
        return lib.gpsig_sig_vjp_ho_route(n1, l1, n2, l2, d, M, order, base, pm, r0, r1, o)
    assert rc() == L.GPSIG_OK
    assert rc(o=None) == L.GPSIG_EINVAL
    assert rc(order=1) == L.GPSIG_EINVAL                    # the first-order VJP is not this query's
    assert rc(order=0) == L.GPSIG_EINVAL
    assert rc(M=1) == L.GPSIG_EINVAL                        # one level runs the first-order VJP too
    assert rc(l2=1) == L.GPSIG_EINVAL
    assert rc(l1=1) == L.GPSIG_EINVAL
    assert rc(d=0) == L.GPSIG_EINVAL
    assert rc(r1=5) == L.GPSIG_EINVAL                       # row window past n1
    assert rc(r0=3, r1=2) == L.GPSIG_EINVAL
    assert rc(r0=-1) == L.GPSIG_EINVAL
    assert rc(pm=L.PAIRS_UPPER) == L.GPSIG_EINVAL           # UPPER pairs X with itself: equal shapes
    assert rc(pm=3) == L.GPSIG_EINVAL
    for base in (L.BASE_MATERN12, L.BASE_MATERN32, L.BASE_MATERN52):
        assert rc(base=base) == L.GPSIG_EUNSUPPORTED and list(out) == [0] * 9
        assert lib.gpsig_sig_vjp_ho_workspace_bytes(4, 45, 2, 40, 3, 4, 3, base) == 0
    assert rc(M=9, order=2) == L.GPSIG_EUNSUPPORTED

    keys = ("kernel", "W", "waves", "slots", "variant", "lds_bytes", "slab_bytes")
    # slot counts of the issue's variant pins
    assert [_ho_vjp_slots(2, M) for M in range(2, 9)] == [6 * M - 5 for M in range(2, 9)]
    assert [_ho_vjp_slots(3, M) for M in range(3, 9)] == [19, 31, 43, 55, 67, 79]
    assert [_ho_vjp_slots(4, M) for M in range(4, 9)] == [39, 59, 79, 99, 119]
    assert [_ho_vjp_slots(5, M) for M in range(5, 8)] == [69, 99, 129]
    assert _ho_vjp_slots(6, 6) == 111
    table = {}
    for split_on in (True, False):
        if not split_on:
            monkeypatch.setenv("GPSIG_HO_SPLIT", "0")
        for M in range(2, 9):
            for o in range(2, M + 1):
                for l2 in (2, 256, 257, 509, 510, 512, 513, 1017, 1018):
                    exp = _ho_vjp_expected(l2, o, M, split_on)
                    for base in ("rbf", "linear"):
                        # order past the level count is the exact kernel: min(order, M)
                        for order in ((o,) if o < M else (o, o + 3)):
                            code = lib.gpsig_sig_vjp_ho_route(1, 7, 2, l2, 3, M, order, ops.base_kind(base),
                                                              L.PAIRS_RECT, 0, 1, out)
                            what = (split_on, l2, o, M, base, order)
                            if exp is None:
                                assert code == L.GPSIG_EUNSUPPORTED, what
                                assert list(out) == [0] * 9, what
                                with pytest.raises(gpsig_amd.GpsigError):
                                    ops.ho_vjp_route(1, 7, 2, l2, 3, M, order, base)
                            else:
                                assert code == L.GPSIG_OK, what
                                r = ops.ho_vjp_route(1, 7, 2, l2, 3, M, order, base)
                                assert tuple(r[k] for k in keys) == exp, what
                                assert (r["chunks"], r["launches"]) == (1, 1), what
                            assert ops.ho_vjp_supported(l2, M, order, base) == (exp is not None), what
                            ws = lib.gpsig_sig_vjp_ho_workspace_bytes(1, 7, 2, l2, 3, M, order, ops.base_kind(base))
                            assert (ws > 0) == (exp is not None), what
                    table[(split_on, l2, o, M)] = None if exp is None else exp[0] + (str(exp[1]) if exp[0] == "LDS" else "")
        monkeypatch.delenv("GPSIG_HO_SPLIT", raising=False)

    # the orientation table of the split-on routes, spelled out
    def where(l2, name, split_on=True):
        return sorted((o, M) for (s, l, o, M), k in table.items() if s == split_on and l == l2 and k == name)

    def pairs(spec):
        return sorted((o, M) for o, Ms in spec.items() for M in Ms)
    for l2 in (2, 256):
        assert where(l2, "REG") == pairs({2: range(2, 9), 3: range(3, 6)})
        assert where(l2, "LDS4") == pairs({3: (6, 7, 8), 4: range(4, 9), 5: (5, 6, 7), 6: (6,)})
    for l2 in (257, 509):
        assert where(l2, "SPLIT4") == pairs({2: range(2, 9), 3: range(3, 8), 4: (4, 5), 5: (5,)})
        assert where(l2, "LDS8") == [] and where(l2, "SPLIT8") == []
        assert where(l2, "LDS8", False) == where(l2, "SPLIT4") and where(l2, "SPLIT4", False) == []
    split8 = pairs({2: range(2, 8), 3: range(3, 7), 4: (4, 5), 5: (5,)})
    for l2 in (510, 512):
        for s in (True, False):  # the 8-wave form does not depend on the switch
            assert where(l2, "SPLIT8", s) == split8
            assert where(l2, "LDS8", s) == [(2, 8), (3, 7)]
    for l2 in (513, 1017):
        assert where(l2, "SPLIT8") == split8
        assert [k for (s, l, o, M), k in table.items() if l == l2 and k not in (None, "SPLIT8")] == []
    assert all(k is None for (s, l, o, M), k in table.items() if l == 1018)
    # every code variant of the W = 4 LDS kernel: unpinned to 60 slots, pinned to 100, fenced past
    variants = {(o, M): ops.ho_vjp_route(1, 7, 2, 256, 3, M, o)["variant"] for (o, M) in where(256, "LDS4")}
    assert variants == {(3, 6): 0, (4, 4): 0, (4, 5): 0, (3, 7): 1, (3, 8): 1, (4, 6): 1, (5, 5): 1, (5, 6): 1,
                        (4, 7): 1, (6, 6): 2, (4, 8): 2, (5, 7): 2}

    # chunks, launches, row windows: l2 decides the kernel, the pair mode and rows the grid
    def route(*a, **kw):
        r = ops.ho_vjp_route(*a, **kw)
        return r["kernel"], r["chunks"], r["launches"]
    assert route(7, 10, 3, 10, 2, 3, 2, rows=(3, 5)) == ("REG", 1, 1)
    assert route(7, 10, 3, 10, 2, 3, 2, rows=(2, 2)) == ("REG", 0, 0)        # an empty window: the geometry alone
    assert route(7, 10, None, None, 2, 4, 4, "linear", rows=(5, 7)) == ("LDS", 1, 1)
    assert route(7, 10, None, None, 2, 4, 4, diag=True) == ("LDS", 1, 1)
    assert route(2, 700, 2, 20, 2, 3, 2) == ("REG", 1, 1)                    # l1 does not enter
    assert route(2, 20, 2, 700, 2, 3, 2) == ("SPLIT8", 1, 1)
    # the 1 GiB point-weight tile holds 44 rows of 64 sequences of 300 points: two chunks
    assert route(64, 300, None, None, 3, 4, 3) == ("SPLIT4", 2, 2)
    # SPLIT8 launches at most 1024 workgroups: the 33 x 33 = 1089 pairs of one chunk go in two, 32 x 32 in one
    r = ops.ho_vjp_route(33, 12, 33, 510, 2, 2, 2, "linear")
    assert (r["kernel"], r["chunks"], r["launches"], r["slab_bytes"]) == ("SPLIT8", 1, 2, 1024 * 8 * 7 * 128 * 4)
    assert route(32, 12, 32, 510, 2, 2, 2, "linear") == ("SPLIT8", 1, 1)
    assert route(65, 12, 32, 510, 2, 2, 2, "linear") == ("SPLIT8", 1, 3)     # 2080 pairs
    # 510 rows per x-sequence: the 1 GiB tile holds 28 of them against 33 x 510 columns, 32 against 32 x 510
    assert route(33, 510, 33, 510, 2, 2, 2, "linear") == ("SPLIT8", 2, 2)
    assert route(32, 510, 32, 510, 2, 2, 2, "linear") == ("SPLIT8", 1, 1)
    assert route(33, 510, None, None, 2, 2, 2) == ("SPLIT8", 2, 2)           # 546 + 15 upper pairs
    assert route(33, 510, None, None, 2, 2, 2, diag=True) == ("SPLIT8", 1, 1)
    # the slab region is what the workspace query adds for the 8-wave form
    w510 = lib.gpsig_sig_vjp_ho_workspace_bytes(2, 510, 2, 510, 2, 5, 5, L.BASE_RBF)
    monkeypatch.setenv("GPSIG_HO_SPLIT", "0")
    assert ops.ho_vjp_route(2, 300, 2, 300, 2, 3, 2)["kernel"] == "LDS"
    monkeypatch.delenv("GPSIG_HO_SPLIT")
    assert ops.ho_vjp_route(2, 300, 2, 300, 2, 3, 2)["kernel"] == "SPLIT4"
    assert w510 > ops.ho_vjp_route(2, 510, 2, 510, 2, 5, 5)["slab_bytes"] == 1024 * 8 * 69 * 128 * 4


def test_graph_capture_refuses_host_tensors_and_kernel_to():
    """gpsig_amd.graphs.GraphedCall takes device tensors only; kern.to() keeps parameter leaves."""
    import torch
    import gpsig_amd
    from gpsig_amd.graphs import GraphedCall
    with pytest.raises(ValueError):
        GraphedCall(lambda a: a, torch.zeros(2))
    k = gpsig_amd.SignatureRBF(20, 2, 3, lengthscales=[1.0, 2.0])
    k.lengthscales.requires_grad_(True)
    k.to("cpu")
    assert k.lengthscales.is_leaf and k.lengthscales.requires_grad
    assert gpsig_amd.UntruncSignatureKernel(20, 2).to("cpu").num_features == 2


def test_release_workspaces_clears_cache():
    from gpsig_amd import ops
    ops._ws[("x", 0)] = object()
    ops.release_workspaces()
    assert not ops._ws
