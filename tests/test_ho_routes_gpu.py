"""GPU parity of the higher-order forward recursion (csrc/sig_ho.hip: sig_ho_kernel plain, blocked and SPLIT, the
tile mode past 32 channels, and the switch of ops.sig_gram / ops.sig_diag to signature features) with the float64
oracle (oracle/kernels_ref.py, signature_algs.py:37-74) on the fp32-rounded inputs the kernels receive, at every
route and geometry seam.  Every case asks gpsig_sig_ho_route (ops.ho_route: host only, the launch path's own
helpers) which route its shape takes and asserts it before it compares, so a case that moves to another route fails
instead of passing for the wrong reason.

Level 1 is a closed form in every kernel, so only levels >= 2 show a wrong cell, scan or carry: every assertion is
per level, norm_rel_err < TOL = 1e-5 on K(X, Y), K(X) and the diagonal.  K(X) equals its transpose exactly, and
sig_diag equals diagonal(K(X)) to 2e-6 (two summation orders of the same cells, as
test_long_gpu.test_higher_order_split_forward_matches_plain).  X is a few points longer than Y; the table's lengths
are Y's, and the symmetric and diagonal modes run on Y as well, so all three pair modes sit on the seam.

Data: random walks cumsum(randn) / sqrt(L D) at scale 1; "jumpy": scale 3 with five increments of two sequences
25 times larger (as test_vjp_regimes_gpu.py's slow rows), on a subset.

Where each value of the route query is oracle-checked (test, case ids):
  tiled 0          every case but the two below          tiled 1   test_tile_seam (D = 33)
  DP 4             D <= 4 everywhere                     DP 8      test_channel_paddings D 8, linear orders 6 / 5
  DP 16            test_channel_paddings D 9, 16         DP 32     test_channel_paddings D 17, 32; test_tile_seam D 32
  W 1 / 2 / 4      test_w_and_block_seams l2 64 / 65, 128 / 129, 256; orders 5 (W 2) and 6..8 (W 1) in
                   test_order5_blocks, test_orders_6_8_*
  blocks 1         the *-one-block cases, l2 <= 64 W
  blocks 2, 3, 4   test_w_and_block_seams 257 (last block = 1 cell), 511, 512; test_order5_blocks 129, 255, 256;
                   test_orders_6_8_blocks 65, 127, 128, 253
  blocks >= 5      test_plain_blocked_five_blocks (order 6 at 254, order 5 at 510), test_lds_limit
  split 1          every 2..4-block case above
  split 0 by block count   test_plain_blocked_five_blocks, test_lds_limit
  split 0 by pair count    test_split_switch_by_pair_count (48 x 43 pairs)
  split 0 by GPSIG_HO_SPLIT=0   test_forced_plain
  features 1       test_feature_path_against_recursion (as is)    features 0   every other case
"""
import numpy as np
import pytest
import torch

from conftest import norm_rel_err
from oracle import chen
from oracle import kernels_ref as kr

pytestmark = pytest.mark.gpu
TOL = 1e-5
SAME = 2e-6  # two summation orders of the same fp32 cells
DEV = "cuda"


def t(x):
    return torch.as_tensor(np.asarray(x, dtype=np.float32), device=DEV)


def r32(x):
    """The fp32-rounded inputs the kernels receive, as the oracle's float64."""
    return np.asarray(x).astype(np.float32).astype(np.float64)


def walks(n, l, d, seed, jumpy=False):
    rng = np.random.default_rng(seed)
    inc = rng.standard_normal((n, l, d)) / np.sqrt(l * d)
    if jumpy:
        inc *= 3.0
        rows = rng.choice(np.arange(1, l), size=min(5, l - 1), replace=False)
        inc[: max(1, n // 2), rows, :] *= 25.0 / 3.0
    return r32(np.cumsum(inc, 1))


def widen(X, d):
    """The same walks with channels added up to d (fresh small walks), so neighbouring channel counts share data."""
    n, l, d0 = X.shape
    if d == d0:
        return X
    extra = walks(n, l, d - d0, 977 + l + d0) * 0.5
    return np.concatenate([X, extra], axis=2)


def assert_levels(got, exp, what, tol=TOL, first=1):
    err = norm_rel_err(got[first:], exp[first:], axis_levels=True)
    print(f"{what}: per-level err {np.array2string(err, precision=2)}")
    assert (err < tol).all(), (what, err)


def assert_route(r, want, what):
    got = {k: r[k] for k in want}
    assert got == want, (what, r)


_ORACLE = {}


def oracle(X, Y, M, order, base, sym_x):
    """The float64 reference of a case, computed once (the forced-plain cases run their data on two routes)."""
    key = (X.tobytes(), Y.tobytes(), X.shape, M, order, base, sym_x)
    if key not in _ORACLE:
        ref = kr.SignatureKernelRef(1, 1, M, normalization=False, base=base, order=order)
        exp = {"xy": ref.K_seq(X, Y)}
        for name, Z in (("Y", Y),) + ((("X", X),) if sym_x else ()):
            exp[name] = (ref.K_seq(Z), ref.K_seq_diag(Z))
        _ORACLE.clear()  # one case's worth: the next use, if any, follows at once
        _ORACLE[key] = exp
    return _ORACLE[key]


def check_case(l2, D, M, order, base, want, n1=4, n2=2, dl=5, jumpy=False, seed=0, X=None, Y=None, sym_x=True):
    """K(X, Y), K(X), diag(X) and, at the seam length itself, K(Y), diag(Y) against the oracle, routes first.
    want: the route of the calls at l2 (tiled, DP, W, nblk, split, features; the keys given are compared)."""
    from gpsig_amd import ops
    l1 = l2 + dl
    if X is None:
        X = walks(n1, l1, D, 1000 * order + l2 + seed, jumpy)
        Y = walks(n2, l2, D, 1000 * order + l2 + seed + 1, jumpy)
    n1, n2 = len(X), len(Y)
    want = {**dict(features=False, tiled=0), **want}
    assert_route(ops.ho_route(n1, l1, n2, l2, D, M, order, base), want, "K(X, Y)")
    assert_route(ops.ho_route(n2, l2, None, None, D, M, order, base), want, "K(Y)")
    assert_route(ops.ho_route(n2, l2, None, None, D, M, order, base, diag=True), want, "diag(Y)")
    rx = ops.ho_route(n1, l1, None, None, D, M, order, base)
    assert not rx["features"] and rx["tiled"] == want["tiled"]
    exp = oracle(X, Y, M, order, base, sym_x)
    Xt, Yt = t(X), t(Y)
    out = {}
    got = ops.sig_gram(Xt, Yt, M, order=order, base=base).cpu().numpy()
    assert_levels(got, exp["xy"], "K(X, Y)")
    out["xy"] = got
    for name, Zt in (("Y", Yt),) + ((("X", Xt),) if sym_x else ()):
        got = ops.sig_gram(Zt, None, M, order=order, base=base).cpu().numpy()
        assert_levels(got, exp[name][0], f"K({name})")
        np.testing.assert_array_equal(got, got.transpose(0, 2, 1))
        dg = ops.sig_diag(Zt, M, order=order, base=base).cpu().numpy()
        assert_levels(dg, exp[name][1], f"diag({name})")
        kd = np.stack([np.diagonal(g) for g in got])
        assert_levels(dg, kd, f"diag({name}) vs diagonal(K({name}))", tol=SAME)
        out[name] = (got, dg)
    return out


# ------------------------------------------------------------------------------------------ orders 6-8, one block
@pytest.mark.parametrize("base,order,M,D", [
    ("rbf", 6, 6, 3), ("rbf", 7, 7, 3), ("rbf", 8, 8, 3), ("rbf", 6, 8, 3),
    # linear at order = M runs the recursion only past SIG_FEATURE_MAX = 16000 coordinates: 19530, 21844, 87380
    ("linear", 6, 6, 5), ("linear", 7, 7, 4), ("linear", 8, 8, 4),
])
def test_orders_6_8_one_block(base, order, M, D):
    check_case(40, D, M, order, base, dict(W=1, nblk=1, split=0, DP=4 if D <= 4 else 8))


def test_orders_6_8_one_block_jumpy():
    check_case(40, 3, 8, 8, "rbf", dict(W=1, nblk=1, split=0), jumpy=True)


# ------------------------------------------------------------------------------------------ W and block seams
LOW = [("rbf", 2), ("linear", 3), ("rbf", 4)]  # M = 5: linear order 3 < M is the recursion at any D


@pytest.mark.parametrize("base,order", LOW)
@pytest.mark.parametrize("l2,W,nblk", [(64, 1, 1), (65, 2, 1), (128, 2, 1), (129, 4, 1), (256, 4, 1),
                                       (257, 4, 2), (511, 4, 2), (512, 4, 3)])
def test_w_and_block_seams(base, order, l2, W, nblk):
    """ho_w switches W at l2 = 64 / 65 and 128 / 129; column blocks of 255 cells from 257 points: 257 is a last
    block of exactly one cell, 511 two full blocks, 512 three."""
    check_case(l2, 3, 5, order, base, dict(W=W, nblk=nblk, split=int(nblk > 1), DP=4), sym_x=l2 < 257)


@pytest.mark.parametrize("base,D", [("rbf", 3), ("linear", 7)])  # linear D 7, M 5: 19607 coordinates
@pytest.mark.parametrize("l2,nblk", [(128, 1), (129, 2), (255, 2), (256, 3)])
def test_order5_blocks(base, D, l2, nblk):
    check_case(l2, D, 5, 5, base, dict(W=2, nblk=nblk, split=int(nblk > 1), DP=4 if D <= 4 else 8), sym_x=l2 < 200)


@pytest.mark.parametrize("base,order,D", [("rbf", 6, 3), ("linear", 8, 4)])
@pytest.mark.parametrize("l2,nblk", [(64, 1), (65, 2), (127, 2), (128, 3), (253, 4)])
def test_orders_6_8_blocks(base, order, D, l2, nblk):
    check_case(l2, D, order, order, base, dict(W=1, nblk=nblk, split=int(nblk > 1), DP=4), n1=3, sym_x=l2 < 200)


def test_blocks_jumpy():
    check_case(257, 3, 5, 4, "rbf", dict(W=4, nblk=2, split=1), jumpy=True, sym_x=False)
    check_case(128, 3, 6, 6, "rbf", dict(W=1, nblk=3, split=1), jumpy=True, n1=3)


# ------------------------------------------------------------------------------------------ the plain blocked kernel
@pytest.mark.parametrize("order,l2,W", [(6, 254, 1), (5, 510, 2)])
def test_plain_blocked_five_blocks(order, l2, W):
    """Five blocks are past SPLIT's four: one wave per pair walks the blocks, the carries in dynamic LDS."""
    from gpsig_amd import ops
    check_case(l2, 3, order, order, "rbf", dict(W=W, nblk=5, split=0), n1=3, sym_x=False)
    assert ops.ho_route(3, l2 + 5, 2, l2, 3, order, order, "rbf")["carry_bytes"] > 0


def test_split_switch_by_pair_count():
    """SPLIT holds while nblocks * 4 <= 2048 workgroups: 12 row groups x 42 sequences = 504 take it, x 43 = 516 the
    plain kernel; both against the oracle.  Order 6 at l2 = 65 (W 1, two blocks): order 2 runs 65 points at W = 2
    in one block and never reaches the switch."""
    from gpsig_amd import ops
    l2, D, M, order = 65, 2, 6, 6
    X = walks(48, l2 + 3, D, 5)
    Y = walks(43, l2, D, 6)
    chk = [0, 3, 17, 44, 47]  # the oracle on five rows of the 48; every pair: plain against split
    exp = kr.SignatureKernelRef(1, 1, M, normalization=False, order=order).K_seq(X[chk], Y)
    got = {}
    for n2, split in ((42, 1), (43, 0)):
        r = ops.ho_route(48, l2 + 3, n2, l2, D, M, order, "rbf")
        assert_route(r, dict(W=1, nblk=2, split=split, tiled=0, features=False), f"n2 = {n2}")
        assert (r["carry_bytes"] > 0) == (split == 0)
        got[n2] = ops.sig_gram(t(X), t(Y[:n2]), M, order=order).cpu().numpy()
        assert_levels(got[n2][:, chk], exp[:, :, :n2], f"K(X, Y[:{n2}])")
    assert_levels(got[43][:, :, :42], got[42], "plain vs split", tol=SAME)


FORCED = [("rbf", 2, 5, 3, 257, 4, 2), ("linear", 3, 5, 3, 512, 4, 3), ("rbf", 5, 5, 3, 129, 2, 2),
          ("linear", 5, 5, 7, 256, 2, 3), ("rbf", 6, 6, 3, 65, 1, 2), ("linear", 8, 8, 4, 253, 1, 4)]


@pytest.mark.parametrize("base,order,M,D,l2,W,nblk", FORCED)
def test_forced_plain(base, order, M, D, l2, W, nblk, monkeypatch):
    """The 2..4-block cases on the plain kernel (GPSIG_HO_SPLIT=0), against the oracle and against SPLIT."""
    split = check_case(l2, D, M, order, base, dict(W=W, nblk=nblk, split=1), n1=3, sym_x=False)
    monkeypatch.setenv("GPSIG_HO_SPLIT", "0")
    plain = check_case(l2, D, M, order, base, dict(W=W, nblk=nblk, split=0), n1=3, sym_x=False)
    assert_levels(plain["xy"], split["xy"], "plain vs split K(X, Y)", tol=SAME)
    assert_levels(plain["Y"][0], split["Y"][0], "plain vs split K(Y)", tol=SAME)
    assert_levels(plain["Y"][1], split["Y"][1], "plain vs split diag(Y)", tol=SAME)


def test_lds_limit():
    """The carries of the plain kernel at l1 = 293, order 8, M 8: 4 waves x 292 rows x 35 scans x 4 B = 163520 B of
    the 163840 allowed; one more point is refused by the route query and by the call, before any launch."""
    from gpsig_amd import _lib as Lb
    from gpsig_amd import ops
    D, M, l2 = 2, 8, 254
    X, Y = walks(3, 293, D, 21), walks(2, l2, D, 22)
    r = ops.ho_route(3, 293, 2, l2, D, M, 8, "rbf")
    assert_route(r, dict(W=1, nblk=5, split=0, tiled=0, carry_bytes=163520, features=False), "l1 = 293")
    ref = kr.SignatureKernelRef(1, 1, M, normalization=False, order=8)
    assert_levels(ops.sig_gram(t(X), t(Y), M, order=8).cpu().numpy(), ref.K_seq(X, Y), "K(X, Y) at the LDS limit")
    import ctypes
    out = (ctypes.c_int * 7)()
    assert Lb.load().gpsig_sig_ho_route(3, 294, 2, l2, D, M, 8, Lb.BASE_RBF, 1, Lb.PAIRS_RECT, 0, 3, out) == \
        Lb.GPSIG_EUNSUPPORTED
    assert out[5] == 4 * 293 * 35 * 4
    with pytest.raises(Lb.GpsigError):
        ops.ho_route(3, 294, 2, l2, D, M, 8, "rbf")
    with pytest.raises(Lb.GpsigError):
        ops.sig_gram(torch.zeros((3, 294, D), device=DEV), t(Y), M, order=8)


# ------------------------------------------------------------------------------------------ channels
@pytest.mark.parametrize("base,order", [("rbf", 3), ("linear", 2)])
@pytest.mark.parametrize("D,DP", [(8, 8), (9, 16), (16, 16), (17, 32), (32, 32)])
def test_channel_paddings(base, order, D, DP):
    check_case(40, D, 4, order, base, dict(W=1, nblk=1, split=0, DP=DP))


@pytest.mark.parametrize("base", ["rbf", "linear"])
@pytest.mark.parametrize("l2,W,nblk", [(40, 1, 1), (150, 4, 1)])
def test_tile_seam(base, l2, W, nblk):
    """32 channels: the padded records; 33 (the same data and one more channel): the increment tiles."""
    X32, Y32 = walks(4, l2 + 5, 32, l2), walks(2, l2, 32, l2 + 1)
    a = check_case(l2, 32, 4, 3, base, dict(W=W, nblk=nblk, split=0, DP=32), X=X32, Y=Y32)
    b = check_case(l2, 33, 4, 3, base, dict(W=W, nblk=nblk, split=0, DP=0, tiled=1), X=widen(X32, 33), Y=widen(Y32, 33))
    assert a["xy"].shape == b["xy"].shape


@pytest.mark.parametrize("base", ["rbf", "linear"])
def test_tile_seam_two_blocks(base):
    """Order 5 at 150 points: two column blocks (W 2), SPLIT, on either side of the tile seam."""
    X32, Y32 = walks(3, 155, 32, 41), walks(2, 150, 32, 42)
    check_case(150, 32, 5, 5, base, dict(W=2, nblk=2, split=1, DP=32), X=X32, Y=Y32, sym_x=False)
    check_case(150, 33, 5, 5, base, dict(W=2, nblk=2, split=1, DP=0, tiled=1), X=widen(X32, 33), Y=widen(Y32, 33),
               sym_x=False)


# ------------------------------------------------------------------------------------------ identities
def test_level_identity_across_orders():
    """Level m of the recursion depends on min(m, order) only: levels 1..p of the order-p output equal those of
    the order-8 output (the float64 oracle's are bit-equal), across the seven ORD instantiations on the same cells."""
    from gpsig_amd import ops
    X, Y = walks(4, 70, 3, 31), walks(2, 66, 3, 32)
    Xt, Yt = t(X), t(Y)
    top = ops.sig_gram(Xt, Yt, 8, order=8).cpu().numpy()
    assert_levels(top, kr.SignatureKernelRef(1, 1, 8, normalization=False, order=8).K_seq(X, Y), "order 8")
    for p in range(2, 8):
        assert not ops.ho_route(4, 70, 2, 66, 3, 8, p, "rbf")["features"]
        got = ops.sig_gram(Xt, Yt, 8, order=p).cpu().numpy()
        assert_levels(got[:p + 1], top[:p + 1], f"order {p} vs order 8", tol=SAME)


@pytest.mark.parametrize("L,D,M,want", [(70, 3, 8, dict(W=1, nblk=2, split=1)), (300, 2, 5, dict(W=2, nblk=3, split=1))])
def test_feature_path_against_recursion(L, D, M, want, monkeypatch):
    """Linear at order = M: signature features + GEMMs as is, the recursion with SIG_FEATURE_MAX = 0; both against
    the oracle and against Chen-identity signature inner products."""
    from gpsig_amd import ops
    X, Y = walks(4, L + 4, D, L), walks(2, L, D, L + 1)
    exp = kr.SignatureKernelRef(1, 1, M, normalization=False, base="linear", order=M).K_seq(X, Y)
    sig = chen.signature_levels_kernel(X, Y, M)
    assert_levels(exp, sig, "oracle vs Chen", tol=1e-9)
    assert ops.ho_route(4, L + 4, 2, L, D, M, M, "linear")["features"]
    got = ops.sig_gram(t(X), t(Y), M, order=M, base="linear").cpu().numpy()
    assert_levels(got, exp, "features vs oracle")
    assert_levels(got, sig, "features vs Chen")
    monkeypatch.setattr(ops, "SIG_FEATURE_MAX", 0)
    assert_route(ops.ho_route(4, L + 4, 2, L, D, M, M, "linear"), dict(features=False, tiled=0, **want), "recursion")
    rec = ops.sig_gram(t(X), t(Y), M, order=M, base="linear").cpu().numpy()
    assert_levels(rec, exp, "recursion vs oracle")
    assert_levels(rec, sig, "recursion vs Chen")
    d = ops.sig_diag(t(Y), M, order=M, base="linear").cpu().numpy()
    assert_levels(d, np.stack([np.diagonal(k) for k in chen.signature_levels_kernel(Y, Y, M)]), "recursion diag vs Chen")


# ------------------------------------------------------------------------------------------ rows, epilogues
def test_row_sharding_not_tiled():
    """rows=(r0, r1) on the fixed-channel kernel: the shards' union is bit-equal to the unsharded call."""
    from gpsig_amd import ops
    N, L, D, M, order = 9, 70, 3, 4, 3
    X, Y = t(walks(N, L, D, 51)), t(walks(3, L - 4, D, 52))
    assert_route(ops.ho_route(N, L, None, None, D, M, order, "rbf", rows=(3, 7)),
                 dict(tiled=0, W=2, nblk=1, split=0, launches=1, features=False), "rows")
    full = ops.sig_gram(X, None, M, order=order)
    for r0, r1 in [(0, 4), (4, 9), (3, 7)]:
        got = ops.sig_gram(X, None, M, order=order, rows=(r0, r1))
        for a in range(r0, r1):
            assert torch.equal(got[:, a - r0, a:], full[:, a, a:]), (r0, r1, a)
    full = ops.sig_gram(X, Y, M, order=order)
    out = torch.full_like(full, float("nan"))
    for r0, r1 in [(0, 4), (4, 9)]:
        ops.sig_gram(X, Y, M, order=order, rows=(r0, r1), out=out, out_row0=0)
    assert torch.equal(out, full)
    mid = ops.sig_gram(X, Y, M, order=order, rows=(3, 7))
    assert torch.equal(mid, full[:, 3:7])


@pytest.mark.parametrize("order,L,nblk", [(3, 70, 1), (3, 300, 2), (6, 40, 1), (6, 70, 2)])
def test_diag_rsqrt_epilogue(order, L, nblk):
    from gpsig_amd import ops
    X = walks(5, L, 3, 61 + L)
    assert_route(ops.ho_route(5, L, None, None, 3, 6, order, "rbf", diag=True),
                 dict(tiled=0, nblk=nblk, split=int(nblk > 1), features=False), "diag")
    d64 = kr.SignatureKernelRef(1, 1, 6, normalization=False, order=order).K_seq_diag(X)
    got = ops.sig_diag(t(X), 6, order=order, jitter=1e-6, rsqrt=True).cpu().numpy()
    assert_levels(got, 1.0 / np.sqrt(d64 + 1e-6), "rsqrt diag", first=0)


@pytest.mark.parametrize("L,nblk", [(40, 1), (130, 3)])
@pytest.mark.parametrize("cls", ["rbf", "linear"])
def test_fused_normalisation(cls, L, nblk):
    """SignatureRBF(num_levels=6, order=0) and SignatureLinear(5 channels, order=6): order 0 and order >= num_levels
    mean order = num_levels; the normalised K with lengthscales and variances through the fused epilogue."""
    import gpsig_amd
    from gpsig_amd import ops
    D, M = (3, 6) if cls == "rbf" else (5, 6)
    rng = np.random.default_rng(L + D)
    ls = 0.7 + rng.random(D)
    var = 0.5 + rng.random(M + 1)
    X = walks(4, L, D, 71 + L).reshape(4, -1)
    X2 = walks(3, L, D, 72 + L).reshape(3, -1)
    assert_route(ops.ho_route(4, L, None, None, D, M, M, cls), dict(tiled=0, W=1, nblk=nblk, features=False), cls)
    if cls == "rbf":
        k = gpsig_amd.SignatureRBF(L * D, D, M, order=0, lengthscales=ls, variances=var)
    else:
        k = gpsig_amd.SignatureLinear(L * D, D, M, order=6, lengthscales=ls, variances=var)
    assert k.order == M
    ref = kr.SignatureKernelRef(L * D, D, M, base=cls, order=0, lengthscales=ls, variances=var)
    lv = k.K(t(X), return_levels=True).cpu().numpy()
    assert_levels(lv, ref.K(X, return_levels=True), "K(X) levels", first=0)
    for m in range(M + 1):
        assert np.abs(np.diagonal(lv[m]) / var[m] - 1.0).max() < SAME, m
    assert norm_rel_err(k.K(t(X)).cpu().numpy(), ref.K(X)) < TOL
    assert norm_rel_err(k.K(t(X), t(X2)).cpu().numpy(), ref.K(X, X2)) < TOL
    assert_levels(k.K(t(X), t(X2), return_levels=True).cpu().numpy(), ref.K(X, X2, return_levels=True),
                  "K(X, X2) levels", first=0)


# ------------------------------------------------------------------------------------------ short and empty
@pytest.mark.parametrize("order", [2, 8])
@pytest.mark.parametrize("l1,l2,n1,n2", [(2, 9, 4, 2), (9, 2, 4, 2), (2, 2, 4, 2), (3, 3, 4, 2), (9, 7, 4, 1),
                                         (9, 7, 5, 2)])
def test_short_sequences(order, l1, l2, n1, n2):
    """One cell (l = 2), two cells, a single y, and a ragged last group of 4 pairs (N1 = 5)."""
    from gpsig_amd import ops
    M = 8
    X, Y = walks(n1, l1, 3, 81 + l1), walks(n2, l2, 3, 82 + l2)
    assert_route(ops.ho_route(n1, l1, n2, l2, 3, M, order, "rbf"), dict(tiled=0, W=1, nblk=1, split=0, features=False), "")
    ref = kr.SignatureKernelRef(1, 1, M, normalization=False, order=order)
    assert_levels(ops.sig_gram(t(X), t(Y), M, order=order).cpu().numpy(), ref.K_seq(X, Y), "K(X, Y)")
    got = ops.sig_gram(t(X), None, M, order=order).cpu().numpy()
    assert_levels(got, ref.K_seq(X), "K(X)")
    np.testing.assert_array_equal(got, got.transpose(0, 2, 1))
    assert_levels(ops.sig_diag(t(X), M, order=order).cpu().numpy(), ref.K_seq_diag(X), "diag(X)")


def test_empty_calls_do_not_launch():
    from gpsig_amd import ops
    X = t(walks(4, 20, 3, 91))
    assert ops.ho_route(4, 20, None, None, 3, 4, 3, "rbf", rows=(2, 2))["launches"] == 0
    out = torch.full((5, 4, 4), 7.0, device=DEV)
    ops.sig_gram(X, None, 4, order=3, rows=(2, 2), out=out, out_row0=0)
    assert (out == 7.0).all()
    assert ops.sig_gram(X[:0], X, 4, order=3).shape == (5, 0, 4)
    assert ops.sig_gram(X, X[:0], 4, order=3).shape == (5, 4, 0)
    assert ops.sig_diag(X[:0], 4, order=3).shape == (5, 0)
