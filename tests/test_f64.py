"""Float64 first-order Gram (gpsig_sig_gram_f64 / gpsig_sig_diag_f64), host side: every return code the header
lists is given before any launch (fake pointers, no GPU), the route table, the workspace formula, and the
precision keyword of SignatureKernel."""
import ctypes

import pytest
import torch

import gpsig_amd
from gpsig_amd import _lib as L
from gpsig_amd import ops

FAKE = ctypes.c_void_p(256)
WS = 1 << 30


def _lib():
    return L.load()


def gram(n1=4, l1=10, n2=4, l2=10, d=3, M=4, kind=L.BASE_RBF, diff=1, pm=L.PAIRS_RECT, r0=2, r1=2, X=FAKE, Y=FAKE,
         rs1=None, rs2=None, out_mode=L.OUT_LEVELS, out=FAKE, ws=FAKE, nb=WS):
    """gpsig_sig_gram_f64 on fake pointers; the default row window is empty, so GPSIG_OK launches nothing."""
    return _lib().gpsig_sig_gram_f64(X, n1, l1, Y, n2, l2, d, M, kind, diff, pm, r0, r1, rs1, rs2, None, 0.0,
                                     out_mode, out, 0, n1, ws, nb, None)


def diag(n=4, l=10, d=3, M=4, kind=L.BASE_RBF, diff=1, out_mode=L.OUT_LEVELS, nb=WS):
    return _lib().gpsig_sig_diag_f64(FAKE, n, l, d, M, kind, diff, 0.0, out_mode, FAKE, FAKE, nb, None)


def route(l1, l2, M=4, diff=1, pm=L.PAIRS_RECT):
    out = (ctypes.c_int * 2)(-1, -1)
    rc = _lib().gpsig_sig_f64_route(l1, l2, M, diff, pm, out)
    return rc, (out[0], out[1])


def test_symbols_exported():
    lib = _lib()
    for name in ("gpsig_sig_f64_workspace_bytes", "gpsig_sig_gram_f64", "gpsig_sig_diag_f64", "gpsig_sig_f64_route"):
        assert hasattr(lib, name)


@pytest.mark.parametrize("kind", [L.BASE_RBF, L.BASE_LINEAR, L.BASE_MATERN12, L.BASE_MATERN32, L.BASE_MATERN52])
@pytest.mark.parametrize("diff", [1, 0])
def test_ok_for_every_kind_and_pair_mode(kind, diff):
    for pm in (L.PAIRS_RECT, L.PAIRS_UPPER, L.PAIRS_DIAG):
        assert gram(kind=kind, diff=diff, pm=pm) == L.GPSIG_OK
    for M in range(1, 9):
        assert gram(kind=kind, diff=diff, M=M) == L.GPSIG_OK


def test_einval():
    E = L.GPSIG_EINVAL
    assert gram(X=None) == E and gram(Y=None) == E and gram(out=None) == E
    assert gram(n1=0) == E and gram(n2=0) == E and gram(d=0) == E and gram(M=0) == E
    assert gram(l1=1) == E and gram(l2=1) == E            # difference needs two points
    assert gram(l1=1, l2=1, diff=0) == L.GPSIG_OK
    assert gram(l1=0, diff=0) == E
    assert gram(pm=3) == E and gram(pm=-1) == E
    assert gram(r0=3, r1=2) == E and gram(r0=-1, r1=2) == E and gram(r0=0, r1=5) == E
    assert gram(pm=L.PAIRS_UPPER, l2=11) == E and gram(pm=L.PAIRS_UPPER, n2=5) == E   # UPPER / DIAG pair X with itself
    assert gram(rs1=FAKE) == E and gram(rs2=FAKE) == E      # rs1 / rs2 come together
    assert gram(out_mode=4) == E and gram(out_mode=-1) == E
    assert gram(out_mode=L.OUT_RSQRT) == E                  # the diagonal's mode
    assert gram(out_mode=L.OUT_RSQRT, pm=L.PAIRS_DIAG) == L.GPSIG_OK
    assert diag(out_mode=L.OUT_NORM_SUM) == E and diag(out_mode=L.OUT_NORM_LEVELS) == E
    assert diag(n=0) == E and diag(l=1) == E


def test_eunsupported_before_any_launch():
    U = L.GPSIG_EUNSUPPORTED
    # a full row window: a kernel launched on these pointers would fault, so the code comes from the checks
    full = dict(r0=0, r1=4)
    assert gram(M=9, **full) == U
    assert gram(l2=514, **full) == U and gram(l1=514, l2=514, pm=L.PAIRS_UPPER, **full) == U
    assert gram(l2=513, diff=0, **full) == U
    assert gram(kind=L.BASE_RBF | L.BASE_SEED_MFMA, **full) == U
    assert gram(kind=L.BASE_RBF | L.GRAM_SPLIT, **full) == U
    assert gram(kind=5, **full) == U and gram(kind=-1, **full) == U
    assert diag(M=9) == U and diag(l=514) == U and diag(kind=7) == U
    # the cap itself is inside, and l1 is not bounded in RECT mode (rows are streamed)
    assert gram(l2=513) == L.GPSIG_OK and gram(l2=512, diff=0) == L.GPSIG_OK and gram(l1=2000, l2=513) == L.GPSIG_OK


def test_eworkspace_before_any_launch():
    W = L.GPSIG_EWORKSPACE
    need = _lib().gpsig_sig_f64_workspace_bytes(4, 10, 4, 10, 3)
    assert gram(r0=0, r1=4, nb=need - 1) == W
    assert gram(r0=0, r1=4, ws=None) == W
    assert diag(nb=_lib().gpsig_sig_f64_workspace_bytes(4, 10, 4, 10, 3) - 1) == W
    assert gram(nb=0) == L.GPSIG_OK  # no rows: nothing to do, as gpsig_sig_gram


def test_workspace_formula():
    lib = _lib()

    def rec(n, l, d):  # x and dx, one double per channel and point, 256-byte aligned
        return (n * 2 * d * l * 8 + 255) // 256 * 256
    for n1, l1, n2, l2, d in [(4, 10, 4, 10, 3), (5, 33, 4, 20, 46), (1, 2, 1, 2, 1), (3, 513, 2, 513, 2),
                              (1024, 128, 1024, 128, 5)]:
        assert lib.gpsig_sig_f64_workspace_bytes(n1, l1, n2, l2, d) == rec(n1, l1, d) + rec(n2, l2, d)
    assert lib.gpsig_sig_f64_workspace_bytes(0, 10, 4, 10, 3) == 0
    assert lib.gpsig_sig_f64_workspace_bytes(4, 10, 4, 10, 0) == 0


# the (W, LP) table by cell columns: <= 64 (4, 16), <= 128 (4, 32), <= 256 (4, 64), <= 512 (8, 64)
SEAMS = [(2, (4, 16)), (3, (4, 16)), (65, (4, 16)), (66, (4, 32)), (129, (4, 32)), (130, (4, 64)), (257, (4, 64)),
         (258, (8, 64)), (513, (8, 64))]


@pytest.mark.parametrize("l,geo", SEAMS)
def test_route_seams(l, geo):
    for pm in (L.PAIRS_RECT, L.PAIRS_UPPER, L.PAIRS_DIAG):
        assert route(l, l, pm=pm) == (L.GPSIG_OK, geo)
        assert route(l - 1, l - 1, diff=0, pm=pm) == (L.GPSIG_OK, geo)  # the same cell columns without differences
    assert route(7, l) == (L.GPSIG_OK, geo)  # the columns decide
    assert ops.f64_route(l, None, 4) == {"W": geo[0], "LP": geo[1]}
    assert ops.f64_route(9, l, 4) == {"W": geo[0], "LP": geo[1]}


def test_route_rejections():
    assert route(514, 514) == (L.GPSIG_EUNSUPPORTED, (0, 0))
    assert route(513, 513, diff=0) == (L.GPSIG_EUNSUPPORTED, (0, 0))
    assert route(512, 512, diff=0) == (L.GPSIG_OK, (8, 64))
    assert route(10, 10, M=9) == (L.GPSIG_EUNSUPPORTED, (0, 0))
    assert route(10, 10, M=8) == (L.GPSIG_OK, (4, 16))
    assert route(1, 10)[0] == L.GPSIG_EINVAL and route(10, 1)[0] == L.GPSIG_EINVAL
    assert route(10, 10, M=0)[0] == L.GPSIG_EINVAL and route(10, 10, pm=5)[0] == L.GPSIG_EINVAL
    assert route(10, 11, pm=L.PAIRS_UPPER)[0] == L.GPSIG_EINVAL
    assert _lib().gpsig_sig_f64_route(10, 10, 4, 1, 0, None) == L.GPSIG_EINVAL
    with pytest.raises(L.GpsigError, match="513"):
        ops.f64_route(514, None, 4)


def test_precision_keyword():
    k = gpsig_amd.SignatureRBF(30, 3, 4)
    assert k.precision == "float32" and k._cfg()["precision"] == "float32"
    k = gpsig_amd.SignatureRBF(30, 3, 4, precision="float64")
    assert k._cfg()["precision"] == "float64"
    with pytest.raises(ValueError):
        gpsig_amd.SignatureRBF(30, 3, 4, precision="bad")
    with pytest.raises(ValueError):
        gpsig_amd.SignatureLinear(30, 3, 4, precision=None)
    with pytest.raises(NotImplementedError, match="float64"):
        gpsig_amd.SignatureRBF(30, 3, 4, order=2, precision="float64")
    # low_rank=True is torch float64 already and ignores the keyword
    k = gpsig_amd.SignatureRBF(30, 3, 4, low_rank=True, precision="float64")
    assert not k._f64()


def test_float64_tensor_methods_raise():
    k = gpsig_amd.SignatureRBF(30, 3, 4, precision="float64")
    Z = torch.zeros(10, 5, 3, dtype=torch.float64)
    X = torch.zeros(4, 30, dtype=torch.float64)
    with pytest.raises(NotImplementedError, match="float64"):
        k.K_tens(Z)
    with pytest.raises(NotImplementedError, match="float64"):
        k.K_tens_vs_seq(Z, X)
    with pytest.raises(NotImplementedError, match="float64"):
        k.K_tens_n_seq_covs(Z, X)


def test_cpu_tensors_raise():
    X = torch.zeros(4, 10, 3, dtype=torch.float64)
    with pytest.raises(L.GpsigError):
        ops.sig_gram_f64(X, None, 4)
    with pytest.raises(L.GpsigError):
        ops.sig_gram_f64(X, X.clone(), 4)
    with pytest.raises(L.GpsigError):
        ops.sig_diag_f64(X, 4)
    k = gpsig_amd.SignatureRBF(30, 3, 4, precision="float64")
    with pytest.raises(L.GpsigError):
        k.K(X.reshape(4, 30))
    k = gpsig_amd.SignatureRBF(30, 3, 4, normalization=False, precision="float64")
    with pytest.raises(L.GpsigError):
        k.Kdiag(X.reshape(4, 30))
