"""GPU parity of the float64 first-order Gram and diagonal (gpsig_sig_gram_f64 / gpsig_sig_diag_f64, and
SignatureKernel(..., precision="float64")) against the float64 CPU oracle (oracle/kernels_ref.py).

Bar: norm_rel_err < 1e-10 on every level.  The oracle's own distance from an 80-bit evaluation of the same
recursion is <= 7.9e-13 on walks like these (<= 1.9e-13 with the 1e3 offset), so 1e-10 leaves two orders over the
reference's floor and is five orders under the fp32 kernels' 1e-5.  Every check prints its figures before it
asserts.

The inputs are walks rounded to fp32 and handed over as float64, on a grid of 2^-12 (every grid value below 2^12
is an fp32 number).  The grid is what keeps the oracle at its floor: it takes r^2 as |x|^2 + |y|^2 - 2 <x, y>, which
is exact in double only while the sums of the 2^-24-grid products stay below 2^29 -- true here at every channel
count and with the 1e3 offset.  With plain fp32 rounding the sums round from about 6 channels on; at D = 46 the
oracle's r^2 between a point and itself is ~1e-16 instead of 0, its Matern-1/2 k there is 1 - 1e-8, and its K(X) is
1.66e-7 from an 80-bit evaluation of the same recursion (the form the kernel uses, r^2 from differences in double,
is 2.5e-16 from it; on the grid the oracle is back at 1.1e-14).
"""
import numpy as np
import pytest
import torch

from conftest import norm_rel_err
from oracle import autodiff_ref as ar
from oracle import kernels_ref as kr

pytestmark = pytest.mark.gpu
TOL = 1e-10
GTOL = 1e-5  # test_grad_gpu.py's bar for the gradients (the backward is the fp32 VJP launch)
DEV = "cuda"
BASES = ["rbf", "linear", "matern12", "matern32", "matern52"]
M5 = 5


def walks(n, l, d, seed, step=0.1, offset=0.0):
    """Random walks (n, l, d), rounded to fp32 on the 2^-12 grid (after the offset), as float64."""
    rng = np.random.default_rng(seed)
    X = np.cumsum(step * rng.standard_normal((n, l, d)), axis=1) + offset
    return on_grid(X)


def on_grid(X):
    X = (np.round(np.asarray(X) * 4096.0) / 4096.0).astype(np.float32)
    assert np.all(np.abs(X) < 4096.0)
    return X.astype(np.float64)


def dev(X):
    return torch.as_tensor(X, device=DEV)


def oracle(l, d, M, base, difference=True, **kw):
    return kr.SignatureKernelRef(l * d, d, M, base=base, difference=difference, **kw)


def check(name, got, ref, tol=TOL):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    assert got.dtype == np.float64 and got.shape == ref.shape, (name, got.dtype, got.shape, ref.shape)
    assert np.isfinite(got).all(), name
    err = norm_rel_err(got, ref, axis_levels=ref.ndim > 1)
    print(f"{name}: norm_rel_err {np.array2string(np.atleast_1d(err), precision=2)}")
    assert np.all(err < tol), (name, err)
    return float(np.max(err))


def forward_cases(X, Y, M, base, difference, tag):
    """K(X, Y), K(X) and the diagonal through ops against the oracle."""
    from gpsig_amd import ops
    ref = oracle(X.shape[1], X.shape[2], M, base, difference)
    check(f"{tag} K(X,Y)", ops.sig_gram_f64(dev(X), dev(Y), M, base, difference), ref.K_seq(X, Y))
    check(f"{tag} K(X)", ops.sig_gram_f64(dev(X), None, M, base, difference), ref.K_seq(X))
    check(f"{tag} diag", ops.sig_diag_f64(dev(X), M, base, difference), ref.K_seq_diag(X))


# ------------------------------------------------------------------------------------------------ routes
# each side of every seam of the (W, LP) table (cell columns 64 | 65, 128 | 129, 256 | 257), and L = 2, 3
ROUTES = [(2, (4, 16)), (3, (4, 16)), (65, (4, 16)), (66, (4, 32)), (129, (4, 32)), (130, (4, 64)), (257, (4, 64)),
          (258, (8, 64))]


@pytest.mark.parametrize("base", ["rbf", "linear", "matern32"])
@pytest.mark.parametrize("l,geo", ROUTES)
def test_routes(l, geo, base):
    from gpsig_amd import ops
    l1 = l + 3  # K(X, Y) with unequal lengths: the columns (Y) decide the route
    assert ops.f64_route(l, None, M5) == {"W": geo[0], "LP": geo[1]}
    assert ops.f64_route(l1, l, M5) == {"W": geo[0], "LP": geo[1]}
    step = 0.5 / np.sqrt(l)
    X, Y = walks(5, l, 3, 10 + l, step), walks(4, l, 3, 11 + l, step)
    ref = oracle(l, 3, M5, base)
    check(f"L={l} K(X)", ops.sig_gram_f64(dev(X), None, M5, base), ref.K_seq(X))
    check(f"L={l} diag", ops.sig_diag_f64(dev(X), M5, base), ref.K_seq_diag(X))
    X1 = walks(5, l1, 3, 12 + l, step)
    check(f"L={l1}x{l} K(X,Y)", ops.sig_gram_f64(dev(X1), dev(Y), M5, base), ref.K_seq(X1, Y))


@pytest.mark.parametrize("difference,l", [(True, 513), (False, 512)])
def test_route_cap(difference, l):
    from gpsig_amd import ops
    from gpsig_amd._lib import GpsigError
    M = 3
    assert ops.f64_route(l, None, M, difference) == {"W": 8, "LP": 64}
    assert ops.f64_route(l, l, M, difference) == {"W": 8, "LP": 64}
    step = 0.5 / np.sqrt(l)
    X, Y = walks(3, l, 2, 20, step), walks(2, l, 2, 21, step)
    forward_cases(X, Y, M, "rbf", difference, f"cap L={l}")
    with pytest.raises(GpsigError, match="513"):
        ops.sig_gram_f64(dev(walks(2, l + 1, 2, 22)), None, M, "rbf", difference)


# ------------------------------------------------------------------------------------------------ channels
@pytest.mark.parametrize("base", BASES)
@pytest.mark.parametrize("difference", [True, False])
@pytest.mark.parametrize("d", [1, 5, 46])
def test_channels(d, difference, base):
    step = 0.1 / np.sqrt(d)
    X, Y = walks(5, 33, d, 30 + d, step), walks(4, 20, d, 31 + d, step)
    forward_cases(X, Y, M5, base, difference, f"D={d} {base} diff={difference}")


@pytest.mark.parametrize("M", [1, 2, 8])
def test_levels(M):
    X, Y = walks(5, 33, 3, 40), walks(4, 20, 3, 41)
    forward_cases(X, Y, M, "rbf", True, f"M={M}")


# ------------------------------------------------------------------------------------------------ class level
@pytest.mark.parametrize("base", ["rbf", "linear", "matern52"])
def test_class_level(base):
    import gpsig_amd
    cls = {"rbf": gpsig_amd.SignatureRBF, "linear": gpsig_amd.SignatureLinear, "matern52": gpsig_amd.SignatureMatern52}[base]
    N, N2, L, D = 5, 4, 33, 3
    ls = np.array([0.7, 1.3, 1.1])
    var = np.array([0.5, 1.0, 2.0, 1.5, 0.8, 1.2])
    X, X2 = walks(N, L, D, 50).reshape(N, -1), walks(N2, L, D, 51).reshape(N2, -1)
    for normalization in (True, False):
        k = cls(L * D, D, M5, lengthscales=ls, variances=var, normalization=normalization, precision="float64")
        ref = oracle(L, D, M5, base, lengthscales=ls, variances=var, normalization=normalization)
        tag = f"{base} norm={normalization}"
        check(f"{tag} K levels", k.K(dev(X), return_levels=True), ref.K(X, return_levels=True))
        check(f"{tag} K sum", k.K(dev(X)), ref.K(X))
        check(f"{tag} K(X,X2)", k.K(dev(X), dev(X2)), ref.K(X, X2))
        check(f"{tag} K(X,X2) levels", k.K(dev(X), dev(X2), return_levels=True), ref.K(X, X2, return_levels=True))
        check(f"{tag} Kdiag levels", k.Kdiag(dev(X), return_levels=True), ref.Kdiag(X, return_levels=True))
        c, d = k.K_norms(dev(X))
        rc, rd = ref.K_norms(X)
        check(f"{tag} K_norms const", c, rc)
        check(f"{tag} K_norms diag", d, rd)
        for full in (False, True):
            got = k.K_seq_n_seq_covs(dev(X), dev(X2), full_X2_cov=full, return_levels=True)
            exp = ref.K_seq_n_seq_covs(X, X2, full_X2_cov=full, return_levels=True)
            for nm, g, e in zip(("Kxx", "Kxx2", "Kx2"), got, exp):
                check(f"{tag} K_seq_n_seq_covs full={full} {nm}", g, e)
    # a float32 input keeps today's dtype rule
    k = cls(L * D, D, M5, precision="float64")
    assert k.K(dev(X).float()).dtype == torch.float32 and k.K(dev(X)).dtype == torch.float64


# ------------------------------------------------------------------------------------------------ offset
@pytest.mark.parametrize("base", ["rbf", "linear", "matern52"])
def test_offset(base):
    """The same walks + 1e3 on every channel: float64 holds the bar; the fp32 path's error is printed beside it."""
    from gpsig_amd import ops
    X, Y = walks(5, 33, 5, 60, offset=1e3), walks(4, 20, 5, 61, offset=1e3)
    ref = oracle(33, 5, M5, base)
    for nm, (got32, r) in {"K(X,Y)": (ops.sig_gram(dev(X), dev(Y), M5, 1, base), ref.K_seq(X, Y)),
                           "K(X)": (ops.sig_gram(dev(X), None, M5, 1, base), ref.K_seq(X)),
                           "diag": (ops.sig_diag(dev(X), M5, 1, base), ref.K_seq_diag(X))}.items():
        e32 = norm_rel_err(got32.cpu().numpy(), r, axis_levels=True)
        print(f"offset 1e3 {base} {nm}: fp32 path norm_rel_err {np.array2string(e32, precision=2)} (not asserted)")
    forward_cases(X, Y, M5, base, True, f"offset 1e3 {base}")


# ------------------------------------------------------------------------------------------------ exactness
@pytest.mark.parametrize("base", ["rbf", "linear", "matern12"])
def test_exactness(base):
    from gpsig_amd import _lib as L
    from gpsig_amd import ops
    N, l, D = 37, 20, 3
    X = walks(N, l, D, 70)
    Xd = dev(X)
    K = ops.sig_gram_f64(Xd, None, M5, base)
    assert torch.equal(K, K.transpose(1, 2)), "K(X) equals its transpose bitwise"
    S = torch.tensor([1, 2, 6, 7, 11, 18, 19, 23, 30, 36], device=DEV)
    KS = ops.sig_gram_f64(Xd[S].contiguous(), None, M5, base)
    assert torch.equal(K[:, S][:, :, S], KS), "K(X)[S][:, S] equals K(X[S]) bitwise"
    # row windows against the slices of the full call, raw and with the fused epilogue
    ref = oracle(l, D, M5, base)
    var = np.array([0.5, 1.0, 2.0, 1.5, 0.8, 1.2])
    Kref = kr.SignatureKernelRef(l * D, D, M5, base=base, variances=var).K(X.reshape(N, -1), return_levels=True)
    rs = ops.sig_diag_f64(Xd, M5, base, jitter=1e-6, rsqrt=True)
    kw = dict(rs1=rs, rs2=rs, scale=dev(var), jitter=1e-6)
    full = {L.OUT_LEVELS: K,
            L.OUT_NORM_LEVELS: ops.sig_gram_f64(Xd, None, M5, base, out_mode=L.OUT_NORM_LEVELS, **kw),
            L.OUT_NORM_SUM: ops.sig_gram_f64(Xd, None, M5, base, out_mode=L.OUT_NORM_SUM, **kw)}
    check(f"{base} raw K", K, ref.K_seq(X))
    check(f"{base} NORM_LEVELS", full[L.OUT_NORM_LEVELS], Kref)
    check(f"{base} NORM_SUM", full[L.OUT_NORM_SUM], Kref.sum(0))
    for mode, Kf in full.items():
        for r0, r1 in [(0, 9), (9, 21), (21, 37), (3, 4)]:
            w = ops.sig_gram_f64(Xd, None, M5, base, rows=(r0, r1), out_mode=mode, **({} if mode == L.OUT_LEVELS else kw))
            # UPPER evaluates b >= a; the window's rows hold their columns b >= r0 and the mirrors inside it
            assert torch.equal(w[..., :, r0:], Kf[..., r0:r1, r0:]), (mode, r0, r1)
    Y = dev(walks(6, 17, D, 71))
    KR = ops.sig_gram_f64(Xd, Y, M5, base)
    for r0, r1 in [(0, 9), (9, 21), (21, 37), (3, 4)]:
        assert torch.equal(ops.sig_gram_f64(Xd, Y, M5, base, rows=(r0, r1)), KR[:, r0:r1]), (r0, r1)


# ------------------------------------------------------------------------------------------------ degenerate
@pytest.mark.parametrize("base", BASES)
def test_degenerate(base):
    from gpsig_amd import ops
    N, l, D = 5, 20, 3
    X = walks(N, l, D, 80)
    X[1, 5] = X[1, 4]          # repeated consecutive points
    X[1, 6] = X[1, 4]
    X[2, -1] = X[2, -2]
    X[3] += 40.0               # one sequence 40 lengthscales away
    X[4] = X[4, 0]             # a constant sequence
    X = on_grid(X)
    Y = walks(4, 17, D, 81)
    ref = oracle(l, D, M5, base)
    forward_cases(X, Y, M5, base, True, f"degenerate {base}")
    Xd = dev(X)
    check(f"degenerate {base} K(X, X.clone())", ops.sig_gram_f64(Xd, Xd.clone(), M5, base), ref.K_seq(X, X))
    K = ops.sig_gram_f64(Xd, None, M5, base)
    d = ops.sig_diag_f64(Xd, M5, base)
    assert torch.all(K[0] == 1.0) and torch.all(d[0] == 1.0)
    assert torch.all(K[1:, 4, :] == 0.0) and torch.all(K[1:, :, 4] == 0.0) and torch.all(d[1:, 4] == 0.0), \
        "a constant sequence: every level past 0 is exactly 0"
    # empty batches
    E = torch.empty((0, l, D), dtype=torch.float64, device=DEV)
    assert ops.sig_gram_f64(E, None, M5, base).shape == (M5 + 1, 0, 0)
    assert ops.sig_gram_f64(E, Xd, M5, base).shape == (M5 + 1, 0, N)
    assert ops.sig_gram_f64(Xd, E, M5, base).shape == (M5 + 1, N, 0)
    assert ops.sig_diag_f64(E, M5, base).shape == (M5 + 1, 0)
    assert ops.sig_gram_f64(Xd, None, M5, base, rows=(2, 2)).shape == (M5 + 1, 0, N)


# ------------------------------------------------------------------------------------------------ gradient
def _grads(out, G, leaves):
    (out * G).sum().backward()
    return [t.grad.detach().cpu().numpy() for t in leaves]


@pytest.mark.parametrize("base", ["rbf", "linear"])
@pytest.mark.parametrize("case", ["K(X).sum", "K(X,X2)", "Kdiag"])
def test_gradient(base, case):
    import gpsig_amd
    N, N2, L, L2, D, M = 6, 4, 24, 17, 3, 4
    X, X2 = walks(N, L, D, 90), walks(N2, L2, D, 91)
    ls = np.array([0.7, 1.3, 1.1])
    var = np.array([0.5, 1.0, 2.0, 1.5, 0.8])
    cls = gpsig_amd.SignatureRBF if base == "rbf" else gpsig_amd.SignatureLinear
    normalization = case != "Kdiag"
    k = cls(L * D, D, M, lengthscales=ls, variances=var, normalization=normalization, precision="float64")
    k.lengthscales = torch.tensor(ls, device=DEV, requires_grad=True)
    k.variances = torch.tensor(var, device=DEV, requires_grad=True)
    Xt = torch.tensor(X.reshape(N, -1), device=DEV, requires_grad=True)
    X2t = torch.tensor(X2.reshape(N2, -1), device=DEV, requires_grad=True)
    Xr, X2r = torch.tensor(X, requires_grad=True), torch.tensor(X2, requires_grad=True)
    lsr, varr = torch.tensor(ls, requires_grad=True), torch.tensor(var, requires_grad=True)
    rng = np.random.default_rng(92)
    if case == "K(X).sum":
        G = np.ones((N, N))
        got, ref = k.K(Xt), ar.K(Xr / lsr, None, M, base=base, scale=varr)
        names, leaves, rleaves = ("dX", "dls", "dvar"), [Xt, k.lengthscales, k.variances], [Xr, lsr, varr]
    elif case == "K(X,X2)":
        G = rng.standard_normal((N, N2))
        got, ref = k.K(Xt, X2t), ar.K(Xr / lsr, X2r / lsr, M, base=base, scale=varr)
        names = ("dX", "dX2", "dls", "dvar")
        leaves, rleaves = [Xt, X2t, k.lengthscales, k.variances], [Xr, X2r, lsr, varr]
    else:
        G = rng.standard_normal((N,))
        got = k.Kdiag(Xt)
        ref = (ar.k_seq_diag(Xr / lsr, M, base=base) * varr[:, None]).sum(0)
        names, leaves, rleaves = ("dX", "dls", "dvar"), [Xt, k.lengthscales, k.variances], [Xr, lsr, varr]
    assert got.dtype == torch.float64
    check(f"{base} {case} forward", got.detach(), ref.detach().numpy())
    gg = _grads(got, torch.as_tensor(G, device=DEV), leaves)
    gr = _grads(ref, torch.as_tensor(G), rleaves)
    for nm, g, r in zip(names, gg, gr):
        err = norm_rel_err(g.reshape(r.shape), r)
        print(f"{base} {case} gradient {nm}: norm_rel_err {err:.2e}")
        assert g.dtype == np.float64
        assert err < GTOL, (nm, err)


def test_matern_backward_raises():
    import gpsig_amd
    N, L, D, M = 4, 12, 2, 3
    Xt = torch.tensor(walks(N, L, D, 95).reshape(N, -1), device=DEV, requires_grad=True)
    k = gpsig_amd.SignatureMatern32(L * D, D, M, precision="float64")
    K = k.K(Xt)
    with pytest.raises(NotImplementedError):
        K.sum().backward()
    k = gpsig_amd.SignatureMatern32(L * D, D, M, normalization=False, precision="float64")
    with pytest.raises(NotImplementedError):
        k.Kdiag(Xt).sum().backward()
