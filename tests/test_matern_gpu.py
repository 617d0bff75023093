"""GPU parity of the Matern 1/2, 3/2, 5/2 signature kernels (the radial seed, gpsig_amd/csrc/sig_common.h
RadialSeed and wide.h RadialSeedWide) against the float64 oracle on the fp32-rounded inputs.

Criterion as tests/test_gram_gpu.py: norm-relative max|K32 - K64| < 1e-5 * max|K64| per level.
Every check prints its figures before it asserts.
"""
import numpy as np
import pytest
import torch

from conftest import norm_rel_err
from oracle import kernels_ref as kr

pytestmark = pytest.mark.gpu
TOL = 1e-5
DEV = "cuda"
BASES = ["matern12", "matern32", "matern52"]


def t(x):
    return torch.as_tensor(np.asarray(x), device=DEV)


def walks(rng, n, L, D, step):
    """Random walks with per-coordinate steps of size `step`, rounded to fp32 (returned as float64)."""
    return (np.cumsum(rng.standard_normal((n, L, D)), 1) * step).astype(np.float32).astype(np.float64)


def cls_of(base):
    import gpsig_amd
    return {"matern12": gpsig_amd.SignatureMatern12, "matern32": gpsig_amd.SignatureMatern32,
            "matern52": gpsig_amd.SignatureMatern52}[base]


def check(what, got, ref, levels=True):
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    assert np.isfinite(got).all(), what
    err = norm_rel_err(got, ref, axis_levels=levels)
    print(f"{what}: err {np.array2string(np.atleast_1d(err), precision=2)}")
    assert (np.atleast_1d(err) < TOL).all(), (what, err)
    return err


def raw_checks(base, X, Y, M, order=1, difference=True):
    """Raw levels of K(X, Y), K(X) and the diagonal through ops against the oracle's recursion."""
    from gpsig_amd import ops
    D = X.shape[-1]
    ref = kr.SignatureKernelRef(X.shape[1] * D, D, M, base=base, order=order, normalization=False,
                                difference=difference)
    kw = dict(order=ref.order, base=base, difference=difference)
    tag = f"{base} D={D} L={X.shape[1]} order={ref.order}"
    check(f"{tag} K(X,Y)", ops.sig_gram(t(X), t(Y), M, **kw), ref.K_seq(X, Y))
    sym = ops.sig_gram(t(X), None, M, **kw)
    check(f"{tag} K(X)", sym, ref.K_seq(X))
    assert torch.equal(sym, sym.transpose(1, 2))
    check(f"{tag} diag", ops.sig_diag(t(X), M, **kw), ref.K_seq_diag(X))


@pytest.mark.parametrize("step", [0.03, 0.3])
@pytest.mark.parametrize("D", [2, 5, 7, 8])
@pytest.mark.parametrize("base", BASES)
def test_first_order_fixed_channels(base, D, step):
    """The fixed-channel instantiations (D = 7 runs padded to 8): cross Gram of unequal lengths through ops, then
    the class: K(X) per level, K(X, X2), the normalised sum, the unnormalised Kdiag, lengthscales, variances."""
    rng = np.random.default_rng(100 * D + int(step * 100))
    N, N2, M, L, L2 = 6, 4, 5, 33, 20
    X = walks(rng, N, L, D, step)
    Y = walks(rng, N2, L2, D, step)
    raw_checks(base, X, Y, M)
    X2 = walks(rng, N2, L, D, step)
    ls = rng.uniform(0.6, 1.8, D)
    var = rng.uniform(0.5, 1.5, M + 1)
    Xf, X2f = X.reshape(N, -1), X2.reshape(N2, -1)
    for kw in (dict(), dict(lengthscales=ls, variances=var)):
        k = cls_of(base)(L * D, D, M, **kw)
        ref = kr.SignatureKernelRef(L * D, D, M, base=base, **kw)
        Kl = k.K(t(Xf), return_levels=True)
        check(f"{base} D={D} K(X) levels {sorted(kw)}", Kl, ref.K(Xf, return_levels=True))
        assert torch.equal(Kl, Kl.transpose(1, 2))  # K(X) equals its transpose exactly
        check(f"{base} D={D} K(X,X2) levels", k.K(t(Xf), t(X2f), return_levels=True), ref.K(Xf, X2f, return_levels=True))
        check(f"{base} D={D} K(X) sum", k.K(t(Xf)), ref.K(Xf), levels=False)
        ku = cls_of(base)(L * D, D, M, normalization=False, **kw)
        refu = kr.SignatureKernelRef(L * D, D, M, base=base, normalization=False, **kw)
        check(f"{base} D={D} Kdiag unnormalised", ku.Kdiag(t(Xf), return_levels=True), refu.Kdiag(Xf, return_levels=True))
        check(f"{base} D={D} compute_K_levels", ku.compute_K_levels(Xf, X2f), refu.K(Xf, X2f, return_levels=True))


@pytest.mark.parametrize("L", [2, 3, 17, 65, 129])
@pytest.mark.parametrize("base", BASES)
def test_geometry_edges(base, L):
    """Shortest sequences, one past a lane group's 16 / 64 / 128 columns."""
    rng = np.random.default_rng(L)
    X = walks(rng, 5, L, 3, 0.1)
    Y = walks(rng, 3, L, 3, 0.1)
    raw_checks(base, X, Y, 4)


@pytest.mark.parametrize("base", BASES)
def test_column_blocks(base):
    """L = 520: past the 512 points one lane group holds, so two column blocks with a halo column."""
    rng = np.random.default_rng(520)
    X = walks(rng, 3, 520, 2, 0.03)
    Y = walks(rng, 2, 520, 2, 0.03)
    raw_checks(base, X, Y, 3)


@pytest.mark.parametrize("L", [40, 70])
@pytest.mark.parametrize("D", [9, 20, 46])
@pytest.mark.parametrize("base", BASES)
def test_wide_channel_loop(base, D, L):
    """Past 8 channels: the runtime channel loop, 39 and 69 cell rows (no multiple of its 8-row chunks), at the
    lengths on either side of the wide kernels' 64-point switch (W = 4 / W = 8 for the RBF seed; the radial seed
    runs W = 8 at both, on 16 lanes, with 33 / 63 columns of Y in use)."""
    rng = np.random.default_rng(D * 100 + L)
    step = 0.3 / np.sqrt(D)
    X = walks(rng, 4, L, D, step)
    Y = walks(rng, 3, L - 7, D, step)
    raw_checks(base, X, Y, 4)
    k = cls_of(base)(L * D, D, 4, normalization=False)
    refu = kr.SignatureKernelRef(L * D, D, 4, base=base, normalization=False)
    check(f"{base} D={D} L={L} Kdiag", k.Kdiag(t(X.reshape(4, -1))), refu.Kdiag(X.reshape(4, -1)), levels=False)


@pytest.mark.parametrize("order,M", [(2, 4), (3, 4), (4, 4)])
@pytest.mark.parametrize("D", [3, 12])
@pytest.mark.parametrize("base", BASES)
def test_higher_order(base, D, order, M):
    rng = np.random.default_rng(D * 10 + order)
    N, L = 4, 30
    step = 0.3 / np.sqrt(D)
    X = walks(rng, N, L, D, step)
    Y = walks(rng, 3, L, D, step)
    raw_checks(base, X, Y, M, order=order)
    k = cls_of(base)(L * D, D, M, order=order)
    ref = kr.SignatureKernelRef(L * D, D, M, base=base, order=order)
    check(f"{base} D={D} order={order} K(X)", k.K(t(X.reshape(N, -1))), ref.K(X.reshape(N, -1)), levels=False)


@pytest.mark.parametrize("base", BASES)
def test_higher_order_column_blocks(base):
    """Order 5 keeps 2 columns per lane: 140 points run in two column blocks of the higher-order kernel."""
    rng = np.random.default_rng(140)
    X = walks(rng, 3, 140, 3, 0.05)
    Y = walks(rng, 2, 140, 3, 0.05)
    raw_checks(base, X, Y, 5, order=5)


@pytest.mark.parametrize("D", [3, 12])
@pytest.mark.parametrize("base", BASES)
def test_point_seed(base, D):
    """difference=False: the recursion over the k grid itself."""
    rng = np.random.default_rng(D)
    step = 0.3 / np.sqrt(D)
    X = walks(rng, 4, 25, D, step)
    Y = walks(rng, 3, 25, D, step)
    raw_checks(base, X, Y, 4, difference=False)


@pytest.mark.parametrize("base", BASES)
def test_degenerate_inputs(base):
    """Repeated consecutive points (r1 + r0 = 0 on self pairs), K(X, X.clone()) (r = 0 on the cross route), and a
    batch where one sequence sits 40 lengthscales away (k underflows): finite everywhere, the batch within the
    bar as a whole."""
    rng = np.random.default_rng(11)
    N, L, D, M = 5, 24, 3, 4
    X = walks(rng, N, L, D, 0.1)
    X[:, 10:13] = X[:, 10:11]
    X[:, -3:] = X[:, -3:-2]
    X[3, :, 0] += 40.0
    X = X.astype(np.float32).astype(np.float64)
    Xf = X.reshape(N, -1)
    raw_checks(base, X, X.copy(), M)
    k = cls_of(base)(L * D, D, M)
    ref = kr.SignatureKernelRef(L * D, D, M, base=base)
    Xt = t(Xf)
    check(f"{base} K(X, X.clone())", k.K(Xt, Xt.clone(), return_levels=True), ref.K(Xf, Xf.copy(), return_levels=True))
    check(f"{base} K(X)", k.K(Xt, return_levels=True), ref.K(Xf, return_levels=True))
    ku = cls_of(base)(L * D, D, M, normalization=False)
    refu = kr.SignatureKernelRef(L * D, D, M, base=base, normalization=False)
    check(f"{base} Kdiag", ku.Kdiag(Xt, return_levels=True), refu.Kdiag(Xf, return_levels=True))
    # a constant sequence: every cell is exactly zero, the kernel is level 0 alone
    C = np.tile(X[:1, :1], (2, L, 1))
    from gpsig_amd import ops
    Kc = ops.sig_gram(t(C), None, M, base=base).cpu().numpy()
    assert (Kc[0] == 1.0).all() and (Kc[1:] == 0.0).all()


@pytest.mark.parametrize("base", BASES)
def test_autograd_and_unsupported_routes(base):
    import gpsig_amd
    rng = np.random.default_rng(3)
    N, L, D, M = 4, 12, 3, 3
    Xf = t(walks(rng, N, L, D, 0.2).reshape(N, -1))
    k = cls_of(base)(L * D, D, M, lengthscales=[1.0, 1.5, 0.7])
    K0 = k.K(Xf)
    Kd0 = cls_of(base)(L * D, D, M, normalization=False).Kdiag(Xf)
    k.to(DEV)
    k.lengthscales.requires_grad_()
    K1 = k.K(Xf)
    assert K1.requires_grad and torch.equal(K1.detach(), K0)
    with pytest.raises(NotImplementedError, match="VJP"):
        K1.sum().backward()
    K2 = k.K(Xf, Xf[:2].clone())
    with pytest.raises(NotImplementedError, match="VJP"):
        K2.sum().backward()
    ku = cls_of(base)(L * D, D, M, normalization=False)
    Xg = Xf.clone().requires_grad_()
    Kd = ku.Kdiag(Xg)
    assert torch.equal(Kd.detach(), Kd0)
    with pytest.raises(NotImplementedError, match="VJP"):
        Kd.sum().backward()
    Z = t(rng.standard_normal((M * (M + 1) // 2, 5, D)))
    with pytest.raises(NotImplementedError):
        k.K_tens(Z)
    with pytest.raises(NotImplementedError):
        k.K_tens_vs_seq(Z, Xf)
    kh = cls_of(base)(L * 40, 40, 4, order=2)
    with pytest.raises(gpsig_amd.GpsigError):
        kh.K(t(walks(rng, 2, L, 40, 0.1).reshape(2, -1)))


@pytest.mark.parametrize("base", BASES)
def test_low_rank_mode_uses_the_host_base_kernel(base):
    """low_rank=True runs on torch GEMMs through _base_kern: with Nystrom on all points level 1 has no projection
    and equals the exact kernel's level 1 (tolerance as tests/test_low_rank.py: 1e-3 of the level's maximum, the
    eigh-based Nystrom map in fp64); the inducing-tensor entry points work there too."""
    rng = np.random.default_rng(5)
    N, L, D, M = 4, 6, 2, 3
    Xt = t(walks(rng, N, L, D, 0.4).reshape(N, -1))
    exact = cls_of(base)(L * D, D, M, normalization=False).K(Xt, return_levels=True).cpu()
    k = cls_of(base)(L * D, D, M, normalization=False, low_rank=True, num_components=N * L, rank_bound=24)
    torch.manual_seed(7)
    Kl = k.K(Xt, return_levels=True).cpu()
    assert Kl.shape == exact.shape and torch.isfinite(Kl).all()
    dev = (Kl[1] - exact[1]).abs().max().item()
    print(f"{base} low-rank level 1: dev {dev:.2e} of {exact[1].abs().max().item():.2e}")
    assert dev < 1e-3 * exact[1].abs().max().item()
    Z = t(rng.standard_normal((M * (M + 1) // 2, 5, D)))
    assert k.K_tens(Z).shape == (5, 5) and k.K_tens_vs_seq(Z, Xt).shape == (5, N)
