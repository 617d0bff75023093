"""GPU parity of the VOSF rescaled kernel's gradient (gpsig_rescaled_vjp, gpsig_amd/csrc/sig_rescaled_bwd.h
rescaled_bwd_kernel<level, W, embedding>) against the float64 autodiff restatement (tests/rescaled_autodiff.py)
on the fp32-rounded inputs.

The kernel is compiled per level 1..6 for W in {1, 2, 4 (level <= 4)} columns per lane (L - 1 <= 64 / 128 / 256)
and both embeddings; a call with M levels runs the levels 1..M, and the channel loop is a runtime loop.

Criterion (the GTOL of every gradient test): max|g32 - g64| < 1e-5 * max|g64| per gradient array.
Every check prints its figure before it asserts, next to the fp32 reference: the restatement's recursion run in
float32 on the float64 second differences rounded to fp32, chained back in float64 (rescaled_autodiff.grads_fp32).
The cases were chosen so that this reference stays at or below a third of the bar.  With Z ~ U[0.97, 0.999] the
output K(ones) - K(t) cancels and dX is held to 1e-5 of the gradient of the minuend alone (sum |gout| K(ones),
the restatement at Z = 0 with weights |gout|); the fp32 reference is off by up to 1.5e-5 of the difference's own
gradient there and below 3e-7 of the minuend's.
"""

import numpy as np
import pytest
import torch

import rescaled_autodiff as ra

pytestmark = pytest.mark.gpu
GTOL = 1e-5
DEV = "cuda"
EMBEDDINGS = ["linear", "rbf"]


def t(x):
    return torch.as_tensor(np.asarray(x), device=DEV)


def f32(x):
    return np.asarray(x).astype(np.float32).astype(np.float64)


def walks(rng, n, L, D, step=None):
    """Random walks with per-coordinate steps of size `step` (1/sqrt(L) by default), rounded to fp32."""
    step = 1.0 / np.sqrt(L) if step is None else step
    return f32(np.cumsum(rng.standard_normal((n, L, D)), 1) * step)


def tensors(rng, M, T, D, lo=0.1, hi=0.9):
    return f32(rng.uniform(lo, hi, (M * (M + 1) // 2, T, D)))


def upstream(rng, M, N, T):
    return f32(rng.standard_normal((M + 1, N, T)))


def rel(got, ref, scale=None):
    scale = np.abs(ref).max() if scale is None else scale
    return np.abs(got - ref).max() / scale


def run(emb, Z, X, M, gout):
    from gpsig_amd import ops
    gZ, gX = ops.rescaled_vjp(t(Z), t(X), M, t(gout), embedding=emb)
    assert gZ.shape == Z.shape and gX.shape == X.shape
    assert gZ.dtype == torch.float32 and gX.dtype == torch.float32
    gZ, gX = gZ.cpu().numpy().astype(np.float64), gX.cpu().numpy().astype(np.float64)
    assert np.isfinite(gZ).all() and np.isfinite(gX).all()
    return gZ, gX


def check(what, emb, Z, X, M, gout, x_scale=None):
    """dZ and dX of ops.rescaled_vjp within the bar of the restatement; x_scale replaces max|dX| in dX's bar."""
    N, L, D = X.shape
    rZ, rX = ra.grads(emb, Z, X, M, gout)
    fZ, fX = ra.grads_fp32(emb, Z, X, M, gout)
    gZ, gX = run(emb, Z, X, M, gout)
    tag = f"{what} {emb} M={M} L={L} D={D} N={N} T={Z.shape[1]}"
    eZ, eX = rel(gZ, rZ), rel(gX, rX, x_scale)
    print(f"{tag}: kernel dZ {eZ:.2e} dX {eX:.2e}")
    print(f"{tag}: reference in fp32 dZ {rel(fZ, rZ):.2e} dX {rel(fX, rX, x_scale):.2e}")
    assert eZ < GTOL, (tag, "dZ", eZ)
    assert eX < GTOL, (tag, "dX", eX)
    return (gZ, gX), (rZ, rX)


# ----------------------------------------------------------------------------- every instantiation
@pytest.mark.parametrize("D", [3, 7, 12])
@pytest.mark.parametrize("M,L", [(m, l) for m in range(1, 7) for l in (40, 100, 200) if l < 200 or m <= 4])
@pytest.mark.parametrize("emb", EMBEDDINGS)
def test_every_band(emb, M, L, D):
    """Levels 1..M at W = 1 / 2 / 4 columns per lane, channel counts below, between and above 4 and 8."""
    rng = np.random.default_rng(1000 * M + 10 * L + D)
    N, T = 2, 2
    check("band", emb, tensors(rng, M, T, D), walks(rng, N, L, D), M, upstream(rng, M, N, T))


# ----------------------------------------------------------------------------- seams
@pytest.mark.parametrize("M,D,L", [(4, 3, L) for L in (2, 3, 65, 66, 129, 130, 257)] + [(6, 5, 129)])
@pytest.mark.parametrize("emb", EMBEDDINGS)
def test_length_seams(emb, M, D, L):
    """One and two increments, and L - 1 on either side of 64 / 128 / 256 columns, up to the longest length."""
    rng = np.random.default_rng(100 * L + M)
    N, T = 2, 2
    check("length", emb, tensors(rng, M, T, D), walks(rng, N, L, D), M, upstream(rng, M, N, T))


@pytest.mark.parametrize("D", [1, 4, 5, 8, 9])
@pytest.mark.parametrize("emb", EMBEDDINGS)
def test_channel_seams(emb, D):
    M, L, N, T = 3, 70, 2, 2
    rng = np.random.default_rng(70 + D)
    check("channels", emb, tensors(rng, M, T, D), walks(rng, N, L, D), M, upstream(rng, M, N, T))


@pytest.mark.parametrize("emb", EMBEDDINGS)
def test_channels_past_the_lds(emb):
    """7000 channels: the gZ / gX accumulators no longer fit the LDS, the row sums leave as atomics at once."""
    M, L, D, N, T = 2, 3, 7000, 1, 1
    rng = np.random.default_rng(7)
    check("wide", emb, tensors(rng, M, T, D), walks(rng, N, L, D, step=0.05), M, upstream(rng, M, N, T))


@pytest.mark.parametrize("N,T", [(1, 1), (3, 1), (1, 3), (3, 2)])
@pytest.mark.parametrize("emb", EMBEDDINGS)
def test_batch_seams(emb, N, T):
    """One tensor, one sequence: the ones tensor's weight sum_t gout and the (n, t') block decomposition."""
    M, L, D = 3, 66, 5
    rng = np.random.default_rng(10 * N + T)
    check("batch", emb, tensors(rng, M, T, D), walks(rng, N, L, D), M, upstream(rng, M, N, T))


# ----------------------------------------------------------------------------- cancelling regime
@pytest.mark.parametrize("M,L,D", [(4, 40, 3), (6, 66, 5)])
@pytest.mark.parametrize("emb", EMBEDDINGS)
def test_cancelling_regime(emb, M, L, D):
    """Lambda close to 1: dZ to the plain bar, dX to 1e-5 of the minuend's gradient."""
    rng = np.random.default_rng(L * M)
    N, T = 2, 2
    X, Z, gout = walks(rng, N, L, D), tensors(rng, M, T, D, 0.97, 0.999), upstream(rng, M, N, T)
    scale = np.abs(ra.minuend_grad_X(emb, X, M, gout, T, D)).max()
    (_, gX), (_, rX) = check("cancelling", emb, Z, X, M, gout, x_scale=scale)
    print(f"cancelling {emb} M={M}: dX of the difference itself {rel(gX, rX):.2e}")


# ----------------------------------------------------------------------------- structure
@pytest.mark.parametrize("M,L,D", [(4, 40, 3), (3, 100, 7)])
@pytest.mark.parametrize("emb", EMBEDDINGS)
def test_ones_tensor(emb, M, L, D):
    """Z = ones: K(ones) - K(t) vanishes identically in X, so dX is zero to 1e-5 of the minuend's gradient."""
    rng = np.random.default_rng(M)
    N, T = 2, 2
    X, gout = walks(rng, N, L, D), upstream(rng, M, N, T)
    Z = np.ones((M * (M + 1) // 2, T, D))
    scale = np.abs(ra.minuend_grad_X(emb, X, M, gout, T, D)).max()
    (_, gX), _ = check("ones", emb, Z, X, M, gout, x_scale=scale)
    print(f"ones {emb} M={M}: max|dX| / max|dX minuend| {np.abs(gX).max() / scale:.2e}")
    assert np.abs(gX).max() < GTOL * scale


@pytest.mark.parametrize("M,L,D", [(4, 40, 3), (3, 100, 7)])
@pytest.mark.parametrize("emb", EMBEDDINGS)
def test_zero_tensor(emb, M, L, D):
    """Z = 0: K(t) vanishes, dX is the minuend's gradient with the weights sum_t gout."""
    rng = np.random.default_rng(M + L)
    N, T = 2, 2
    X, gout = walks(rng, N, L, D), upstream(rng, M, N, T)
    Z = np.zeros((M * (M + 1) // 2, T, D))
    check("zero", emb, Z, X, M, gout)


@pytest.mark.parametrize("emb", EMBEDDINGS)
def test_constant_sequence(emb):
    """No increments: every seed is zero; the gradients are finite and within 1e-5 max(|ref|, 1e-3)."""
    M, L, D, N, T = 4, 40, 3, 2, 2
    rng = np.random.default_rng(L)
    X = np.tile(f32(rng.standard_normal((N, 1, D))), (1, L, 1))
    Z, gout = tensors(rng, M, T, D), upstream(rng, M, N, T)
    rZ, rX = ra.grads(emb, Z, X, M, gout)
    gZ, gX = run(emb, Z, X, M, gout)
    for name, g, r in (("dZ", gZ, rZ), ("dX", gX, rX)):
        bar = GTOL * max(np.abs(r).max(), 1e-3)
        print(f"constant {emb} {name}: max|ref| {np.abs(r).max():.2e} max|diff| {np.abs(g - r).max():.2e} bar {bar:.1e}")
        assert np.abs(g - r).max() < bar


@pytest.mark.parametrize("emb", EMBEDDINGS)
def test_large_steps(emb):
    """Steps of size 1: the RBF seed leaves its expm1 form for the corner form."""
    M, L, D, N, T = 3, 40, 3, 2, 2
    rng = np.random.default_rng(17)
    check("large steps", emb, tensors(rng, M, T, D), walks(rng, N, L, D, step=1.0), M, upstream(rng, M, N, T))


@pytest.mark.parametrize("emb", EMBEDDINGS)
def test_level_zero_of_gout_is_ignored(emb):
    """Level 0 of the output is the constant 0: a NaN there reaches nothing.  The two runs differ by the order of
    the fp32 atomics only ((T + 1) M addends per element: a few ulp)."""
    M, L, D, N, T = 3, 40, 3, 2, 2
    rng = np.random.default_rng(5)
    Z, X, gout = tensors(rng, M, T, D), walks(rng, N, L, D), upstream(rng, M, N, T)
    a = run(emb, Z, X, M, gout)
    g0 = gout.copy()
    g0[0] = np.nan
    b = run(emb, Z, X, M, g0)
    for name, u, v in (("dZ", a[0], b[0]), ("dX", a[1], b[1])):
        print(f"level 0 {emb} {name}: {rel(v, u):.2e}")
        assert rel(v, u) < 1e-6


@pytest.mark.parametrize("emb", [0, 1])
def test_abi_accumulates(emb):
    """gpsig_rescaled_vjp adds into gZ and gX: a second call into the same buffers doubles them (up to the order
    of the fp32 atomics)."""
    import gpsig_amd._lib as L_
    from gpsig_amd import ops
    lib = L_.load()
    M, L, D, N, T = 3, 70, 5, 2, 2
    rng = np.random.default_rng(9)
    Z, X, gout = (t(a).float().contiguous() for a in (tensors(rng, M, T, D), walks(rng, N, L, D), upstream(rng, M, N, T)))
    gZ, gX = torch.zeros_like(Z), torch.zeros_like(X)
    ws = ops.workspace(X.device, lib.gpsig_rescaled_workspace_bytes(N, M))

    def call():
        rc = lib.gpsig_rescaled_vjp(Z.data_ptr(), M * (M + 1) // 2, T, X.data_ptr(), N, L, D, M, emb, gout.data_ptr(),
                                    gZ.data_ptr(), gX.data_ptr(), ws.data_ptr(), ws.numel(), ops._stream(X.device))
        assert rc == 0
        torch.cuda.synchronize()
    call()
    z1, x1 = gZ.cpu().numpy().astype(np.float64), gX.cpu().numpy().astype(np.float64)
    call()
    z2, x2 = gZ.cpu().numpy().astype(np.float64), gX.cpu().numpy().astype(np.float64)
    assert np.abs(z1).max() > 0 and np.abs(x1).max() > 0
    print(f"accumulate emb={emb}: dZ {rel(z2, 2 * z1):.2e} dX {rel(x2, 2 * x1):.2e}")
    assert rel(z2, 2 * z1) < 1e-6 and rel(x2, 2 * x1) < 1e-6


def test_shape_mismatches_raise():
    from gpsig_amd import ops
    M = 3
    X = torch.zeros((2, 10, 4), device=DEV)
    g = torch.zeros((M + 1, 2, 2), device=DEV)
    with pytest.raises(ValueError, match="channel"):
        ops.rescaled_vjp(torch.zeros((6, 2, 3), device=DEV), X, M, g)
    with pytest.raises(ValueError, match="components"):
        ops.rescaled_vjp(torch.zeros((5, 2, 4), device=DEV), X, M, g)
    with pytest.raises(ValueError, match="gout"):
        ops.rescaled_vjp(torch.zeros((6, 2, 4), device=DEV), X, M, g[:, :1])


@pytest.mark.parametrize("M,L", [(4, 258), (5, 130), (7, 10)])
def test_unsupported_shapes_raise(M, L):
    import gpsig_amd
    from gpsig_amd import ops
    X = torch.zeros((2, L, 3), device=DEV)
    Z = torch.full((M * (M + 1) // 2, 2, 3), 0.5, device=DEV)
    with pytest.raises(gpsig_amd.GpsigError):
        ops.rescaled_vjp(Z, X, M, torch.ones((M + 1, 2, 2), device=DEV))


# ----------------------------------------------------------------------------- kernel classes
def class_case(rng, N, T, L, D, M, lo=0.1, hi=0.9):
    X = walks(rng, N, L, D)
    ls = np.linspace(0.7, 1.6, D)
    Zfull = np.concatenate([f32(rng.uniform(0.3, 0.9, (1, T, D))), tensors(rng, M, T, D, lo, hi)], axis=0)
    return X, ls, Zfull


def class_reference(emb, Zfull, X, ls, M, sigma):
    """out.sum() of the method in float64: sigma sum_i rescaled(Z[1:], X / ls)_i + 1 - Z[0, :, 0]."""
    Zt = torch.tensor(Zfull, requires_grad=True)
    Xt = torch.tensor(X, requires_grad=True)
    lt = torch.tensor(ls, requires_grad=True)
    out = sigma * ra.rescaled(emb, Zt[1:], Xt / lt, M).sum(0) + 1.0 - Zt[0, :, 0][None, :]
    out.sum().backward()
    return out.detach().numpy(), Zt.grad.numpy(), Xt.grad.numpy(), lt.grad.numpy()


def make_kernel(which, L, D, M, ls):
    import gpsig_amd
    from gpsig_amd import kernels_pde as kp
    if which == "linear":
        k = gpsig_amd.SignatureLinear(L * D, D, M, order=M, lengthscales=ls, normalization=False)
    elif which == "pde_rbf":
        k = kp.SignatureRBF(L * D, D, order=M, num_levels=M, lengthscales=ls)
    else:
        k = kp.SignatureLinear(L * D, D, order=M, num_levels=M, lengthscales=ls)
    k.lengthscales = torch.tensor(ls, dtype=torch.float64, device=DEV, requires_grad=True)
    return k, ("rbf" if which == "pde_rbf" else "linear")


@pytest.mark.parametrize("which", ["linear", "pde_rbf", "pde_linear"])
@pytest.mark.parametrize("zdtype", [torch.float32, torch.float64])
def test_kernel_classes(which, zdtype):
    """Mahalanobis_term_approx_posterior with Z, X and the lengthscales requiring a gradient: the value is the
    no-grad value exactly, and out.sum().backward() reaches Z (row 0 through the 1 - Z[0] term), X and the
    lengthscales within the bar."""
    N, T, L, D, M = 3, 2, 66, 3, 4
    rng = np.random.default_rng(100)
    X, ls, Zfull = class_case(rng, N, T, L, D, M)
    k, emb = make_kernel(which, L, D, M, ls)
    Zg = t(Zfull).to(zdtype).requires_grad_(True)
    Xg = t(X.reshape(N, -1)).float().requires_grad_(True)
    with torch.no_grad():
        plain = k.Mahalanobis_term_approx_posterior(Zg.detach(), Xg.detach())
    out = k.Mahalanobis_term_approx_posterior(Zg, Xg)
    assert out.requires_grad and out.grad_fn is not None
    assert out.shape == (N, T) and torch.equal(out.detach(), plain)
    out.sum().backward()
    assert Zg.grad.dtype == zdtype and Xg.grad.dtype == torch.float32
    ref, rZ, rX, rl = class_reference(emb, Zfull, X, ls, M, float(k.sigma))
    got = {"out": out.detach().cpu().numpy(), "dZ": Zg.grad.cpu().numpy(), "dX": Xg.grad.cpu().numpy().reshape(N, L, D),
           "dls": k.lengthscales.grad.cpu().numpy()}
    refs = {"out": ref, "dZ": rZ, "dX": rX, "dls": rl}
    errs = {n: rel(got[n].astype(np.float64), refs[n]) for n in refs}
    print(f"{which} {zdtype}: " + " ".join(f"{n} {e:.2e}" for n, e in errs.items()))
    assert (got["dZ"][0, :, 1:] == 0).all() and np.allclose(got["dZ"][0, :, 0], -float(N))
    for n, e in errs.items():
        assert e < GTOL, (which, n, e)


def test_kernel_class_cancelling_lengthscales():
    """The lengthscale contraction in the cancelling regime (Z ~ U[0.97, 0.999]), where the fp32 reference's own
    contraction measured 1.3e-6."""
    N, T, L, D, M = 3, 2, 40, 3, 4
    rng = np.random.default_rng(101)
    X, ls, Zfull = class_case(rng, N, T, L, D, M, 0.97, 0.999)
    k, emb = make_kernel("pde_rbf", L, D, M, ls)
    Zg = t(Zfull).requires_grad_(True)
    Xg = t(X.reshape(N, -1)).float().requires_grad_(True)
    k.Mahalanobis_term_approx_posterior(Zg, Xg).sum().backward()
    _, rZ, _, rl = class_reference(emb, Zfull, X, ls, M, float(k.sigma))
    eZ, el = rel(Zg.grad.cpu().numpy(), rZ), rel(k.lengthscales.grad.cpu().numpy(), rl)
    print(f"cancelling lengthscales: dZ {eZ:.2e} dls {el:.2e}")
    assert eZ < GTOL and el < GTOL


def test_no_grad_inputs_give_no_graph():
    """Nothing requires a gradient: the method returns a plain tensor, bit-identical to ops.rescaled's assembly."""
    from gpsig_amd import ops
    from gpsig_amd import kernels_pde as kp
    N, T, L, D, M = 2, 2, 40, 3, 3
    rng = np.random.default_rng(3)
    X, ls, Zfull = class_case(rng, N, T, L, D, M)
    k = kp.SignatureRBF(L * D, D, order=M, num_levels=M, lengthscales=ls)
    Z, Xf = t(Zfull), t(X.reshape(N, -1))
    out = k.Mahalanobis_term_approx_posterior(Z, Xf)
    assert not out.requires_grad
    K = ops.rescaled(Z[1:], k._prep(Xf), M, embedding="rbf") * float(k.sigma)
    assert torch.equal(out, (K.sum(0) + 1.0 - Z[0, :, 0].to(K)[None, :]).to(out.dtype))
