"""GPU parity of the VOSF rescaled kernel (gpsig_amd/csrc/sig_tens.hip rescaled_kernel<M, W, DP>) at every
instantiation and route, against the float64 oracle on the fp32-rounded inputs.

The kernel is compiled for M = 1..6, W in {1, 2, 4 (M <= 4)} columns per lane (L - 1 <= 64 / 128 / 256) and
DP in {4, 8, 0 = runtime channel loop (d >= 9)}, each taking the linear or the per-coordinate RBF embedding.

References: the linear embedding is SignatureKernelRef.mahalanobis_raw; the RBF embedding is
sigalgs.signature_kern_rescaled_higher_order on the per-coordinate Gram (tests/golden/make_golden.py F5).  Where
d**M <= 1e5 the linear embedding is also compared with the recursion-free Chen form
sum S_m^2 - sum S_m lambda_m S_m (oracle/chen.py).

Criterion: norm-relative max|K32 - K64| < 1e-5 * max|K64| per level 1..M; level 0 is exactly 0.
The reference recursion run in float32 on exact seeds rounded to fp32 (oracle_fp32 below) stays at or below
1e-6 per level at most shapes here with Z ~ U[0.1, 0.9] and reaches 3.3e-6 at the worst one (M = 6, L = 66,
D = 5), so the bar leaves three to ten times the reference's own fp32 error; the long cases print that figure
beside the kernel's.  With Z ~ U[0.97, 0.999] the output K(ones) - K(t) cancels (the fp32 reference is off
by up to 6e-5 of the difference, < 5e-7 of the minuend): the bar there is max|K32 - K64| < 1e-5 * max|K(ones)|,
K(ones) being the reference at Z = 0.  Every check prints its figures before it asserts.
"""
import numpy as np
import pytest
import torch

from conftest import norm_rel_err
from oracle import chen
from oracle import kernels_ref as kr
from oracle import sigalgs

pytestmark = pytest.mark.gpu
TOL = 1e-5
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


def seeds(emb, Z, X):
    """The oracle's (N, L, LT, 2T, L) base-kernel tensor of the concatenation [Z | ones]."""
    Zc = np.concatenate([Z, np.ones_like(Z)], axis=1)
    if emb == "linear":
        return np.einsum("npd,rtd,nqd->nprtq", X, Zc, X, optimize=True)
    E = np.exp(-(X[:, :, None, :] - X[:, None, :, :]) ** 2 / 2.0)
    return np.einsum("npqd,rtd->nprtq", E, Zc, optimize=True)


def oracle(emb, Z, X, M):
    if emb == "linear":
        return kr.SignatureKernelRef(X.shape[1] * X.shape[2], X.shape[2], M, base="linear",
                                     normalization=False).mahalanobis_raw(Z, X)
    return sigalgs.signature_kern_rescaled_higher_order(seeds(emb, Z, X), M)


def oracle_fp32(emb, Z, X, M):
    """The reference recursion in float32 on exact second differences rounded to fp32: the error a correct fp32
    implementation makes (the float64 second difference is taken before the rounding, as the kernel's seeds are
    formed without cancellation)."""
    exact = sigalgs._second_difference
    sigalgs._second_difference = lambda A: exact(A).astype(np.float32)
    try:
        return sigalgs.signature_kern_rescaled_higher_order(seeds(emb, Z, X), M)
    finally:
        sigalgs._second_difference = exact


def naive_chen(Z, X, M):
    """sum S_m^2 - sum S_m lambda_m S_m from Chen signatures: no recursion (tests/golden/make_golden.py F5)."""
    lam = chen.simple_tensors(Z, M)
    out = np.zeros((M + 1, X.shape[0], Z.shape[1]))
    for n, x in enumerate(X):
        S = chen.signature(x, M)
        for m in range(1, M + 1):
            out[m, n] = np.sum(S[m] * S[m]) - lam[m] @ (S[m] * S[m])
    return out


def run(emb, Z, X, M):
    from gpsig_amd import ops
    got = ops.rescaled(t(Z), t(X), M, embedding=emb).cpu().numpy()
    assert got.shape == (M + 1, X.shape[0], Z.shape[1]) and got.dtype == np.float32
    assert np.isfinite(got).all()
    assert (got[0] == 0.0).all()  # level 0 is exactly 0
    return got


def check(what, emb, Z, X, M, fp32_ref=False, ref=None):
    """Levels 1..M of ops.rescaled within the bar of the oracle (and of the Chen form where it is affordable)."""
    N, L, D = X.shape
    got = run(emb, Z, X, M)
    ref = oracle(emb, Z, X, M) if ref is None else ref
    err = norm_rel_err(got[1:], ref[1:], axis_levels=True)
    tag = f"{what} {emb} M={M} L={L} D={D} N={N} T={Z.shape[1]}"
    print(f"{tag}: kernel {np.array2string(err, precision=2)}")
    if fp32_ref:
        e32 = norm_rel_err(oracle_fp32(emb, Z, X, M)[1:], ref[1:], axis_levels=True)
        print(f"{tag}: reference in fp32 {np.array2string(e32, precision=2)}")
    errn = None
    if emb == "linear" and D ** M <= 1e5:
        naive = naive_chen(Z, X, M)
        errn = norm_rel_err(got[1:], naive[1:], axis_levels=True)
        print(f"{tag}: kernel vs Chen form {np.array2string(errn, precision=2)}")
    assert (err < TOL).all(), (tag, err)
    if errn is not None:
        assert (errn < TOL).all(), (tag, errn)
    return got, ref


def length_of(W):
    return {1: 40, 2: 100, 4: 200}[W]


# ----------------------------------------------------------------------------- A.1 every instantiation
@pytest.mark.parametrize("D", [3, 7, 12])
@pytest.mark.parametrize("M,W", [(m, w) for m in range(1, 7) for w in (1, 2, 4) if w < 4 or m <= 4])
@pytest.mark.parametrize("emb", EMBEDDINGS)
def test_every_instantiation(emb, M, W, D):
    """rescaled_kernel<M, W, DP> for all 16 (M, W) and DP = 4 / 8 / runtime loop (D = 3 / 7 / 12)."""
    L = length_of(W)
    rng = np.random.default_rng(1000 * M + 10 * L + D)
    check(f"W={W}", emb, tensors(rng, M, 2, D), walks(rng, 3, L, D), M)


# ----------------------------------------------------------------------------- A.2 length edges
@pytest.mark.parametrize("M,D,L", [(4, 3, L) for L in (2, 3, 64, 65, 66, 128, 129, 130, 256, 257)]
                         + [(6, 5, L) for L in (2, 65, 66, 129)] + [(5, 12, L) for L in (66, 129)])
@pytest.mark.parametrize("emb", EMBEDDINGS)
def test_length_edges(emb, M, D, L):
    """One increment, and L - 1 on either side of 64 / 128 / 256 columns (the W = 1 / 2 / 4 switch), up to the
    longest supported length of each M."""
    rng = np.random.default_rng(100 * L + M)
    check("length", emb, tensors(rng, M, 2, D), walks(rng, 3, L, D), M, fp32_ref=L > 64)


# ----------------------------------------------------------------------------- A.3 channel edges
@pytest.mark.parametrize("D", [1, 4, 5, 8, 9, 33])
@pytest.mark.parametrize("emb", EMBEDDINGS)
def test_channel_edges(emb, D):
    """One channel, the padding boundaries 4 | 5 and 8 | 9 (the first runtime-loop count), one past 32."""
    M, L = 3, 70
    rng = np.random.default_rng(70 + D)
    check("channels", emb, tensors(rng, M, 2, D), walks(rng, 3, L, D), M)


# ----------------------------------------------------------------------------- A.4 batch and layout
@pytest.mark.parametrize("N,T", [(1, 1), (7, 1), (1, 5), (5, 3)])
@pytest.mark.parametrize("emb", EMBEDDINGS)
def test_batch_and_layout(emb, N, T):
    """(M+1, N, T) with all sequences and tensors different: a swapped n / t index or a wrong stride in the
    combine pass fails."""
    M, L, D = 3, 66, 5
    rng = np.random.default_rng(10 * N + T)
    X = walks(rng, N, L, D) * np.linspace(0.7, 1.3, N)[:, None, None]
    Z = tensors(rng, M, T, D)
    _, ref = check("layout", emb, Z, f32(X), M)
    # the cases are told apart: every (n, t) entry of the reference differs from every other
    flat = ref[M].reshape(-1)
    assert len(np.unique(flat)) == flat.size


# ----------------------------------------------------------------------------- A.5 seed regimes
def regime_paths(rng, L, D):
    """Paths of the seed regimes, each (3, L, D), fp32-rounded: small steps (the series branch of
    rbf_second_diff), rough steps (the corner form), two jumps of 5 between small steps, a repeated point."""
    jumpy = rng.standard_normal((3, L, D)) * 0.02
    # both jumps of a channel go the same way: opposite ones would cancel in every level (x_L - x_0 small against
    # the jumps), a regime where the reference recursion in fp32 is itself off by 1e-4 of the level
    sign = rng.choice([-1.0, 1.0], (3, 1, D))
    jumpy[:, L // 3:L // 3 + 1, :] += 5.0 * sign
    jumpy[:, 2 * L // 3:2 * L // 3 + 1, :] += 5.0 * sign
    rep = walks(rng, 3, L, D)
    rep[:, 10:13] = rep[:, 10:11]
    return {"small": walks(rng, 3, L, D, 0.02), "rough": walks(rng, 3, L, D, 0.5),
            "jumps": f32(np.cumsum(jumpy, 1)), "repeat": rep}


@pytest.mark.parametrize("regime", ["small", "rough", "jumps", "repeat"])
@pytest.mark.parametrize("M,L,D", [(4, 130, 3), (3, 66, 12)])
@pytest.mark.parametrize("emb", EMBEDDINGS)
def test_seed_regimes(emb, M, L, D, regime):
    rng = np.random.default_rng(L + D)
    X = regime_paths(rng, L, D)[regime]
    check(regime, emb, tensors(rng, M, 2, D), X, M)


@pytest.mark.parametrize("M,L,D", [(4, 130, 3), (3, 66, 12)])
def test_offset_path_linear(M, L, D):
    """The linear embedding sees increments only: a path moved by +40 in one channel gives the unshifted result.
    The points are multiples of 2^-18 in (-8, 24), so the shifted points are exact in fp32 and the increments of
    both paths are the same numbers."""
    rng = np.random.default_rng(40 + L)
    X = np.round(walks(rng, 3, L, D) * 2.0 ** 18) / 2.0 ** 18
    assert X.min() > -8.0 and X.max() < 24.0
    Xo = X.copy()
    Xo[:, :, 0] += 40.0
    assert (f32(Xo) == Xo).all() and (f32(X) == X).all()
    Z = tensors(rng, M, 2, D)
    got, ref = check("unshifted", "linear", Z, X, M)
    goto, _ = check("offset +40", "linear", Z, Xo, M, ref=ref)
    print(f"offset vs unshifted kernel output: max diff {np.abs(goto - got).max():.2e}")


# ----------------------------------------------------------------------------- A.6 cancellation
@pytest.mark.parametrize("M,L,D", [(4, 130, 3), (6, 129, 5)])
@pytest.mark.parametrize("emb", EMBEDDINGS)
def test_cancellation(emb, M, L, D):
    """Lambda close to 1: K(ones) - K(t) cancels, the bar is 1e-5 of the minuend K(ones) per level."""
    rng = np.random.default_rng(L * M)
    X = walks(rng, 3, L, D)
    Z = tensors(rng, M, 2, D, 0.97, 0.999)
    got = run(emb, Z, X, M)
    ref = oracle(emb, Z, X, M)
    kones = oracle(emb, np.zeros_like(Z), X, M)
    dev = np.array([np.abs(got[m] - ref[m]).max() for m in range(1, M + 1)])
    ko = np.array([np.abs(kones[m]).max() for m in range(1, M + 1)])
    r32 = oracle_fp32(emb, Z, X, M)
    d32 = np.array([np.abs(r32[m] - ref[m]).max() for m in range(1, M + 1)])
    tag = f"cancellation {emb} M={M} L={L} D={D}"
    print(f"{tag}: kernel / max|K_ones| {np.array2string(dev / ko, precision=2)}")
    print(f"{tag}: reference in fp32 / max|K_ones| {np.array2string(d32 / ko, precision=2)}")
    print(f"{tag}: kernel, of the difference {np.array2string(norm_rel_err(got[1:], ref[1:], True), precision=2)}")
    assert (dev < TOL * ko).all(), (tag, dev / ko)


# ----------------------------------------------------------------------------- A.7 exact properties
@pytest.mark.parametrize("M,L,D", [(4, 40, 3), (6, 100, 7), (3, 200, 12)])
@pytest.mark.parametrize("emb", EMBEDDINGS)
def test_ones_tensor_gives_exact_zeros(emb, M, L, D):
    """Z = ones: the tensor block and the ones block do identical arithmetic, the levels are exactly 0.0."""
    rng = np.random.default_rng(M)
    got = run(emb, np.ones((M * (M + 1) // 2, 2, D)), walks(rng, 3, L, D), M)
    print(f"ones {emb} M={M} L={L} D={D}: max|out| {np.abs(got).max():.1e}")
    assert (got == 0.0).all()


@pytest.mark.parametrize("M,L,D", [(4, 40, 3), (5, 100, 5), (3, 200, 12)])
def test_zero_tensor_is_squared_signature_norm(M, L, D):
    """Z = 0 with the linear embedding: K(t) vanishes, the output is |S_m(x)|^2 of the Chen signature."""
    rng = np.random.default_rng(M + L)
    X = walks(rng, 3, L, D)
    got = run("linear", np.zeros((M * (M + 1) // 2, 2, D)), X, M)
    S = [chen.signature(x, M) for x in X]
    ref = np.stack([np.zeros((3, 2))] + [np.tile(np.array([np.sum(s[m] ** 2) for s in S])[:, None], (1, 2))
                                          for m in range(1, M + 1)])
    err = norm_rel_err(got[1:], ref[1:], axis_levels=True)
    print(f"zero tensor M={M} L={L} D={D}: err {np.array2string(err, precision=2)}")
    assert (err < TOL).all(), err


@pytest.mark.parametrize("L,D", [(40, 3), (100, 12)])
@pytest.mark.parametrize("emb", EMBEDDINGS)
def test_constant_sequence(emb, L, D):
    """No increments: every seed is zero, the output is all zeros and finite."""
    rng = np.random.default_rng(L)
    M = 4
    X = np.tile(f32(rng.standard_normal((3, 1, D))), (1, L, 1))
    got = run(emb, tensors(rng, M, 2, D), X, M)
    print(f"constant {emb} L={L} D={D}: max|out| {np.abs(got).max():.1e}")
    assert (got == 0.0).all()


# ----------------------------------------------------------------------------- A.9 / B refusals, host checks
@pytest.mark.parametrize("M,L", [(4, 258), (5, 130), (7, 10)])
@pytest.mark.parametrize("emb", EMBEDDINGS)
def test_unsupported_shapes_raise(emb, M, L):
    """Past 257 points (129 at M >= 5) and past 6 levels: rs_w / dispatch return GPSIG_EUNSUPPORTED before any
    launch, the wrapper raises."""
    import gpsig_amd
    from gpsig_amd import ops
    X = torch.zeros((2, L, 3), device=DEV)
    Z = torch.full((M * (M + 1) // 2, 2, 3), 0.5, device=DEV)
    with pytest.raises(gpsig_amd.GpsigError):
        ops.rescaled(Z, X, M, embedding=emb)


def test_shape_mismatches_raise_before_any_launch():
    """Z and X with different channel counts (the kernel would index X with Z's stride) and a component count
    other than M(M+1)/2 are ValueErrors of the wrapper."""
    from gpsig_amd import ops
    M = 3
    X = torch.zeros((2, 10, 4), device=DEV)
    with pytest.raises(ValueError, match="channel"):
        ops.rescaled(torch.zeros((6, 2, 3), device=DEV), X, M)
    with pytest.raises(ValueError, match="channel"):
        ops.rescaled(torch.zeros((6, 2, 5), device=DEV), X, M)
    with pytest.raises(ValueError, match="components"):
        ops.rescaled(torch.zeros((5, 2, 4), device=DEV), X, M)
    with pytest.raises(ValueError, match="components"):
        ops.rescaled(torch.zeros((10, 2, 4), device=DEV), X, M)


@pytest.mark.parametrize("emb", EMBEDDINGS)
def test_empty_batch(emb):
    """No sequences: an empty (M+1, 0, T) float32 tensor, as every other entry point."""
    from gpsig_amd import ops
    M, T, D = 3, 4, 5
    out = ops.rescaled(torch.zeros((6, T, D), device=DEV), torch.zeros((0, 12, D), device=DEV, dtype=torch.float64), M,
                       embedding=emb)
    assert out.shape == (M + 1, 0, T) and out.dtype == torch.float32 and out.is_cuda


# ----------------------------------------------------------------------------- A.10 kernel-class layer
def test_kernel_classes_two_columns_per_lane():
    """Mahalanobis_term_approx_posterior of both classes at a W = 2 shape with lengthscales: SignatureLinear
    against the oracle's method, the PDE-side SignatureRBF against the RBF oracle assembled as the method does."""
    import gpsig_amd
    from gpsig_amd import kernels_pde as kp
    rng = np.random.default_rng(100)
    N, T, L, D, M = 3, 2, 100, 3, 4
    X = walks(rng, N, L, D)
    ls = np.array([0.7, 1.0, 1.6])
    Zfull = np.concatenate([f32(rng.uniform(0.3, 0.9, (1, T, D))), tensors(rng, M, T, D)], axis=0)
    Xf = X.reshape(N, -1)
    k = gpsig_amd.SignatureLinear(L * D, D, M, lengthscales=ls, normalization=False)
    ref = kr.SignatureKernelRef(L * D, D, M, base="linear", lengthscales=ls, normalization=False)
    got = k.Mahalanobis_term_approx_posterior(t(Zfull), t(Xf)).cpu().numpy()
    exp = ref.Mahalanobis_term_approx_posterior(Zfull, Xf)
    err = norm_rel_err(got, exp)
    print(f"SignatureLinear.Mahalanobis_term_approx_posterior L={L}: err {err:.2e}")
    assert got.shape == (N, T) and err < TOL
    kv = kp.SignatureRBF(L * D, D, order=M, num_levels=M, lengthscales=ls)
    gotv = kv.Mahalanobis_term_approx_posterior(t(Zfull), t(Xf)).cpu().numpy()
    expv = oracle("rbf", Zfull[1:], X / ls, M).sum(0) + 1.0 - Zfull[0, :, 0][None, :]
    errv = norm_rel_err(gotv, expv)
    print(f"kernels_pde.SignatureRBF.Mahalanobis_term_approx_posterior L={L}: err {errv:.2e}")
    assert gotv.shape == (N, T) and errv < TOL
