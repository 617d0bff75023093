"""Signature features (iisignature.sig / sigbackprop replacement): host helpers on CPU, the gfx950
kernels vs the Chen-identity oracle (oracle/chen.py, pinned to the esig relation in test_oracle.py)."""
import numpy as np
import pytest
import torch

from conftest import norm_rel_err
from oracle import autodiff_ref as ar
from oracle import chen

DEV = "cuda"


def test_compute_trunc_and_powers():
    from gpsig_amd import signatures as sg
    assert sg.compute_trunc(6, 5) == 1 and sg.compute_trunc(7, 5) == 2 and sg.compute_trunc(100, 5) == 3
    P = sg.get_powers(3, 2)
    assert P.shape == (3 + 9, 3)
    np.testing.assert_array_equal(P[3], [2, 0, 0])  # (1,1)
    np.testing.assert_array_equal(P[4], [1, 1, 0])  # (1,2)
    np.testing.assert_array_equal(P[3 + 5], [0, 1, 1])  # (2,3)
    np.testing.assert_array_equal(P.sum(1), [1] * 3 + [2] * 9)


def test_torch_signature_oracle_matches_chen():
    rng = np.random.default_rng(0)
    x = np.cumsum(rng.standard_normal((7, 3)), 0) * 0.3
    ref = np.concatenate(chen.signature(x, 4)[1:])
    np.testing.assert_allclose(ar.signature(torch.tensor(x), 4).numpy(), ref, rtol=1e-12, atol=1e-14)


@pytest.mark.gpu
@pytest.mark.parametrize("d,depth,L", [(2, 6, 30), (3, 4, 50), (5, 5, 40), (1, 3, 10), (8, 3, 20),
                                       (6, 6, 12), (40, 3, 8)])
def test_signature_matches_chen(d, depth, L):
    """(6, 6) and (40, 3) have 55 986 / 65 640 coordinates: past the 160 KiB of LDS, the levels live in
    per-path slabs of the workspace (gpsig_signature_workspace_bytes)."""
    from gpsig_amd import ops
    rng = np.random.default_rng(d + depth)
    X = np.cumsum(rng.standard_normal((9, L, d)), 1) / np.sqrt(L)
    got = ops.signature(torch.tensor(X, device=DEV), depth).cpu().numpy()
    off = 0
    for m in range(1, depth + 1):
        ref = np.stack([chen.signature(x, depth)[m] for x in X])
        assert norm_rel_err(got[:, off:off + d ** m], ref) < 1e-5, m
        off += d ** m
    assert off == got.shape[1]


@pytest.mark.gpu
@pytest.mark.parametrize("d,depth,L", [(2, 4, 12), (3, 3, 20), (5, 3, 15), (4, 7, 8), (12, 4, 6)])
def test_signature_backprop_matches_autodiff(d, depth, L):
    """(4, 7) and (12, 4): 21 844 / 22 620 coordinates, the VJP's levels, adjoints and exponential tables
    (4 x the coordinates) past the LDS, in the workspace slabs."""
    from gpsig_amd import signatures as sg
    rng = np.random.default_rng(10 + d)
    X = np.cumsum(rng.standard_normal((5, L, d)), 1) / np.sqrt(L)
    C = sum(d ** m for m in range(1, depth + 1))
    G = rng.standard_normal((5, C))
    Xt = torch.tensor(X, device=DEV, requires_grad=True)
    (sg.Sig(Xt, depth) * torch.as_tensor(G, device=DEV)).sum().backward()
    ref = np.zeros_like(X)
    for a in range(5):
        xa = torch.tensor(X[a], requires_grad=True)
        (ar.signature(xa, depth) * torch.tensor(G[a])).sum().backward()
        ref[a] = xa.grad.numpy()
    assert norm_rel_err(Xt.grad.cpu().numpy(), ref) < 1e-5


def level_errors(got, X, d, depth):
    """Norm-relative error of each level of the (n, channels) signatures against the Chen oracle."""
    refs = [chen.signature(x, depth) for x in X]
    err, off = [], 0
    for m in range(1, depth + 1):
        err.append(norm_rel_err(got[:, off:off + d ** m], np.stack([r[m] for r in refs])))
        off += d ** m
    assert off == got.shape[1]
    return np.array(err)


def autodiff_gradient(X, G, depth):
    ref = np.zeros_like(X)
    for a in range(X.shape[0]):
        xa = torch.tensor(X[a], requires_grad=True)
        (ar.signature(xa, depth) * torch.tensor(G[a])).sum().backward()
        ref[a] = xa.grad.numpy()
    return ref


@pytest.mark.gpu
@pytest.mark.parametrize("d,depth,L", [(3, 1, 10), (1, 16, 12), (2, 16, 6), (2, 12, 40), (3, 4, 2), (3, 4, 1)])
def test_signature_depth_and_length_edges(d, depth, L):
    """Depth 1; depth 16 (all of c_invfact; at d = 2 its 131 070 coordinates live in the global slabs); depth 12
    over 39 steps; one increment; a single point (no increment: exact zeros).

    The depth-16 paths move one way in every channel.  On a path that backtracks, level m passes through values
    (excursion / final displacement)^m times its final size, and any fp32 Chen update keeps that rounding: the
    oracle's own recursion in float32 on random walks is off by 3.3e-5 at level 16 of (1, 16, 12) and 4.5e-6 at
    (2, 16, 6) (the kernel: 4.2e-5 and 1.0e-5 on the same walks), but by <= 1.5e-7 on the one-way paths, so there
    the 1e-5 bar tests the kernel and not the number format."""
    from gpsig_amd import ops
    rng = np.random.default_rng(100 * d + depth + L)
    steps = rng.standard_normal((4, L, d))
    if depth == 16:
        steps = np.abs(steps) * rng.choice([-1.0, 1.0], (4, 1, d))
    X = np.cumsum(steps, 1) / np.sqrt(L)
    X = X.astype(np.float32).astype(np.float64)
    got = ops.signature(torch.tensor(X, device=DEV), depth).cpu().numpy()
    assert got.shape == (4, sum(d ** m for m in range(1, depth + 1))) and np.isfinite(got).all()
    if L == 1:
        assert (got == 0.0).all()
        return
    err = level_errors(got, X, d, depth)
    print(f"signature d={d} depth={depth} L={L}: err {np.array2string(err, precision=2)}")
    assert (err < 1e-5).all(), err


@pytest.mark.gpu
@pytest.mark.parametrize("d,depth,L", [(1, 3, 10), (3, 1, 10), (2, 12, 5), (9, 3, 12), (3, 4, 2), (3, 4, 1)])
def test_signature_backprop_edges(d, depth, L):
    """One channel; depth 1; depth 12; 9 channels (the first count past the GH_REG = 8 register accumulators:
    LDS atomics); one increment; a single point (exact zero gradient)."""
    from gpsig_amd import signatures as sg
    rng = np.random.default_rng(200 * d + depth + L)
    N = 4
    X = (np.cumsum(rng.standard_normal((N, L, d)), 1) / np.sqrt(L)).astype(np.float32).astype(np.float64)
    G = rng.standard_normal((N, sum(d ** m for m in range(1, depth + 1))))
    Xt = torch.tensor(X, device=DEV, requires_grad=True)
    (sg.Sig(Xt, depth) * torch.as_tensor(G, device=DEV)).sum().backward()
    got = Xt.grad.cpu().numpy()
    assert got.shape == X.shape and np.isfinite(got).all()
    if L == 1:
        assert (got == 0.0).all()
        return
    err = norm_rel_err(got, autodiff_gradient(X, G, depth))
    print(f"signature backprop d={d} depth={depth} L={L}: err {err:.2e}")
    assert err < 1e-5


@pytest.mark.gpu
@pytest.mark.parametrize("d,depth,L,step", [(3, 4, 200, None), (3, 4, 200, 0.3), (5, 3, 500, 0.2)])
def test_signature_backprop_long_paths(d, depth, L, step):
    """The backward pass rebuilds S before each increment as T (x) exp(-h): over hundreds of steps it relies on
    fp32 undoing its own forward pass.  A float32 Chen forward followed by the full reverse leaves <= 3e-7 of each
    level's maximum at (3, 4, 200) and <= 7.3e-7 at (5, 3, 500, 0.2), so the 1e-5 bar has room."""
    from gpsig_amd import ops
    rng = np.random.default_rng(d * L)
    N = 3
    step = 1.0 / np.sqrt(L) if step is None else step
    X = (np.cumsum(rng.standard_normal((N, L, d)), 1) * step).astype(np.float32).astype(np.float64)
    G = rng.standard_normal((N, sum(d ** m for m in range(1, depth + 1))))
    got = ops.signature_vjp(torch.tensor(X, device=DEV), depth, torch.tensor(G, device=DEV)).cpu().numpy()
    err = norm_rel_err(got, autodiff_gradient(X, G, depth))
    print(f"signature backprop d={d} depth={depth} L={L} step={step:.3f}: err {err:.2e}")
    assert np.isfinite(got).all() and err < 1e-5


def chunk_paths():
    """Three paths of three points, d = 2: at depth 16 a path's levels take a 512 KiB slab (forward) or a 2 MiB
    one (backward), so the 1 GiB of slabs holds 2048 / 512 paths per launch."""
    rng = np.random.default_rng(16)
    return (np.cumsum(rng.standard_normal((3, 3, 2)), 1) * 0.5).astype(np.float32)


@pytest.mark.gpu
def test_signature_backprop_second_chunk():
    """N = 513 at d = 2, depth = 16: one path past the 512 of a launch chunk, so the chunk loop's second launch
    (path0 = 512, slab 0) runs.  Three distinct paths and gout rows, tiled; every gradient against its reference."""
    import time
    from gpsig_amd import ops
    d, depth, N = 2, 16, 513
    X3 = chunk_paths()
    C = sum(d ** m for m in range(1, depth + 1))
    G3 = np.random.default_rng(17).standard_normal((3, C)).astype(np.float32)
    ref = autodiff_gradient(X3.astype(np.float64), G3.astype(np.float64), depth)
    X = torch.tensor(X3, device=DEV).repeat(N // 3, 1, 1)
    G = torch.tensor(G3, device=DEV).repeat(N // 3, 1)
    try:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        gX = ops.signature_vjp(X, depth, G)
        torch.cuda.synchronize()
        print(f"signature backprop N={N} d={d} depth={depth}: {time.perf_counter() - t0:.2f} s")
        got = gX.cpu().numpy()
    finally:
        del X, G
        ops.release_workspaces()
        torch.cuda.empty_cache()
    assert got.shape == (N, 3, d) and np.isfinite(got).all()
    err = norm_rel_err(got, np.tile(ref, (N // 3, 1, 1)))
    err_last = norm_rel_err(got[512], ref[512 % 3])
    print(f"signature backprop N={N}: err {err:.2e}, path 512 alone {err_last:.2e}")
    assert err < 1e-5 and err_last < 1e-5


@pytest.mark.gpu
def test_signature_second_chunk():
    """N = 2049 at d = 2, depth = 16: one path past the 2048 of a forward launch chunk.  Three distinct paths,
    tiled; the forward has no atomics, so equal paths give equal bits: all rows equal the first three on the
    device (the 1.07 GB output stays there), and those three are checked against Chen."""
    import time
    from gpsig_amd import ops
    d, depth, N = 2, 16, 2049
    X3 = chunk_paths()
    X = torch.tensor(X3, device=DEV).repeat(N // 3, 1, 1)
    try:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = ops.signature(X, depth)
        torch.cuda.synchronize()
        print(f"signature N={N} d={d} depth={depth}: {time.perf_counter() - t0:.2f} s")
        assert out.shape == (N, sum(d ** m for m in range(1, depth + 1)))
        same = torch.equal(out[3:N], out[:3].repeat(N // 3 - 1, 1))
        last = torch.equal(out[N - 1], out[(N - 1) % 3])
        got = out[:3].cpu().numpy()
    finally:
        del X
        out = None
        ops.release_workspaces()
        torch.cuda.empty_cache()
    err = level_errors(got, X3.astype(np.float64), d, depth)
    print(f"signature N={N}: rows equal {same}, last row equal {last}, err {np.array2string(err, precision=2)}")
    assert same and last
    assert (err < 1e-5).all(), err


@pytest.mark.gpu
def test_signature_depth_past_16_raises_and_empty_backprop():
    """Depth 17 is refused before any launch (c_invfact and the level offsets hold 16 levels); no paths give an
    empty gradient, as ops.signature gives an empty output."""
    import gpsig_amd
    from gpsig_amd import ops
    X = torch.zeros((2, 4, 2), device=DEV)
    with pytest.raises(gpsig_amd.GpsigError):
        ops.signature(X, 17)
    with pytest.raises(gpsig_amd.GpsigError):
        ops.signature_vjp(X, 17, torch.zeros((2, 2 ** 18 - 2), device=DEV))
    E = torch.zeros((0, 7, 3), device=DEV)
    g = ops.signature_vjp(E, 3, torch.zeros((0, 39), device=DEV))
    assert g.shape == (0, 7, 3) and g.dtype == torch.float32 and g.is_cuda
    assert ops.signature(E, 3).shape == (0, 39)


@pytest.mark.gpu
def test_vosf_untrunc_features():
    """UntruncInducingOrthogonalTensors.Kuu_Kuf_Kff (inducing_variables_vosf.py:68-146)."""
    import gpsig_amd
    from gpsig_amd import inducing_variables_vosf as iv
    from gpsig_amd import signatures as sg
    from oracle import pde
    rng = np.random.default_rng(3)
    N, L, d, M = 6, 20, 3, 10
    X = np.cumsum(rng.standard_normal((N, L, d)), 1) / np.sqrt(L)
    ls = np.array([0.5, 1.0, 2.0])
    k = gpsig_amd.UntruncSignatureKernel(L * d, d, lengthscales=ls, order=1)
    feat = iv.UntruncInducingOrthogonalTensors(L * d, d, M, compute_sig=True)
    Kzz, Kzx, Kxx = iv.Kuu_Kuf_Kff(feat, k, torch.tensor(X.reshape(N, -1), device=DEV))
    lvl = sg.compute_trunc(M, d)
    S = np.stack([np.concatenate(chen.signature(x, lvl)[1:]) for x in X])[:, :M - 1]
    S = S / np.prod(ls[None, :] ** sg.get_powers(d, lvl)[:M - 1], axis=1)[None, :]
    np.testing.assert_allclose(Kzz.cpu().numpy(), np.eye(M))
    assert Kzx.shape == (M, N)
    np.testing.assert_allclose(Kzx[0].cpu().numpy(), 1.0)
    assert norm_rel_err(Kzx[1:].T.cpu().numpy(), S) < 1e-5
    assert norm_rel_err(Kxx.cpu().numpy(), pde.pde_diag(X / ls, 1, 1)) < 1e-5
    # compute_and_diff_sig: signatures of the scaled paths, differentiable in the lengthscales
    feat2 = iv.UntruncInducingOrthogonalTensors(L * d, d, M, compute_and_diff_sig=True)
    k.lengthscales = torch.tensor(ls, device=DEV, requires_grad=True)
    Kzx2 = feat2.Kuf(k, torch.tensor(X.reshape(N, -1), device=DEV))
    assert norm_rel_err(Kzx2[1:].T.detach().cpu().numpy(), S) < 1e-5  # same numbers, other route
    Kzx2.sum().backward()
    assert torch.isfinite(k.lengthscales.grad).all()


@pytest.mark.gpu
@pytest.mark.parametrize("normalization", [True, False])
def test_vosf_trunc_features(normalization):
    """TruncInducingOrthogonalTensors.Kuu_Kuf_Kff (inducing_variables_vosf.py:180-269)."""
    import gpsig_amd
    from gpsig_amd import inducing_variables_vosf as iv
    from gpsig_amd import signatures as sg
    from oracle import kernels_ref as kr
    rng = np.random.default_rng(4)
    N, L, d, M, lev = 5, 16, 2, 9, 4
    X = np.cumsum(rng.standard_normal((N, L, d)), 1) / np.sqrt(L)
    var = np.array([1.0, 0.5, 2.0, 1.5, 0.7])
    k = gpsig_amd.SignatureLinear(L * d, d, lev, variances=var, normalization=normalization)
    feat = iv.TruncInducingOrthogonalTensors(L * d, d, M, compute_sig=True)
    Kzz, Kzx, Kxx = feat.Kuu_Kuf_Kff(k, torch.tensor(X.reshape(N, -1), device=DEV))
    slv = sg.compute_trunc(M, d)
    S = np.stack([np.concatenate([[1.0]] + chen.signature(x, slv)[1:]) for x in X])[:, :M].T  # (M, N)
    reps = np.repeat(np.arange(slv + 1), [d ** i for i in range(slv + 1)])[:M]
    S = S * np.sqrt(var[reps])[:, None]
    ref = kr.SignatureKernelRef(L * d, d, lev, base="linear", variances=var, normalization=normalization)
    if normalization:
        Kun = ref.K_seq_diag(X)
        S = S / np.sqrt(Kun[reps] + 1e-6)
        np.testing.assert_allclose(Kxx.cpu().numpy(), var.sum())
    else:
        assert norm_rel_err(Kxx.cpu().numpy(), ref.Kdiag(X.reshape(N, -1))) < 1e-5
    assert norm_rel_err(Kzx.cpu().numpy(), S) < 1e-5
