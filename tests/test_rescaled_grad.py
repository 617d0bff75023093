"""CPU: the gradient oracle of the VOSF rescaled kernel (tests/rescaled_autodiff.py) is pinned to the NumPy
oracle, and gpsig_rescaled_vjp is declared, exported and validates its arguments without a GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import rescaled_autodiff as ra
from conftest import ROOT
from oracle import sigalgs

HEADER = os.path.join(ROOT, "include", "gpsig_amd.h")
EMBEDDINGS = ["linear", "rbf"]


def inputs(seed, M, N, T, L, D):
    rng = np.random.default_rng(seed)
    X = np.cumsum(rng.standard_normal((N, L, D)), 1) / np.sqrt(L)
    Z = rng.uniform(0.1, 0.9, (M * (M + 1) // 2, T, D))
    return Z, X, rng


def numpy_oracle(emb, Z, X, M):
    Zc = np.concatenate([Z, np.ones_like(Z)], axis=1)
    if emb == "linear":
        S = np.einsum("npd,rtd,nqd->nprtq", X, Zc, X, optimize=True)
    else:
        S = np.einsum("npqd,rtd->nprtq", np.exp(-(X[:, :, None, :] - X[:, None, :, :]) ** 2 / 2.0), Zc, optimize=True)
    return sigalgs.signature_kern_rescaled_higher_order(S, M)


@pytest.mark.parametrize("emb", EMBEDDINGS)
def test_restatement_forward_equals_numpy_oracle(emb):
    M, L, D = 4, 12, 3
    Z, X, _ = inputs(0, M, 3, 2, L, D)
    got = ra.forward(emb, Z, X, M)
    ref = numpy_oracle(emb, Z, X, M)
    err = np.abs(got - ref).max() / np.abs(ref).max()
    print(f"restatement vs oracle.sigalgs {emb}: {err:.2e}")
    assert got.shape == ref.shape == (M + 1, 3, 2)
    assert err < 1e-12


@pytest.mark.parametrize("emb", EMBEDDINGS)
def test_restatement_gradient_equals_finite_differences(emb):
    """Autodiff of the restatement against central differences of the NumPy oracle, 1e-6 norm-relative.  The step
    1e-5 leaves a truncation error of order h^2 = 1e-10 and a rounding error of order 1e-16 / h = 1e-11."""
    M, L, D, N, T = 3, 6, 2, 2, 2
    Z, X, rng = inputs(1, M, N, T, L, D)
    gout = rng.standard_normal((M + 1, N, T))
    gZ, gX = ra.grads(emb, Z, X, M, gout)
    h = 1e-5

    def loss(Zv, Xv):
        return float((gout * numpy_oracle(emb, Zv, Xv, M)).sum())

    def central(A, which):
        out = np.zeros_like(A)
        for idx in np.ndindex(*A.shape):
            Ap, Am = A.copy(), A.copy()
            Ap[idx] += h
            Am[idx] -= h
            out[idx] = ((loss(Ap, X) - loss(Am, X)) if which == "Z" else (loss(Z, Ap) - loss(Z, Am))) / (2 * h)
        return out

    fZ, fX = central(Z, "Z"), central(X, "X")
    eZ = np.abs(gZ - fZ).max() / np.abs(fZ).max()
    eX = np.abs(gX - fX).max() / np.abs(fX).max()
    print(f"autodiff vs finite differences {emb}: dZ {eZ:.2e} dX {eX:.2e}")
    assert eZ < 1e-6 and eX < 1e-6


def test_level_zero_has_no_gradient():
    """Level 0 of the output is the constant 0: its upstream gradient reaches nothing."""
    M = 3
    Z, X, rng = inputs(2, M, 2, 2, 6, 2)
    gout = rng.standard_normal((M + 1, 2, 2))
    g0 = gout.copy()
    g0[0] = 7.0
    a, b = ra.grads("rbf", Z, X, M, gout), ra.grads("rbf", Z, X, M, g0)
    assert (a[0] == b[0]).all() and (a[1] == b[1]).all()


# --------------------------------------------------------------------------------------- the C ABI, host only
def test_vjp_declared_exported_and_bound():
    import gpsig_amd._lib as L
    txt = open(HEADER).read()
    syms = set(re.findall(r"\b(gpsig_[a-z_]+)\s*\(", txt))
    lib = L.load()
    s = "gpsig_rescaled_vjp"
    assert s in syms and hasattr(lib, s) and s in L.SIGNATURES


def vjp_call(lib, M=4, lt=None, t=2, n=3, l=40, d=3, emb=0, missing=None, ws=None, ws_bytes=None):
    fake = ctypes.c_void_p(256)  # never dereferenced: every check comes before the first launch
    p = {k: (None if k == missing else fake) for k in ("Z", "X", "gout", "gZ", "gX")}
    lt = M * (M + 1) // 2 if lt is None else lt
    need = lib.gpsig_rescaled_workspace_bytes(n, M)  # the VJP's workspace is the forward's
    return lib.gpsig_rescaled_vjp(p["Z"], lt, t, p["X"], n, l, d, M, emb, p["gout"], p["gZ"], p["gX"],
                                  fake if ws is None else ws, need if ws_bytes is None else ws_bytes, None)


def test_vjp_rejects_bad_arguments_without_gpu():
    import gpsig_amd._lib as L
    lib = L.load()
    for missing in ("Z", "X", "gout", "gZ", "gX"):
        assert vjp_call(lib, missing=missing) == L.GPSIG_EINVAL, missing
    assert vjp_call(lib, M=4, lt=9) == L.GPSIG_EINVAL      # lt != M (M + 1) / 2
    assert vjp_call(lib, M=4, lt=15) == L.GPSIG_EINVAL
    assert vjp_call(lib, emb=2) == L.GPSIG_EINVAL          # neither linear nor RBF
    assert vjp_call(lib, l=1) == L.GPSIG_EINVAL            # no increment
    assert vjp_call(lib, t=0) == L.GPSIG_EINVAL
    assert vjp_call(lib, n=0) == L.GPSIG_EINVAL
    assert vjp_call(lib, d=0) == L.GPSIG_EINVAL
    assert vjp_call(lib, M=0, lt=0) == L.GPSIG_EINVAL


def test_vjp_workspace_and_envelope_without_gpu():
    import gpsig_amd._lib as L
    lib = L.load()
    need = lib.gpsig_rescaled_workspace_bytes(3, 4)
    assert need > 0 and need % 256 == 0
    assert vjp_call(lib, ws_bytes=need - 1) == L.GPSIG_EWORKSPACE
    assert vjp_call(lib, ws=ctypes.c_void_p(None)) == L.GPSIG_EWORKSPACE
    # the forward's envelope: 129 points at 5 and 6 levels, 257 up to 4, 6 levels at the most
    assert vjp_call(lib, M=5, l=130) == L.GPSIG_EUNSUPPORTED
    assert vjp_call(lib, M=6, l=130) == L.GPSIG_EUNSUPPORTED
    assert vjp_call(lib, M=4, l=258) == L.GPSIG_EUNSUPPORTED
    assert vjp_call(lib, M=7, l=10) == L.GPSIG_EUNSUPPORTED


def test_ops_vjp_checks_shapes_before_the_device():
    """ops.rescaled_vjp refuses host tensors like every product path, so no GPU is needed to see it."""
    import torch
    import gpsig_amd
    from gpsig_amd import ops
    with pytest.raises(gpsig_amd.GpsigError):
        ops.rescaled_vjp(torch.zeros(6, 2, 3), torch.zeros(2, 5, 3), 3, torch.zeros(4, 2, 2))
    from gpsig_amd import autograd
    assert issubclass(autograd.Rescaled, torch.autograd.Function)
