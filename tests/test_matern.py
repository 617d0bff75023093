"""CPU: the Matern base kernels at the host layer -- classes and aliases, base-kind numbers against
include/gpsig_amd.h, the torch base kernel against the NumPy oracle, and the C ABI's acceptance of the three
kinds (forward entry points only) without touching a GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from oracle import kernels_ref as kr

HEADER = os.path.join(ROOT, "include", "gpsig_amd.h")
NAMES = {"matern12": 2, "laplace": 2, "exponential": 2, "matern32": 3, "matern52": 4}


def header_enum():
    txt = open(HEADER).read()
    return {k: int(v, 0) for k, v in re.findall(r"\b(GPSIG_BASE_[A-Z0-9_]+)\s*=\s*(0x[0-9a-fA-F]+|\d+)", txt)}


def test_classes_aliases_and_base_kinds():
    import gpsig_amd
    import gpsig_amd._lib as L
    from gpsig_amd import kernels, ops
    for cls, base in [(gpsig_amd.SignatureMatern12, "matern12"), (gpsig_amd.SignatureMatern32, "matern32"),
                      (gpsig_amd.SignatureMatern52, "matern52")]:
        k = cls(20, 2, 3, lengthscales=[1.0, 2.0])
        assert k.base == base and k.num_levels == 3 and k.len_examples == 10
    assert gpsig_amd.SignatureLaplace is gpsig_amd.SignatureMatern12
    assert gpsig_amd.SignatureExponential is gpsig_amd.SignatureMatern12
    assert kernels.SignatureLaplace(12, 3, 2).base == "matern12"
    enum = header_enum()
    assert (enum["GPSIG_BASE_MATERN12"], enum["GPSIG_BASE_MATERN32"], enum["GPSIG_BASE_MATERN52"]) == (2, 3, 4)
    assert (L.BASE_MATERN12, L.BASE_MATERN32, L.BASE_MATERN52) == (2, 3, 4)
    for name, kind in NAMES.items():
        assert ops.base_kind(name) == kind and ops.base_kind(name.upper()) == kind
        assert ops.forward_only(name)
    assert not ops.forward_only("rbf") and not ops.forward_only("linear")
    with pytest.raises(gpsig_amd.GpsigError):
        ops.base_kind("cosine")


@pytest.mark.parametrize("base", ["matern12", "matern32", "matern52"])
def test_base_kern_matches_oracle(base):
    """_base_kern on float64 CPU tensors against kernels_ref.base_matern*: generic points, and a set with
    duplicates on exactly representable coordinates (multiples of 1/8: there the reference's squared distance
    of a point with its copy is exactly 0 and the 1e-40 clamp decides; with generic coordinates the
    reference's own -2 <x, y> + |x|^2 + |y|^2 leaves rounding noise of 1e-16, i.e. 1e-8 in r)."""
    import gpsig_amd
    rng = np.random.default_rng(7)
    cls = {"matern12": gpsig_amd.SignatureMatern12, "matern32": gpsig_amd.SignatureMatern32,
           "matern52": gpsig_amd.SignatureMatern52}[base]
    k = cls(12, 3, 2)
    ref = kr.BASE_KERNELS[base]
    P = rng.standard_normal((9, 3))
    Q = rng.standard_normal((5, 3))
    got = k._base_kern(torch.as_tensor(P), torch.as_tensor(Q)).numpy()
    assert np.abs(got - ref(P, Q)).max() < 1e-12
    D = np.round(rng.standard_normal((6, 3)) * 8.0) / 8.0
    D = np.concatenate([D, D[[1, 4]], D[:1]], 0)  # duplicates
    got = k._base_kern(torch.as_tensor(D)).numpy()
    assert np.isfinite(got).all()
    assert np.abs(got - ref(D)).max() < 1e-12
    assert np.abs(np.diag(got) - 1.0).max() < 1e-12 and abs(got[1, 6] - 1.0) < 1e-12
    # the inspection helper of the reference's autoflow functions goes through the same base kernel
    X = rng.standard_normal((2, 12))
    Mx = k.compute_base_kern_symm(torch.as_tensor(X))
    Pts = X.reshape(2 * 4, 3)
    assert np.abs(Mx - ref(Pts).reshape(2, 4, 2, 4).transpose(0, 2, 1, 3)).max() < 1e-12


def test_abi_accepts_the_three_kinds_without_gpu():
    """Argument validation as in test_abi.py: no pointer is dereferenced and no HIP call is made on these paths."""
    import gpsig_amd._lib as L
    lib = L.load()
    fake = ctypes.c_void_p(256)

    def gram(kind, order=1, d=3, difference=1, pair_mode=L.PAIRS_RECT):
        # empty row range: every check runs, nothing is launched
        return lib.gpsig_sig_gram(fake, 4, 10, fake, 4, 10, d, 4, order, kind, difference, pair_mode, 2, 2, None, None,
                                  None, 0.0, 0, fake, 0, 4, fake, 1 << 20, None)

    for kind in (2, 3, 4):
        assert gram(kind) == L.GPSIG_OK
        assert gram(kind, difference=0) == L.GPSIG_OK
        assert gram(kind, d=46) == L.GPSIG_OK            # the runtime channel loop
        assert gram(kind, order=3, d=12) == L.GPSIG_OK   # higher order up to 32 channels
        assert gram(kind, pair_mode=L.PAIRS_UPPER) == L.GPSIG_OK
        assert gram(kind, order=3, d=40) == L.GPSIG_EUNSUPPORTED  # the tile mode past 32 channels
        assert gram(kind | L.BASE_SEED_MFMA) == L.GPSIG_EUNSUPPORTED
        assert gram(kind | L.GRAM_SPLIT) == L.GPSIG_EUNSUPPORTED
        # saved VJP state, the VJPs and their workspace queries
        nb = lib.gpsig_sig_state_bytes(4, 4, 10, 4, L.PAIRS_RECT)
        assert lib.gpsig_sig_gram_state(fake, 4, 10, fake, 4, 10, 3, 4, kind, L.PAIRS_RECT, 0, 4, None, None, None, 0.0,
                                        0, fake, 0, 4, fake, nb, fake, 1 << 20, None) == L.GPSIG_EUNSUPPORTED
        assert lib.gpsig_sig_gram_vjp(fake, 4, 10, fake, 4, 10, 3, 4, kind, 1, L.PAIRS_RECT, 0, 4, fake, 0, None, None,
                                      None, 0.0, fake, fake, None, None, None, None, fake, 1 << 20,
                                      None) == L.GPSIG_EUNSUPPORTED
        assert lib.gpsig_sig_vjp_ho_workspace_bytes(4, 10, 4, 10, 3, 4, 1, kind) == 0
        assert lib.gpsig_sig_vjp_ho_workspace_bytes(4, 10, 4, 10, 3, 4, 2, kind) == 0
        assert lib.gpsig_tens_gram_vjp_workspace_bytes(10, 64, 1, 46, 4, kind) == 0
        assert lib.gpsig_tens_gram(fake, 6, 2, 0, 3, 3, kind, fake, fake, 1 << 20, None) == L.GPSIG_EUNSUPPORTED
    assert gram(5) == L.GPSIG_EUNSUPPORTED
    assert gram(0) == L.GPSIG_OK and gram(1) == L.GPSIG_OK
    assert lib.gpsig_sig_vjp_ho_workspace_bytes(4, 10, 4, 10, 3, 4, 1, L.BASE_RBF) > 0


def test_other_base_kernels_still_unsupported():
    from gpsig_amd import kernels
    for cls in (kernels.SignatureCosine, kernels.SignaturePoly, kernels.SignatureMix, kernels.SignatureSpectral):
        with pytest.raises(NotImplementedError, match="Matern"):
            cls(20, 2, 3)


def test_tensor_kernels_and_backward_raise_before_any_launch():
    """K_tens* raise NotImplementedError (not a status code from the library) on host tensors: the check comes
    before the device is needed."""
    import gpsig_amd
    k = gpsig_amd.SignatureMatern32(20, 2, 3)
    Z = torch.zeros(6, 4, 2, dtype=torch.float64)
    X = torch.zeros(3, 20, dtype=torch.float64)
    with pytest.raises(NotImplementedError, match="matern32"):
        k.K_tens(Z)
    with pytest.raises(NotImplementedError, match="matern32"):
        k.K_tens_vs_seq(Z, X)
    with pytest.raises(NotImplementedError, match="matern32"):
        k.K_tens_n_seq_covs(Z, X)
    from gpsig_amd.inducing_variables import InducingTensors, Kuu
    with pytest.raises(NotImplementedError, match="matern32"):
        Kuu(InducingTensors(Z, 3), k)
