"""Gradient oracle of the VOSF rescaled kernel: a float64 torch restatement of the reference graph,
differentiated by torch.autograd the way the reference is differentiated by TF autodiff.

TEST INFRASTRUCTURE ONLY, in the style of oracle/autodiff_ref.py: only tests/ import it, as the checker of
gpsig_rescaled_vjp / gpsig_amd.autograd.Rescaled.

What it restates (file:line relative to the reference):
  * the concatenation [Z | ones] and the seeds   gpsig/kernels.py:800-822 (linear embedding),
                                                 gpsig/kernels_pde.py:191-222 (per-coordinate RBF embedding)
  * second difference + block recursion          gpsig/signature_algs_vosf.py:11-48
with the materialised (N, L, LT, 2T, L) base-kernel tensor, exclusive cumsums as ``cumsum - a`` and
``-first half + second half`` at the end.  The forward is pinned to oracle.sigalgs and the gradient to central
finite differences of that NumPy oracle in tests/test_rescaled_grad.py.
"""
from __future__ import annotations

import numpy as np
import torch


def _xcumsum(a: torch.Tensor, dim: int) -> torch.Tensor:
    """tf.cumsum(a, exclusive=True, axis=dim)."""
    return torch.cumsum(a, dim) - a


def base_tensor(emb: str, Z: torch.Tensor, X: torch.Tensor) -> torch.Tensor:
    """(N, L, LT, 2T, L) base-kernel tensor of the concatenation [Z | ones]; Z (LT, T, D), X (N, L, D)."""
    Zc = torch.cat([Z, torch.ones_like(Z)], 1)
    if emb == "linear":
        return torch.einsum("npd,rtd,nqd->nprtq", X, Zc, X)
    E = torch.exp(-(X[:, :, None, :] - X[:, None, :, :]) ** 2 / 2.0)
    return torch.einsum("npqd,rtd->nprtq", E, Zc)


def second_difference(M: torch.Tensor) -> torch.Tensor:
    return (M[:, 1:, ..., 1:] + M[:, :-1, ..., :-1]) - M[:, :-1, ..., 1:] - M[:, 1:, ..., :-1]


def recursion(M: torch.Tensor, num_levels: int) -> torch.Tensor:
    """signature_algs_vosf.py:16-48 on the second differences M (N, L-1, LT, 2T, L-1) -> (num_levels+1, N, T)."""
    num_tensors = M.shape[3]
    K = [torch.ones((M.shape[0], num_tensors), dtype=M.dtype)]
    r = 0
    for i in range(1, num_levels + 1):
        R = [[M[:, :, r]]]
        r += 1
        for j in range(1, i):
            d = min(j + 1, num_levels)
            Mr = M[:, :, r]
            Rn = [[None] * d for _ in range(d)]
            tot = sum(x for row in R for x in row)
            Rn[0][0] = Mr * _xcumsum(_xcumsum(tot, 1), -1)
            for l in range(1, d):
                col = sum(R[a][l - 1] for a in range(len(R)))
                row = sum(R[l - 1][b] for b in range(len(R)))
                Rn[0][l] = 1.0 / (l + 1) * Mr * _xcumsum(col, 1)
                Rn[l][0] = 1.0 / (l + 1) * Mr * _xcumsum(row, -1)
                for k in range(1, d):
                    Rn[l][k] = 1.0 / ((l + 1) * (k + 1)) * Mr * R[l - 1][k - 1]
            R = Rn
            r += 1
        K.append(sum(x for row in R for x in row).sum(dim=(1, -1)))
    K = [-e[:, : num_tensors // 2] + e[:, num_tensors // 2:] for e in K]
    return torch.stack(K, 0)


def rescaled(emb: str, Z: torch.Tensor, X: torch.Tensor, num_levels: int) -> torch.Tensor:
    return recursion(second_difference(base_tensor(emb, Z, X)), num_levels)


def _leaf(a):
    return torch.tensor(np.asarray(a, dtype=np.float64), requires_grad=True)


def forward(emb, Z, X, num_levels) -> np.ndarray:
    with torch.no_grad():
        return rescaled(emb, torch.as_tensor(Z, dtype=torch.float64), torch.as_tensor(X, dtype=torch.float64),
                        num_levels).numpy()


def grads(emb, Z, X, num_levels, gout):
    """(dZ, dX) of sum(gout * rescaled(Z, X)) in float64."""
    Zt, Xt = _leaf(Z), _leaf(X)
    out = rescaled(emb, Zt, Xt, num_levels)
    (out * torch.as_tensor(gout, dtype=torch.float64)).sum().backward()
    return Zt.grad.numpy(), Xt.grad.numpy()


def grads_fp32(emb, Z, X, num_levels, gout):
    """The error a correct fp32 implementation makes: the recursion and its reverse run in float32 on the float64
    second differences rounded to fp32 (the kernel forms its seeds without cancellation), chained back to Z and X
    in float64."""
    Zt, Xt = _leaf(Z), _leaf(X)
    D64 = second_difference(base_tensor(emb, Zt, Xt))
    D32 = D64.detach().to(torch.float32).requires_grad_(True)
    out = recursion(D32, num_levels)
    (out * torch.as_tensor(gout, dtype=torch.float32)).sum().backward()
    (D64 * D32.grad.to(torch.float64)).sum().backward()
    return Zt.grad.numpy(), Xt.grad.numpy()


def minuend_grad_X(emb, X, num_levels, gout, T, D):
    """dX of sum |gout| * K(ones): the restatement at Z = 0 with weights |gout| (the bar of the cancelling regime)."""
    Z0 = np.zeros((num_levels * (num_levels + 1) // 2, T, D))
    return grads(emb, Z0, X, num_levels, np.abs(gout))[1]
