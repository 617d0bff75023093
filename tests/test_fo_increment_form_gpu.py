"""GPU parity of the first-order Gram's increment-form cells and closed-form level-1 prefix (sig_common.h
RbfSeedPk::cells, sig_fo.h levels) vs the float64 oracle, raw levels, at every column geometry and in the
regimes where the chained row increment d and the prefix state u are reset and resumed.

The cell is dM = d Eq + k' w with d = k(x_{i+1}, y_j) - k(x_i, y_j) chained along a lane's columns
(d_{j+1} = d_j + dM_j), and level 1's exclusive 2-D prefix is u_ij - u_i0 with u the running sum of d, where
one lane group holds the whole sequence (fewer than 64 lanes per pair); u_i0 is broadcast from the group's
first lane.

Criterion, as tests/test_gram_gpu.py: norm-relative max|K32 - K64| < 1e-5 per level.
"""
import numpy as np
import pytest
import torch

from conftest import norm_rel_err
from oracle import kernels_ref as kr

pytestmark = pytest.mark.gpu
TOL = 1e-5
DEV = "cuda"


def t(x):
    return torch.as_tensor(np.asarray(x), device=DEV)


def walks(N, L, D, seed, step=None):
    """The benchmark's walks, cumsum(N(0,1)) / sqrt(L D) (step = None), or walks of a given step size."""
    inc = np.random.default_rng(seed).standard_normal((N, L, D))
    inc *= (1.0 / np.sqrt(L * D)) if step is None else step
    return np.cumsum(inc, 1).astype(np.float32).astype(np.float64)


def kernels(L, D, M):
    import gpsig_amd
    return (gpsig_amd.SignatureRBF(L * D, D, M, normalization=False),
            kr.SignatureKernelRef(L * D, D, M, normalization=False))


def assert_levels(got, exp, what):
    err = norm_rel_err(got, exp, axis_levels=True)
    print(what, "norm_rel_err per level:", err)
    assert (err < TOL).all(), (what, err)


def check_all(X, M, X2=None, diag=True):
    """K(X), K(X, X2) and Kdiag of the sequences X (N, L, D), X2 (N2, L2, D), raw levels."""
    N, L, D = X.shape
    k, ref = kernels(L, D, M)
    Xf = X.reshape(N, -1)
    assert_levels(k.K(t(Xf), return_levels=True).cpu().numpy(), ref.K(Xf, return_levels=True), "K(X)")
    if X2 is not None:
        X2f = X2.reshape(len(X2), -1)
        assert_levels(k.K(t(Xf), t(X2f), return_levels=True).cpu().numpy(), ref.K(Xf, X2f, return_levels=True), "K(X, X2)")
    if diag:
        assert_levels(k.Kdiag(t(Xf), return_levels=True).cpu().numpy(), ref.Kdiag(Xf, return_levels=True), "Kdiag")


# (L, D, M, N, (W, LP, column blocks)): columns per lane x lanes per pair of the launch that L points take
ROUTES = [
    (9, 5, 5, 9, (2, 16, 1)),      # 2 x 16
    (33, 5, 5, 13, (4, 16, 1)),    # 4 x 16 (L2 = 30: 2 x 16)
    (64, 5, 5, 9, (4, 16, 1)),     # 4 x 16, every column a point
    (100, 5, 5, 13, (10, 10, 1)),  # 10 x 10: groups off the DPP rows, u_i0 through the LDS crossbar
    (128, 5, 5, 9, (8, 16, 1)),    # 8 x 16: the headline geometry, u_i0 by the DPP row broadcast
    (200, 5, 5, 13, (8, 32, 1)),   # 8 x 32: two DPP rows per group
    (300, 5, 5, 9, (8, 64, 1)),    # 8 x 64, one column block: level 1 scanned
    (600, 5, 5, 9, (8, 64, 2)),    # 8 x 64, two column blocks: level 1 scanned, carries through LDS
    (128, 8, 5, 13, (8, 16, 1)),   # D = 8: the points of column pairs >= 1 re-read on exact rows
    (128, 5, 1, 9, (8, 16, 1)),    # level 1 only (closed form, no recursion)
    (128, 5, 2, 13, (8, 16, 1)),   # level 2 reads the closed-form prefix and nothing is scanned
    (128, 5, 3, 9, (8, 16, 1)),    # one scanned level beside the closed-form one
]


def geometry(L, D, M, **kw):
    """(W, LP, column blocks) of the fixed-channel launch that K(X) of L points takes (ops.fo_route: host only)."""
    from gpsig_amd import ops
    r = ops.fo_route(6, L, None, None, D, M, **kw)
    assert r["path"] == 0, r
    return r["W"], r["LP"], r["nblk"]


@pytest.mark.parametrize("L,D,M,N", [r[:4] for r in ROUTES])
def test_routes(L, D, M, N):
    """N = 9 and 13 leave the tiles of 4 sequences by 4 pairs (16-lane groups) or 6 pairs (10-lane groups)
    partly filled; X2 has L - 3 points, so the columns past the sequence sit inside a lane's chain."""
    geo = {r[:4]: r[4] for r in ROUTES}[L, D, M, N]
    assert geometry(L, D, M) == geo and geometry(L, D, M, diag=True) == geo
    assert geometry(L - 3, D, M) == ((2, 16, 1) if L == 33 else geo)
    X = walks(N, L, D, 1000 + L + D + M)
    X2 = walks(N - 2, L - 3, D, 2000 + L + D + M)
    check_all(X, M, X2)


def test_route_d8_m6():
    """D = 8, M = 6 (8 x 16 at two waves per SIMD, four scanned levels beside the closed-form one), K(X) only."""
    assert geometry(128, 8, 6) == (8, 16, 1)
    check_all(walks(9, 128, 8, 77), 6, diag=False)


def regime(name, N, L, D=5):
    if name == "walks":        # cubic expm1(c)
        return walks(N, L, D, 31)
    if name == "steps015":     # |c| past the cubic's bound: quintic expm1(c)
        return walks(N, L, D, 32, step=0.15)
    if name == "jumps":        # every ninth increment x 25: slow rows between hot rows, on every sequence
        inc = np.random.default_rng(33).standard_normal((N, L, D)) * 0.03
        inc[:, 9::9, :] *= 25.0
        return np.cumsum(inc, 1)
    if name == "jumps_seq0":   # the same on sequence 0 only: the pairs sharing its waves go slow with it
        inc = np.random.default_rng(34).standard_normal((N, L, D)) * 0.03
        inc[0, 9::9, :] *= 25.0
        return np.cumsum(inc, 1)
    if name == "offset":       # two groups 3 lengthscales apart in one channel: k falls steeply along a lane's chain
        X = walks(N, L, D, 35)
        X[N // 2:, :, 0] += 3.0
        return X
    if name == "constant":     # two constant paths (every cell with them is an exact zero) among walks
        X = walks(N, L, D, 36)
        X[:2] = X[:2, :1]
        return X
    raise ValueError(name)


@pytest.mark.parametrize("L", [128, 40])
@pytest.mark.parametrize("name", ["walks", "steps015", "jumps", "jumps_seq0", "offset", "constant"])
def test_regimes(name, L):
    X = regime(name, 9, L)
    check_all(X, 5, regime(name, 9, L)[2:, : L - 3])


def test_anchor_rows_inside_a_pair():
    """L = 300: the anchor rows 127 and 255 reset k and expm1(q) inside a pair, on jumpy data too."""
    assert geometry(300, 5, 5) == geometry(300, 5, 4) == (8, 64, 1)
    check_all(regime("walks", 9, 300), 5, diag=False)
    check_all(regime("jumps", 9, 300), 4, diag=False)


def test_anchor_rows_with_the_closed_form_prefix():
    """L = 200 (two DPP rows per group): the anchor row 127 falls inside a pair that takes level 1 from u, and u
    goes on from the exact rows' difference."""
    assert geometry(200, 5, 5) == geometry(200, 5, 4) == (8, 32, 1)
    check_all(regime("walks", 9, 200), 5, diag=False)
    check_all(regime("jumps", 9, 200), 4, diag=False)


@pytest.mark.parametrize("L", [100, 128])
def test_slot_independence(L):
    """K(X)[S, S] == K(X[S]) bit for bit: a pair's value does not depend on its group's slot in the wave, so
    every lane of a group subtracts the same lane's u_i0."""
    N, D, M = 13, 5, 5
    k, _ = kernels(L, D, M)
    X = t(walks(N, L, D, 55).reshape(N, -1))
    S = [1, 2, 5, 7, 8, 11, 12]
    full = k.K(X, return_levels=True)
    sub = k.K(X[S], return_levels=True)
    assert torch.equal(full[:, S][:, :, S], sub)


@pytest.mark.parametrize("L", [40, 100, 128, 200])
def test_saved_state_launch_writes_the_same_gram(L):
    """The launch that also saves the VJP's state takes level 1's prefix from u like the plain launch and keeps
    the column sums of level 1 only for the state it stores: the same Gram, bit for bit."""
    from gpsig_amd import ops
    N, D, M = 6, 5, 5
    assert geometry(L, D, M, state=True) == {40: (4, 16, 1), 100: (10, 10, 1), 128: (8, 16, 1), 200: (8, 32, 1)}[L]
    X3 = t(walks(N, L, D, 56)).float()
    state = torch.empty(ops.sig_state_numel(N, None, L, M), dtype=torch.float32, device=DEV)
    assert torch.equal(ops.sig_gram(X3, None, M, state=state), ops.sig_gram(X3, None, M))
    Y3 = t(walks(N - 1, L, D, 57)).float()
    state = torch.empty(ops.sig_state_numel(N, N - 1, L, M), dtype=torch.float32, device=DEV)
    assert torch.equal(ops.sig_gram(X3, Y3, M, state=state), ops.sig_gram(X3, Y3, M))
