"""GPU parity of the first-order Gram's row loop (sig_fo.h: runs of hot rows, each ended by an anchor row
or a slow row; row records loaded one row ahead) vs the float64 oracle, at the smallest shapes that reach
each edge of that structure.

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
SLOW_ROWS = (0, 126, 127, 128, 258)  # first row, the rows beside and on the anchor row 127, the last row


def t(x):
    return torch.as_tensor(np.asarray(x), device=DEV)


def smooth(N, L, D, seed):
    return np.cumsum(np.random.default_rng(seed).standard_normal((N, L, D)) * 0.03, 1)


def jumpy(N, L, D, rows, seqs, seed):
    """Walks with N(0,1) 0.03 increments, those of `rows` (of the sequences `seqs`) 25 times larger.  Row r
    of the kernel's grid is the increment x_{r+1} - x_r, inc[r + 1] of the cumulative sum."""
    inc = np.random.default_rng(seed).standard_normal((N, L, D)) * 0.03
    for r in rows:
        if r + 1 < L:
            inc[seqs, r + 1, :] *= 25.0
    return np.cumsum(inc, 1)


def check_K(X, M, X2=None):
    import gpsig_amd
    N, L, D = X.shape
    k = gpsig_amd.SignatureRBF(L * D, D, M)
    ref = kr.SignatureKernelRef(L * D, D, M)
    if X2 is None:
        got = k.K(t(X.reshape(N, -1)), return_levels=True).cpu().numpy()
        exp = ref.K(X.reshape(N, -1), return_levels=True)
    else:
        got = k.K(t(X.reshape(N, -1)), t(X2.reshape(len(X2), -1)), return_levels=True).cpu().numpy()
        exp = ref.K(X.reshape(N, -1), X2.reshape(len(X2), -1), return_levels=True)
    err = norm_rel_err(got, exp, axis_levels=True)
    print("norm_rel_err per level:", err)
    assert (err < TOL).all(), err


@pytest.mark.parametrize("L,D,M", [(2, 5, 5), (3, 5, 5), (128, 5, 5), (129, 5, 5), (130, 5, 5), (257, 5, 5),
                                   (130, 8, 6), (100, 5, 5), (130, 8, 7), (128, 8, 7)])
def test_prefetch_ends_and_anchor_positions(L, D, M):
    """Rows = L - 1: one row; two; 127 (no anchor row); 128 (the anchor row is the last row, the prefetch index
    clamps on it); 129 (one row after an anchor row); 256 (two anchor rows).  D = 8 re-reads the points of
    column pairs >= 1 on exact rows; L = 100 takes the 10-lane groups.  D = 8, M = 7 takes 4 columns per lane
    on 64 lanes at L = 130 (across an anchor row) and 4 columns per lane on 32 lanes at L = 128."""
    from gpsig_amd import ops
    r = ops.fo_route(6, L, None, None, D, M)
    want = (10, 10) if L == 100 else ((4, 64) if L == 130 else (4, 32)) if (D, M) == (8, 7) else \
        (2, 16) if L <= 3 else (8, 16) if L == 128 else (8, 32) if L <= 130 else (8, 64)
    assert (r["path"], r["W"], r["LP"], r["nblk"]) == (0,) + want + (1,), r
    check_K(smooth(6, L, D, 100 + L + D), M)


@pytest.mark.parametrize("D", [5, 8])
@pytest.mark.parametrize("every_seq", [True, False])
def test_slow_rows_at_and_beside_anchors(D, every_seq):
    """Rows with cells outside the polynomial range at rows 0, 126, 127 (the anchor row), 128 and 258 (the
    last row): they leave the run of hot rows and take the exact path.  With the jumps on sequence 0 only,
    the smooth pairs that share a wave with it are taken along by the wave-uniform ballot."""
    N = 5
    check_K(jumpy(N, 260, D, SLOW_ROWS, slice(None) if every_seq else [0], 7), 4)


@pytest.mark.parametrize("D", [5, 8])
@pytest.mark.parametrize("every_seq", [True, False])
def test_consecutive_slow_rows(D, every_seq):
    """Jumps on rows 40..43: the slow path entered from a row that was itself evaluated exactly."""
    N = 5
    check_K(jumpy(N, 260, D, (40, 41, 42, 43), slice(None) if every_seq else [0], 8), 4)


@pytest.mark.parametrize("L", [130, 260])
def test_slow_rows_four_columns_per_lane(L):
    """The slow-row data at D = 8, M = 7: 4 columns per lane, in one column block at L = 130 and in two (the
    row carries between them through LDS) at L = 260."""
    from gpsig_amd import ops
    r = ops.fo_route(5, L, None, None, 8, 7)
    assert (r["path"], r["W"], r["LP"], r["nblk"]) == (0, 4, 64, 1 if L == 130 else 2), r
    check_K(jumpy(5, L, 8, SLOW_ROWS, [0], 13), 7)


def test_rect_pairs_and_diag_on_slow_rows():
    """K(X, X2) (rectangular pair mode) and Kdiag (the diagonal instantiation) on the slow-row data."""
    import gpsig_amd
    L, D, M = 130, 5, 4
    X = jumpy(5, L, D, SLOW_ROWS, slice(None), 9)
    X2 = jumpy(4, L, D, SLOW_ROWS, [0], 10)
    check_K(X, M, X2)
    k = gpsig_amd.SignatureRBF(L * D, D, M, normalization=False)
    ref = kr.SignatureKernelRef(L * D, D, M, normalization=False)
    got = k.Kdiag(t(X.reshape(len(X), -1)), return_levels=True).cpu().numpy()
    exp = ref.Kdiag(X.reshape(len(X), -1), return_levels=True)
    err = norm_rel_err(got, exp, axis_levels=True)
    print("Kdiag norm_rel_err per level:", err)
    assert (err < TOL).all(), err


def test_saved_state_launch_writes_the_same_gram():
    """The training forward (autograd: the launch that also saves the VJP's state) writes the plain
    launch's Gram bit for bit (sig_fo.h, the comment at the row loop).  Compared launch against launch:
    without normalisation the autograd forward returns its launch's output as it is (with it, the forward
    takes raw levels and normalises them in fp64, which is not the fused epilogue's rounding), and the raw
    levels of that normalised forward's launch are compared through ops.sig_gram with a state buffer."""
    import gpsig_amd
    from gpsig_amd import ops
    N, L, D, M = 6, 130, 5, 5
    Xs = smooth(N, L, D, 12)
    X = t(Xs.reshape(N, -1))
    k = gpsig_amd.SignatureRBF(L * D, D, M, normalization=False)
    plain = k.K(X, return_levels=True)
    Xg = X.clone().requires_grad_(True)
    train = k.K(Xg, return_levels=True)
    assert train.requires_grad
    assert torch.equal(train.detach(), plain)
    X3 = t(Xs).float()
    state = torch.empty(ops.sig_state_numel(N, None, L, M), dtype=torch.float32, device=DEV)
    assert torch.equal(ops.sig_gram(X3, None, M, state=state), ops.sig_gram(X3, None, M))
