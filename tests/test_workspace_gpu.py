"""GPU: every entry point runs in a workspace of exactly the size its query reports.

ops.workspace hands every call max(nbytes, 1 MiB) and passes the buffer's size, so a size query that
under-reports by less than that, or a region carved past the reported size, passes the rest of the suite.
Here ops.workspace / ops.scratch are replaced by an allocator that gives the library a view of exactly
nbytes, followed by a 1 MiB guard filled with a byte pattern.  After each call the guard must be untouched
and the result must equal the same call made with the ordinary cached workspace: bitwise for the Gram and
PDE forwards (deterministic kernels, held bitwise elsewhere in the suite), max|got - ref| / max|ref| <= 1e-5
(the suite's normalised criterion) for the other forwards and for the gradients, which accumulate with
atomics.  One case per carve site, at the smallest shape that reaches it (thresholds read off the geometry
functions: W = 4 cells for the split diagnostic from 33 points, the matrix-core Gram's column-block carries
past 160 points, the register VJP's column blocks past 256, the higher-order VJP's global slabs past 509).
"""
import numpy as np
import pytest
import torch

from conftest import norm_rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 1 << 20
PATTERN = 0xA5
M = 3


class GuardedAllocator:
    def __init__(self):
        self.bufs = []

    def alloc(self, device, nbytes):
        buf = torch.empty(int(nbytes) + GUARD, dtype=torch.uint8, device=device)
        buf[int(nbytes):].fill_(PATTERN)
        self.bufs.append((buf, int(nbytes)))
        return buf[:int(nbytes)]

    def scratch(self, device, nbytes):
        return self.alloc(device, nbytes) if nbytes > 0 else None

    def check(self):
        assert self.bufs, "the call asked for no workspace"
        torch.cuda.synchronize()
        for buf, n in self.bufs:
            assert bool((buf[n:] == PATTERN).all()), f"guard after a {n}-byte workspace was written"


def walks(n, l, d, seed):
    rng = np.random.default_rng(seed)
    x = np.cumsum(rng.standard_normal((n, l, d)), axis=1) / np.sqrt(l * d)
    return torch.as_tensor(x, device=DEV, dtype=torch.float32)


def randn(shape, seed, scale=1.0):
    return torch.as_tensor(np.random.default_rng(seed).standard_normal(shape) * scale, device=DEV, dtype=torch.float32)


def tensors(m, t, d, seed, increments=False):
    shape = (m * (m + 1) // 2, t, 2, d) if increments else (m * (m + 1) // 2, t, d)
    return randn(shape, seed, 1.0 / np.sqrt(d))


def guarded(monkeypatch, run, bitwise):
    """run() with the cached workspaces, then with exact-size guarded ones; the guards and the results."""
    from gpsig_amd import ops
    ref = run()
    g = GuardedAllocator()
    with monkeypatch.context() as mp:
        mp.setattr(ops, "workspace", g.alloc)
        mp.setattr(ops, "scratch", g.scratch)
        got = run()
        g.check()
    ref = ref if isinstance(ref, (tuple, list)) else (ref,)
    got = got if isinstance(got, (tuple, list)) else (got,)
    assert len(ref) == len(got)
    for r, o in zip(ref, got):
        if r is None:
            assert o is None
        elif bitwise:
            assert torch.equal(o, r)
        else:
            err = norm_rel_err(o.cpu().numpy(), r.cpu().numpy())
            print(f"normalised error {err:.3e}")
            assert err <= 1e-5


# ------------------------------------------------------------------------------------ Gram forward
@pytest.mark.parametrize("mode", ["rect", "upper", "diag"])
def test_gram_fixed_channels(monkeypatch, mode):
    from gpsig_amd import ops
    X, Y = walks(5, 8, 3, 1), walks(4, 8, 3, 2)
    run = {"rect": lambda: ops.sig_gram(X, Y, M), "upper": lambda: ops.sig_gram(X, None, M),
           "diag": lambda: ops.sig_diag(X, M)}[mode]
    guarded(monkeypatch, run, bitwise=True)


def test_gram_saved_state(monkeypatch):
    from gpsig_amd import ops
    X, Y = walks(5, 8, 3, 3), walks(4, 8, 3, 4)

    def run():
        st = torch.zeros(ops.sig_state_numel(5, 4, 8, M), dtype=torch.float32, device=DEV)
        return ops.sig_gram(X, Y, M, state=st), st
    guarded(monkeypatch, run, bitwise=True)


def test_gram_split_diagnostic(monkeypatch):
    from gpsig_amd import _lib as L
    from gpsig_amd import ops
    X, Y = walks(5, 33, 3, 5), walks(4, 33, 3, 6)  # 33 points: the first geometry with W = 4 columns per lane
    assert L.load().gpsig_sig_split_bytes(33, 33, 3, M) > 0
    for Yt in (None, Y):
        guarded(monkeypatch, lambda: ops.sig_gram(X, Yt, M, base=L.BASE_RBF | L.GRAM_SPLIT), bitwise=True)


def test_gram_wide_diagonal_tiles(monkeypatch):
    from gpsig_amd import ops
    X = walks(5, 8, 9, 7)
    guarded(monkeypatch, lambda: ops.sig_diag(X, M), bitwise=True)
    guarded(monkeypatch, lambda: ops.sig_diag(X, M, base="linear"), bitwise=True)  # the channel loop, no tiles


@pytest.mark.parametrize("l", [8, 161])  # 161: the shortest sequence with column-block carries
def test_gram_matrix_core(monkeypatch, l):
    from gpsig_amd import ops
    X, Y = walks(5, l, 9, 8), walks(4, l, 9, 9)
    guarded(monkeypatch, lambda: ops.sig_gram(X, Y, M), bitwise=True)
    guarded(monkeypatch, lambda: ops.sig_gram(X, None, M), bitwise=True)


def test_gram_higher_order_and_increment_tiles(monkeypatch):
    from gpsig_amd import ops
    X, Y = walks(5, 8, 3, 10), walks(4, 8, 3, 11)
    guarded(monkeypatch, lambda: ops.sig_gram(X, Y, M, order=2), bitwise=True)
    Xw, Yw = walks(5, 8, 33, 12), walks(4, 8, 33, 13)  # past 32 channels: cells from an increment-Gram tile
    guarded(monkeypatch, lambda: ops.sig_gram(Xw, Yw, M, order=2, base="rbf"), bitwise=True)
    guarded(monkeypatch, lambda: ops.sig_gram(Xw, None, M, order=2, base="rbf"), bitwise=True)


# ------------------------------------------------------------------------------------ Gram VJP
def gram_vjp_case(monkeypatch, n, l, d, order=1, base="rbf"):
    from gpsig_amd import ops
    X, Y = walks(n, l, d, 20), walks(n - 1, l, d, 21)
    G = randn((M + 1, n, n - 1), 22)
    Gs = randn((M + 1, n, n), 23)
    Gd = randn((M + 1, n), 24)
    sc = torch.ones(M + 1, dtype=torch.float32, device=DEV)

    def rect():
        gs = torch.zeros(M + 1, dtype=torch.float32, device=DEV)
        gX, gY = ops.sig_gram_vjp(X, Y, M, G, base=base, gout_levels=True, order=order, scale=sc, gscale=gs)
        return gX, gY, gs
    guarded(monkeypatch, rect, bitwise=False)
    guarded(monkeypatch, lambda: ops.sig_gram_vjp(X, None, M, Gs, base=base, gout_levels=True, order=order), bitwise=False)
    guarded(monkeypatch, lambda: ops.sig_gram_vjp(X, None, M, Gd, base=base, diag=True, order=order), bitwise=False)


def test_gram_vjp_fixed_channels(monkeypatch):
    gram_vjp_case(monkeypatch, 5, 8, 3)


def test_gram_vjp_saved_state(monkeypatch):
    from gpsig_amd import ops
    X, Y = walks(5, 8, 3, 25), walks(4, 8, 3, 26)
    G = randn((5, 4), 27)
    st = torch.zeros(ops.sig_state_numel(5, 4, 8, M), dtype=torch.float32, device=DEV)
    ops.sig_gram(X, Y, M, state=st)
    guarded(monkeypatch, lambda: ops.sig_gram_vjp(X, Y, M, G, state=st), bitwise=False)


def test_gram_vjp_column_blocks(monkeypatch):
    gram_vjp_case(monkeypatch, 5, 257, 3)  # 257: past one block of 64 lanes x 4 columns, the scratch region exists


def test_gram_vjp_wide_channels(monkeypatch):
    gram_vjp_case(monkeypatch, 5, 8, 17)


@pytest.mark.parametrize("l", [8, 510])  # 510: the shortest sequence on the 8-wave kernel's global slabs
def test_gram_vjp_higher_order(monkeypatch, l):
    from gpsig_amd import _lib as Lb
    assert (Lb.load().gpsig_sig_vjp_ho_workspace_bytes(5, 510, 4, 510, 3, M, 2, Lb.BASE_RBF) >
            Lb.load().gpsig_sig_vjp_ho_workspace_bytes(5, 509, 4, 509, 3, M, 2, Lb.BASE_RBF) + (1 << 16))
    gram_vjp_case(monkeypatch, 5 if l == 8 else 3, l, 3, order=2)


# ------------------------------------------------------------------------------------ PDE
@pytest.mark.parametrize("l,d,dyadic", [(8, 17, 0), (4, 3, 4)])
def test_pde_forward(monkeypatch, l, d, dyadic):
    from gpsig_amd import _lib as Lb
    from gpsig_amd import ops
    X, Y = walks(5, l, d, 30), walks(4, l, d, 31)
    assert d <= 16 or Lb.load().gpsig_pde_scratch_bytes(5, l, 4, l, d, dyadic, Lb.PAIRS_RECT) > 0
    g = GuardedAllocator()
    for run in (lambda: ops.pde_gram(X, Y, dyadic), lambda: ops.pde_gram(X, None, dyadic), lambda: ops.pde_diag(X, dyadic)):
        if d > 16:
            guarded(monkeypatch, run, bitwise=True)
        else:  # no scratch on the fixed-channel kernels: the entry takes null
            ref = run()
            with monkeypatch.context() as mp:
                mp.setattr(ops, "scratch", g.scratch)
                assert torch.equal(run(), ref) and not g.bufs


@pytest.mark.parametrize("l,d,dyadic", [(8, 3, 0), (8, 17, 0), (4, 3, 4)])  # direct; tiled by channels, by dyadic order
def test_pde_vjp(monkeypatch, l, d, dyadic):
    from gpsig_amd import ops
    X, Y = walks(5, l, d, 32), walks(4, l, d, 33)
    G, Gd = randn((5, 4), 34), randn((5,), 35)
    guarded(monkeypatch, lambda: ops.pde_gram_vjp(X, Y, G, dyadic), bitwise=False)
    guarded(monkeypatch, lambda: ops.pde_diag_vjp(X, Gd, dyadic), bitwise=False)

    def fronts(diag):
        nb = ops.pde_fronts_bytes(5 if diag else 20, l, l, dyadic)
        fr = torch.zeros(nb // 4, dtype=torch.float32, device=DEV)
        K = ops.pde_fronts(X, None if diag else Y, dyadic, 1, fr, diag=diag)
        g = ops.pde_vjp_fronts(X, None if diag else Y, Gd if diag else G, dyadic, 1, fr, diag=diag)
        return (K, g) if diag else (K,) + tuple(g)
    if d > 16 or dyadic > 3:  # the fronts entries take a scratch only on the tiled adjoint
        guarded(monkeypatch, lambda: fronts(False), bitwise=False)
        guarded(monkeypatch, lambda: fronts(True), bitwise=False)


# ------------------------------------------------------------------------------------ inducing tensors, signatures
@pytest.mark.parametrize("d", [3, 12, 17])
def test_tens_vs_seq(monkeypatch, d):
    from gpsig_amd import ops
    Z, X = tensors(M, 4, d, 40), walks(5, 8, d, 41)
    G = randn((M + 1, 4, 5), 42)
    guarded(monkeypatch, lambda: ops.tens_vs_seq(Z, X, M), bitwise=False)

    def with_state():
        st = torch.zeros(ops.tens_state_numel(4, 5, M), dtype=torch.float32, device=DEV)
        return ops.tens_vs_seq(Z, X, M, state=st)
    guarded(monkeypatch, with_state, bitwise=False)
    guarded(monkeypatch, lambda: ops.tens_vs_seq_vjp(Z, X, M, G), bitwise=False)
    Zi = tensors(M, 4, d, 43, increments=True)
    guarded(monkeypatch, lambda: ops.tens_vs_seq_vjp(Zi, X, M, G, increments=True), bitwise=False)


def test_tens_gram_wide(monkeypatch):
    from gpsig_amd import ops
    Z = tensors(M, 4, 46, 44, increments=True)
    G = randn((M + 1, 4, 4), 45)
    guarded(monkeypatch, lambda: ops.tens_gram(Z, M, increments=True), bitwise=False)
    guarded(monkeypatch, lambda: ops.tens_gram_vjp(Z, M, G, increments=True), bitwise=False)


def test_rescaled(monkeypatch):
    from gpsig_amd import ops
    Z, X = tensors(M, 4, 3, 46), walks(5, 8, 3, 47)
    guarded(monkeypatch, lambda: ops.rescaled(Z, X, M), bitwise=False)


def test_signature_level_slabs(monkeypatch):
    from gpsig_amd import _lib as Lb
    from gpsig_amd import ops
    X = walks(2, 8, 6, 48)  # d = 6 at depth 6: past the LDS, the level slabs live in the workspace
    assert Lb.load().gpsig_signature_workspace_bytes(2, 6, 6, 0) > 0
    assert Lb.load().gpsig_signature_workspace_bytes(2, 6, 6, 1) > 0
    G = randn((2, int(Lb.load().gpsig_signature_channels(6, 6))), 49)
    guarded(monkeypatch, lambda: ops.signature(X, 6), bitwise=False)
    guarded(monkeypatch, lambda: ops.signature_vjp(X, 6, G), bitwise=False)
