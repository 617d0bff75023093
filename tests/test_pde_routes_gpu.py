"""GPU parity of the Goursat-PDE kernels (gpsig_pde_gram / gpsig_pde_diag, gpsig_pde_vjp, gpsig_pde_fronts,
gpsig_pde_vjp_fronts) at every dispatch route, route seam and gradient path, against the float64 oracle on the
fp32-rounded inputs the kernels receive.  Every case asks gpsig_pde_route (ops.pde_route: host only, the helpers of
the launch path) which instantiation the launch takes and asserts it before it compares values, so a retuned cost
model or threshold shows up here as a route failure, not as silently lost coverage.

Dispatch, as gpsig_amd/csrc has it (d = channels, n = dyadic order, REP = 2^n, IC / JC = l1 - 1 / l2 - 1 coarse
rows / columns, J = REP JC fine columns), and the parameter ids that reach each route:

forward (gpsig_pde_gram_ex / gpsig_pde_diag_ex, pde.hip: pde_launch_args -> pde_w)
  DP (pde_dp): d for d <= 8, 16 with channels k >= d masked for d = 9 .. 16, 0 = increment tiles for d > 16
      DP 1 .. 8, 16 (d = 9, 12, 16), tiles (d = 17)   test_channels[d-n-s], d in 1..9, 12, 16, 17, n in 0, 1, s in 0, 1
                                                      (cross, symmetric, diagonal; s = 1 and d <= 8: lane group (16, 8))
  lane groups pde_rep_kernel<DP, W, REP, 1, LP> (solver 1, not DIAG, d <= 8, n <= 2; pde_pick_lp's cost model);
  ids g<LP>x<W>-rep<REP>-J<J>-d<d> of test_lane_groups, the first at J = LP W, the second the first J past the
  geometry before it; "pair-..." ids are one column past the widest group and land on one pair per wave
      (16, 8)   REP 1, 2, 4   g16x8-rep1-J128-d8 (registers: 8 x 8 = 64)  g16x8-rep2-J128-d8  g16x8-rep4-J128-d8
      (16, 14)  REP 1, 2      g16x14-rep1-J224-d4 g16x14-rep1-J129-d4     g16x14-rep2-J224-d8 g16x14-rep2-J130-d8
      (16, 16)  REP 1, 2, 4   g16x16-rep1-J256-d4 (16 x 4 = 64) g16x16-rep1-J225-d4   g16x16-rep2-J256-d8 (8 x 8 = 64)
                              g16x16-rep2-J226-d8   g16x16-rep4-J256-d8 g16x16-rep4-J132-d8
      (16, 24)  REP 1, 2, 4   g16x24-rep1-J384-d2 g16x24-rep1-J257-d2     g16x24-rep2-J384-d5 g16x24-rep2-J258-d5
                              g16x24-rep4-J384-d8 g16x24-rep4-J260-d8
      (16, 26)  REP 1, 2      g16x26-rep1-J416-d2 g16x26-rep1-J385-d2     g16x26-rep2-J416-d5 (13 x 5 = 65, its own
                              budget) g16x26-rep2-J386-d5
      (32, 8)   REP 1, d >= 5 g32x8-rep1-J256-d8 (8 x 8 = 64) g32x8-rep1-J129-d8   then pair-rep1-J257-d8
      (32, 14)  REP 1, 2      g32x14-rep1-J448-d4 g32x14-rep1-J257-d4 g32x14-rep1-J417-d2   g32x14-rep2-J448-d8
                              g32x14-rep2-J258-d8 g32x14-rep2-J418-d5
      (32, 16)  REP 1, 2, 4   g32x16-rep1-J512-d4 g32x16-rep1-J449-d4 then pair-rep1-J513-d4   g32x16-rep2-J512-d8
                              (8 x 8 = 64) g32x16-rep2-J450-d8 then pair-rep2-J514-d8   g32x16-rep4-J512-d8
                              g32x16-rep4-J388-d8
      (32, 24)  REP 1, 2, 4   g32x24-rep1-J768-d2 g32x24-rep1-J513-d2 then pair-rep1-J769-d2   g32x24-rep2-J768-d5
                              g32x24-rep2-J514-d5 then pair-rep2-J770-d5   g32x24-rep4-J768-d8 g32x24-rep4-J516-d8
                              then pair-rep4-J772-d8
      unreachable at any shape: (16, 14), (16, 26), (32, 14) at REP 4 (W is no multiple of REP); (32, 8) at REP 2
      and 4 and at REP 1 with d <= 4 ((16, 16) holds the same columns in the registers with twice the pairs per
      wave at a lower estimate; a scan of the query over l1, l2 <= 1100 and d <= 8 agrees)
      the symmetric Gram of the same length takes the same geometry except where long x tips the estimate back
      to one pair per wave (the last column of LANE_CASES); both are asserted
  one pair per wave pde_rep_kernel<DP, W, REP, solver> (solver 0, DIAG, d = 9 .. 16, longer grids; W = pde_w64)
      REP 1, 2, 4: W = REP, 2 REP, 3 REP, 4 REP at JC <= 64, 128, 192, 256; two column blocks past 256
                              test_one_pair_per_wave[rep<REP>-JC<64|65|128|129|192|193|256|257>]
      REP 8: W = 8, 16, two blocks          [rep8-JC64] [rep8-JC65] [rep8-JC128] [rep8-JC129]
      REP 16: W = 16, one and two blocks    [rep16-JC64] [rep16-JC65]
      each: solver-0 cross pairs (DP 3), solver-1 cross pairs at d = 12 (DP 16), DIAG with both solvers; DIAG +
      solver 0 (the hybrid diagonal cell, c0 + lane W + w == i) inside the second column block: [rep1|2|4-JC257]
      and with 128 REP diagonal cells in lanes 0 .. 31 of the second block: test_hybrid_diagonal_in_second_block[rep1|2|4]
  increment tiles pde_rep_kernel<0, W, REP> (d > 16 or n > 4)
      sub = 0                 test_channels[17-*], test_row_windows[tile-*], test_symmetric_gradient[17-*],
                              test_tile_chunk_loop (two chunks of x-rows, the second partial)
      sub > 0 (n > 4)         tests/test_pde_wide_gpu.py (dyadic 5 .. 8); not repeated here
  per-row pde_kernel<DP, W>   unreachable: launch_pde_rep refuses only (W / REP) DP > 64, and pde_w64 keeps
                              W / REP <= 4 (REP <= 4) or W <= 16 (REP 8, 16) with DP <= 16; REP > 16 never reaches
                              pde_rep_w (pde_tiled).  Recorded in DESIGN.md 2.5.
  rows=(r0, r1), out, out_row0  test_row_windows[lane|pair|tile-r0-r1], (r0, r1) in (1, 6), (5, 7), (6, 11)

adjoint (gpsig_pde_vjp_ex, gpsig_pde_fronts_ex, gpsig_pde_vjp_fronts_ex; pde_bwd.hip pde_adj_impl, pde_bwd.h)
  pde_adj_kernel<DP, W, REP, COLS, MODE>: DP as the forward   test_channels (cross: COLS, MODE 0; diagonal)
  W (pde_bwd_cols: the power of two from REP with 64 W >= J, at most 16, REP 8: 8), H = max(1, 32 / (REP W))
  steps per stored front, column blocks of 64 W:
      REP 1: W 1|2|4|8|16, H 32|16|8|4|2, 1 -> 2 -> 3 blocks   test_adjoint_column_seams[rep1-JC64 .. JC2049]
      REP 2: W 2|4|8|16, H 8|4|2|1, 1 -> 2 -> 3 blocks         [rep2-JC64 .. JC1025]
      REP 4: W 4|8|16, H 2|1|1, 1 -> 2 -> 3 blocks             [rep4-JC64 .. JC513]
      REP 8: W 8, H 1, 1 -> 2 -> 3 blocks                      [rep8-JC64 .. JC129]
      each: MODE 0, and MODE 1 + MODE 2 (the fronts split), cross and (to 1025 points) diagonal
  IC + U - 1 at a multiple of H, one less, one more    test_adjoint_front_chunks[rep1-W1-H32|rep2-W2-H8|rep1-W8-H4|
                                                       rep4-W4-H2 - off - solver]
  pairs per workgroup (pde_adj_wpb): 4; 2 and 1 for long x at DP 16   test_adjoint_pairs_per_workgroup[l200-wpb2-
                              fronts4] (MODE 1 still 4) [l220-wpb2] [l450-wpb1]
  row windows off the row tiles (ta0 = row_begin / wpb; tiles: c0 > r0)   test_adjoint_row_windows[wpb4|wpb2|wpb1|
                              tile - r0 - r1], (r0, r1) in (1, 4), (3, 5), through the C entry
  increment tiles (pde_adj_tiled; d > 16 or n > 3, kernel cells 2^sub finer, REP 8 layout)
      sub = 0                 test_channels[17-*], test_symmetric_gradient[17-0|1], test_tile_chunk_loop
      sub = 1                 test_symmetric_gradient[3-4] [12-4] [17-4]
  symmetric K(X): RECT launch with Y = X, gY aliased onto gX   test_symmetric_gradient[d-n], d in 3, 12, 17,
                              n in 0, 1, 4: ops, autograd with the fronts kept, autograd recomputing them

References: values oracle.pde.pde_gram / pde_diag (C restatement of sigKer_fast.pyx), cross adjoint
oracle.pde.pde_gram_grad (pinned to oracle/pde_grad.py on the CPU, tests/test_pde_grad.py), k(x, x) adjoint
oracle/pde_grad.py kdiag_grad on the restated grids (with solver 0 its diagonal cells take the second-order update).
The adjoint is the reference's continuous-PDE adjoint, not the derivative of the discrete solve: finite differences
are no reference.  Criterion: max|got - ref| < 1e-5 max|ref| for values and per gradient array.
Every test prints its figures before it asserts, asserts that its reference is not degenerate (K away from 1,
gradients away from 0) and that the edge it aims at matters: the oracle with the last channel zeroed (channel
tests) or the last time point of y dropped (length seams) differs from the reference by more than 100 x the
tolerance.
"""
import os

import numpy as np
import pytest
import torch

from conftest import norm_rel_err
from oracle import kernels_ref as kr
from oracle import pde, pde_grad

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif("GPSIG_PDE_LP" in os.environ,
                                 reason="GPSIG_PDE_LP pins the lane group: the routes asserted here are the cost model's")]
DEV = "cuda"
TOL = 1e-5    # values
GTOL = 1e-5   # per gradient array
EDGE = 100 * TOL
RECT, UPPER, DIAG = 0, 1, 2
# observed maxima on an MI355X, values / gradients: a. channels 4.9e-7 / 8.6e-7; b. lane groups 3.2e-7; c. one pair
# per wave 2.9e-7 (hybrid diagonal in the second block 2.5e-7, per sequence); d. adjoint seams 9.3e-7, front chunks 3.7e-7, pairs per workgroup 2.8e-7; e. row windows 1.7e-7;
# f. tile chunk loop 3.3e-8 / 8.4e-7; g. symmetric gradient 3.6e-7 / 3.8e-7; h. kernel class 2.9e-7 / 4.0e-7; i. edges
# 6.0e-7 / 4.8e-7 (small), 1.2e-7 / 1.5e-7 (constant, identical), 1.1e-7 / 2.7e-7 (large), 5.8e-8 / 3.3e-7 (small
# increments).  No case was ever outside the criterion: no before / after figures to record.


def f32(x):
    return np.asarray(x).astype(np.float32).astype(np.float64)


def walks(rng, n, L, d, scale=2.0):
    """Random walks at the scale of the other PDE tests (tests/test_pde_wide_gpu.py paths), rounded to fp32."""
    return f32(np.cumsum(rng.standard_normal((n, L, d)), 1) / np.sqrt(L * d) * scale)


def t(x):
    return torch.tensor(np.asarray(x), device=DEV, dtype=torch.float32)


def route(l1, l2, d, n, solver, pm, adjoint=False):
    from gpsig_amd import ops
    return ops.pde_route(l1, l2, d, n, solver, pm, adjoint)


def expect(r, **kv):
    for k, v in kv.items():
        assert r[k] == v, (k, v, r)


def check(tag, got, ref, tol=TOL, floor=1e-3):
    """Norm-relative parity; the reference must not be degenerate (values: away from 1; gradients: away from 0)."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (tag, got.shape, ref.shape)
    assert np.isfinite(got).all(), tag
    err = norm_rel_err(got, ref)
    print(f"{tag}: {err:.2e}")
    assert np.abs(ref).max() > floor, (tag, "degenerate reference")
    assert err < tol, (tag, err)
    return err


def matters(tag, ref_edge, ref):
    """The edge the case aims at carries weight: without it the oracle moves by more than 100 x the tolerance."""
    dev = norm_rel_err(ref_edge, ref)
    print(f"{tag}: edge weight {dev:.2e}")
    assert dev > EDGE, (tag, dev)


def away_from_one(tag, ref):
    assert np.abs(np.asarray(ref) - 1.0).max() > 1e-2, (tag, "degenerate reference: K = 1")


def zero_last_channel(X):
    Z = X.copy()
    Z[..., -1] = 0.0
    return Z


def diag_grad_ref(X, w, n, solver):
    """sum_a w[a] dk(x_a, x_a)/dX by _KdiagGrad restated (oracle/pde_grad.py) on the C grids."""
    K, Kr = pde.pde_diag_grids(X, n, solver)
    return pde_grad.kdiag_grad(X, np.tril(K), np.tril(Kr), n) * np.asarray(w)[:, None, None]


def diag_grad_ref_c(X, w, n):
    """The same for solver 1 by the C adjoint of the pairs (x_a, x_a) (x-part + y-part): no (A, G, G) NumPy grids,
    for long sequences."""
    ref = np.zeros_like(X)
    for a in range(len(X)):
        gx, gy = pde.pde_gram_grad(X[a:a + 1], X[a:a + 1], np.ones((1, 1)), n, 1)
        ref[a] = w[a] * (gx[0] + gy[0])
    return ref


def fronts_split(tag, X, Y, G, n, solver, rx, ry, Kgram):
    """The training step's split at this shape: gpsig_pde_fronts' values are gpsig_pde_gram's bit for bit, and
    gpsig_pde_vjp_fronts from its fronts is held against the oracle."""
    from gpsig_amd import ops
    fr = torch.empty(ops.pde_fronts_bytes(len(X) * len(Y), X.shape[1], Y.shape[1], n) // 4, device=DEV)
    K = ops.pde_fronts(t(X), t(Y), n, solver, fr)
    torch.testing.assert_close(K, Kgram, rtol=0, atol=0)
    fX, fY = ops.pde_vjp_fronts(t(X), t(Y), t(G), n, solver, fr)
    return max(check(f"{tag} fronts dX", fX.cpu().numpy(), rx, GTOL), check(f"{tag} fronts dY", fY.cpu().numpy(), ry, GTOL))


def fronts_split_diag(tag, X, w, n, solver, ref, Kdiag):
    from gpsig_amd import ops
    l = X.shape[1]
    fr = torch.empty(ops.pde_fronts_bytes(len(X), l, l, n) // 4, device=DEV)
    kd = ops.pde_fronts(t(X), None, n, solver, fr, diag=True)
    torch.testing.assert_close(kd, Kdiag, rtol=0, atol=0)
    gd = ops.pde_vjp_fronts(t(X), None, t(w), n, solver, fr, diag=True)
    return check(f"{tag} fronts diag dX", gd.cpu().numpy(), ref, GTOL)


def dp_of(d):
    return d if d <= 8 else (16 if d <= 16 else 0)


def expect_short_routes(l1, l2, d, n, solver, lane=(16, 8), lane_sym=(16, 8)):
    """Routes of a short shape (one column block, J <= 64 REP, n <= 3), asserted for every entry the edge tests
    run: forward cross / symmetric / diagonal, adjoint cross / diagonal.  lane, lane_sym: the lane group of the
    solver-1 cross / symmetric Gram at d <= 8 (None: the cost model leaves it at one pair per wave)."""
    rep, tile = 1 << n, d > 16
    for pm, la, lb, g in ((RECT, l1, l2, lane), (UPPER, l1, l1, lane_sym), (DIAG, l1, l1, None)):
        if tile:
            expect(route(la, lb, d, n, solver, pm), family="tile", DP=0, REP=rep, W=rep, LP=64, nblk=1, sub=0)
        elif solver == 1 and d <= 8 and g is not None:
            expect(route(la, lb, d, n, solver, pm), family="lane_group", DP=d, REP=rep, W=g[1], LP=g[0], nblk=1, sub=0)
        else:
            expect(route(la, lb, d, n, solver, pm), family="pair", DP=dp_of(d), REP=rep, W=rep, LP=64, nblk=1, sub=0)
    for pm, lb in ((RECT, l2), (DIAG, l1)):
        expect(route(l1, lb, d, n, solver, pm, True), tiled=int(tile), DP=dp_of(d), REP=rep, W=rep,
               H=max(1, 32 // (rep * rep)), nblk=1, sub=0, wpb=4, wpb_fronts=4)


# ----------------------------------------------------------------------------- a. channels
@pytest.mark.parametrize("solver", [0, 1])
@pytest.mark.parametrize("n", [0, 1])
@pytest.mark.parametrize("d", [1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 16, 17])
def test_channels(d, n, solver):
    """Every channel instantiation (DP = d for d <= 8; DP = 16 with the channels k >= d masked for d = 9 .. 16;
    d = 17: the first increment-tile count), forward and adjoint, cross / symmetric / diagonal."""
    from gpsig_amd import ops
    tag = f"chan-d{d}-n{n}-s{solver}"
    rng = np.random.default_rng(1000 + 100 * d + 10 * n + solver)
    l1, l2 = 11, 9
    X, Y = walks(rng, 7, l1, d), walks(rng, 5, l2, d)
    rep = 1 << n
    lane = solver == 1 and d <= 8
    fam = "tile" if d > 16 else ("lane_group" if lane else "pair")
    for pm, la, lb in ((RECT, l1, l2), (UPPER, l1, l1)):
        expect(route(la, lb, d, n, solver, pm), family=fam, DP=dp_of(d), REP=rep, LP=16 if lane else 64,
               W=8 if lane else rep, nblk=1, sub=0)
    expect(route(l1, l1, d, n, solver, DIAG), family="tile" if d > 16 else "pair", DP=dp_of(d), REP=rep, LP=64, W=rep,
           nblk=1, sub=0)
    for pm, lb in ((RECT, l2), (DIAG, l1)):
        expect(route(l1, lb, d, n, solver, pm, True), tiled=int(d > 16), DP=dp_of(d), REP=rep, W=rep,
               H=32 // (rep * rep), nblk=1, sub=0, wpb=4, wpb_fronts=4)

    ref = pde.pde_gram(X, Y, n, solver)
    away_from_one(tag, ref)
    matters(tag, pde.pde_gram(zero_last_channel(X), zero_last_channel(Y), n, solver), ref)
    Kx = ops.pde_gram(t(X), t(Y), n, solver)
    check(f"{tag} cross", Kx.cpu().numpy(), ref)
    S = ops.pde_gram(t(X), None, n, solver).cpu().numpy()
    check(f"{tag} sym", S, pde.pde_gram(X, X, n, solver))
    np.testing.assert_array_equal(S, S.T)
    Kd = ops.pde_diag(t(X), n, solver)
    check(f"{tag} diag", Kd.cpu().numpy(), pde.pde_diag(X, n, solver))

    G = f32(rng.standard_normal((7, 5)))
    rx, ry = pde.pde_gram_grad(X, Y, G, n, solver)
    zx, _ = pde.pde_gram_grad(zero_last_channel(X), zero_last_channel(Y), G, n, solver)
    matters(f"{tag} dX", zx, rx)
    gX, gY = ops.pde_gram_vjp(t(X), t(Y), t(G), n, solver)
    check(f"{tag} dX", gX.cpu().numpy(), rx, GTOL)
    check(f"{tag} dY", gY.cpu().numpy(), ry, GTOL)
    w = f32(rng.standard_normal(7))
    rd = diag_grad_ref(X, w, n, solver)
    check(f"{tag} diag dX", ops.pde_diag_vjp(t(X), t(w), n, solver).cpu().numpy(), rd, GTOL)


# ----------------------------------------------------------------------------- b. lane groups
# id, l1, l2, d, dyadic, the (LP, W) the cost model picks for the l1 x l2 cross pairs and for the symmetric Gram of
# sequences of length l2 (None: one pair per wave; the model weighs the skew IC + U - 1, so long x can tip it back).
# Each geometry: its last J (= LP W where the id says so) and the first J past the one before it.
LANE_CASES = [
    ('g16x8-rep1-J128-d8', 9, 129, 8, 0, (16, 8), (16, 8)),
    ('g32x8-rep1-J129-d8', 9, 130, 8, 0, (32, 8), (32, 8)),
    ('g16x14-rep1-J129-d4', 9, 130, 4, 0, (16, 14), (16, 14)),
    ('g16x14-rep1-J224-d4', 9, 225, 4, 0, (16, 14), (16, 14)),
    ('g16x16-rep1-J225-d4', 9, 226, 4, 0, (16, 16), (16, 16)),
    ('g16x16-rep1-J256-d4', 9, 257, 4, 0, (16, 16), (16, 16)),
    ('g32x14-rep1-J257-d4', 9, 258, 4, 0, (32, 14), None),
    ('g16x24-rep1-J257-d2', 9, 258, 2, 0, (16, 24), (16, 24)),
    ('g16x24-rep1-J384-d2', 9, 385, 2, 0, (16, 24), (16, 24)),
    ('g16x26-rep1-J385-d2', 9, 386, 2, 0, (16, 26), None),
    ('g16x26-rep1-J416-d2', 9, 417, 2, 0, (16, 26), None),
    ('g32x14-rep1-J417-d2', 9, 418, 2, 0, (32, 14), None),
    ('g32x8-rep1-J256-d8', 9, 257, 8, 0, (32, 8), (32, 8)),
    ('pair-rep1-J257-d8', 9, 258, 8, 0, None, None),
    ('g32x14-rep1-J448-d4', 9, 449, 4, 0, (32, 14), None),
    ('g32x16-rep1-J449-d4', 9, 450, 4, 0, (32, 16), None),
    ('g32x16-rep1-J512-d4', 9, 513, 4, 0, (32, 16), None),
    ('pair-rep1-J513-d4', 9, 514, 4, 0, None, None),
    ('g32x24-rep1-J513-d2', 9, 514, 2, 0, (32, 24), None),
    ('g32x24-rep1-J768-d2', 9, 769, 2, 0, (32, 24), None),
    ('pair-rep1-J769-d2', 9, 770, 2, 0, None, None),
    ('g16x8-rep2-J128-d8', 9, 65, 8, 1, (16, 8), (16, 8)),
    ('g16x14-rep2-J130-d8', 9, 66, 8, 1, (16, 14), (16, 14)),
    ('g16x14-rep2-J224-d8', 9, 113, 8, 1, (16, 14), (16, 14)),
    ('g16x16-rep2-J226-d8', 9, 114, 8, 1, (16, 16), (16, 16)),
    ('g16x16-rep2-J256-d8', 9, 129, 8, 1, (16, 16), (16, 16)),
    ('g32x14-rep2-J258-d8', 9, 130, 8, 1, (32, 14), (32, 14)),
    ('g16x24-rep2-J258-d5', 9, 130, 5, 1, (16, 24), (16, 24)),
    ('g16x24-rep2-J384-d5', 9, 193, 5, 1, (16, 24), (16, 24)),
    ('g16x26-rep2-J386-d5', 9, 194, 5, 1, (16, 26), (16, 26)),
    ('g16x26-rep2-J416-d5', 9, 209, 5, 1, (16, 26), (16, 26)),
    ('g32x14-rep2-J418-d5', 9, 210, 5, 1, (32, 14), (32, 14)),
    ('g32x14-rep2-J448-d8', 9, 225, 8, 1, (32, 14), (32, 14)),
    ('g32x16-rep2-J450-d8', 9, 226, 8, 1, (32, 16), (32, 16)),
    ('g32x16-rep2-J512-d8', 9, 257, 8, 1, (32, 16), (32, 16)),
    ('pair-rep2-J514-d8', 9, 258, 8, 1, None, None),
    ('g32x24-rep2-J514-d5', 9, 258, 5, 1, (32, 24), None),
    ('g32x24-rep2-J768-d5', 9, 385, 5, 1, (32, 24), None),
    ('pair-rep2-J770-d5', 9, 386, 5, 1, None, None),
    ('g16x8-rep4-J128-d8', 9, 33, 8, 2, (16, 8), (16, 8)),
    ('g16x16-rep4-J132-d8', 9, 34, 8, 2, (16, 16), (16, 16)),
    ('g16x16-rep4-J256-d8', 9, 65, 8, 2, (16, 16), (16, 16)),
    ('g16x24-rep4-J260-d8', 9, 66, 8, 2, (16, 24), (16, 24)),
    ('g16x24-rep4-J384-d8', 9, 97, 8, 2, (16, 24), (16, 24)),
    ('g32x16-rep4-J388-d8', 9, 98, 8, 2, (32, 16), (32, 16)),
    ('g32x16-rep4-J512-d8', 9, 129, 8, 2, (32, 16), (32, 16)),
    ('g32x24-rep4-J516-d8', 9, 130, 8, 2, (32, 24), (32, 24)),
    ('g32x24-rep4-J768-d8', 9, 193, 8, 2, (32, 24), (32, 24)),
    ('pair-rep4-J772-d8', 9, 194, 8, 2, None, None),
]


@pytest.mark.parametrize("l1,l2,d,n,geom,gsym", [pytest.param(*c[1:], id=c[0]) for c in LANE_CASES])
def test_lane_groups(l1, l2, d, n, geom, gsym):
    """Solver-1 Gram pairs in lane groups: each (LP, W, REP) the cost model reaches, at J = LP W (or the longest J
    it still sends there), one coarse column past it, and at the register limit (W / REP) DP = 64 (65 at W = 26).
    7 x 5 cross pairs and 7 symmetric sequences: two rows of workgroups, and a last lane group that is partial."""
    from gpsig_amd import ops
    tag = f"lane-l{l1}x{l2}-d{d}-n{n}"
    rng = np.random.default_rng(2000 + 7 * l1 + 3 * l2 + 11 * d + n)
    rep = 1 << n
    X, Y = walks(rng, 7, l1, d), walks(rng, 5, l2, d)
    Z = walks(rng, 7, l2, d)
    J = rep * (l2 - 1)
    for pm, la, g in ((RECT, l1, geom), (UPPER, l2, gsym)):
        r = route(la, l2, d, n, 1, pm)
        if g is None:
            expect(r, family="pair", LP=64, DP=d, REP=rep)
        else:
            expect(r, family="lane_group", LP=g[0], W=g[1], DP=d, REP=rep, nblk=1, sub=0)
            assert g[0] * g[1] >= J and (g[1] // rep) * d <= (65 if g[1] == 26 else 64)
    ref = pde.pde_gram(X, Y, n, 1)
    away_from_one(tag, ref)
    matters(tag, pde.pde_gram(X, Y[:, :-1], n, 1), ref)
    check(f"{tag} cross", ops.pde_gram(t(X), t(Y), n, 1).cpu().numpy(), ref)
    S = ops.pde_gram(t(Z), None, n, 1).cpu().numpy()
    check(f"{tag} sym", S, pde.pde_gram(Z, Z, n, 1))
    np.testing.assert_array_equal(S, S.T)


# ----------------------------------------------------------------------------- c. one pair per wave
def w64(JC, rep):
    """pde_rep_w's geometry by coarse columns: (W, column blocks)."""
    if rep <= 4:
        W = rep * (1 if JC <= 64 else 2 if JC <= 128 else 3 if JC <= 192 else 4)
    else:
        W = 8 if (rep == 8 and JC <= 64) else 16
    return W, -(-JC * rep // (64 * W))


ONE_PAIR = [(n, jc) for n in (0, 1, 2) for jc in (64, 65, 128, 129, 192, 193, 256, 257)] + \
           [(3, 64), (3, 65), (3, 128), (3, 129), (4, 64), (4, 65)]


@pytest.mark.parametrize("n,JC", [pytest.param(n, jc, id=f"rep{1 << n}-JC{jc}") for n, jc in ONE_PAIR])
def test_one_pair_per_wave(n, JC):
    """pde_rep_kernel<DP, W, REP> with LP = 64 at every W seam of pde_rep_w (J = 64 REP, 128 REP, 192 REP, 256 REP and
    one coarse column more; the last is the first column block; REP 8: W 8 -> 16 -> two blocks; REP 16: one -> two
    blocks): solver-0 cross pairs, d = 12 (DP 16) solver-1 cross pairs, and k(x, x) with both solvers -- with solver
    0 the hybrid diagonal cell, inside the second column block at JC = 257."""
    from gpsig_amd import ops
    rep = 1 << n
    l2 = JC + 1
    tag = f"pair-rep{rep}-JC{JC}"
    W, nblk = w64(JC, rep)
    rng = np.random.default_rng(3000 + 10 * JC + n)
    worst = 0.0
    for d, solver in ((3, 0), (12, 1)):
        X, Y = walks(rng, 5, 9, d), walks(rng, 3, l2, d)
        expect(route(9, l2, d, n, solver, RECT), family="pair", DP=dp_of(d), REP=rep, W=W, LP=64, nblk=nblk, sub=0)
        ref = pde.pde_gram(X, Y, n, solver)
        away_from_one(tag, ref)
        matters(f"{tag} d{d}", pde.pde_gram(X, Y[:, :-1], n, solver), ref)
        worst = max(worst, check(f"{tag} cross d{d} s{solver}", ops.pde_gram(t(X), t(Y), n, solver).cpu().numpy(), ref))
    X = walks(rng, 5, l2, 3)
    for solver in (0, 1):
        expect(route(l2, l2, 3, n, solver, DIAG), family="pair", DP=3, REP=rep, W=W, LP=64, nblk=nblk, sub=0)
        ref = pde.pde_diag(X, n, solver)
        away_from_one(tag, ref)
        matters(f"{tag} diag", pde.pde_diag(X[:, :-1], n, solver), ref)
        worst = max(worst, check(f"{tag} diag s{solver}", ops.pde_diag(t(X), n, solver).cpu().numpy(), ref))
    if n <= 2 and JC == 257:
        # the hybrid cell alone: solver 0 with and without it differ (k(x, x) vs the cross pair (x, x))
        matters(f"{tag} hybrid", np.diag(pde.pde_gram(X, X, n, 0)), pde.pde_diag(X, n, 0))


def hybrid_kxx(x, n, upto):
    """k(x, x) by the first-order scheme with the second-order update on the diagonal cells i == j < upto (fine
    index): sigKer_fast.pyx:46-59 restated over anti-diagonals in NumPy.  upto past the grid is pde.pde_diag with
    solver 0; a smaller upto leaves the diagonal cells from there on to the first-order update."""
    rep = 1 << n
    dx = np.diff(x, axis=0)
    C = dx @ dx.T / (rep * rep)
    I = rep * len(dx)
    K = np.ones((I + 1, I + 1))
    for k in range(2 * I - 1):
        i = np.arange(max(0, k - I + 1), min(k, I - 1) + 1)
        j = k - i
        inc = C[i >> n, j >> n]
        new = K[i, j + 1] + K[i + 1, j] + K[i, j] * (inc - 1)
        dg = (i == j) & (i < upto)
        new[dg] = ((K[i, j + 1] + K[i + 1, j]) * (1 + 0.5 * inc + inc * inc / 12) - K[i, j] * (1 - inc * inc / 12))[dg]
        K[i + 1, j + 1] = new
    return K[-1, -1]


@pytest.mark.parametrize("n,scale", [pytest.param(0, 2.0, id="rep1"), pytest.param(1, 2.5, id="rep2"),
                                     pytest.param(2, 3.0, id="rep4")])
def test_hybrid_diagonal_in_second_block(n, scale):
    """k(x, x) with solver 0 at 384 coarse columns: the second column block (c0 = 256 REP) holds 128 REP diagonal
    cells in lanes 0 .. 31, found by c0 + lane W + w == i.  The restated oracle with the second-order update switched
    off on exactly those cells must move every value by more than 100 x the tolerance: a wrong c0 term cannot hide."""
    from gpsig_amd import ops
    rep, l, d = 1 << n, 385, 3
    tag = f"hybrid-rep{rep}"
    expect(route(l, l, d, n, 0, DIAG), family="pair", DP=d, REP=rep, W=4 * rep, LP=64, nblk=2, sub=0)
    rng = np.random.default_rng(3300 + n)
    X = walks(rng, 2, l, d, scale)
    ref = pde.pde_diag(X, n, 0)
    full = np.array([hybrid_kxx(x, n, rep * l) for x in X])
    np.testing.assert_allclose(full, ref, rtol=1e-12)          # the restatement is the oracle
    first_block_only = np.array([hybrid_kxx(x, n, 256 * rep) for x in X])
    weight = np.abs(first_block_only - ref) / np.abs(ref)
    print(f"{tag}: weight of the second block's diagonal cells {weight}")
    assert (weight > EDGE).all(), (tag, weight)
    away_from_one(tag, ref)
    got = ops.pde_diag(t(X), n, 0).cpu().numpy()
    err = np.abs(got - ref) / np.abs(ref)                      # per sequence: both hold the criterion on their own
    print(f"{tag} diag s0: {err.max():.2e}")
    assert (err < TOL).all(), (tag, err)


# ----------------------------------------------------------------------------- d. adjoint geometry
def bwd_cols(J, rep):
    wmax = 16 if rep * 16 <= 64 else 64 // rep
    W = rep
    while W <= wmax:
        if 64 * W >= J:
            return W
        W *= 2
    return wmax


ADJ_SEAMS = [(0, jc) for jc in (64, 65, 128, 129, 256, 257, 512, 513, 1024, 1025, 2048, 2049)] + \
            [(1, jc) for jc in (64, 65, 128, 129, 256, 257, 512, 513, 1024, 1025)] + \
            [(2, jc) for jc in (64, 65, 128, 129, 256, 257, 512, 513)] + \
            [(3, jc) for jc in (64, 65, 128, 129)]


@pytest.mark.parametrize("n,JC", [pytest.param(n, jc, id=f"rep{1 << n}-JC{jc}") for n, jc in ADJ_SEAMS])
def test_adjoint_column_seams(n, JC):
    """pde_adj_kernel<DP, W, REP> at every W seam of pde_bwd_cols (J = 64 W and one coarse column more, W = REP ..
    16, REP 8: W = 8 only), into the second and the third column block: cross pairs (gpsig_pde_vjp, and the
    gpsig_pde_fronts / gpsig_pde_vjp_fronts split) and k(x, x) up to 1025 points."""
    from gpsig_amd import ops
    rep = 1 << n
    l1, l2, d = 8, JC + 1, 3
    J = rep * JC
    W = bwd_cols(J, rep)
    nblk = -(-J // (64 * W))
    tag = f"adj-rep{rep}-JC{JC}"
    expect(route(l1, l2, d, n, 1, RECT, True), tiled=0, DP=d, REP=rep, W=W, H=max(1, 32 // (rep * W)), nblk=nblk, sub=0,
           wpb=4, wpb_fronts=4)
    rng = np.random.default_rng(4000 + 10 * JC + n)
    X, Y = walks(rng, 5, l1, d), walks(rng, 3, l2, d)
    G = f32(rng.standard_normal((5, 3)))
    rx, ry = pde.pde_gram_grad(X, Y, G, n, 1)
    ex, _ = pde.pde_gram_grad(X, Y[:, :-1], G, n, 1)
    matters(tag, ex, rx)
    gX, gY = ops.pde_gram_vjp(t(X), t(Y), t(G), n, 1)
    check(f"{tag} dX", gX.cpu().numpy(), rx, GTOL)
    check(f"{tag} dY", gY.cpu().numpy(), ry, GTOL)
    fronts_split(tag, X, Y, G, n, 1, rx, ry, ops.pde_gram(t(X), t(Y), n, 1))
    if JC <= 1025:
        Z = walks(rng, 3, l2, d)
        w = f32(rng.standard_normal(3))
        expect(route(l2, l2, d, n, 1, DIAG, True), tiled=0, DP=d, REP=rep, W=W, nblk=nblk)
        ref = diag_grad_ref_c(Z, w, n)
        check(f"{tag} diag dX", ops.pde_diag_vjp(t(Z), t(w), n, 1).cpu().numpy(), ref, GTOL)
        fronts_split_diag(tag, Z, w, n, 1, ref, ops.pde_diag(t(Z), n, 1))


@pytest.mark.parametrize("solver", [0, 1])
@pytest.mark.parametrize("off", [-1, 0, 1])
@pytest.mark.parametrize("n,JC,IC0", [pytest.param(0, 20, 13, id="rep1-W1-H32"), pytest.param(1, 10, 7, id="rep2-W2-H8"),
                                      pytest.param(0, 300, 7, id="rep1-W8-H4"), pytest.param(2, 40, 9, id="rep4-W4-H2")])
def test_adjoint_front_chunks(n, JC, IC0, off, solver):
    """The stored fronts: IC + U - 1 coarse steps at a multiple of the chunk H (the last chunk full), one less and
    one more (a last chunk of one step)."""
    from gpsig_amd import ops
    rep = 1 << n
    l1, l2, d = IC0 + off + 1, JC + 1, 4
    r = route(l1, l2, d, n, solver, RECT, True)
    U = -(-rep * JC // r["W"])
    assert r["nblk"] == 1 and r["H"] > 1 and (IC0 + U - 1) % r["H"] == 0, r
    tag = f"chunk-rep{rep}-H{r['H']}-{off:+d}-s{solver}"
    rng = np.random.default_rng(4500 + 10 * JC + n + off)
    X, Y = walks(rng, 5, l1, d), walks(rng, 3, l2, d)
    G = f32(rng.standard_normal((5, 3)))
    rx, ry = pde.pde_gram_grad(X, Y, G, n, solver)
    ex, _ = pde.pde_gram_grad(X[:, :-1], Y, G, n, solver)
    matters(tag, ex, rx[:, :-1])
    gX, gY = ops.pde_gram_vjp(t(X), t(Y), t(G), n, solver)
    check(f"{tag} dX", gX.cpu().numpy(), rx, GTOL)
    check(f"{tag} dY", gY.cpu().numpy(), ry, GTOL)
    fronts_split(tag, X, Y, G, n, solver, rx, ry, ops.pde_gram(t(X), t(Y), n, solver))


@pytest.mark.parametrize("l1,wpb,wpbf", [pytest.param(200, 2, 4, id="l200-wpb2-fronts4"), pytest.param(220, 2, 2, id="l220-wpb2"),
                                         pytest.param(450, 1, 1, id="l450-wpb1")])
def test_adjoint_pairs_per_workgroup(l1, wpb, wpbf):
    """Long x at d = 16: the per-wave LDS (row accumulators, dx, the cross pairs' column sums) leaves 2 pairs or 1
    pair per workgroup (tiles of wpb rows: ta0 = row_begin / wpb), n1 = 5 rows: a partial last tile; at l1 = 200 the
    fronts forward still takes 4 where the adjoint takes 2."""
    from gpsig_amd import ops
    d, l2, n = 16, 7, 0
    tag = f"wpb-l{l1}"
    expect(route(l1, l2, d, n, 1, RECT, True), tiled=0, DP=16, REP=1, W=1, nblk=1, wpb=wpb, wpb_fronts=wpbf)
    rd = route(l1, l1, d, n, 1, DIAG, True)
    expect(rd, tiled=0, DP=16, wpb=wpbf, wpb_fronts=wpbf)
    rng = np.random.default_rng(4800 + l1)
    X, Y = walks(rng, 5, l1, d), walks(rng, 3, l2, d)
    G = f32(rng.standard_normal((5, 3)))
    rx, ry = pde.pde_gram_grad(X, Y, G, n, 1)
    ex, _ = pde.pde_gram_grad(zero_last_channel(X), zero_last_channel(Y), G, n, 1)
    matters(tag, ex, rx)
    gX, gY = ops.pde_gram_vjp(t(X), t(Y), t(G), n, 1)
    check(f"{tag} dX", gX.cpu().numpy(), rx, GTOL)
    check(f"{tag} dY", gY.cpu().numpy(), ry, GTOL)
    fronts_split(tag, X, Y, G, n, 1, rx, ry, ops.pde_gram(t(X), t(Y), n, 1))
    w = f32(rng.standard_normal(5))
    ref = diag_grad_ref_c(X, w, n)
    check(f"{tag} diag dX", ops.pde_diag_vjp(t(X), t(w), n, 1).cpu().numpy(), ref, GTOL)
    fronts_split_diag(tag, X, w, n, 1, ref, ops.pde_diag(t(X), n, 1))


@pytest.mark.parametrize("r0,r1", [(1, 4), (3, 5)])
@pytest.mark.parametrize("l1,d,wpb", [pytest.param(9, 16, 4, id="wpb4"), pytest.param(220, 16, 2, id="wpb2"),
                                      pytest.param(450, 16, 1, id="wpb1"), pytest.param(9, 17, 4, id="tile")])
def test_adjoint_row_windows(l1, d, wpb, r0, r1):
    """gpsig_pde_vjp_ex over a window of x-rows that starts off the workgroup's row tile (ta0 = row_begin / wpb; on
    tiles the chunk loop starts at (row_begin / 4) 4 and the window at c0 > r0): the gradients of the window's pairs
    only, the other rows of gX exactly zero.  ops always starts its row chunks on multiples of 4, so the C entry is
    called directly."""
    from gpsig_amd import _lib as L
    lib = L.load()
    n1, n2, l2, n = 5, 3, 7, 0
    tag = f"adjrows-l{l1}-d{d}-{r0}-{r1}"
    expect(route(l1, l2, d, n, 1, RECT, True), tiled=int(d > 16), DP=dp_of(d), REP=1, W=1, nblk=1, wpb=wpb)
    rng = np.random.default_rng(4900 + l1 + d)
    X, Y = walks(rng, n1, l1, d), walks(rng, n2, l2, d)
    G = f32(rng.standard_normal((n1, n2)))
    rx, ry = pde.pde_gram_grad(X[r0:r1], Y, G[r0:r1], n, 1)
    fx, _ = pde.pde_gram_grad(X, Y, G, n, 1)
    matters(tag, rx[0], fx[0])     # row r0 of the window is not row 0 of the batch
    Xt, Yt, Gt = t(X), t(Y), t(G)
    gX, gY = torch.zeros_like(Xt), torch.zeros_like(Yt)
    nb = lib.gpsig_pde_vjp_workspace_bytes((r1 - r0) * n2, l1, l2, n)
    ws = torch.empty(nb // 4, device=DEV)
    sb = lib.gpsig_pde_vjp_scratch_bytes(n1, l1, n2, l2, d, n, RECT)
    assert (sb > 0) == (d > 16)
    sc = torch.empty(max(sb, 4) // 4, device=DEV)
    L.check(lib.gpsig_pde_vjp_ex(Xt.data_ptr(), n1, l1, Yt.data_ptr(), n2, l2, d, n, 1, RECT, r0, r1, Gt.data_ptr(),
                                 gX.data_ptr(), gY.data_ptr(), ws.data_ptr(), nb, sc.data_ptr() if sb else None, sb,
                                 torch.cuda.current_stream().cuda_stream), tag)
    gx = gX.cpu().numpy()
    check(f"{tag} dX", gx[r0:r1], rx, GTOL)
    check(f"{tag} dY", gY.cpu().numpy(), ry, GTOL)
    assert not np.delete(gx, np.arange(r0, r1), axis=0).any()


# ----------------------------------------------------------------------------- e. row windows
SENT = -777.0


@pytest.mark.parametrize("r0,r1", [(1, 6), (5, 7), (6, 11)])
@pytest.mark.parametrize("d,solver,fam", [pytest.param(3, 1, "lane_group", id="lane"), pytest.param(3, 0, "pair", id="pair"),
                                          pytest.param(17, 1, "tile", id="tile")])
def test_row_windows(d, solver, fam, r0, r1):
    """rows=(r0, r1) with out / out_row0 (the sharded Gram's interface) against the oracle's rows: r0 off the
    multiples of 4 (tile mode starts its chunk loop at (r0 / 4) 4), r1 off them too; cross pairs into a larger buffer
    at a row offset, and the symmetric window (entries a in the window, b >= a, and their mirrors inside it).  The
    buffer is filled with a sentinel first: nothing outside the window is written."""
    from gpsig_amd import ops
    n, l1, l2, n1, n2 = 1, 11, 9, 11, 5
    tag = f"rows-{fam}-{r0}-{r1}"
    expect(route(l1, l2, d, n, solver, RECT), family=fam)
    expect(route(l1, l1, d, n, solver, UPPER), family=fam)
    rng = np.random.default_rng(5000 + d + solver)
    X, Y = walks(rng, n1, l1, d), walks(rng, n2, l2, d)
    ref = pde.pde_gram(X, Y, n, solver)
    away_from_one(tag, ref)
    # cross: the window's rows land at r - out_row0 of a buffer that starts one row before the window
    buf = torch.full((r1 - r0 + 2, n2), SENT, device=DEV)
    ops.pde_gram(t(X), t(Y), n, solver, rows=(r0, r1), out=buf, out_row0=r0 - 1)
    got = buf.cpu().numpy()
    check(f"{tag} cross", got[1:-1], ref[r0:r1])
    assert (got[0] == SENT).all() and (got[-1] == SENT).all()
    # the whole Gram's buffer: rows outside the window untouched
    full = torch.full((n1, n2), SENT, device=DEV)
    ops.pde_gram(t(X), t(Y), n, solver, rows=(r0, r1), out=full, out_row0=0)
    got = full.cpu().numpy()
    np.testing.assert_array_equal(got[r0:r1], buf.cpu().numpy()[1:-1])
    assert (np.delete(got, np.arange(r0, r1), axis=0) == SENT).all()
    # symmetric: guard rows around the window's own buffer
    refs = pde.pde_gram(X, X, n, solver)
    big = torch.full((r1 - r0 + 2, n1), SENT, device=DEV)
    ops.pde_gram(t(X), None, n, solver, rows=(r0, r1), out=big[1:-1], out_row0=r0)
    got = big.cpu().numpy()
    check(f"{tag} sym", got[1:-1, r0:], refs[r0:r1, r0:])
    assert (got[0] == SENT).all() and (got[-1] == SENT).all() and (got[1:-1, :r0] == SENT).all()


# ----------------------------------------------------------------------------- f. tile chunk loop
def test_tile_chunk_loop():
    """Increment tiles past one chunk (pde_tiled_run, pde_adj_tiled: tiles of 1 GiB): four x-rows against
    n2 (l2 - 1) = 6.1e6 coarse columns exceed it, so n1 = 6 rows run as a chunk of four and a partial chunk of two
    (r0, c0, inc_a0 and the fronts' pair offset off zero).  The chunk count comes from the scratch plans.  The loss
    weights four y-sequences only: the oracle runs on those, every other y-gradient must be exactly zero.  The
    one-call adjoint is split by ops into rows (0, 4) and (4, 6) (a chunk loop that starts at r0 = 4); the fronts
    forward and the adjoint from its fronts each run both chunks in one call."""
    from gpsig_amd import _lib as L
    from gpsig_amd import ops
    lib = L.load()
    n1, l1, n2, l2, d, n = 6, 12, 96000, 65, 17, 0
    IC, cols = l1 - 1, n2 * (l2 - 1)
    expect(route(l1, l2, d, n, 1, RECT), family="tile", DP=0, REP=1, W=1, nblk=1, sub=0)
    expect(route(l1, l2, d, n, 1, RECT, True), tiled=1, DP=0, REP=1, W=1, H=32, nblk=1, sub=0)

    def a256(b):
        return (b + 255) // 256 * 256

    dx, dy = a256(n1 * IC * d * 4), a256(cols * d * 4)
    tile = lib.gpsig_pde_scratch_bytes(n1, l1, n2, l2, d, n, RECT) - dx - dy
    rows = tile // (IC * cols * 4)
    assert rows == 4 and tile > (1 << 30) and -(-n1 // rows) == 2 and n1 % rows == 2     # forward: two chunks
    part = a256(max(lib.gpsig_gemm_splitk_bytes(rows * IC, d, cols), lib.gpsig_gemm_splitk_bytes(cols, d, rows * IC)))
    assert lib.gpsig_pde_vjp_scratch_bytes(n1, l1, n2, l2, d, n, RECT) == 2 * (dx + dy) + 2 * tile + part  # adjoint: too

    rng = np.random.default_rng(6000)
    X = walks(rng, n1, l1, d)
    gen = torch.Generator(device=DEV).manual_seed(6000)
    Yt = torch.cumsum(torch.randn((n2, l2, d), device=DEV, generator=gen), 1) * (2.0 / np.sqrt(l2 * d))
    sel = [0, 1, n2 // 2, n2 - 1]
    Y = Yt[sel].cpu().numpy().astype(np.float64)
    ref = pde.pde_gram(X, Y, n, 1)
    away_from_one("chunks", ref)
    matters("chunks", pde.pde_gram(X, Y[:, :-1], n, 1), ref)
    K = ops.pde_gram(t(X), Yt, n, 1)
    assert K.shape == (n1, n2) and bool(torch.isfinite(K).all())
    check("chunks cross", K[:, sel].cpu().numpy(), ref)
    G = np.zeros((n1, n2))
    G[:, sel] = f32(rng.standard_normal((n1, len(sel))))
    rx, ry = pde.pde_gram_grad(X, Y, G[:, sel], n, 1)
    others = torch.ones(n2, dtype=torch.bool, device=DEV)
    others[sel] = False
    gX, gY = ops.pde_gram_vjp(t(X), Yt, t(G), n, 1)
    check("chunks dX", gX.cpu().numpy(), rx, GTOL)
    check("chunks dY", gY[sel].cpu().numpy(), ry, GTOL)
    assert not bool(gY[others].any())
    del gY
    fr = torch.empty(ops.pde_fronts_bytes(n1 * n2, l1, l2, n) // 4, device=DEV)
    Kf = ops.pde_fronts(t(X), Yt, n, 1, fr)
    assert torch.equal(Kf, K)
    fX, fY = ops.pde_vjp_fronts(t(X), Yt, t(G), n, 1, fr)
    check("chunks fronts dX", fX.cpu().numpy(), rx, GTOL)
    check("chunks fronts dY", fY[sel].cpu().numpy(), ry, GTOL)
    assert not bool(fY[others].any())


# ----------------------------------------------------------------------------- g. symmetric gradient
@pytest.mark.parametrize("n", [0, 1, 4])
@pytest.mark.parametrize("d", [3, 12, 17])
def test_symmetric_gradient(d, n, monkeypatch):
    """The gradient of the symmetric K(X) (the training step of every PDE model): a RECT launch with Y = X and gY
    aliased onto gX, against x-part + y-part of the oracle's adjoint with a non-symmetric G; then through
    UntruncSignatureKernel.K and autograd (forward mirrored with triu), with the forward's fronts kept and with the
    backward recomputing them."""
    import gpsig_amd
    from gpsig_amd import autograd as ag
    from gpsig_amd import ops
    tag = f"symgrad-d{d}-n{n}"
    N, l = 7, 9
    expect(route(l, l, d, n, 1, RECT, True), tiled=int(d > 16 or n > 3), DP=0 if (d > 16 or n > 3) else dp_of(d),
           sub=max(0, n - 3), REP=1 << min(n, 3))
    rng = np.random.default_rng(7000 + 10 * d + n)
    X = walks(rng, N, l, d)
    G = f32(rng.standard_normal((N, N)))
    assert np.abs(G - G.T).max() > 0.1
    gx, gy = pde.pde_gram_grad(X, X, G, n, 1)
    ref = gx + gy
    zx, zy = pde.pde_gram_grad(zero_last_channel(X), zero_last_channel(X), G, n, 1)
    matters(tag, zx + zy, ref)
    gX, none = ops.pde_gram_vjp(t(X), None, t(G), n, 1)
    assert none is None
    check(f"{tag} ops", gX.cpu().numpy(), ref, GTOL)
    Kref = pde.pde_gram(X, X, n, 1)
    k = gpsig_amd.UntruncSignatureKernel(l * d, d, order=n)
    calls = []
    for name in ("pde_gram", "pde_fronts", "pde_gram_vjp", "pde_vjp_fronts"):
        def spy(*a, _f=getattr(ops, name), _n=name, **kw):
            calls.append(_n)
            return _f(*a, **kw)
        monkeypatch.setattr(ops, name, spy)
    for path, cap, ran in (("fronts", ag.PDE_FRONTS_BYTES, ["pde_fronts", "pde_vjp_fronts"]),
                           ("recompute", 0, ["pde_gram", "pde_gram_vjp"])):
        monkeypatch.setattr(ag, "PDE_FRONTS_BYTES", cap)
        del calls[:]
        Xt = torch.tensor(X.reshape(N, -1), device=DEV, dtype=torch.float64, requires_grad=True)
        K = k.K(Xt)
        assert torch.equal(K, K.T)
        check(f"{tag} {path} K", K.detach().cpu().numpy(), Kref)
        (K * torch.tensor(G, device=DEV)).sum().backward()
        assert calls == ran, (path, calls)      # the path the pass is named after is the one autograd took
        check(f"{tag} {path} dX", Xt.grad.reshape(X.shape).cpu().numpy(), ref, GTOL)


# ----------------------------------------------------------------------------- h. kernel class
class _OraclePde(torch.autograd.Function):
    """The oracle's value and adjoint spliced into an fp64 torch graph on the CPU (mode: 'cross', 'sym', 'diag'); the
    sequences are rounded to fp32 as the kernels receive them (straight-through)."""

    @staticmethod
    def forward(ctx, Xs, Ys, mode, n):
        X = f32(Xs.detach().numpy())
        Y = X if Ys is None else f32(Ys.detach().numpy())
        ctx.X, ctx.Y, ctx.mode, ctx.n = X, Y, mode, n
        out = pde.pde_diag(X, n, 1) if mode == "diag" else pde.pde_gram(X, Y, n, 1)
        return torch.as_tensor(out)

    @staticmethod
    def backward(ctx, g):
        g = g.numpy()
        if ctx.mode == "diag":
            return torch.as_tensor(diag_grad_ref_c(ctx.X, g, ctx.n)), None, None, None
        gx, gy = pde.pde_gram_grad(ctx.X, ctx.Y, g, ctx.n, 1)
        if ctx.mode == "sym":
            return torch.as_tensor(gx + gy), None, None, None
        return torch.as_tensor(gx), torch.as_tensor(gy), None, None


def _ref_prep(X, l, d, lengthscales, lags, gamma):
    """UntruncSignatureKernel._apply_scaling_and_lags_to_sequences in fp64 torch on the CPU; the lag interpolation
    (linear in the sequence) as the matrix the NumPy oracle's add_lags_to_sequences gives on the unit sequences."""
    A = torch.as_tensor(kr.add_lags_to_sequences(np.eye(l)[None], lags)[0])      # (l, lags + 1, l)
    Xl = torch.einsum("lkm,nmd->nlkd", A, X.reshape(-1, l, d))
    Xl = Xl / torch.as_tensor(lengthscales)[None, None, None, :] * torch.as_tensor(gamma)[None, None, :, None]
    return Xl.reshape(-1, l, (len(lags) + 1) * d)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("n", [0, 1])
def test_kernel_class(n, dtype):
    """UntruncSignatureKernel with per-feature lengthscales, two lags and sigma = 1.7: K(X, X2), K(X), Kdiag(X) and
    their gradients with respect to X (and X2) against the fp64 chain with the oracle spliced in."""
    import gpsig_amd
    tag = f"class-n{n}-{str(dtype)[-7:]}"
    N, N2, l, d = 7, 5, 12, 3   # t - lag never on the time grid k / 11: no tie in the interpolation's left index
    ls = np.array([0.7, 1.3, 2.1])
    rng = np.random.default_rng(8000 + n)
    X, X2 = walks(rng, N, l, d, 3.0).reshape(N, -1), walks(rng, N2, l, d, 3.0).reshape(N2, -1)
    k = gpsig_amd.UntruncSignatureKernel(l * d, d, lengthscales=ls, order=n, num_lags=2)
    k.sigma = torch.tensor(1.7, dtype=torch.float64)
    k.to(DEV)
    expect(route(l, l, 3 * d, n, 1, RECT), DP=8 + 8 * (3 * d > 8))
    lags, gamma = k.lags.cpu().numpy(), k.gamma.cpu().numpy()
    G = f32(rng.standard_normal((N, N2)))
    Gs = f32(rng.standard_normal((N, N)))
    w = f32(rng.standard_normal(N))

    def ref(mode):
        Xr = torch.tensor(X, requires_grad=True)
        Yr = torch.tensor(X2, requires_grad=True) if mode == "cross" else None
        Ys = None if Yr is None else _ref_prep(Yr, l, d, ls, lags, gamma)
        K = 1.7 * _OraclePde.apply(_ref_prep(Xr, l, d, ls, lags, gamma), Ys, mode, n)
        (K * torch.as_tensor({"cross": G, "sym": Gs, "diag": w}[mode])).sum().backward()
        return K.detach().numpy(), Xr.grad.numpy(), None if Yr is None else Yr.grad.numpy()

    def run(mode):
        Xt = torch.tensor(X, device=DEV, dtype=dtype, requires_grad=True)
        Yt = torch.tensor(X2, device=DEV, dtype=dtype, requires_grad=True) if mode == "cross" else None
        K = k.Kdiag(Xt) if mode == "diag" else k.K(Xt, Yt)
        assert K.dtype == dtype
        (K * torch.tensor({"cross": G, "sym": Gs, "diag": w}[mode], device=DEV, dtype=dtype)).sum().backward()
        return K.detach().cpu().numpy(), Xt.grad.cpu().numpy(), None if Yt is None else Yt.grad.cpu().numpy()

    for mode in ("cross", "sym", "diag"):
        Kr, gxr, gyr = ref(mode)
        away_from_one(tag, Kr / 1.7)
        Kg, gx, gy = run(mode)
        check(f"{tag} {mode} K", Kg, Kr)
        check(f"{tag} {mode} dX", gx, gxr, GTOL)
        if gyr is not None:
            check(f"{tag} {mode} dX2", gy, gyr, GTOL)
    # plain kernel (lengthscales 1, no lags, sigma 1) differs: the scaling chain carries weight
    k0 = gpsig_amd.UntruncSignatureKernel(l * d, d, order=n)
    matters(tag, k0.K(torch.tensor(X, device=DEV), torch.tensor(X2, device=DEV)).cpu().numpy(), ref("cross")[0])


# ----------------------------------------------------------------------------- i. edges
@pytest.mark.parametrize("solver", [0, 1])
@pytest.mark.parametrize("l1,l2,n1,n2,lane", [
    pytest.param(2, 2, 3, 3, (16, 8), id="one-cell"), pytest.param(2, 9, 3, 2, (16, 16), id="l1-2"),
    pytest.param(9, 2, 2, 3, (16, 8), id="l2-2"), pytest.param(7, 6, 1, 5, (16, 8), id="n1-1"),
    pytest.param(7, 6, 5, 1, (16, 8), id="n2-1"), pytest.param(6, 6, 1, 1, (16, 8), id="one-pair")])
def test_edges_small(l1, l2, n1, n2, lane, solver):
    """A single cell on either side, single sequences.  lane: the solver-1 cross Gram's lane group; with one coarse
    row of x (l1 = 2) the cost model takes all 16 columns of y into one lane, (16, 16) with a single lane used, and
    the one-cell case is a single lane of (16, 8)."""
    from gpsig_amd import ops
    tag = f"edge-l{l1}x{l2}-n{n1}x{n2}-s{solver}"
    d, n = 3, 1
    rng = np.random.default_rng(9000 + 10 * l1 + l2 + n1)
    X, Y = walks(rng, n1, l1, d, 2.0 * np.sqrt(max(l1, l2))), walks(rng, n2, l2, d, 2.0 * np.sqrt(max(l1, l2)))
    expect_short_routes(l1, l2, d, n, solver, lane)
    ref = pde.pde_gram(X, Y, n, solver)
    away_from_one(tag, ref)
    check(f"{tag} cross", ops.pde_gram(t(X), t(Y), n, solver).cpu().numpy(), ref)
    S = ops.pde_gram(t(X), None, n, solver).cpu().numpy()
    check(f"{tag} sym", S, pde.pde_gram(X, X, n, solver))
    np.testing.assert_array_equal(S, S.T)
    check(f"{tag} diag", ops.pde_diag(t(X), n, solver).cpu().numpy(), pde.pde_diag(X, n, solver))
    G = f32(rng.standard_normal((n1, n2)))
    rx, ry = pde.pde_gram_grad(X, Y, G, n, solver)
    gX, gY = ops.pde_gram_vjp(t(X), t(Y), t(G), n, solver)
    check(f"{tag} dX", gX.cpu().numpy(), rx, GTOL)
    check(f"{tag} dY", gY.cpu().numpy(), ry, GTOL)
    fronts_split(tag, X, Y, G, n, solver, rx, ry, ops.pde_gram(t(X), t(Y), n, solver))
    w = f32(rng.standard_normal(n1))
    ref = diag_grad_ref(X, w, n, solver)
    check(f"{tag} diag dX", ops.pde_diag_vjp(t(X), t(w), n, solver).cpu().numpy(), ref, GTOL)
    fronts_split_diag(tag, X, w, n, solver, ref, ops.pde_diag(t(X), n, solver))


@pytest.mark.parametrize("d", [3, 17])
def test_edges_empty_batches(d):
    """Empty batches through every ops.pde_* entry point: the shapes are right and nothing is launched in error."""
    from gpsig_amd import ops
    l, n = 6, 1
    expect_short_routes(l, l, d, n, 1)
    X, E = t(walks(np.random.default_rng(1), 3, l, d)), torch.zeros((0, l, d), device=DEV)
    assert ops.pde_diag(E, n).shape == (0,)
    assert ops.pde_gram(E, X, n).shape == (0, 3) and ops.pde_gram(X, E, n).shape == (3, 0)
    assert ops.pde_gram(E, None, n).shape == (0, 0)
    assert ops.pde_gram(X, X, n, rows=(2, 2)).shape == (0, 3)
    assert ops.pde_diag_vjp(E, torch.zeros(0, device=DEV), n).shape == (0, l, d)
    gX, gY = ops.pde_gram_vjp(E, X, torch.zeros((0, 3), device=DEV), n)
    assert gX.shape == (0, l, d) and gY.shape == (3, l, d) and not gY.any()
    gX, gY = ops.pde_gram_vjp(X, E, torch.zeros((3, 0), device=DEV), n)
    assert gX.shape == (3, l, d) and gY.shape == (0, l, d) and not gX.any()
    gX, gY = ops.pde_gram_vjp(E, None, torch.zeros((0, 0), device=DEV), n)
    assert gX.shape == (0, l, d) and gY is None
    fr = torch.empty(0, device=DEV)
    assert ops.pde_fronts(E, X, n, 1, fr).shape == (0, 3) and ops.pde_fronts(X, E, n, 1, fr).shape == (3, 0)
    assert ops.pde_fronts(E, None, n, 1, fr).shape == (0, 0) and ops.pde_fronts(E, None, n, 1, fr, diag=True).shape == (0,)
    gX, gY = ops.pde_vjp_fronts(X, E, torch.zeros((3, 0), device=DEV), n, 1, fr)
    assert gX.shape == (3, l, d) and gY.shape == (0, l, d) and not gX.any()
    gX, gY = ops.pde_vjp_fronts(E, X, torch.zeros((0, 3), device=DEV), n, 1, fr)
    assert gX.shape == (0, l, d) and gY.shape == (3, l, d) and not gY.any()
    assert ops.pde_vjp_fronts(E, None, torch.zeros(0, device=DEV), n, 1, fr, diag=True).shape == (0, l, d)
    torch.cuda.synchronize()


@pytest.mark.parametrize("d,n", [(3, 0), (3, 2), (12, 1), (17, 1)])
def test_edges_constant_and_identical(d, n):
    """A constant path (all increments zero): K is exactly 1 against anything, and the gradient (not zero: dK/dx of
    the first-order term <dx, dy>) matches the oracle.  Identical x and y: cross pair (x, x) against the oracle, and
    equal to the symmetric Gram's diagonal bit for bit."""
    from gpsig_amd import ops
    tag = f"const-d{d}-n{n}"
    rng = np.random.default_rng(9500 + d + n)
    X, Y = walks(rng, 5, 8, d), walks(rng, 3, 7, d)
    X[1] = X[1, :1]
    Y[2] = Y[2, :1]
    expect_short_routes(8, 7, d, n, 1)
    K = ops.pde_gram(t(X), t(Y), n, 1).cpu().numpy()
    assert (K[1] == 1.0).all() and (K[:, 2] == 1.0).all()
    assert ops.pde_diag(t(X), n, 1).cpu().numpy()[1] == 1.0
    check(f"{tag} cross", K, pde.pde_gram(X, Y, n, 1))
    G = np.zeros((5, 3))
    G[1], G[:, 2] = f32(rng.standard_normal(3)), f32(rng.standard_normal(5))   # only pairs with a constant path
    rx, ry = pde.pde_gram_grad(X, Y, G, n, 1)
    gX, gY = ops.pde_gram_vjp(t(X), t(Y), t(G), n, 1)
    check(f"{tag} dX", gX.cpu().numpy(), rx, GTOL)
    check(f"{tag} dY", gY.cpu().numpy(), ry, GTOL)
    Kxx = ops.pde_gram(t(X), t(X.copy()), n, 1).cpu().numpy()
    check(f"{tag} identical", Kxx, pde.pde_gram(X, X, n, 1))
    np.testing.assert_array_equal(np.diag(Kxx), np.diag(ops.pde_gram(t(X), None, n, 1).cpu().numpy()))


def _well_posed(tag, f, args64):
    """The fp64 oracle on the fp32-rounded inputs and on the unrounded ones agree within the tolerance: the case is
    well-posed for an fp32 interface.  Returns the oracle's arrays on the rounded inputs."""
    exact, rounded = f(*args64), f(*[f32(a) for a in args64])
    exact, rounded = (exact, rounded) if isinstance(exact, tuple) else ((exact,), (rounded,))
    for e, r in zip(exact, rounded):
        dev = norm_rel_err(r, e)
        print(f"{tag}: fp32 rounding of the inputs moves the oracle by {dev:.2e}")
        assert dev < TOL, (tag, dev)
    return rounded


@pytest.mark.parametrize("d,n", [(3, 1), (12, 0), (17, 1)])
def test_edges_large_values(d, n):
    """|K| in the thousands."""
    from gpsig_amd import ops
    tag = f"large-d{d}-n{n}"
    rng = np.random.default_rng(9700 + d)
    l = 12
    # one common direction: <dx_i, dy_j> > 0 in every cell, K grows like exp(2 sqrt(<x, y>))
    u = rng.standard_normal(d)
    u /= np.linalg.norm(u)
    s = 1.6
    X = np.cumsum(np.abs(rng.standard_normal((5, l, 1))) * u + 0.05 * rng.standard_normal((5, l, d)), 1) * s / np.sqrt(l)
    Y = np.cumsum(np.abs(rng.standard_normal((3, l, 1))) * u + 0.05 * rng.standard_normal((3, l, d)), 1) * s / np.sqrt(l)
    expect_short_routes(l, l, d, n, 1)
    (ref,) = _well_posed(tag, lambda a, b: pde.pde_gram(a, b, n, 1), (X, Y))
    print(f"{tag}: |K| in [{np.abs(ref).min():.3g}, {np.abs(ref).max():.3g}]")
    assert 1e3 < np.abs(ref).max() < 2e4
    check(f"{tag} cross", ops.pde_gram(t(f32(X)), t(f32(Y)), n, 1).cpu().numpy(), ref)
    G = f32(rng.standard_normal((5, 3)))
    rx, ry = _well_posed(tag, lambda a, b: pde.pde_gram_grad(a, b, G, n, 1), (X, Y))
    gX, gY = ops.pde_gram_vjp(t(f32(X)), t(f32(Y)), t(G), n, 1)
    check(f"{tag} dX", gX.cpu().numpy(), rx, GTOL)
    check(f"{tag} dY", gY.cpu().numpy(), ry, GTOL)


@pytest.mark.parametrize("d,n", [(3, 1), (12, 0), (17, 1)])
def test_edges_small_increments(d, n):
    """Increments ~1e-3: K - 1 ~ 1e-6 and the gradient is a sum of small terms (held to 1e-5 of its own size)."""
    from gpsig_amd import ops
    tag = f"small-d{d}-n{n}"
    rng = np.random.default_rng(9800 + d)
    l = 10
    # increments with few mantissa bits (multiples of 2^-20), paths from 0: rounding to fp32 leaves them exact
    X = np.cumsum(np.round(rng.standard_normal((5, l, d)) * 1e-3 * 2 ** 20) / 2 ** 20, 1)
    Y = np.cumsum(np.round(rng.standard_normal((3, l, d)) * 1e-3 * 2 ** 20) / 2 ** 20, 1)
    expect_short_routes(l, l, d, n, 1)
    G = f32(rng.standard_normal((5, 3)))
    rx, ry = _well_posed(tag, lambda a, b: pde.pde_gram_grad(a, b, G, n, 1), (X, Y))
    (ref,) = _well_posed(tag, lambda a, b: pde.pde_gram(a, b, n, 1), (X, Y))
    print(f"{tag}: max|K - 1| {np.abs(ref - 1).max():.2e}, max|dX| {np.abs(rx).max():.2e}")
    assert 1e-7 < np.abs(ref - 1).max() < 1e-4
    check(f"{tag} cross", ops.pde_gram(t(f32(X)), t(f32(Y)), n, 1).cpu().numpy(), ref)
    gX, gY = ops.pde_gram_vjp(t(f32(X)), t(f32(Y)), t(G), n, 1)
    check(f"{tag} dX", gX.cpu().numpy(), rx, GTOL, floor=1e-6)
    check(f"{tag} dY", gY.cpu().numpy(), ry, GTOL, floor=1e-6)
    w = f32(rng.standard_normal(5))
    check(f"{tag} diag dX", ops.pde_diag_vjp(t(f32(X)), t(w), n, 1).cpu().numpy(), diag_grad_ref(f32(X), w, n, 1), GTOL,
          floor=1e-6)
