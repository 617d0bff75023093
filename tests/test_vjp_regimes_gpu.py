"""GPU parity of the first-order Gram VJP (sig_bwd_pk.h, sig_bwd.h, sig_bwd_wide.*) on jumpy data, at every
kernel route and at the edges of the regenerated-cell chunks, vs torch fp64 autodiff of the reference graph
(oracle/autodiff_ref.py) evaluated at the fp32-rounded inputs.  The forward's counterpart is
tests/test_fo_rowloop_gpu.py; the other gradient files run smooth walks only.

Data (numpy, fp64, seeded): walks with N(0, 1) * 0.03 increments.  Row r of a pair's grid is the increment
x_{r+1} - x_r = steps[:, r + 1], column c the increment y_{c+1} - y_c (as `jumpy` of test_fo_rowloop_gpu.py).
Four regimes, each applied to chosen sequences only:
  slow   X increments of the listed rows x 25 (`jump_factor`: less at D > 8): the whole row leaves the
         polynomial range |p|, |c| < EM1_TAU = 0.5 and takes the corner differences of an exact next row, with
         the next lane's k in every lane;
  mixed  X increments of the listed rows x 10 at D = 8 (`mixed_factor`: x 10 sqrt(8 / D)) and Y increments of
         a few columns x `jump_factor`: on the listed rows part of the cells is in range and part is not;
  qcols  Y increments of the listed columns x `jump_factor`, X smooth: p and c stay in range, |q| leaves it
         (the exp path of Eq in exact_row, the Eq recurrence from a large value);
  rough  i.i.d. N(0, 1) * 0.7 points: every cell out of range.
The premise tests (no GPU) assert from `cell_grids` that each GPU case's data is in the regime it names.

Criterion, as tests/test_grad_gpu.py: norm_rel_err(g, g64) < GTOL for gX (and gY in RECT mode), and the same
bound per sequence (over the leading N axis): the whole-tensor norm is set by the jump points and would hide
a wrong gradient on a smooth sequence that shares a wave with a jumpy one.
"""
import numpy as np
import pytest
import torch

from conftest import norm_rel_err
from oracle import autodiff_ref as ar

# Largest observed errors vs fp64 (MI355X), whole tensor / per sequence, by route:
#   packed RBF {4,16} 1.9e-6 / 1.9e-6   {4,32} 1.6e-6 / 3.0e-6   {4,64} 1.7e-6 / 3.5e-6
#   seg {5,20} 1.9e-6 / 3.3e-6          blocked W = 4 6.6e-6 / 8.4e-6     DP = 16 3.0e-6 / 3.8e-6
#   wide tiles 2.3e-6 / 4.9e-6          packed linear 1.5e-6 / 1.5e-6     ragged 1.7e-7 / 2.3e-7
#   saved state 3.4e-6 / 4.7e-6, recompute 3.1e-6 (both blocked; packed {4,64} 1.5e-6)
#   SignatureRBF gradients (X, X2, lengthscales, variances): 1.7e-6
# Before the emissions dropped the self pairs' diagonal weight (sig_bwd.h, sig_bwd_pk.h, sig_bwd_wide.hip) K(X)
# stood at 1.08e-5 / 1.54e-5 on packed {4,64} (L = 256, D = 8, slow rows on every sequence), 9.5e-6 / 1.66e-5 at
# DP = 16 and, on the wide tiles, 2.2e-4 / 1.0e-3 on rough data and 1.39e-5 on slow rows.
GTOL = 1e-5
DEV = "cuda"
TAU = 0.5  # EM1_TAU, csrc/common.h
ROWS_ANCH = (126, 127, 128)  # the rows beside and on the forward's anchor row 127 (RbfSeedPk::ANCHOR = 128)
ROWS_RUN = (40, 41, 42, 43)  # a whole RC = 4 chunk of slow rows (a chunk and a half at RC = 6)


# ----------------------------------------------------------------------------- data
def steps(N, L, D, seed):
    return np.random.default_rng(seed).standard_normal((N, L, D)) * 0.03


def scale_steps(inc, idx, seqs, factor):
    """Increment idx[k] (grid row or column idx[k]: steps[:, idx[k] + 1]) of the sequences `seqs` x factor."""
    L = inc.shape[1]
    for r in sorted(set(idx)):
        if 0 <= r and r + 1 < L:
            inc[seqs, r + 1, :] *= factor
    return inc


def mixed_factor(D):
    """|dx|^2 / 2 of a step x f is about 0.00045 f^2 D, and p = -|dx|^2 / 2 + <y_j - x_i, dx_i>: x 10 at
    D = 8 puts the first term at 0.36, near enough to EM1_TAU for the second to take part of the row's cells
    across it; the other channel counts take the factor that gives the same value."""
    return 10.0 * np.sqrt(8.0 / D)


def jump_factor(D):
    """x 25 up to D = 8.  A step x f has |dx|^2 / 2 about 0.00045 f^2 D (2.25 at D = 8, far out of range) and
    moves the sequence by 0.03 f sqrt(D); wider channels take the factor that holds D = 8's values, so that
    the displacement a jump leaves does not push the smooth rows after it out of range as well."""
    return 25.0 * min(1.0, np.sqrt(8.0 / D))


def rough(N, L, D, seed):
    return np.random.default_rng(seed).standard_normal((N, L, D)) * 0.7


def cell_grids(x, y):
    """fp64 grids (l1 - 1, l2 - 1) of the quantities the kernels' range checks see for the pair (x, y):
        c_ij = <dx_i, dy_j>,  p_ij = <y_j - x_i, dx_i> - |dx_i|^2 / 2,  q_ij = <x_i - y_j, dy_j> - |dy_j|^2 / 2.
    Confirmed against the code: the point record holds g_i = <x_i, dx_i> + |dx_i|^2 / 2 (features kernel,
    sig_fo.hip) and the rows take p = <y_j, dx_i> - g_i (RbfSeedPk::row in sig_common.h, the chunk lambdas of
    sig_bwd_pk.h and sig_bwd.h), so k(x_{i+1}, y_j) = k(x_i, y_j) e^p; their exact_row takes
    q = <x - y_j, dy_j> - |dy_j|^2 / 2, so k(x_i, y_{j+1}) = k(x_i, y_j) e^q; c is the dot of the increments."""
    dx, dy = np.diff(x, axis=0), np.diff(y, axis=0)
    x0, y0 = x[:-1], y[:-1]
    c = dx @ dy.T
    p = (y0 @ dx.T).T - (x0 * dx).sum(1)[:, None] - 0.5 * (dx * dx).sum(1)[:, None]
    q = x0 @ dy.T - (y0 * dy).sum(1)[None, :] - 0.5 * (dy * dy).sum(1)[None, :]
    return p, c, q


# Seeds of the cases whose group seed does not give data in the named regime (test_premise): the smallest
# other seed that does.  The choice looks at the fp64 premises only, never at a GPU result.
SEEDS = {
    "pk4x16-mixed-rbf-L64-D5-M5-r0_3_4_7_61_62-seq0-rect": 10,
    "pk4x16-qcols-rbf-L64-D5-M5-rnone-seq0-rect": 10,
    "pk4x32-qcols-rbf-L128-D5-M5-rnone-seq0-rect": 10,
    "pk4x64-mixed-rbf-L130-D5-M4-r0_3_4_7_127_128-seq0-rect": 10,
    "pk4x64-mixed-rbf-L130-D5-M4-r0_3_4_7_127_128-all-rect": 10,
    "pk4x64-slow-rbf-L256-D5-M4-r0_3_4_7_253_254-seq0-sym": 10,
    "pk4x64-mixed-rbf-L256-D5-M4-r0_3_4_7_253_254-all-rect": 10,
    "pk4x64-mixed-rbf-L256-D8-M4-r0_3_4_7_253_254-all-rect": 10,
    "blocked-slow-rbf-L257-D3-M4-r0_3_4_7_254_255-seq0-sym": 10,
    "blocked-qcols-rbf-L257-D3-M4-rnone-seq0-rect": 12,
    "blocked-mixed-rbf-L300-D3-M4-r0_3_4_7_297_298-seq0-rect": 10,
    "blocked-mixed-rbf-L300-D3-M4-r0_3_4_7_297_298-all-rect": 10,
    "dp16-mixed-rbf-L128-D12-M3-r0_7_8_15_125_126-all-rect": 15,
    "dp16-slow-rbf-L130-D12-M3-r0_7_8_15_127_128-seq0-sym": 10,
    "dp16-mixed-rbf-L130-D12-M3-r0_7_8_15_127_128-all-rect": 12,
    "wide-slow-rbf-L136-D20-M3-r0_3_4_7_133_134-seq0-sym": 10,
    "state-blocked-slow-rbf-L260-D5-M4-r0_126_127_128_258-seq02-sym": 10,
    "state-blocked-slow-rbf-L260-D5-M4-r0_126_127_128_258-seq02-rect": 10,
    "state-blocked-mixed-rbf-L260-D5-M4-r0_126_127_128_258-seq02-sym": 11,
    "state-blocked-mixed-rbf-L260-D5-M4-r0_126_127_128_258-seq02-rect": 10,
    "state-blocked-slow-rbf-L260-D8-M4-r0_126_127_128_258-seq02-sym": 11,
    "state-blocked-slow-rbf-L260-D8-M4-r0_126_127_128_258-seq02-rect": 19,
    "state-blocked-mixed-rbf-L260-D8-M4-r0_126_127_128_258-seq02-sym": 12,
    "state-blocked-mixed-rbf-L260-D8-M4-r0_126_127_128_258-seq02-rect": 23,
    "state-blocked-slow-rbf-L530-D3-M4-r0_126_127_128_528-seq02-rect": 10,
    "state-blocked-mixed-rbf-L530-D3-M4-r0_126_127_128_528-seq02-rect": 10,
}


class Case:
    """One GPU case: its data recipe, the rows / columns that jump and on which sequences."""

    def __init__(self, route, regime, l1, l2, D, M, rows=(), cols=(), seqs=(0,), base="rbf", rect=None, seed=0):
        self.route, self.regime, self.l1, self.l2, self.D, self.M = route, regime, l1, l2, D, M
        self.rows = tuple(sorted({r for r in rows if 0 <= r < l1 - 1}))
        self.cols = tuple(sorted({c for c in cols if 0 <= c < l2 - 1}))
        self.seqs, self.base, self.seed = seqs, base, seed  # seqs: the jumping sequences, None for every one
        self.N = 4 if max(l1, l2) > 200 else 5
        # K(X) where one sequence set plays both sides; K(X, Y) where the Y side differs from the X side
        self.rect = (regime in ("mixed", "qcols") or l1 != l2) if rect is None else rect
        self.N2 = self.N - 1 if self.rect else self.N

    @property
    def id(self):
        who = "all" if self.seqs is None else "seq" + "".join(map(str, self.seqs))
        return (f"{self.route}-{self.regime}-{self.base}-L{self.l1}" + (f"x{self.l2}" if self.l1 != self.l2 else "")
                + f"-D{self.D}-M{self.M}-r{'_'.join(map(str, self.rows)) or 'none'}-{who}-"
                + ("rect" if self.rect else "sym"))

    def jumping(self, n):
        return list(range(n)) if self.seqs is None else [s for s in self.seqs if s < n]

    def data(self):
        """(X, Y): fp64 (N, l1, D) and (N2, l2, D), or Y None for K(X)."""
        s = 1000 * SEEDS.get(self.id, self.seed) + 7 * self.l1 + 3 * self.l2 + self.D
        if self.regime == "rough":
            return rough(self.N, self.l1, self.D, s), None
        ix = steps(self.N, self.l1, self.D, s)
        iy = steps(self.N2, self.l2, self.D, s + 1) if self.rect else None
        if self.regime == "slow":
            scale_steps(ix, self.rows, self.jumping(self.N), jump_factor(self.D))
        elif self.regime == "mixed":
            scale_steps(ix, self.rows, self.jumping(self.N), mixed_factor(self.D))
            scale_steps(iy if self.rect else ix, self.cols, self.jumping(self.N2), jump_factor(self.D))
        elif self.regime == "qcols":
            scale_steps(iy, self.cols, self.jumping(self.N2), jump_factor(self.D))
        else:
            assert self.regime == "smooth"
        return np.cumsum(ix, 1), None if iy is None else np.cumsum(iy, 1)


def rows_chunk(nrows, RC):
    """The first row, the rows beside the first two chunk edges, the last two rows (the last one's exact next
    row is the last point; with nrows % RC != 0 they sit in the trailing partial chunk)."""
    return (0, RC - 1, RC, 2 * RC - 1, nrows - 2, nrows - 1)


def y_cols(l2, W, extra=()):
    """Two mid-lane columns (second column of a lane of W) near l2 / 3 and 3 l2 / 4, and the route's own."""
    return tuple(c - c % W + 1 for c in (l2 // 3, 3 * l2 // 4)) + tuple(extra)


# Routes of gpsig_sig_gram_vjp (sig_bwd.hip: vjp_plan, bwd_pk_geo; bwd_pk_geometry in sig_bwd_pk.h; bwd_geometry
# and bwd_blocks in sig_bwd.h; bwd_wide), with RC = rows per regenerated chunk and W = columns per lane:
#   name      kernel, geometry {W, LP}                              RC  shapes (L, D, M)
ROUTES = [
    # packed RBF {4,16}: l2 <= 64.  L = 64: the last lane's last column ends on the end point; 61: partial
    # lane; 60 rows are whole chunks, 63 leave a partial one
    ("pk4x16", 4, 4, [(64, 5, 5), (61, 5, 5)], ()),
    # packed RBF {4,32}: 65..128 points where the segmented geometry does not apply (l2 > 100, or D = 8)
    ("pk4x32", 4, 4, [(128, 5, 5), (100, 8, 6)], ()),
    # packed RBF {4,64}: 129..256 points
    ("pk4x64", 4, 4, [(130, 5, 4), (256, 5, 4), (130, 8, 4), (256, 8, 4)], ()),
    # sig_bwd_kernel {5,20}: 65..100 points at D <= 5, M <= 6; three pairs per wave, RC = 6
    ("seg5x20", 5, 6, [(100, 5, 5), (96, 5, 5), (66, 5, 5)], ()),
    # sig_bwd_kernel {4,64} in column blocks of 255 cells: past 256 points; Y jumps beside the block edge
    ("blocked", 4, 4, [(257, 3, 4), (300, 3, 4)], (254, 255, 256)),
    # sig_bwd_kernel at DP = 16, W = 2, RC = 8: {2,16} at L = 30, {2,64} at 128, two blocks of 127 cells at 130
    ("dp16", 2, 8, [(30, 12, 3), (128, 12, 3), (130, 12, 3)], (126, 127)),
    # point-weight tiles and emission GEMMs (sig_bwd_wide.*): D > 16, RC = 4
    ("wide", 4, 4, [(40, 20, 3), (136, 20, 3)], ()),
]
RUN_ROUTES = ("pk4x64", "seg5x20", "blocked")  # the consecutive slow rows 40..43


def _cases():
    out = []
    for name, W, RC, shapes, extra in ROUTES:
        for k, (L, D, M) in enumerate(shapes):
            rows, cols = rows_chunk(L - 1, RC), y_cols(L, W, extra)
            for seqs in ((0,), None):  # jumps on sequence 0 only (smooth pairs share its waves), on every one
                out.append(Case(name, "slow", L, L, D, M, rows, (), seqs, seed=1))
                out.append(Case(name, "mixed", L, L, D, M, rows, cols, seqs, seed=2))
            if k == 0:  # one shape per route: the table's first, so rough runs at L = 64 and L = 128
                out.append(Case(name, "qcols", L, L, D, M, (), cols, (0,), seed=3))
                out.append(Case(name, "rough", L, L, D, M, (), (), None, seed=4))
            if name in RUN_ROUTES and k == 0:
                for seqs in ((0,), None):
                    out.append(Case(name, "slow", L, L, D, M, ROWS_RUN, (), seqs, seed=5))
    # packed linear {6,20} (l2 = 101..120), {6,32} (129..192) and their neighbours {4,32} (121), {4,64} (193):
    # linear cells have no range, the slow rows give magnitude contrast
    for l2 in (101, 120, 121, 129, 192, 193):
        out.append(Case("pklin", "smooth", l2, l2, 5, 5, base="linear", seed=6))
        out.append(Case("pklin", "slow", l2, l2, 5, 5, rows_chunk(l2 - 1, 4), base="linear", seed=6))
    # ragged RECT: 8, 9 and 129 rows against {4,64} and {4,16} columns; slow rows on X including its last
    for l1, l2 in ((9, 130), (10, 130), (130, 9)):
        out.append(Case("ragged", "slow", l1, l2, 5, 4, rows_chunk(l1 - 1, 4), seed=7))
    return out


CASES = _cases()
RBF_JUMPY = [c for c in CASES if c.base == "rbf" and c.regime in ("slow", "mixed", "qcols")]


def _state_cases():
    out = []
    for L, D in ((130, 5), (260, 5), (130, 8), (260, 8), (530, 3)):
        rows = ROWS_ANCH + (0, L - 2)
        blocked = L > 256  # packed {4,64} at 130, sig_bwd_kernel in 2 and 3 column blocks at 260 and 530
        cols = y_cols(L, 4, (254, 255, 256) if blocked else ())
        for regime in ("slow", "mixed"):
            for rect in (False, True):
                # jumps on sequences 0 and 2: jumpy-jumpy, jumpy-smooth and smooth-smooth pairs in one launch
                out.append(Case("state-blocked" if blocked else "state-pk4x64", regime, L, L, D, 4, rows, cols, (0, 2),
                                rect=rect, seed=8))
    return out


STATE_CASES = _state_cases()
# the user-facing path: SignatureRBF.K(X) and K(X, X2), L = 130, D = 5, M = 4
USER_CASES = [Case("user", regime, 130, 130, 5, 4, ROWS_ANCH, y_cols(130, 4), (0, 2), rect=rect, seed=9)
              for regime in ("slow", "mixed") for rect in (False, True)]


# ----------------------------------------------------------------------------- premises (no GPU)
def pair_grids(case):
    """[(a, b, p, c, q)] of the pairs the launch runs (K(X): b >= a), at the fp32-rounded inputs."""
    X, Y = case.data()
    X = X.astype(np.float32).astype(np.float64)
    Y = X if Y is None else Y.astype(np.float32).astype(np.float64)
    sym = not case.rect
    return [(a, b) + cell_grids(X[a], Y[b]) for a in range(len(X)) for b in range(a if sym else 0, len(Y))]


def listed(case, a, b):
    """(rows, columns) of pair (a, b)'s grid that hold a scaled increment.  K(X, Y): the case's rows where
    sequence a of X jumps, its columns where sequence b of Y does.  K(X): one sequence set plays both sides,
    so every scaled increment of a sequence shows as a row where it is x and as a column where it is y."""
    jx = a in case.jumping(case.N) and case.regime != "qcols"
    jy = b in case.jumping(case.N2) and (case.regime != "slow" or not case.rect)
    if case.rect:
        return (case.rows if jx else ()), (case.cols if jy else ())
    own = case.rows + (case.cols if case.regime == "mixed" else ())
    return (own if jx else ()), (own if jy else ())


def premise_problems(case):
    """What the case's data fails to be, of what its regime claims (conditions on cell_grids; empty: none)."""
    bad, slow_cells, in_band, q_cols = [], [], [], {}
    for a, b, p, c, q in pair_grids(case):
        rows, cols = (np.array(v, dtype=int) for v in listed(case, a, b))
        out_pc = np.maximum(np.abs(p), np.abs(c)) >= TAU
        # Rows and columns that are not listed stay in range.  Claimed where one side of the pair jumps, and
        # for the mixed regime's K(X, Y); not where both sides take x 25 jumps: the displacement they leave
        # between the two sequences pushes later smooth rows out of range as well.
        if not (len(rows) and len(cols)) or (case.regime == "mixed" and case.rect):
            keep = np.ones(p.shape, bool)
            keep[rows, :] = False
            keep[:, cols] = False
            worst = max(np.abs(g)[keep].max() for g in (p, c, q))
            if not worst < TAU:
                bad.append(f"pair {a},{b}: smooth rows and columns reach {worst:.3f}")
        if a in case.jumping(case.N):
            if case.regime == "slow":
                slow_cells += [out_pc[r] for r in case.rows]
            if case.regime == "mixed":
                in_band += [0.1 < out_pc[r].mean() < 0.9 for r in case.rows]
        if case.regime == "qcols":
            if out_pc.any():
                bad.append(f"pair {a},{b}: |p| or |c| reaches {max(np.abs(p).max(), np.abs(c).max()):.3f}")
            for j in cols:
                q_cols.setdefault(j, []).append(np.abs(q[:, j]) >= TAU)
    # slow: on the listed rows of jumping pairs at least half the cells are out of range
    if case.regime == "slow" and not np.concatenate(slow_cells).mean() >= 0.5:
        bad.append(f"out-of-range share of the slow rows {np.concatenate(slow_cells).mean():.2f}")
    # mixed: on a quarter of the (pair, listed row) combinations, 10 % .. 90 % of the row's cells are out of range
    if case.regime == "mixed" and not np.mean(in_band) >= 0.25:
        bad.append(f"rows partly in range: {np.mean(in_band):.2f} of them")
    # qcols: |q| out of range on more than half of each listed column's cells
    if case.regime == "qcols":
        share = {int(j): round(float(np.concatenate(v).mean()), 2) for j, v in q_cols.items()}
        if not (share and min(share.values()) > 0.5):
            bad.append(f"|q| out of range per listed column: {share}")
    return bad


@pytest.mark.parametrize("case", RBF_JUMPY + STATE_CASES + USER_CASES, ids=lambda c: c.id)
def test_premise(case):
    """The data of each RBF GPU case is in the regime the case names."""
    assert premise_problems(case) == []


@pytest.mark.parametrize("L,D", sorted({(c.l1, c.D) for c in CASES if c.regime == "rough"}))
def test_premise_rough(L, D):
    """i.i.d. N(0, 1) * 0.7 points: nearly every cell is out of range."""
    case = next(c for c in CASES if c.regime == "rough" and (c.l1, c.D) == (L, D))
    share = np.mean([(np.maximum(np.abs(p), np.abs(c)) >= TAU).mean() for _, _, p, c, _ in pair_grids(case)])
    assert share > 0.5, share


# ----------------------------------------------------------------------------- GPU parity
def f32(a):
    return torch.tensor(np.asarray(a), device=DEV, dtype=torch.float32)


def level_weights(M, n1, n2, sym, seed):
    """Random per-level dLoss/dK; K(X) evaluates the upper triangle and mirrors it, so its weights are
    symmetrised (dK(a, b) and dK(b, a) both flow to the pair)."""
    G = np.random.default_rng(seed).standard_normal((M + 1, n1, n2))
    return G + G.transpose(0, 2, 1) if sym else G


def ref_grads(X, Y, M, G, base):
    """fp64 autodiff of the reference graph at the fp32-rounded inputs (what the GPU computes on)."""
    Xr = torch.tensor(np.asarray(X, np.float32).astype(np.float64), requires_grad=True)
    Yr = Xr if Y is None else torch.tensor(np.asarray(Y, np.float32).astype(np.float64), requires_grad=True)
    (ar.k_seq(Xr, Yr, M, base) * torch.tensor(np.asarray(G, np.float32).astype(np.float64))).sum().backward()
    return (Xr.grad.numpy(),) if Y is None else (Xr.grad.numpy(), Yr.grad.numpy())


def hold(label, got, ref):
    """Criterion of the module docstring on each gradient tensor; prints the errors before it asserts."""
    errs = []
    for name, g, r in zip(("gX", "gY"), got, ref):
        g = g.cpu().numpy()
        whole, per_seq = norm_rel_err(g, r), norm_rel_err(g, r, axis_levels=True)
        print(f"VJPERR {label} {name} whole={whole:.3e} per_seq_max={per_seq.max():.3e} "
              f"per_seq={np.array2string(per_seq, precision=2)}")
        errs.append((name, whole, per_seq.max()))
    for name, whole, per_seq in errs:
        assert np.isfinite(whole) and whole < GTOL, (label, name, whole)
        assert per_seq < GTOL, (label, name, "per sequence", per_seq)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_gram_vjp_regime(case):
    """ops.sig_gram_vjp of the raw per-level Gram (recomputed forward sweep) on the case's route and data."""
    from gpsig_amd import ops
    X, Y = case.data()
    G = level_weights(case.M, case.N, case.N2, Y is None, case.seed + 50)
    got = ops.sig_gram_vjp(f32(X), None if Y is None else f32(Y), case.M, f32(G), base=case.base, gout_levels=True)
    ref = ref_grads(X, Y, case.M, G, case.base)
    hold(case.id, got[:len(ref)], ref)


# ----------------------------------------------------------------------------- saved state on jumpy data
@pytest.mark.gpu
@pytest.mark.parametrize("case", STATE_CASES, ids=lambda c: c.id)
def test_saved_state_vjp_jumpy(case):
    """The forward launch that saves the VJP's state (hot-row runs, anchor period 128, slow rows whole) writes
    the plain launch's Gram bit for bit on jumpy data, and the VJP that inverts that state with its own
    regenerated cells (rev_row, sig_bwd.h) meets the fp64 gradient like the VJP that recomputes its sweep."""
    from gpsig_amd import ops
    X, Y = case.data()
    M = case.M
    G = level_weights(M, case.N, case.N2, Y is None, 58)
    Xt, Yt, Gt = f32(X), None if Y is None else f32(Y), f32(G)
    st = torch.empty(ops.sig_state_numel(case.N, None if Y is None else case.N2, case.l2, M), dtype=torch.float32,
                     device=DEV)
    assert torch.equal(ops.sig_gram(Xt, Yt, M, state=st), ops.sig_gram(Xt, Yt, M))
    g1 = ops.sig_gram_vjp(Xt, Yt, M, Gt, gout_levels=True, state=st)
    g0 = ops.sig_gram_vjp(Xt, Yt, M, Gt, gout_levels=True)
    ref = ref_grads(X, Y, M, G, "rbf")
    hold(case.id + "-state", g1[:len(ref)], ref)
    hold(case.id + "-recompute", g0[:len(ref)], ref)


# ----------------------------------------------------------------------------- the user-facing path
@pytest.mark.gpu
@pytest.mark.parametrize("case", USER_CASES, ids=lambda c: c.id)
def test_signature_rbf_gradients_jumpy(case):
    """SignatureRBF(...).K(X) and K(X, X2), normalised, per level, with trainable lengthscales and variances
    (as test_gram_vjp_return_levels_lengthscales_variances of test_grad_gpu.py) on jumpy data: the autograd
    forward's saved-state launch, the VJP from that state and the normalisation's rs / grs terms.  The
    sequences are the case's data times the lengthscales, so the kernel sees the data of the premise."""
    import gpsig_amd
    L, D, M = case.l1, case.D, case.M
    ls = np.array([0.7, 1.3, 1.0, 0.8, 1.2])
    var = np.array([0.5, 1.0, 2.0, 1.5, 0.8])
    X, X2 = (None if v is None else v * ls for v in case.data())
    G = np.random.default_rng(59).standard_normal((M + 1, case.N, case.N2))
    k = gpsig_amd.SignatureRBF(L * D, D, M, lengthscales=ls, variances=var)
    k.lengthscales = torch.tensor(ls, device=DEV, requires_grad=True)
    k.variances = torch.tensor(var, device=DEV, requires_grad=True)
    Xt = torch.tensor(X.reshape(case.N, -1), device=DEV, requires_grad=True)
    X2t = None if X2 is None else torch.tensor(X2.reshape(case.N2, -1), device=DEV, requires_grad=True)
    K = k.K(Xt, X2t, return_levels=True)
    (K * torch.as_tensor(G, device=DEV)).sum().backward()

    Xr = torch.tensor(X, requires_grad=True)
    X2r = None if X2 is None else torch.tensor(X2, requires_grad=True)
    lr, vr = torch.tensor(ls, requires_grad=True), torch.tensor(var, requires_grad=True)
    Kr = ar.K(Xr / lr, None if X2r is None else X2r / lr, M, scale=vr, return_levels=True)
    (Kr * torch.tensor(G)).sum().backward()
    pairs = [("K", K.detach(), Kr.detach()), ("gX", Xt.grad.reshape(X.shape), Xr.grad),
             ("gls", k.lengthscales.grad, lr.grad), ("gvar", k.variances.grad, vr.grad)]
    if X2 is not None:
        pairs.append(("gX2", X2t.grad.reshape(X2.shape), X2r.grad))
    errs = {name: norm_rel_err(g.cpu().numpy(), r.numpy()) for name, g, r in pairs}
    print("VJPERR", case.id, " ".join(f"{n}={e:.3e}" for n, e in errs.items()))
    for name, e in errs.items():
        assert e < GTOL, (name, e)
