"""GPU parity of the inducing-tensor kernels (gpsig_tens_vs_seq, gpsig_tens_vs_seq_state, gpsig_tens_vs_seq_vjp,
gpsig_tens_gram, gpsig_tens_gram_vjp) at every dispatch route and route seam, against the float64 oracle on the
fp32-rounded inputs the kernels receive.

Dispatch, as gpsig_amd/csrc has it (d = channels, M = levels), and the parameter ids that reach each route:

tens-vs-seq forward (gpsig_tens_vs_seq / gpsig_tens_vs_seq_state, sig_tens.hip; tvs_pk_launch / tvs_wide_launch,
sig_tvs_pk.hip)
  order 1, difference, d <= 8, M <= 6   tvs_pk_kernel<d, M, INCR> (rbf) / tvs_lin_kernel<d, M, INCR> (linear): one
                                        instantiation per exact d, M and increments; two sequences per lane, 128 per
                                        block, re-anchored every 32 cells      pk-d1-M6 pk-d4-M2 pk-d6-M4 pk-d7-M6
                                        pk-d8-M2 pk-d2-M4 (N = 131: a second block of three sequences);
                                        pk-L2 pk-L33 pk-L34 (1 cell, one anchor period, one cell past it)
  order 1, difference, d > 8, M <= 8    tvs_wide_kernel<M, INCR, RBF> on GEMM seed tiles          wide-M7 wide-M8
  everything else                       tvs_kernel<DP>, DP = dpad4(d) = 4 / 8 / 16 / 32, 0 for d > 32
      order 2 or difference=False       generic-dp16-d12 generic-dp16-d16 generic-dp32-d17 generic-dp32-d32
      d <= 8 with M = 7                 generic-dp8-M7

tens-vs-seq VJP (gpsig_tens_vs_seq_vjp, sig_tvs_bwd.hip; tvs_bwd_pad: d -> 2, 4, 6, 8, 12, 16; d > 16: the wide VJP
of sig_tvs_bwd_wide.hip)
  tvs_bwd_launch_dp<12, INCR>           vjp-pad12-d9 vjp-pad12-d12 nodiff-pad12 vjp-pad12-M8
  tvs_bwd_launch_dp<16, INCR>           vjp-pad16-d13 vjp-pad16-d16 nodiff-pad16
  tvs_bwd_wide                          vjp-wide-d17 vjp-wide-M8
  saved state: at d = 9 .. 16 the wide forward writes the (T, n, LT) end state and the narrow VJP <12> / <16> reads
  it (every training step at these channel counts); at d = 17 wide forward -> wide VJP.  test_tvs_vjp_kernel_api
  takes the state through autograd.py, test_tvs_vjp_ops_with_and_without_state holds both against the oracle.

tensor Gram forward and VJP (gpsig_tens_gram, gpsig_tens_gram_vjp, sig_tens.hip; dpad4: d -> 4, 8, 16, 32; d > 32:
pair tiles + GEMM, tens_vjp_mm.hip)
  tens_gram_kernel<8> / vjp<8>          gram-dp8-d8
  tens_gram_kernel<16> / vjp<16>        gram-dp16-d9 gram-dp16-d16 gram-dp16-M8
  tens_gram_kernel<32> / vjp<32>        gram-dp32-d17 gram-dp32-d32
  tens_gram_mm / tens_gram_vjp_mm       gram-mm-d33
  tens_gram_kernel<4> / vjp<4>          gram-T257 (forward: second column block holds one lane), gram-T129 (VJP: third
                                        lane block and third t' chunk hold one tensor)
  T = 70 everywhere else: two lane blocks and two t' chunks in the VJP, the second of each partial.
  small-d3 small-d16 small-d46          increments with z1 - z0 ~ 1e-3: the entry is a second difference of four RBF
                                        values that cancel to ~1e-6 of their size (rbf_second_diff's stable form)

References: forwards SignatureKernelRef.K_tens_vs_seq_raw / K_tens_raw (fp64 NumPy), gradients fp64 torch autodiff of
oracle/autodiff_ref.py (K_tens_vs_seq, k_tens_vs_seq, k_tens).  Criterion: norm-relative
max|K32 - K64| < 1e-5 * max|K64| per level; level 0 is exactly 1; gradients norm-relative < 1e-5 per array.  Every
test asserts that no level of the reference output is degenerate (max|ref| >= 1e-30), and prints its figures before
it asserts.  The one structural exception is pk-L2: a sequence of one time cell has no two ordered cells, so levels 2
and 3 are identically zero; there the reference and the kernel must both hold exact zeros.
"""
import numpy as np
import pytest
import torch

from conftest import norm_rel_err
from oracle import autodiff_ref as ar
from oracle import kernels_ref as kr

pytestmark = pytest.mark.gpu
DEV = "cuda"
# observed <= 1.3e-6 (1. packed grid and time edges), 2.7e-6 (2. generic and wide forwards), 3.1e-6 (3. forward
# with the saved state, M = 8), 3.7e-7 (4. Gram), 5.5e-7 (5. Gram with small increments), per level on an MI355X
TOL = 1e-5
# observed <= 9.7e-7 (3. tens-vs-seq VJP, kernel API and ops, with and without the state), 3.1e-6 (4. Gram VJP),
# 5.1e-7 (5. Gram VJP with small increments, per level; 3.3e-5 / 2.3e-5 / 1.7e-4 at d = 3 / 16 / 46 before the
# VJP's corner products were regrouped on dB, see tens_gram_vjp_kernel)
GTOL = 1e-5
BASES = ["rbf", "linear"]
INCR = [pytest.param(False, id="pts"), pytest.param(True, id="incr")]


def t(x):
    return torch.as_tensor(np.asarray(x), device=DEV)


def f32(x):
    return np.asarray(x).astype(np.float32).astype(np.float64)


def zscale(D):
    return 0.5 if D <= 8 else 2.0 / np.sqrt(D)


def tensors(rng, M, T, D, incr):
    LT = M * (M + 1) // 2
    return f32(zscale(D) * rng.standard_normal((LT, T, 2, D) if incr else (LT, T, D)))


def walks(rng, n, L, D):
    """Random walks at the scale the other tensor tests use (unit for D <= 8, twice that above), rounded to fp32."""
    scale = 1.0 if D <= 8 else 2.0
    return f32(np.cumsum(rng.standard_normal((n, L, D)), 1) * scale / np.sqrt(L * D))


def nondegenerate(ref_levels):
    ref_levels = np.asarray(ref_levels)
    assert (np.abs(ref_levels).reshape(len(ref_levels), -1).max(1) >= 1e-30).all(), "degenerate reference level"


def check_levels(tag, got, exp, cells=None):
    """Raw levels: level 0 exactly 1, every level within TOL of the oracle (normalised per level).  cells: the
    number of time cells of the sequences where it is below the level count -- level i sums over i strictly
    ordered cells, so the levels past it are identically zero: the reference must hold exact zeros there (no
    other level may be degenerate) and the kernel must return exact zeros too."""
    assert got.shape == exp.shape and got.dtype == np.float32
    assert np.isfinite(got).all()
    live = len(exp) if cells is None else min(len(exp), cells + 1)
    nondegenerate(exp[:live])
    assert not exp[live:].any() and not got[live:].any(), (tag, "levels past the cell count must be exactly 0")
    err = norm_rel_err(got[:live], exp[:live], axis_levels=True)
    print(f"{tag}: levels {np.array2string(err, precision=2, max_line_width=200)}")
    assert (got[0] == 1.0).all()
    assert (err < TOL).all(), (tag, err)


def check_grad(tag, what, got, ref):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape and np.isfinite(got).all()
    assert np.abs(ref).max() >= 1e-30
    err = norm_rel_err(got, ref)
    print(f"{tag}: d/d{what} {err:.2e}")
    assert err < GTOL, (tag, what, err)


def tvs_forward(tag, Z, X, M, base, incr, order=1, difference=True):
    from gpsig_amd import ops
    D = X.shape[2]
    ref = kr.SignatureKernelRef(X.shape[1] * D, D, M, normalization=False, base=base, order=order,
                                difference=difference)
    exp = ref.K_tens_vs_seq_raw(Z, X, increments=incr)
    got = ops.tens_vs_seq(t(Z), t(X), M, order=order, base=base, difference=difference, increments=incr).cpu().numpy()
    check_levels(tag, got, exp, cells=X.shape[1] - 1 if difference else None)


# ----------------------------------------------------------------------------- 1. packed forward grid
@pytest.mark.parametrize("incr", INCR)
@pytest.mark.parametrize("base", BASES)
@pytest.mark.parametrize("D,M", [pytest.param(d, m, id=f"pk-d{d}-M{m}")
                                 for d, m in [(1, 6), (4, 2), (6, 4), (7, 6), (8, 2), (2, 4)]])
def test_packed_forward_grid(D, M, base, incr):
    """tvs_pk_kernel / tvs_lin_kernel<d, M, INCR> at channel and level counts no other test holds against a
    reference; N = 131 = one full block of 128 sequences (two per lane) and a block holding three; L = 34 crosses
    the 32-cell re-anchoring once."""
    N, T, L = 131, 3, 34
    rng = np.random.default_rng(1000 * D + 10 * M + incr)
    tvs_forward(f"pk d={D} M={M} {base} incr={incr}", tensors(rng, M, T, D, incr), walks(rng, N, L, D), M, base, incr)


@pytest.mark.parametrize("incr", INCR)
@pytest.mark.parametrize("base", BASES)
@pytest.mark.parametrize("L", [pytest.param(L, id=f"pk-L{L}") for L in (2, 33, 34)])
def test_packed_forward_time_edges(L, base, incr):
    """One cell, exactly one anchor period (32 cells) and one cell past it; N = 65: one sequence past the 64 lanes'
    first slots.  With one cell (L = 2) levels 2 and 3 are identically zero: exact zeros on both sides."""
    D, M, N, T = 3, 3, 65, 3
    rng = np.random.default_rng(2000 + 10 * L + incr)
    tvs_forward(f"pk L={L} {base} incr={incr}", tensors(rng, M, T, D, incr), walks(rng, N, L, D), M, base, incr)


# ----------------------------------------------------------------------------- 2. generic DP 16 / 32, wide M = 7, 8
@pytest.mark.parametrize("base", BASES)
@pytest.mark.parametrize("order,difference", [pytest.param(2, True, id="order2"), pytest.param(1, False, id="nodiff")])
@pytest.mark.parametrize("D", [pytest.param(12, id="generic-dp16-d12"), pytest.param(16, id="generic-dp16-d16"),
                               pytest.param(17, id="generic-dp32-d17"), pytest.param(32, id="generic-dp32-d32")])
def test_generic_forward_dp16_dp32(D, order, difference, base):
    """tvs_kernel<16> (d = 12: padded channels, d = 16: none) and tvs_kernel<32> (d = 17, 32) on the two routes
    that reach the generic kernel at these widths: the higher-order recursion and difference=False."""
    M, N, T, L = 3, 20, 4, 10
    rng = np.random.default_rng(3000 + 10 * D + order)
    tvs_forward(f"generic d={D} order={order} diff={difference} {base}", tensors(rng, M, T, D, True),
                walks(rng, N, L, D), M, base, True, order=order, difference=difference)


@pytest.mark.parametrize("incr", INCR)
@pytest.mark.parametrize("base", BASES)
def test_generic_forward_narrow_seven_levels(base, incr):
    """d <= 8 with M = 7: past the packed kernels' six levels, below the wide kernel's nine channels, so the
    order-1 difference recursion runs in tvs_kernel<8> (id generic-dp8-M7)."""
    D, M, N, T, L = 5, 7, 20, 4, 10
    rng = np.random.default_rng(3500 + incr)
    tvs_forward(f"generic-dp8-M7 {base} incr={incr}", tensors(rng, M, T, D, incr), walks(rng, N, L, D), M, base, incr)


@pytest.mark.parametrize("incr", INCR)
@pytest.mark.parametrize("base", BASES)
@pytest.mark.parametrize("D,M", [pytest.param(9, 7, id="wide-M7"), pytest.param(12, 8, id="wide-M8")])
def test_wide_forward_seven_eight_levels(D, M, base, incr):
    """tvs_wide_kernel<7, ...> / <8, ...>; N = 70: two blocks of sequences, the second partial."""
    N, T, L = 70, 3, 12
    rng = np.random.default_rng(4000 + 10 * D + incr)
    tvs_forward(f"wide d={D} M={M} {base} incr={incr}", tensors(rng, M, T, D, incr), walks(rng, N, L, D), M, base, incr)


# ----------------------------------------------------------------------------- 3. tens-vs-seq VJP, 9 .. 17 channels
VJP_D = [pytest.param(9, id="vjp-pad12-d9"), pytest.param(12, id="vjp-pad12-d12"), pytest.param(13, id="vjp-pad16-d13"),
         pytest.param(16, id="vjp-pad16-d16"), pytest.param(17, id="vjp-wide-d17")]


def kernel_api_grads(tag, Z, X, M, base, incr, difference, learn):
    """Gradients of the normalised, level-summed K_tens_vs_seq through the kernel classes (the training path: the
    forward saves its end state where it offers one) against fp64 autodiff."""
    import gpsig_amd
    T, (N, L, D) = Z.shape[1], X.shape
    rng = np.random.default_rng(N + L + D)
    G = f32(rng.standard_normal((T, N)))
    ls = f32(0.8 + 0.4 * rng.random(D)) if learn else np.ones(D)
    var = f32(np.linspace(0.5, 1.5, M + 1)) if learn else np.ones(M + 1)
    cls = gpsig_amd.SignatureRBF if base == "rbf" else gpsig_amd.SignatureLinear
    k = cls(L * D, D, M, difference=difference)
    if learn:
        k.lengthscales = torch.tensor(ls, device=DEV, requires_grad=True)
        k.variances = torch.tensor(var, device=DEV, requires_grad=True)
    Zt = torch.tensor(Z, device=DEV, requires_grad=True)
    Xt = torch.tensor(X.reshape(N, -1), device=DEV, requires_grad=True)
    K = k.K_tens_vs_seq(Zt, Xt, increments=incr)
    (K * t(G)).sum().backward()
    Zr, Xr = torch.tensor(Z, requires_grad=True), torch.tensor(X, requires_grad=True)
    lr, vr = torch.tensor(ls, requires_grad=True), torch.tensor(var, requires_grad=True)
    Kl = ar.K_tens_vs_seq(Zr / lr, Xr / lr, M, base=base, increments=incr, scale=vr, return_levels=True,
                          difference=difference)
    nondegenerate(Kl.detach().numpy())
    Kr = Kl.sum(0)
    (Kr * torch.tensor(G)).sum().backward()
    errK = norm_rel_err(K.detach().cpu().numpy(), Kr.detach().numpy())
    print(f"{tag}: K {errK:.2e}")
    assert errK < TOL
    check_grad(tag, "Z", Zt.grad.cpu().numpy(), Zr.grad.numpy())
    check_grad(tag, "X", Xt.grad.reshape(X.shape).cpu().numpy(), Xr.grad.numpy())
    if learn:
        check_grad(tag, "lengthscales", k.lengthscales.grad.cpu().numpy(), lr.grad.numpy())
        check_grad(tag, "variances", k.variances.grad.cpu().numpy(), vr.grad.numpy())


@pytest.mark.parametrize("incr", INCR)
@pytest.mark.parametrize("base", BASES)
@pytest.mark.parametrize("D", VJP_D)
def test_tvs_vjp_kernel_api(D, base, incr):
    """(a) K_tens_vs_seq (normalised, summed) gradients in Z, X, lengthscales and variances: at d = 9 .. 16 the
    wide forward's saved state feeds tvs_bwd_launch_dp<12> / <16>, at d = 17 the wide VJP."""
    M, N, T, L = 3, 67, 4, 11
    rng = np.random.default_rng(5000 + 10 * D + incr)
    kernel_api_grads(f"vjp api d={D} {base} incr={incr}", tensors(rng, M, T, D, incr), walks(rng, N, L, D), M, base,
                     incr, True, learn=True)


def ops_vjp_with_and_without_state(tag, Z, X, M, base, incr):
    """ops.tens_vs_seq_vjp of the raw levels, recomputing its forward sweep and from the state the forward launch
    saved: both (gZ, gX) pairs against fp64 autodiff of (k_tens_vs_seq * G).sum()."""
    from gpsig_amd import ops
    T, N = Z.shape[1], X.shape[0]
    G = f32(np.random.default_rng(N + T + M).standard_normal((M + 1, T, N)))
    Zt, Xt, Gt = t(Z).float(), t(X).float(), t(G).float()
    st = torch.empty(ops.tens_state_numel(T, N, M), dtype=torch.float32, device=DEV)
    out, st2 = ops.tens_vs_seq(Zt, Xt, M, 1, base, True, incr, state=st)
    assert st2 is st, "the forward offered no saved state"
    Zr, Xr = torch.tensor(Z, requires_grad=True), torch.tensor(X, requires_grad=True)
    Kr = ar.k_tens_vs_seq(Zr, Xr, M, base=base, increments=incr)
    (Kr * torch.tensor(G)).sum().backward()
    check_levels(f"{tag} forward with state", out.cpu().numpy(), Kr.detach().numpy())
    for how, state in (("recompute", None), ("state", st)):
        gZ, gX = ops.tens_vs_seq_vjp(Zt, Xt, M, Gt, base, incr, state=state)
        check_grad(f"{tag} {how}", "Z", gZ.cpu().numpy(), Zr.grad.numpy())
        check_grad(f"{tag} {how}", "X", gX.cpu().numpy(), Xr.grad.numpy())


@pytest.mark.parametrize("incr", INCR)
@pytest.mark.parametrize("base", BASES)
@pytest.mark.parametrize("D", VJP_D)
def test_tvs_vjp_ops_with_and_without_state(D, base, incr):
    """(b) The state's layout between the wide forward and the narrow VJP (d = 9 .. 16), and wide -> wide at 17."""
    M, N, T, L = 3, 67, 4, 11
    rng = np.random.default_rng(6000 + 10 * D + incr)
    ops_vjp_with_and_without_state(f"vjp ops d={D} {base} incr={incr}", tensors(rng, M, T, D, incr),
                                   walks(rng, N, L, D), M, base, incr)


@pytest.mark.parametrize("incr", INCR)
@pytest.mark.parametrize("base", BASES)
@pytest.mark.parametrize("D", [pytest.param(12, id="nodiff-pad12"), pytest.param(16, id="nodiff-pad16")])
def test_tvs_vjp_no_difference(D, base, incr):
    """(c) difference=False (generic forward tvs_kernel<16>, no saved state) through the narrow VJP <12> / <16>."""
    M, N, T, L = 3, 67, 4, 11
    rng = np.random.default_rng(7000 + 10 * D + incr)
    kernel_api_grads(f"vjp nodiff d={D} {base} incr={incr}", tensors(rng, M, T, D, incr), walks(rng, N, L, D), M,
                     base, incr, False, learn=False)


@pytest.mark.parametrize("D", [pytest.param(12, id="vjp-pad12-M8"), pytest.param(17, id="vjp-wide-M8")])
def test_tvs_vjp_eight_levels(D):
    """(d) M = 8 (36 components) in the narrow VJP <12, true> and in the wide VJP, with and without the state of
    tvs_wide_kernel<8, true, true>."""
    M, N, T, L = 8, 20, 3, 9
    rng = np.random.default_rng(8000 + D)
    ops_vjp_with_and_without_state(f"vjp M=8 d={D}", tensors(rng, M, T, D, True), walks(rng, N, L, D), M, "rbf", True)


# ----------------------------------------------------------------------------- 4. tensor Gram, DP 8 | 16 | 32 | tiles
GRAM_D = [pytest.param(8, id="gram-dp8-d8"), pytest.param(9, id="gram-dp16-d9"), pytest.param(16, id="gram-dp16-d16"),
          pytest.param(17, id="gram-dp32-d17"), pytest.param(32, id="gram-dp32-d32"), pytest.param(33, id="gram-mm-d33")]


def gram_forward(tag, Z, M, base, incr):
    from gpsig_amd import ops
    D = Z.shape[-1]
    exp = kr.SignatureKernelRef(4 * D, D, M, base=base).K_tens_raw(Z, increments=incr)
    got = ops.tens_gram(t(Z), M, base=base, increments=incr).cpu().numpy()
    check_levels(tag, got, exp)


def gram_vjp(tag, Z, M, base, incr, per_level=False):
    """ops.tens_gram_vjp with a random non-symmetric gout against autodiff of (k_tens * G).sum(); per_level: each
    level's components normalised on their own."""
    from gpsig_amd import ops
    T = Z.shape[1]
    G = f32(np.random.default_rng(T + M).standard_normal((M + 1, T, T)))
    gZ = ops.tens_gram_vjp(t(Z).float(), M, t(G).float(), base=base, increments=incr).cpu().numpy()
    Zr = torch.tensor(Z, requires_grad=True)
    Kr = ar.k_tens(Zr, M, base, incr)
    nondegenerate(Kr.detach().numpy())
    (Kr * torch.tensor(G)).sum().backward()
    ref = Zr.grad.numpy()
    if not per_level:
        check_grad(tag, "Z", gZ, ref)
        return
    for i in range(1, M + 1):
        k0 = i * (i - 1) // 2
        check_grad(f"{tag} level {i}", "Z", gZ[k0:k0 + i], ref[k0:k0 + i])


@pytest.mark.parametrize("incr", INCR)
@pytest.mark.parametrize("base", BASES)
@pytest.mark.parametrize("D", GRAM_D)
def test_tens_gram_forward(D, base, incr):
    M, T = 4, 70
    rng = np.random.default_rng(9000 + 10 * D + incr)
    gram_forward(f"gram d={D} {base} incr={incr}", tensors(rng, M, T, D, incr), M, base, incr)


@pytest.mark.parametrize("incr", INCR)
@pytest.mark.parametrize("base", BASES)
@pytest.mark.parametrize("D", GRAM_D)
def test_tens_gram_vjp(D, base, incr):
    """T = 70: two lane blocks and two t' chunks, the second of each partial (6 tensors)."""
    M, T = 4, 70
    rng = np.random.default_rng(9500 + 10 * D + incr)
    gram_vjp(f"gram vjp d={D} {base} incr={incr}", tensors(rng, M, T, D, incr), M, base, incr)


def test_tens_gram_eight_levels():
    """M = 8 (TV_MMAX) at d = 16, forward and VJP (id gram-dp16-M8)."""
    M, T, D = 8, 20, 16
    Z = tensors(np.random.default_rng(9900), M, T, D, True)
    gram_forward("gram-dp16-M8", Z, M, "rbf", True)
    gram_vjp("gram-dp16-M8 vjp", Z, M, "rbf", True)


def test_tens_gram_forward_second_column_block():
    """T = 257: the forward's second block of 256 columns holds one lane (id gram-T257)."""
    M, T, D = 2, 257, 3
    gram_forward("gram-T257", tensors(np.random.default_rng(9901), M, T, D, True), M, "rbf", True)


def test_tens_gram_vjp_third_lane_block():
    """T = 129: the VJP's third lane block and third t' chunk hold one tensor (id gram-T129)."""
    M, T, D = 2, 129, 3
    gram_vjp("gram-T129", tensors(np.random.default_rng(9902), M, T, D, True), M, "rbf", True)


# ----------------------------------------------------------------------------- 5. tensor Gram, small increments
@pytest.mark.parametrize("D", [pytest.param(3, id="small-d3"), pytest.param(16, id="small-d16"),
                               pytest.param(46, id="small-d46")])
def test_tens_gram_small_increments(D):
    """z1 = z0 + 1e-3 * noise per coordinate, z0 of scale 0.5: every entry of level i is ~1e-6i of the four RBF
    values it is the second difference of, so taking that difference in fp32 would leave no correct digit at level 1;
    rbf_second_diff / rbf_second_diff_rt (d = 46, tens_vjp_mm.hip) form it without the cancellation.  Forward per
    level, and the VJP with each level's components normalised on their own (level 1 is 1e6 times level 2).
    Observed: forward <= 5.5e-7 per level; VJP <= 5.1e-7 per level.  The VJP kernels used to form dM/dA1 as
    k11 (B1 - A1) - k10 (B0 - A1), two products that agree to |dB| of their size, and missed the bar at level 1
    (3.3e-5, 2.3e-5, 1.7e-4 at d = 3, 16, 46); the same grouping restated in fp32 torch on the CPU gave 4.2e-5 and
    2.3e-5 at d = 3 and 16, the regrouped form (k11 - k10)(B0 - A1) + k11 dB with k11 - k10 = k10 expm1(.) 1.2e-7
    to 2.4e-7: a defect of the form, not fp32's limit, fixed in sig_tens.hip and tens_vjp_mm.hip."""
    M, T = 3, 20
    rng = np.random.default_rng(9950 + D)
    LT = M * (M + 1) // 2
    z0 = f32(0.5 * rng.standard_normal((LT, T, D)))
    z1 = f32(z0 + 1e-3 * rng.standard_normal((LT, T, D)))
    Z = np.stack([z0, z1], axis=2)
    gram_forward(f"small d={D}", Z, M, "rbf", True)
    gram_vjp(f"small d={D} vjp", Z, M, "rbf", True, per_level=True)
