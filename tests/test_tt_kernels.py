"""Low-rank (d = 2 TT) kernels: MFMA Gram / tall-skinny products, the factor
expansion and the dense five-point step, each against a plain PyTorch fp64
reference of the same op; the factored diffusion step against dense stepping.
"""
import math

import numpy as np
import pytest
import torch

from stsphere.models import tt


def _panel(N, dtype=torch.float64, device="cpu"):
    x = torch.linspace(0, 1, N + 2, dtype=torch.float64)[1:-1]
    U = torch.sin(math.pi * x)[:, None] * torch.sin(2 * math.pi * x)[None, :] + \
        0.3 * torch.sin(3 * math.pi * x)[:, None] * torch.sin(math.pi * x)[None, :] + \
        0.05 * torch.exp(-40 * ((x[:, None] - 0.3) ** 2 + (x[None, :] - 0.6) ** 2))
    return U.to(dtype=dtype, device=device)


def test_gram_core_recompression_matches_qr_path_cpu():
    """The Gram/eigen route of the hip step, evaluated with torch on the CPU,
    gives the same rank-2r recompression as the QR route."""
    N = 96
    s = tt.LowRankDiffusion(N, kappa=1.0, eps=1e-9, max_rank=24)
    lr = tt.LowRankField.from_dense(_panel(N), eps=1e-12)
    c = 0.5 * s.dt_max
    D = tt.second_difference(N, s.h)
    Ah = torch.cat([lr.A, c * (D @ lr.A)], 1)
    Bh = torch.cat([lr.B + c * (D @ lr.B), lr.B], 1)
    Xa, Xb = s._core(torch.stack([Ah.T @ Ah, Bh.T @ Bh]).numpy())
    got = (Ah @ torch.from_numpy(Xa)) @ (Bh @ torch.from_numpy(Xb)).T
    want = s.step(lr, c).dense()
    assert float((got - want).norm() / want.norm()) < 1e-8
    dense = s.dense_step(lr.dense(), c)
    assert float((got - dense).norm() / dense.norm()) < 1e-8


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("N,k,m", [(1, 1, 1), (7, 3, 5), (1000, 16, 16), (4099, 20, 37), (20000, 48, 48),
                                   (513, 64, 64), (300, 33, 17)])
def test_gram_matches_torch(N, k, m, dtype):
    from stsphere.ops import tt_ops
    g = torch.Generator().manual_seed(N + k + m)
    A = torch.randn(N, k + 3, generator=g, dtype=torch.float64)[:, 1:k + 1]   # strided rows
    B = torch.randn(N, m, generator=g, dtype=torch.float64)
    want = A.T @ B
    got = tt_ops.gram(A.to(dtype).cuda(), B.to(dtype).cuda(), alpha=0.5).double().cpu()
    tol = 1e-12 if dtype == torch.float64 else 2e-5
    scale = A.abs().T.matmul(B.abs()).clamp_min(1e-30)
    assert float(((got - 0.5 * want).abs() / scale).max()) < tol


@pytest.mark.gpu
def test_gram_is_bitwise_reproducible():
    from stsphere.ops import tt_ops
    A = torch.randn(123457, 40, dtype=torch.float64, device="cuda")
    a = tt_ops.gram(A, A)
    b = tt_ops.gram(A, A)
    assert torch.equal(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("N,k,m", [(1, 1, 1), (65, 3, 5), (1000, 16, 16), (4099, 40, 20), (513, 64, 64),
                                   (300, 33, 17)])
def test_tsmm_matches_torch(N, k, m, dtype):
    from stsphere.ops import tt_ops
    g = torch.Generator().manual_seed(7 * N + k + m)
    A = torch.randn(N, k, generator=g, dtype=torch.float64)
    X = torch.randn(k + 2, m, generator=g, dtype=torch.float64)[1:k + 1]
    C0 = torch.randn(N, m + 4, generator=g, dtype=torch.float64)
    want = 2.0 * A @ X - 0.5 * C0[:, 2:m + 2]
    Cd = C0.to(dtype).cuda()
    tt_ops.tsmm(A.to(dtype).cuda(), X.to(dtype).cuda(), out=Cd[:, 2:m + 2], alpha=2.0, beta=-0.5)
    got = Cd.double().cpu()
    tol = 1e-12 if dtype == torch.float64 else 2e-5
    scale = (2 * A.abs() @ X.abs() + 0.5 * C0[:, 2:m + 2].abs()).clamp_min(1e-30)
    assert float(((got[:, 2:m + 2] - want).abs() / scale).max()) < tol
    assert torch.equal(got[:, :2], C0[:, :2].to(dtype).double())          # untouched columns
    assert torch.equal(got[:, m + 2:], C0[:, m + 2:].to(dtype).double())


@pytest.mark.gpu
@pytest.mark.parametrize("bc", ["dirichlet", "periodic"])
def test_expand_matches_torch(bc):
    from stsphere.ops import tt_ops
    N, r = 257, 9
    X = torch.randn(N, r, dtype=torch.float64)
    D = tt.second_difference(N, 0.1, bc)
    want = torch.cat([1.5 * X + 0.25 * (D @ X), -X + 2.0 * (D @ X)], 1)
    got = tt_ops.expand(X.cuda(), 1.5, 0.25, -1.0, 2.0, 100.0, bc == "periodic").cpu()
    assert torch.allclose(got, want, rtol=1e-13, atol=1e-11)


@pytest.mark.gpu
def test_dense_diffusion_matches_torch():
    from stsphere.ops import tt_ops
    U = torch.randn(130, 75, dtype=torch.float64)
    P = torch.nn.functional.pad(U, (1, 1, 1, 1))
    lap = P[:-2, 1:-1] + P[2:, 1:-1] + P[1:-1, :-2] + P[1:-1, 2:] - 4 * U
    got = tt_ops.dense_diffusion(U.cuda(), 0.2).cpu()
    assert torch.allclose(got, U + 0.2 * lap, rtol=1e-14, atol=1e-14)


@pytest.mark.gpu
@pytest.mark.parametrize("bc", ["dirichlet", "periodic"])
def test_low_rank_diffusion_hip_matches_dense(bc):
    N = 512
    s = tt.LowRankDiffusion(N, kappa=1.0, bc=bc, eps=1e-9, max_rank=24, backend="hip")
    U = _panel(N)
    ref = tt.LowRankDiffusion(N, kappa=1.0, bc=bc, eps=1e-9, max_rank=24)
    lr = tt.LowRankField.from_dense(U.cuda(), eps=1e-12)
    dt = 0.5 * s.dt_max
    dense = U.clone()
    for _ in range(30):
        lr = s.step(lr, dt)
        dense = ref.dense_step(dense, dt)
    got = lr.dense().cpu()
    assert lr.rank <= 24
    assert float((got - dense).norm() / dense.norm()) < 1e-7


@pytest.mark.parametrize("k", [2, 6, 16, 40])
def test_native_core_matches_numpy_core_cpu(k):
    """Host C++ core of the fused step (Jacobi eigen + one-sided Jacobi SVD)
    reproduces the numpy route, including exactly rank-deficient Grams."""
    from stsphere.ops import native
    L = native.require_native()
    rng = np.random.default_rng(k)
    A = rng.standard_normal((300, k))
    B = rng.standard_normal((300, k))
    A[:, -1] = 2.0 * A[:, 0]
    s = tt.LowRankDiffusion(64, eps=1e-9, max_rank=24)
    G = np.ascontiguousarray(np.stack([A.T @ A, B.T @ B]))
    X = np.zeros((k, 2 * k))
    rn = L.stsp_tt_core(k, G.ctypes.data, 1e-9, 24, X.ctypes.data, 2 * k)
    Xa, Xb = s._core(G)
    assert rn == Xa.shape[1] == min(k - 1, 24)
    got = (A @ X[:, :rn]) @ (B @ X[:, rn:2 * rn]).T
    want = (A @ Xa) @ (B @ Xb).T
    assert np.linalg.norm(got - want) / np.linalg.norm(want) < 1e-12


@pytest.mark.gpu
def test_cube_low_rank_diffusion_hip_matches_torch():
    """The cube's factored step on the gfx950 path (MFMA Gram, native core,
    MFMA products; one host round trip per step for all six panels) against
    the torch QR path and the dense six-panel step."""
    N = 64
    x = (torch.arange(N, dtype=torch.float64) + 0.5) / N
    U = torch.stack([torch.outer(torch.sin(math.pi * x * (p + 1) / 3), torch.cos(math.pi * x * (p % 3 + 1) / 2))
                     for p in range(6)]).cuda()
    mh = tt.CubedSphereLowRankDiffusion(N, eps=1e-7, max_rank=24, device="cuda", backend="hip")
    mt = tt.CubedSphereLowRankDiffusion(N, eps=1e-7, max_rank=24, device="cuda")
    Fh, Ft, D = mh.to_factored(U), mt.to_factored(U), U.clone()
    dt = 0.8 * mh.dt_max
    for _ in range(10):
        Fh, Ft, D = mh.step(Fh, dt), mt.step(Ft, dt), mh.dense_step(D, dt)
    torch.cuda.synchronize()
    Rh, Rt = mh.to_dense(Fh), mt.to_dense(Ft)
    assert float((Rh - D).norm() / D.norm()) < 1e-6
    assert float((Rh - Rt).norm() / Rt.norm()) < 1e-6
    assert mh.stats["host_syncs"] == 10


@pytest.mark.gpu
@pytest.mark.parametrize("substeps", [2, 3])
def test_low_rank_diffusion_hip_substeps_match_dense(substeps):
    """Several exact explicit steps per recompression on the gfx950 path
    (stsp_tt_lr_step2: the factors double their rank each substep, k = 2^s r
    <= 64, one Gram / host core / MFMA product pass) against the torch path
    with the same substeps and rank cap (same truncation), and against dense
    stepping for the same simulated time (truncation error only)."""
    N = 512
    mr = 64 >> substeps
    s = tt.LowRankDiffusion(N, kappa=1.0, eps=1e-9, max_rank=mr, backend="hip", substeps=substeps, qr="gram")
    ref = tt.LowRankDiffusion(N, kappa=1.0, eps=1e-9, max_rank=mr, substeps=substeps)
    U = _panel(N)
    lr = tt.LowRankField.from_dense(U.cuda(), eps=1e-12)
    lt = tt.LowRankField.from_dense(U, eps=1e-12)
    dt = 0.5 * s.dt_max
    dense = U.clone()
    for _ in range(24 // substeps):
        lr = s.step(lr, dt)
        lt = ref.step(lt, dt)
    for _ in range(24):
        dense = ref.dense_step(dense, dt)
    assert lr.rank <= mr
    got = lr.dense().cpu()
    # the Gram route squares the conditioning of the factors, and the columns
    # of a 2- or 3-substep expansion (A, c D A, c^2 D^2 A, ...) span a wider
    # range than one step's: measured 4.1e-7 at 2 substeps (1 substep: < 1e-7)
    assert float((got - lt.dense()).norm() / lt.dense().norm()) < 2e-6
    assert float((got - dense).norm() / dense.norm()) < 2e-6


@pytest.mark.gpu
def test_chol_inv_kernel_matches_torch():
    """The k x k shifted-Cholesky kernel of CholeskyQR3: R^T R = G + s I and
    R R^-1 = I, for full-rank and exactly rank-deficient Gram matrices (the
    adaptive form falls back to the shift only for the latter)."""
    from stsphere.ops import tt_ops
    g = torch.Generator().manual_seed(3)
    for k in (3, 17, 40, 64):
        X = torch.randn(500, k, dtype=torch.float64, generator=g)
        if k > 3:
            X[:, -1] = 2.0 * X[:, 0]
        G = (X.T @ X).cuda()
        c = tt.cholqr3_shift(500, k, torch.float64)
        for sc in (c, -c):
            R, Ri, info = tt_ops.chol_inv(G, sc)
            torch.cuda.synchronize()
            assert int(info[0]) == 0
            s = c * float(torch.trace(G))
            shifted = G + s * torch.eye(k, dtype=torch.float64, device="cuda")
            err = lambda want: float((R[0].T @ R[0] - want).abs().max() / want.abs().max())
            if sc > 0:
                assert err(shifted) < 1e-13
            else:   # adaptive: the plain factor unless a pivot failed (a duplicated column may or may not)
                assert min(err(G), err(shifted)) < 1e-13
                if k == 3:
                    assert err(G) < 1e-13
            assert float((R[0] @ Ri[0] - torch.eye(k, dtype=torch.float64, device="cuda")).abs().max()) < 1e-8
            assert float(torch.tril(R[0], -1).abs().max()) == 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("bc", ["dirichlet", "periodic"])
def test_low_rank_diffusion_hip_cholqr3_machine_precision(bc):
    """Round-2 verdict item 7: the device recompression (CholeskyQR3 with MFMA
    Gram / product kernels) has no sqrt(eps) floor: with a 1e-13 tolerance and
    no rank cap the factored run stays within 1e-10 of dense stepping, where the
    Gram/eigen route (qr="gram") stops near 1e-8."""
    N = 512
    s = tt.LowRankDiffusion(N, kappa=1.0, bc=bc, eps=1e-13, backend="hip")
    ref = tt.LowRankDiffusion(N, kappa=1.0, bc=bc, eps=1e-13)
    U = _panel(N)
    lr = tt.LowRankField.from_dense(U.cuda(), eps=1e-15)
    dt = 0.5 * s.dt_max
    dense = U.clone()
    for _ in range(30):
        lr = s.step(lr, dt)
        dense = ref.dense_step(dense, dt)
    got = lr.dense().cpu()
    assert float((got - dense).norm() / dense.norm()) < 1e-10


@pytest.mark.gpu
def test_cube_low_rank_diffusion_hip_cholqr3_machine_precision():
    N = 64
    x = (torch.arange(N, dtype=torch.float64) + 0.5) / N
    U = torch.stack([torch.outer(torch.sin(math.pi * x * (p + 1) / 3), torch.cos(math.pi * x * (p % 3 + 1) / 2))
                     for p in range(6)]).cuda()
    mh = tt.CubedSphereLowRankDiffusion(N, eps=1e-13, device="cuda", backend="hip")
    F, D = mh.to_factored(U), U.clone()
    dt = 0.8 * mh.dt_max
    for _ in range(10):
        F, D = mh.step(F, dt), mh.dense_step(D, dt)
    torch.cuda.synchronize()
    assert max(f.rank for f in F) <= 30
    assert float((mh.to_dense(F) - D).norm() / D.norm()) < 1e-10


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,tol", [(torch.float64, 1e-12), (torch.float32, 1e-5)])
def test_native_cholqr3_step_matches_python_composition(dtype, tol):
    """stsp_tt_lr_step3 (one native call) and the Python-composed CholeskyQR3
    step give the same factored field (to rounding), 1 and 2 substeps, fp64
    and fp32 (the fp32 branch packs floats into the host buffer and uses the
    fp32 shift).  Repeated steps at changing rank reuse one
    workspace."""
    N = 384
    U = _panel(N)
    for ns in (1, 2):
        s = tt.LowRankDiffusion(N, kappa=1.0, eps=1e-12 if dtype == torch.float64 else 1e-6,
                                max_rank=16 if ns == 2 else None, backend="hip", substeps=ns, qr="cholqr3n",
                                dtype=dtype)
        lr = tt.LowRankField.from_dense(U.cuda().to(dtype), eps=1e-14 if dtype == torch.float64 else 1e-7)
        dt = 0.5 * s.dt_max
        a = s.step(lr, dt)
        b = s._step_hip_cqr_py(lr, dt)
        torch.cuda.synchronize()
        da, db = a.dense().double(), b.dense().double()
        assert float((da - db).norm() / db.norm()) < tol
        ws = s._ws3.data_ptr()
        for _ in range(3):
            a = s.step(a, dt)
        assert s._ws3.data_ptr() == ws


@pytest.mark.gpu
def test_lowrank_shallow_water_hip_matches_dense():
    """The factored SWE on the gfx950 recompression (CholeskyQR3 kernels, one
    host transfer of the three cores per stage) against the dense operator."""
    import math
    sw = tt.LowRankShallowWater(256, g=1.0, H=1.0, f=2.0, eps=1e-13, device="cuda", backend="hip")
    W, _, _ = sw.gravity_wave(1, 2, amp=0.1)
    W2, _, _ = sw.gravity_wave(5, 3, amp=0.05)
    W = (W + W2).cuda()
    F, D = sw.to_factored(W), W.clone()
    dt = 0.5 * sw.dt_max
    for _ in range(30):
        F, D = sw.step(F, dt), sw.dense_step(D, dt)
    torch.cuda.synchronize()
    R = sw.to_dense(F)
    assert float((R - D).norm() / D.norm()) < 1e-10
    assert max(f.rank for f in F) <= 8


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,tol", [(torch.float64, 1e-12), (torch.float32, 1e-5)])
@pytest.mark.parametrize("ns,max_rank", [(1, None), (2, None), (2, 6)])
def test_device_core_matches_host_core(dtype, tol, ns, max_rank):
    """the k x k core of the CholeskyQR3 step (R products,
    one-sided Jacobi SVD, truncation) on the device (tt_core_kernel, k <= 32)
    gives the host core's factored field to rounding, with and without a rank
    cap, and the same rank."""
    N = 320
    U = _panel(N)
    if max_rank is None and dtype == torch.float32:
        max_rank = 64 >> ns          # fp32 rounding noise grows the rank past the 64-column kernels
    kw = dict(kappa=1.0, eps=1e-12 if dtype == torch.float64 else 1e-6, max_rank=max_rank, backend="hip",
              substeps=ns, qr="cholqr3n", dtype=dtype)
    dev = tt.LowRankDiffusion(N, core="device", **kw)
    host = tt.LowRankDiffusion(N, core="host", **kw)
    lr = tt.LowRankField.from_dense(U.cuda().to(dtype), eps=1e-14 if dtype == torch.float64 else 1e-7,
                                    max_rank=16 >> ns)
    dt = 0.5 * dev.dt_max
    a, b = lr, lr
    for _ in range(4):
        a = dev.step(a, dt)
        b = host.step(b, dt)
        torch.cuda.synchronize()
        assert a.rank == b.rank
        da, db = a.dense().double(), b.dense().double()
        assert float((da - db).norm() / db.norm()) < tol


def _modes(N, device):
    x = torch.linspace(0, 1, N + 2, dtype=torch.float64, device=device)[1:-1]
    A = torch.stack([torch.sin(math.pi * x), 0.3 * torch.sin(3 * math.pi * x), 0.1 * torch.sin(5 * math.pi * x)], 1)
    B = torch.stack([torch.sin(2 * math.pi * x), torch.sin(math.pi * x), torch.sin(4 * math.pi * x)], 1)
    return A.contiguous(), B.contiguous()


@pytest.mark.gpu
@pytest.mark.parametrize("N,substeps,ncalls,bc", [(1024, 2, 1, "dirichlet"), (1024, 2, 6, "dirichlet"),
                                                  (512, 1, 4, "periodic"), (200, 2, 3, "dirichlet")])
def test_persistent_factored_step_matches_native_chain(N, substeps, ncalls, bc):
    """The one-launch persistent step (ops/csrc/tt_persist.hip: factors in LDS,
    CholeskyQR3 and the core on the device, ncalls steps per launch) against
    the round-4 kernel chain (stsp_tt_lr_step3) of the same numerics, and
    against dense stepping of the same explicit scheme."""
    A, B = _modes(N, "cuda")
    s = tt.LowRankDiffusion(N, kappa=1.0, eps=1e-10, backend="hip", device="cuda", substeps=substeps, bc=bc)
    dt = 0.5 * s.dt_max
    ref = tt.LowRankField(A.clone(), B.clone())
    for _ in range(ncalls):
        ref = s.step(ref, dt)
    got = s.run_persistent(tt.LowRankField(A.clone(), B.clone()), dt, ncalls)
    R, G = ref.dense(), got.dense()
    assert got.rank == ref.rank
    assert float((G - R).norm() / R.norm()) < 1e-12
    sd = tt.LowRankDiffusion(N, kappa=1.0, bc=bc, device="cuda")
    U = A @ B.T
    for _ in range(ncalls * substeps):
        U = sd.dense_step(U, dt)
    assert float((G - U).norm() / U.norm()) < 1e-9


@pytest.fixture
def core_mode(request):
    """The core mode of stsp_tt_recompress / stsp_tt_lr_step3 is a
    process-global (stsp_tt_set_core; a LowRankDiffusion step sets it and
    leaves it): set it to request.param ("device": tt_core_kernel for
    k <= 32, or "host") for one test and restore the old value."""
    from stsphere.ops import native
    L = native.require_native()
    old = L.stsp_tt_set_core(1 if request.param == "device" else 0)
    try:
        yield request.param
    finally:
        L.stsp_tt_set_core(old)


@pytest.mark.gpu
@pytest.mark.parametrize("core_mode", ["device", "host"], indirect=True)
@pytest.mark.parametrize("NA,NB,k,r", [(300, 301, 8, 5), (1024, 1025, 24, 12), (500, 480, 40, 30), (2000, 2001, 64, 20),
                                       (64, 65, 64, 64)])
def test_native_recompress_matches_qr_svd(NA, NB, k, r, core_mode):
    """stsp_tt_recompress (one native call: CholeskyQR3 of both factors, the
    k x k core on the device or the host, two MFMA products) against the
    Householder QR + SVD rounding of the same product: same rank, product to
    1e-12; rank-deficient inputs (k columns, rank r) are rounded to r.  Both
    core modes, set here and not inherited from whichever test ran before."""
    from stsphere.ops import tt_ops
    g = torch.Generator().manual_seed(NA + k)
    X = torch.randn(NA, r, generator=g, dtype=torch.float64)
    Y = torch.randn(NB, r, generator=g, dtype=torch.float64)
    M = torch.randn(r, k, generator=g, dtype=torch.float64)
    s = torch.logspace(0, -6, r, dtype=torch.float64)
    A = (X * s) @ M          # [NA, k] of rank r
    B = Y @ torch.linalg.pinv(M).T
    want = tt.recompress(A, B, 1e-13, None)
    a, b = tt_ops.recompress(A.cuda(), B.cuda(), 1e-13)
    got = (a @ b.T).cpu()
    ref = A @ B.T
    assert a.shape[1] == want.rank, (a.shape, want.rank)
    assert float((got - ref).norm() / ref.norm()) < 1e-12
    # max_rank caps the rank (the leading singular triplets survive)
    a2, b2 = tt_ops.recompress(A.cuda(), B.cuda(), 1e-13, max_rank=3)
    w2 = tt.recompress(A, B, 1e-13, 3).dense()
    assert a2.shape[1] == 3
    assert float(((a2 @ b2.T).cpu() - w2).norm() / ref.norm()) < 1e-10


@pytest.mark.gpu
@pytest.mark.parametrize("N", [20, 48])
def test_cube_lowrank_shallow_water_hip_matches_dense(N):
    """Six-panel factored linear SWE with backend "hip" (every product of
    <= 64 columns rounded by the native CholeskyQR3 call) against the dense
    six-panel operator on the GPU: 1e-10 after four SSP-RK3 steps, mass
    conserved; the native path rounds the narrow products."""
    sw = tt.CubedSphereLowRankShallowWater(N, eps=1e-13, device="cuda", backend="hip")
    W = sw.gaussian_hill()
    F = sw.to_factored(W)
    Wd = W.clone()
    dt = sw.dt_max
    for _ in range(4):
        F = sw.step(F, dt)
        Wd = sw.dense_step(Wd, dt)
    D = sw.to_dense(F)
    err = float((D - Wd).abs().amax() / Wd.abs().amax())
    st = sw.stats
    print(f"N={N}: rel err {err:.2e}, {st['recompressions']} roundings: {st['native']} native calls, "
          f"{st['library']} library, max k {st['max_k']}")
    assert err < 1e-10
    m0 = sw.mass(W)
    assert abs(sw.mass(D) - m0) < 1e-10 * abs(m0)
    assert st["native"] > 0


@pytest.mark.gpu
def test_native_recompress_zero_product():
    """An exactly zero factor (a field at rest times a coefficient) rounds to
    the rank-1 zero field, as the QR + SVD path does, instead of failing the
    Cholesky pivot."""
    from stsphere.ops import tt_ops
    A = torch.zeros(300, 12, dtype=torch.float64, device="cuda")
    B = torch.randn(301, 12, dtype=torch.float64, device="cuda")
    for x, y in ((A, B), (B[:300], A[:, :12].new_zeros(301, 12)), (A, A[:1].new_zeros(301, 12))):
        a, b = tt_ops.recompress(x, y, 1e-13)
        assert a.shape == (x.shape[0], 1) and b.shape == (y.shape[0], 1)
        assert float((a @ b.T).abs().max()) == 0.0
