"""Edge tests of the low-rank (TT) kernels: the persistent step's admission
rule and its rank growth inside one launch, and every primitive of
ops/csrc/tt_kernels.hip (batched Cholesky + inverse, the recompression on
both cores, Gram, tall-skinny product, expansion, dense five-point step) at
the shapes, strides and types where it takes another path, each against the
same operation in fp64 (or extended precision) on the CPU.

Every test prints the error it measured next to its bound
(profiles/tt_edges/README.md keeps a copy of those lines).
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from stsphere.models import tt
from test_tt_kernels import _panel, core_mode  # noqa: F401  (core_mode: the fixture of the core switch)

U64, U32 = 2.0 ** -53, 2.0 ** -24


def _u(dtype):
    return U64 if dtype == torch.float64 else U32


# ----------------------------------------------------------------------------
# persistent step: admission rule (host only)
# ----------------------------------------------------------------------------

def _persist_check(N, r, nsub, max_rank):
    from stsphere.ops import native
    cap = ctypes.c_int(-7)
    rc = native.require_native().stsp_tt_persist_check(N, r, nsub, max_rank, ctypes.byref(cap))
    return int(rc), int(cap.value)


def _persist_limits():
    from stsphere.ops import native
    nk, km = ctypes.c_int(0), ctypes.c_int(0)
    native.require_native().stsp_tt_persist_limits(ctypes.byref(nk), ctypes.byref(km))
    return int(nk.value), int(km.value)


def test_persist_admission_cases_cpu():
    """stsp_tt_persist_check: the rank cap is the largest rank whose NEXT
    expansion still fits the LDS factor, min(16 >> nsub, (12288 / N) >> nsub);
    a starting rank above it is -2, an explicit max_rank above it -3."""
    assert _persist_check(1024, 3, 2, 0) == (0, 3)
    assert _persist_check(1024, 3, 2, 3) == (0, 3)
    assert _persist_check(1024, 3, 2, 4)[0] == -3          # 1024 x (4 << 2) = 16384 doubles > 12288
    assert _persist_check(768, 3, 2, 0) == (0, 4)
    assert _persist_check(768, 3, 2, 4) == (0, 4)
    assert _persist_check(768, 3, 2, 5)[0] == -3
    assert _persist_check(1024, 3, 1, 0) == (0, 6)
    assert _persist_check(1024, 4, 2, 0)[0] == -2
    assert _persist_check(200, 3, 2, 0) == (0, 4)
    assert _persist_check(4, 1, 1, 0)[0] == 0
    assert _persist_check(3, 1, 1, 0)[0] != 0
    assert _persist_check(1025, 1, 1, 0)[0] == -2
    assert _persist_check(512, 0, 1, 0)[0] == -1


def test_persist_admission_cap_fits_lds_cpu():
    """For every accepted (N, nsub) a rank at the cap expands to at most
    nk_max doubles and k_max columns; cap + 1 would not; the cap itself is
    accepted as a starting rank and as max_rank, cap + 1 as neither."""
    nk_max, k_max = _persist_limits()
    seen = 0
    for N in (4, 5, 17, 200, 383, 384, 385, 511, 512, 513, 767, 768, 769, 1023, 1024):
        for nsub in (0, 1, 2, 3, 4):
            rc, cap = _persist_check(N, 1, nsub, 0)
            if rc != 0:
                assert cap < 1, (N, nsub, rc, cap)
                continue
            seen += 1
            assert cap >= 1
            assert N * (cap << nsub) <= nk_max and (cap << nsub) <= k_max, (N, nsub, cap)
            assert N * ((cap + 1) << nsub) > nk_max or ((cap + 1) << nsub) > k_max, (N, nsub, cap)
            assert _persist_check(N, cap, nsub, cap) == (0, cap)
            assert _persist_check(N, cap + 1, nsub, 0)[0] == -2
            assert _persist_check(N, 1, nsub, cap + 1)[0] == -3
    assert seen >= 40


def test_persistent_rank_cap_of_the_solver_cpu():
    for N, ns, cap in ((1024, 2, 3), (768, 2, 4), (1024, 1, 6), (200, 2, 4), (512, 1, 8), (3, 1, 0), (2000, 1, 0)):
        s = tt.LowRankDiffusion(N, eps=1e-12, backend="hip", substeps=ns)
        assert s.persistent_rank_cap(N) == cap, (N, ns)


def test_second_difference_periodic_tiny_n_cpu():
    """The periodic second difference at n = 1 (the cell is its own neighbour
    on both sides: zero) and n = 2 (both neighbours are the other cell), the
    wrap the expansion kernel implements."""
    assert tt.second_difference(1, 1.0, "periodic").tolist() == [[0.0]]
    assert tt.second_difference(2, 1.0, "periodic").tolist() == [[-2.0, 2.0], [2.0, -2.0]]
    assert tt.second_difference(3, 1.0, "periodic").tolist() == [[-2.0, 1.0, 1.0], [1.0, -2.0, 1.0], [1.0, 1.0, -2.0]]
    assert tt.second_difference(2, 1.0).tolist() == [[-2.0, 1.0], [1.0, -2.0]]


# ----------------------------------------------------------------------------
# persistent step: rank growth inside one launch
# ----------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _torch_run(N, r0, ns, eps, cap, ncalls, bc):
    """The torch path (Householder QR + SVD rounding) on the CPU from
    ``_panel(N)`` truncated to rank r0: the start factors, the final dense
    field, the rank after every call and whether the cap decided a rank.
    Every rank decision must have a margin: either the cap decides it (even
    rank ``cap`` leaves a tail above 10 eps^2 total) or no tail sum lies
    within a factor 10 of eps^2 total."""
    s = tt.LowRankDiffusion(N, kappa=1.0, eps=eps, max_rank=cap, substeps=ns, bc=bc)
    lr = tt.LowRankField.from_dense(_panel(N), eps=1e-14, max_rank=r0)
    assert lr.rank == r0
    start = (lr.A.clone(), lr.B.clone())
    dt = 0.5 * s.dt_max
    c = dt * s.kappa
    ranks, capped = [lr.rank], False
    for call in range(ncalls):
        A, B = lr.A, lr.B
        for _ in range(ns):
            A, B = torch.cat([A, c * (s.D @ A)], 1), torch.cat([B + c * (s.D @ B), B], 1)
        sv = torch.linalg.svdvals(torch.linalg.qr(A)[1] @ torch.linalg.qr(B)[1].T)
        tail = [float(x) for x in torch.flip(torch.cumsum(torch.flip(sv * sv, [0]), 0), [0])] + [0.0]
        thr = eps * eps * tail[0]
        if cap < len(sv) and tail[cap] > 10 * thr:
            capped, want = True, cap
        else:
            want = max(1, min(j for j in range(len(tail)) if tail[j] <= thr))
            assert want <= cap
            assert tail[want] < 0.1 * thr and (want == 1 or tail[want - 1] > 10 * thr), \
                f"call {call}: rank {want} has no margin ({tail[want] / thr:.2e}, {tail[want - 1] / thr:.2e})"
        lr = s.step(lr, dt)
        assert lr.rank == want
        ranks.append(lr.rank)
    return start, lr.dense(), tuple(ranks), capped


def _rel(X, Y):
    return float((X - Y).norm() / Y.norm())


def _persist_case(N, r0, ns, eps, ncalls, bc, max_rank=None, strided=False):
    """run_persistent (one launch, and one launch per call) against the
    kernel chain ``step`` at the same cap and the CPU torch path."""
    sp = tt.LowRankDiffusion(N, kappa=1.0, eps=eps, max_rank=max_rank, backend="hip", device="cuda", substeps=ns,
                             bc=bc)
    cap = sp.persistent_rank_cap(N)
    eff = max_rank or cap
    (A0, B0), T, ranks, capped = _torch_run(N, r0, ns, eps, eff, ncalls, bc)
    sc = tt.LowRankDiffusion(N, kappa=1.0, eps=eps, max_rank=eff, backend="hip", device="cuda", substeps=ns, bc=bc)
    dt = 0.5 * sp.dt_max

    def start():
        if not strided:
            return tt.LowRankField(A0.cuda(), B0.cuda())
        g = torch.Generator().manual_seed(N)
        wa = torch.randn(N, r0 + 3, generator=g, dtype=torch.float64).cuda()
        wb = torch.randn(N, r0 + 5, generator=g, dtype=torch.float64).cuda()
        wa[:, 1:r0 + 1] = A0.cuda()
        wb[:, 4:r0 + 4] = B0.cuda()
        f = tt.LowRankField(wa[:, 1:r0 + 1], wb[:, 4:r0 + 4])
        assert f.A.stride(0) > r0 and f.B.stride(0) > r0
        return f

    got = sp.run_persistent(start(), dt, ncalls)
    ref = start()
    for _ in range(ncalls):
        ref = sc.step(ref, dt)
    one = start()
    for _ in range(ncalls):
        one = sp.run_persistent(one, dt, 1)
    torch.cuda.synchronize()
    G, R, O, Tc = got.dense().cpu(), ref.dense().cpu(), one.dense().cpu(), T
    e_pc, e_pt, e_ct, e_ot = _rel(G, R), _rel(G, Tc), _rel(R, Tc), _rel(O, Tc)
    sd = tt.LowRankDiffusion(N, kappa=1.0, bc=bc, device="cuda")
    Ud = A0.cuda() @ B0.cuda().T
    for _ in range(ncalls * ns):
        Ud = sd.dense_step(Ud, dt)
    e_dense = _rel(G, Ud.cpu())
    print(f"TTEDGE persist N={N} r0={r0} substeps={ns} eps={eps:g} ncalls={ncalls} {bc} max_rank={max_rank} "
          f"cap={cap} strided={strided}: torch ranks {list(ranks)} ({'cap' if capped else 'eps'} decides), "
          f"persist/chain/one-per-call rank {got.rank}/{ref.rank}/{one.rank}, persist vs chain {e_pc:.2e}, "
          f"vs torch path: persist {e_pt:.2e} chain {e_ct:.2e} one-per-call {e_ot:.2e} "
          f"(bound {'2 chain + 1e-12' if capped else '1e-12 persist vs chain'}), persist vs dense {e_dense:.2e}")
    assert got.rank == ref.rank == one.rank == ranks[-1]
    assert got.rank <= cap
    if capped:
        assert e_pt <= 2 * e_ct + 1e-12
        assert e_ot <= 2 * e_ct + 1e-12
    else:
        assert e_pc < 1e-12
        assert _rel(O, R) < 1e-12
    return got, ranks, e_dense


@pytest.mark.gpu
@pytest.mark.parametrize("max_rank", [None, 4])
def test_persistent_rank_growth_at_the_lds_limit(max_rank):
    """N = 768, 2 substeps: the rank grows 3 -> 4 in the first call, and a
    rank-4 factor expands to 768 x 16 = 12288 doubles, the last element of the
    LDS factor.  eps = 1e-13 wants rank >= 5, so the cap (4) decides."""
    got, ranks, _ = _persist_case(768, 3, 2, 1e-13, 3, "dirichlet", max_rank=max_rank)
    assert ranks == (3, 4, 4, 4) and got.rank == 4


@pytest.mark.gpu
def test_persistent_shape_that_overran():
    """N = 1024, 2 substeps, eps = 1e-13 from a general field: the rank wants to
    grow to 4, whose expansion (1024 x 16) is past the 12288-double LDS factor.
    The cap is 3, the rank stays 3, the result is within 1e-9 of dense stepping
    (CPU torch path at cap 3: 6.6e-11), and max_rank = 4 is refused by name
    before any launch."""
    got, ranks, e_dense = _persist_case(1024, 3, 2, 1e-13, 3, "dirichlet")
    assert ranks == (3, 3, 3, 3) and got.rank == 3
    assert e_dense < 1e-9
    s4 = tt.LowRankDiffusion(1024, kappa=1.0, eps=1e-13, max_rank=4, backend="hip", device="cuda", substeps=2)
    (A0, B0), _, _, _ = _torch_run(1024, 3, 2, 1e-13, 3, 3, "dirichlet")
    with pytest.raises(RuntimeError, match=r"rank cap of this shape is 3"):
        s4.run_persistent(tt.LowRankField(A0.cuda(), B0.cuda()), 0.5 * s4.dt_max, 3)
    assert getattr(s4, "_pkey", None) is None       # refused before the launch buffers exist


@pytest.mark.gpu
def test_persistent_rank_changes_from_call_to_call():
    """N = 512, 1 substep, cap 8, eps = 1e-12: the torch path's ranks are
    3, 4, 5, 5, 5, every decision with a margin of more than 10 in the tail
    sums (asserted in _torch_run)."""
    got, ranks, _ = _persist_case(512, 3, 1, 1e-12, 4, "dirichlet")
    assert len(set(ranks[1:])) >= 2 and got.rank == ranks[-1]


@pytest.mark.gpu
@pytest.mark.parametrize("N,r0,ns,bc,strided", [(4, 1, 1, "dirichlet", False), (4, 1, 1, "periodic", False),
                                                (5, 1, 2, "dirichlet", False), (17, 3, 2, "dirichlet", True),
                                                (17, 3, 2, "periodic", False), (1023, 3, 2, "dirichlet", False)])
def test_persistent_small_and_odd_sizes(N, r0, ns, bc, strided):
    _persist_case(N, r0, ns, 1e-13, 3, bc, strided=strided)


# ----------------------------------------------------------------------------
# chol_inv, batched
# ----------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("k", [1, 2, 16, 17, 32, 33, 64])
def test_chol_inv_batched_edges(k, dtype):
    """One batched call over five matrices (well conditioned, exactly rank
    deficient, exactly zero, symmetric indefinite, well conditioned), a strided
    view of a larger buffer, with the shift and adaptively.  fp64: the 1e-13 /
    1e-8 of the contiguous test; fp32: the componentwise backward error bound
    of Cholesky, |G_s - R^T R| <= 2 (k + 1) u |R^T| |R| (Higham, Accuracy and
    Stability, Theorem 10.3; the factor 2 for a square root or division that
    is not correctly rounded), and of the triangular solves behind R^-1,
    |R Ri - I| <= 2 (k + 1) u |R| |Ri| (ibid., Theorem 8.5)."""
    from stsphere.ops import tt_ops
    N = 200
    u = _u(dtype)
    g = torch.Generator().manual_seed(100 + k)
    Gs = []
    for b in range(5):
        X = torch.randn(N, k, generator=g, dtype=torch.float64)
        Gs.append(X.T @ X)
    kinds = ["well", "well", "zero", "well", "well"]
    if k >= 2:
        kinds[1], kinds[3] = "deficient", "indefinite"
        Gs[1][:, k - 1] = Gs[1][:, 0]            # column k-1 duplicates column 0
        Gs[1][k - 1, :] = Gs[1][0, :]
        Gs[3][1, 1] = -Gs[3][1, 1]
    Gs[2].zero_()
    big = torch.full((5, k + 2, k + 3), 777.0, dtype=dtype)
    big[:, 1:k + 1, 2:k + 2] = torch.stack(Gs).to(dtype)
    Gh = big[:, 1:k + 1, 2:k + 2].double()        # what the kernel reads, exactly
    bigd = big.cuda()
    keep = bigd.clone()
    Gd = bigd[:, 1:k + 1, 2:k + 2]
    assert Gd.stride(1) > k and Gd.stride(2) == 1
    c = tt.cholqr3_shift(N, k, dtype)
    eye = torch.eye(k, dtype=torch.float64)
    for sc in (c, -c):
        R, Ri, info = tt_ops.chol_inv(Gd, sc)
        torch.cuda.synchronize()
        assert torch.equal(bigd, keep)             # the input and the guard elements around it
        R, Ri, info = R.double().cpu(), Ri.double().cpu(), info.cpu().tolist()
        for b, kind in enumerate(kinds):
            tag = f"TTEDGE chol_inv {str(dtype)[6:]} k={k} {'shifted' if sc > 0 else 'adaptive'} entry {b} ({kind})"
            if kind == "indefinite":
                print(f"{tag}: info {info[b]} (want 2)")
                assert info[b] == 2                # first failing pivot 1, reported as pivot + 1
                continue
            assert info[b] == 0, (tag, info[b])
            if kind == "zero":
                print(f"{tag}: info 0, R == 0 {bool((R[b] == 0).all())}, Ri == I {bool(torch.equal(Ri[b], eye))}")
                assert bool((R[b] == 0).all()) and torch.equal(Ri[b], eye)
                continue
            assert float(torch.tril(R[b], -1).abs().max()) == 0.0
            plain = Gh[b]
            shifted = plain + (c * float(torch.trace(plain))) * eye
            RtR = R[b].T @ R[b]
            RRi = R[b] @ Ri[b]
            if dtype == torch.float64:
                err = lambda want: float((RtR - want).abs().max() / want.abs().max())
                e_inv = float((RRi - eye).abs().max())
                bound, bound_inv = 1e-13, 1e-8
            else:       # worst ratio of the error to the componentwise bound (<= 1 passes)
                def ratio(E, bnd):      # 0 / 0 (the exactly zero lower triangle of R Ri) counts as 0
                    return float(torch.where(E == 0, torch.zeros_like(E), E / bnd).max())
                cb = 2 * (k + 1) * u * (R[b].abs().T @ R[b].abs())
                err = lambda want: ratio((RtR - want).abs(), cb)
                e_inv = ratio((RRi - eye).abs(), 2 * (k + 1) * u * (R[b].abs() @ Ri[b].abs()))
                bound, bound_inv = 1.0, 1.0
            if sc > 0:
                e, which = err(shifted), "shifted"
            elif kind == "well":
                e, which = err(plain), "plain"       # no pivot of a well-conditioned Gram fails
            else:
                ep, es = err(plain), err(shifted)
                e, which = (ep, "plain") if ep <= es else (es, "shifted")
            unit = "" if dtype == torch.float64 else " x its componentwise bound"
            print(f"{tag}: R^T R vs {which} matrix {e:.2e}{unit} (bound {bound:g}), R Ri vs I {e_inv:.2e}{unit} "
                  f"(bound {bound_inv:g})")
            assert e < bound, tag
            assert e_inv < bound_inv, tag


# ----------------------------------------------------------------------------
# recompress, both cores
# ----------------------------------------------------------------------------

def _product_of_rank(NA, NB, k, s, seed, dtype=torch.float64):
    """A [NA, k], B [NB, k] with A B^T = P diag(s) Q^T, P and Q orthonormal
    (the singular values of the product are s, ties included), as column
    slices of wider matrices (lda, ldb > k)."""
    g = torch.Generator().manual_seed(seed)
    r = len(s)
    P = torch.linalg.qr(torch.randn(NA, r, generator=g, dtype=torch.float64))[0]
    Q = torch.linalg.qr(torch.randn(NB, r, generator=g, dtype=torch.float64))[0]
    M = torch.randn(r, k, generator=g, dtype=torch.float64)
    wa = torch.randn(NA, k + 3, generator=g, dtype=torch.float64)
    wb = torch.randn(NB, k + 2, generator=g, dtype=torch.float64)
    wa[:, 2:k + 2] = (P * torch.as_tensor(s, dtype=torch.float64)) @ M
    wb[:, 1:k + 1] = Q @ torch.linalg.pinv(M).T
    wa, wb = wa.to(dtype), wb.to(dtype)
    return wa[:, 2:k + 2], wb[:, 1:k + 1]


_CORE_K = [("device", k) for k in (1, 2, 5, 17, 31, 32)] + [("host", k) for k in (1, 2, 5, 17, 31, 32, 33, 63)]


def _recompress_check(tag, A, B, eps, cap, tol):
    """tt_ops.recompress of strided A, B against tt.recompress on the CPU:
    same rank; the product against A B^T (no cap) or against the torch
    rounding at the same cap, relative to |A B^T|."""
    from stsphere.ops import tt_ops
    want = tt.recompress(A.contiguous(), B.contiguous(), eps, cap)
    Ad = torch.empty_strided(A.shape, A.stride(), dtype=A.dtype, device="cuda").copy_(A)
    Bd = torch.empty_strided(B.shape, B.stride(), dtype=B.dtype, device="cuda").copy_(B)
    assert Ad.stride(0) > A.shape[1] and Bd.stride(0) > B.shape[1]
    a, b = tt_ops.recompress(Ad, Bd, eps, max_rank=cap)
    ref = A @ B.T
    got = (a @ b.T).cpu()
    e = float((got - (ref if cap is None else want.dense())).norm() / ref.norm())
    print(f"TTEDGE recompress {tag} max_rank={cap}: rank {a.shape[1]} (torch {want.rank}), "
          f"product error {e:.2e} (bound {tol:g})")
    assert a.shape[1] == want.rank, (tag, a.shape, want.rank)
    assert e < tol, tag
    return a.shape[1]


@pytest.mark.gpu
@pytest.mark.parametrize("core_mode,k", _CORE_K, indirect=["core_mode"])
def test_recompress_edges_both_cores(core_mode, k):
    """Odd k (the round-robin dummy column), k = 1, 2, the device / host switch
    at 32 / 33, rank-deficient inputs, exact ties in the spectrum and a cap
    below the eps rank, all as column slices (lda, ldb > k)."""
    NA, NB = 300, 301
    # the logspace spectrum of the contiguous test, rank r < k
    r = max(1, (k + 1) // 2) if k > 1 else 1
    A, B = _product_of_rank(NA, NB, k, torch.logspace(0, -6, r, dtype=torch.float64).tolist(), 7 * k)
    rn = _recompress_check(f"{core_mode} core k={k} logspace r={r}", A, B, 1e-13, None, 1e-12)
    assert rn == r
    if r >= 2:   # a cap below the eps rank: the leading triplets survive
        _recompress_check(f"{core_mode} core k={k} logspace r={r}", A, B, 1e-13, max(1, r // 2), 1e-10)
    # exact ties: the vectors inside a tie are arbitrary, the product and the rank are not
    ties = [1.0, 1.0, 1.0, 0.5, 0.5, 1e-3][:max(1, k - 1) if k > 1 else 1]
    A, B = _product_of_rank(NA, NB, k, ties, 7 * k + 1)
    rn = _recompress_check(f"{core_mode} core k={k} ties {ties}", A, B, 1e-13, None, 1e-12)
    assert rn == len(ties)
    if len(ties) > 3:   # a cap at the end of the first tie (sigma_3 = 1 > sigma_4 = 0.5): unique
        _recompress_check(f"{core_mode} core k={k} ties {ties}", A, B, 1e-13, 3, 1e-10)
    # full column rank (r = k), capped: with rank-deficient factors the trailing columns of the
    # core are tiny before any rotation (R is triangular with tiny trailing pivots), so only this
    # class needs the last column -- the partner of the dummy when k is odd -- to be rotated
    A, B = _product_full_rank(NA, NB, k, torch.logspace(0, -6, k, dtype=torch.float64).tolist(), 7 * k + 2,
                              torch.float64)
    rn = _recompress_check(f"{core_mode} core k={k} full rank", A, B, 1e-13, None, 1e-12)
    assert rn == k
    if k >= 2:
        _recompress_check(f"{core_mode} core k={k} full rank", A, B, 1e-13, max(1, k // 2), 1e-10)


@pytest.mark.gpu
@pytest.mark.parametrize("core_mode", ["device", "host"], indirect=True)
def test_recompress_fewer_rows_than_columns(core_mode):
    """NA = 10 < k = 24: the Gram of A is exactly rank deficient (rank <= 10)."""
    g = torch.Generator().manual_seed(24)
    A = torch.randn(10, 27, generator=g, dtype=torch.float64)[:, 1:25]
    B = torch.randn(300, 26, generator=g, dtype=torch.float64)[:, 2:26]
    rn = _recompress_check(f"{core_mode} core NA=10 NB=300 k=24", A, B, 1e-13, None, 1e-12)
    assert rn <= 10
    _recompress_check(f"{core_mode} core NA=10 NB=300 k=24", A, B, 1e-13, 4, 1e-10)


def _product_full_rank(NA, NB, k, s, seed, dtype):
    """A [NA, k], B [NB, k] of full column rank with A B^T = P diag(s) Q^T:
    A = P diag(sqrt s) M, B = Q diag(sqrt s) M with M orthogonal, so each
    factor has the condition number sqrt(s_1 / s_k); column slices."""
    g = torch.Generator().manual_seed(seed)
    P = torch.linalg.qr(torch.randn(NA, k, generator=g, dtype=torch.float64))[0]
    Q = torch.linalg.qr(torch.randn(NB, k, generator=g, dtype=torch.float64))[0]
    M = torch.linalg.qr(torch.randn(k, k, generator=g, dtype=torch.float64))[0]
    h = torch.as_tensor(s, dtype=torch.float64).sqrt()
    wa = torch.randn(NA, k + 3, generator=g, dtype=torch.float64)
    wb = torch.randn(NB, k + 2, generator=g, dtype=torch.float64)
    wa[:, 2:k + 2] = (P * h) @ M
    wb[:, 1:k + 1] = (Q * h) @ M
    wa, wb = wa.to(dtype), wb.to(dtype)
    return wa[:, 2:k + 2], wb[:, 1:k + 1]


def _fp32_pair(A, B, eps):
    """(rank, error) of tt_ops.recompress and of tt.recompress in fp32 on the
    same fp32 inputs, the errors against the fp64 product of those inputs."""
    from stsphere.ops import tt_ops
    ref = A.double() @ B.double().T
    want = tt.recompress(A.contiguous(), B.contiguous(), eps, None)
    e_torch = float((want.dense().double() - ref).norm() / ref.norm())
    Ad = torch.empty_strided(A.shape, A.stride(), dtype=A.dtype, device="cuda").copy_(A)
    Bd = torch.empty_strided(B.shape, B.stride(), dtype=B.dtype, device="cuda").copy_(B)
    a, b = tt_ops.recompress(Ad, Bd, eps)
    e_hip = float(((a.double() @ b.double().T).cpu() - ref).norm() / ref.norm())
    return a.shape[1], e_hip, want.rank, e_torch, ref


@pytest.mark.gpu
@pytest.mark.parametrize("core_mode,k", [("device", 12), ("host", 40)], indirect=["core_mode"])
def test_recompress_fp32_against_torch_fp32(core_mode, k):
    """fp32, eps = 1e-5: the same rank as tt.recompress run in fp32 by torch on
    the same inputs, and an error against the fp64 product of those inputs of
    at most 4 x the torch fp32 rounding's (the margin this suite gives an fp32
    kernel over its fp32 twin).

    The inputs have full column rank and factors of condition number 100
    (product spectrum 1 ... 1e-4, every value 100 x above eps^2 total, so the
    rank is k with margin).  That is the domain of shifted CholeskyQR3 in
    fp32: with the shift coefficient c = 11 (N k + k (k + 1)) u (9e-3 at
    N = 301, k = 40) pass 1 leaves a direction of relative weight w with
    w / sqrt(c) in Q, and the unshifted passes 2 and 3 repair that only while
    (sqrt(c) / w)^2 k u < 1, a factor condition number of a few hundred.
    Outside it -- an exactly rank-deficient fp32 factor -- see
    test_recompress_fp32_rank_deficient_keeps_the_bound."""
    A, B = _product_full_rank(300, 301, k, torch.logspace(0, -4, k, dtype=torch.float64).tolist(), 11 * k,
                              torch.float32)
    rn, e_hip, rt, e_torch, ref = _fp32_pair(A, B, 1e-5)
    sv = torch.linalg.svdvals(ref)
    assert float(sv[k - 1] ** 2) > 10 * 1e-10 * float((sv * sv).sum())    # rank k (of min(NA, NB) values) with margin
    print(f"TTEDGE recompress fp32 {core_mode} core k={k} full rank: rank {rn} (torch fp32 {rt}), "
          f"error vs fp64 product: kernel {e_hip:.2e}, torch fp32 {e_torch:.2e} (bound 4 x torch)")
    assert rn == rt == k
    assert e_hip <= 4 * e_torch


@pytest.mark.gpu
@pytest.mark.parametrize("core_mode,k", [("device", 12), ("host", 40)], indirect=["core_mode"])
def test_recompress_fp32_rank_deficient_keeps_the_bound(core_mode, k):
    """fp32 factors of k columns and rank k / 2 (spectrum 1 ... 1e-4),
    eps = 1e-5.  The error bound holds (<= 4 x the torch fp32 rounding's) and
    the rank is never below the torch rank, but it is NOT guaranteed to equal
    it: a null direction of a factor survives each shifted pass with the
    weight sqrt(c), so the core keeps a spurious singular value of up to
    c^(3/2) per factor (c the shift coefficient: 1.2e-4 at k = 12, 8.5e-4 at
    k = 40, far above eps), and the rounding then keeps up to all k columns.
    The torch composition of the same algorithm (tt.recompress_many in fp32)
    does the same: measured rank 40 of 40 at k = 40 where Householder QR +
    SVD gives 20, rank 6 at k = 12.  fp64 is inside the domain
    (c^(3/2) = 6e-17 < eps = 1e-13): the rank-deficient fp64 cases above
    assert the rank."""
    r = k // 2
    A, B = _product_of_rank(300, 301, k, torch.logspace(0, -4, r, dtype=torch.float64).tolist(), 11 * k,
                            dtype=torch.float32)
    rn, e_hip, rt, e_torch, ref = _fp32_pair(A, B, 1e-5)
    sv = torch.linalg.svdvals(ref)
    thr = 1e-10 * float((sv * sv).sum())
    assert float((sv[r:] ** 2).sum()) < 0.1 * thr and float((sv[r - 1:] ** 2).sum()) > 10 * thr   # rank r with margin
    print(f"TTEDGE recompress fp32 {core_mode} core k={k} rank-deficient r={r}: rank {rn} (torch fp32 {rt}), "
          f"error vs fp64 product: kernel {e_hip:.2e}, torch fp32 {e_torch:.2e} (bound 4 x torch; rank >= torch's)")
    assert rt == r and r <= rn <= k
    assert e_hip <= 4 * e_torch


# ----------------------------------------------------------------------------
# gram, tsmm
# ----------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("k,m", [(5, 64), (64, 64)])
def test_gram_value_above_65536_rows(k, m):
    """N = 70001: the partial blocks are capped at 256, so a wave makes more
    than one unrolled trip.  One dropped or doubled 4-row chunk is ~1e-5 of
    |A|^T |B|; the bound is the 1e-12 of the small shapes."""
    from stsphere.ops import tt_ops
    N = 70001
    assert tt_ops.gram_blocks(N) == 256 and (N + 3) // 4 > 256 * 4 * 4
    g = torch.Generator().manual_seed(k + m)
    A = torch.randn(N, k + 3, generator=g, dtype=torch.float64)[:, 2:k + 2]
    B = torch.randn(N, m, generator=g, dtype=torch.float64)
    want = A.T @ B
    scale = A.abs().T @ B.abs()
    wide = torch.full((k, m + 5), -3.0, dtype=torch.float64, device="cuda")
    Ad = torch.empty_strided(A.shape, A.stride(), dtype=A.dtype, device="cuda").copy_(A)
    assert Ad.stride(0) > k
    out = tt_ops.gram(Ad, B.cuda(), out=wide[:, 2:m + 2])
    got = wide.cpu()
    e = float(((got[:, 2:m + 2] - want).abs() / scale).max())
    print(f"TTEDGE gram N={N} k={k} m={m} strided A and out: max |error| / (|A|^T |B|) {e:.2e} (bound 1e-12)")
    assert e < 1e-12
    assert bool((got[:, :2] == -3.0).all()) and bool((got[:, m + 2:] == -3.0).all())
    assert out.data_ptr() == wide[:, 2:m + 2].data_ptr()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("N", [1, 63, 64, 65])
def test_tsmm_beta_zero_does_not_read_out(N, dtype):
    """beta = 0 overwrites: an ``out`` full of NaN gives the finite product
    (one block holds 64 rows); alpha = 0 with beta = 1 leaves ``out``
    bit-identical."""
    from stsphere.ops import tt_ops
    tol = 1e-12 if dtype == torch.float64 else 2e-5          # the tolerances of test_tsmm_matches_torch
    for k, m in ((5, 7), (33, 17)):
        g = torch.Generator().manual_seed(N + k)
        A = torch.randn(N, k, generator=g, dtype=torch.float64).to(dtype)
        X = torch.randn(k, m, generator=g, dtype=torch.float64).to(dtype)
        want = 2.0 * A.double() @ X.double()
        scale = (2 * A.double().abs() @ X.double().abs()).clamp_min(1e-30)
        wide = torch.full((N, m + 4), float("nan"), dtype=dtype, device="cuda")
        tt_ops.tsmm(A.cuda(), X.cuda(), out=wide[:, 1:m + 1], alpha=2.0, beta=0.0)
        got = wide.double().cpu()
        assert bool(torch.isfinite(got[:, 1:m + 1]).all())
        e = float(((got[:, 1:m + 1] - want).abs() / scale).max())
        print(f"TTEDGE tsmm {str(dtype)[6:]} N={N} k={k} m={m} beta=0 into NaN: max |error| / scale {e:.2e} "
              f"(bound {tol:g})")
        assert e < tol
        assert bool(torch.isnan(got[:, :1]).all()) and bool(torch.isnan(got[:, m + 1:]).all())
        C0 = torch.randn(N, m + 4, generator=g, dtype=torch.float64).to(dtype).cuda()
        C = C0.clone()
        tt_ops.tsmm(A.cuda(), X.cuda(), out=C[:, 1:m + 1], alpha=0.0, beta=1.0)
        same = torch.equal(C.view(torch.int64 if dtype == torch.float64 else torch.int32),
                           C0.view(torch.int64 if dtype == torch.float64 else torch.int32))
        print(f"TTEDGE tsmm {str(dtype)[6:]} N={N} k={k} m={m} alpha=0 beta=1: out bit-identical {same}")
        assert same


# ----------------------------------------------------------------------------
# expand, dense_diffusion
# ----------------------------------------------------------------------------

def _ld(t):
    return t.double().numpy().astype(np.longdouble)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("bc", ["dirichlet", "periodic"])
def test_expand_edges(bc, dtype):
    """N around the 256-element block, N = 1, 2 (periodic: the row is its own
    neighbour / both neighbours are the other row), r = 1, 7, 32, X a column
    slice and out wider than 2r.  Reference: second_difference applied in
    extended precision, so the bound is the kernel's alone:
    8 u (|x0 c| + |x1| ih2 (|l| + |h| + 2 |c|)) per element (at most five
    roundings on that chain, with or without FMA contraction)."""
    from stsphere.ops import tt_ops
    u = _u(dtype)
    x0, x1, y0, y1, ih2 = 1.5, 0.25, -1.0, 2.0, 100.0       # exact in fp32
    for N in (1, 2, 3, 255, 256, 257):
        D = tt.second_difference(N, 1.0, bc)
        Dl, Da = _ld(D), _ld(D.abs())
        for r in (1, 7, 32):
            g = torch.Generator().manual_seed(N * 40 + r)
            wide = torch.randn(N, r + 4, generator=g, dtype=torch.float64).to(dtype)
            X = wide[:, 3:r + 3]
            Xl = _ld(X)
            DX, aDX = (Dl @ Xl) * ih2, (Da @ np.abs(Xl)) * ih2      # aDX = ih2 (|l| + |h| + 2 |c|)
            want = np.concatenate([x0 * Xl + x1 * DX, y0 * Xl + y1 * DX], 1)
            bound = 8 * u * np.concatenate([abs(x0) * np.abs(Xl) + abs(x1) * aDX,
                                            abs(y0) * np.abs(Xl) + abs(y1) * aDX], 1)
            Xd = wide.cuda()[:, 3:r + 3]
            outw = torch.full((N, 2 * r + 3), 5.0, dtype=dtype, device="cuda")
            assert Xd.stride(0) > r
            tt_ops.expand(Xd, x0, x1, y0, y1, ih2, bc == "periodic", out=outw)
            got = outw.cpu()
            err = np.abs(_ld(got[:, :2 * r]) - want)
            ratio = float((err / np.maximum(bound, np.longdouble(1e-300))).max())
            print(f"TTEDGE expand {str(dtype)[6:]} {bc} N={N} r={r}: max |error| {float(err.max()):.2e}, "
                  f"{ratio:.3f} of the bound 8 u (|x0 c| + |x1| ih2 (|l| + |h| + 2 |c|))")
            assert bool((err <= bound).all()), (N, r, ratio)
            assert bool((got[:, 2 * r:] == 5.0).all())


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("N,M", [(1, 1), (1, 64), (4, 64), (5, 65), (3, 129), (130, 75)])
def test_dense_diffusion_edges(N, M, dtype):
    """Shapes at the 4-row x 64-column block boundaries.  Reference in extended
    precision; bound 8 u (|u| + |c| (|n| + |s| + |w| + |e| + 4 |u|))."""
    from stsphere.ops import tt_ops
    u = _u(dtype)
    c = 0.2
    g = torch.Generator().manual_seed(N * 1000 + M)
    U = torch.randn(N, M, generator=g, dtype=torch.float64).to(dtype)
    P = np.pad(_ld(U), 1)
    nb = P[:-2, 1:-1], P[2:, 1:-1], P[1:-1, :-2], P[1:-1, 2:]
    Ul = P[1:-1, 1:-1]
    want = Ul + np.longdouble(c) * (nb[0] + nb[1] + nb[2] + nb[3] - 4 * Ul)
    bound = 8 * u * (np.abs(Ul) + abs(c) * (sum(np.abs(x) for x in nb) + 4 * np.abs(Ul)))
    got = tt_ops.dense_diffusion(U.cuda(), c).cpu()
    err = np.abs(_ld(got) - want)
    ratio = float((err / bound).max())
    print(f"TTEDGE dense_diffusion {str(dtype)[6:]} {N}x{M}: max |error| {float(err.max()):.2e}, {ratio:.3f} of the "
          f"bound 8 u (|u| + |c| (|n| + |s| + |w| + |e| + 4 |u|))")
    assert bool((err <= bound).all()), ratio
