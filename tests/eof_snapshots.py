"""Snapshots with a known EOF decomposition, shared by test_eof.py and
test_eof_gpu.py.

``snapshots(N, S, r)``: r patterns on C<N>, low polynomials of the cell centres'
x, y, z (x^a y^b z^c with c <= 1, which are independent on the sphere, in
ascending degree without the constant) made orthonormal under the area weights
a_i; r orthonormal mean-free time series; singular values 1, 1/2, 1/4, ..; a
constant offset of 3 and normal noise of 1e-6.  The eigenvalues of the
covariance are then close to 4^-j / (S-1): the leading gaps are wide.
"""
import numpy as np

from stsphere.models.geometry import CubedSphereGrid


def snapshots(N, S, r, seed=0):
    """(x [S, 6, N, N] float64, areas [6, N, N]); r <= S - 1."""
    grid = CubedSphereGrid(N)
    area = grid.areas()
    a = (area / area.sum()).reshape(-1)
    c = grid.centers().reshape(-1, 3)
    deg = 1
    while (deg + 1) ** 2 - 1 < r:
        deg += 1
    cols = [c[:, 0] ** i * c[:, 1] ** j * c[:, 2] ** l
            for d in range(1, deg + 1) for l in (0, 1) for i in range(d - l, -1, -1) for j in [d - l - i]]
    P = np.stack(cols[:r], 1)
    E = np.linalg.qr(np.sqrt(a)[:, None] * P)[0] / np.sqrt(a)[:, None]          # sum_i a_i E_k E_l = delta_kl
    rng = np.random.default_rng(seed)
    Tm = np.linalg.qr(np.concatenate([np.ones((S, 1)), rng.standard_normal((S, r))], 1))[0][:, 1:]
    sig = 0.5 ** np.arange(r)
    x = 3.0 + (Tm * sig) @ E.T + 1e-6 * rng.standard_normal((S, a.size))
    return x.reshape(S, 6, N, N), area
