"""Initial conditions / physics setups (PDF s.6 "Initial Conditions: Physics").

All functions take unit position vectors ``p[..., 3]`` and return NumPy float64
arrays; winds are returned as **Cartesian** (x, y, z) vectors, the panel-
invariant representation the reference exchanges across cube edges (PDF s.18
"Cartesian Velocity Exchange").

* ``cosine_bell``       Williamson et al. (1992) test case 1 (PDF s.13 / s.18:
                        bell at 270 E, 0 N, peak ~1000).
* ``solid_body_wind``   TC1/TC2 wind, rotation angle alpha.
* ``williamson_tc2``    steady geostrophic flow (analytic solution = IC).
* ``williamson_tc5``    zonal flow over an isolated mountain.
* ``williamson_tc6``    Rossby-Haurwitz wave, wavenumber 4.
* ``galewsky``          barotropically unstable jet (Galewsky, Scott & Polvani
                        2004), balanced depth by quadrature, with or without
                        the perturbation.
* ``tracer_field``      mixing ratios in [0, 1] for the shallow-water tracers:
                        ``constant``, ``cosine_bell``, ``cap``, ``gradient``.
* ``layered_fields``    two-layer (stacked shallow water) states: ``tc2``, ``rest``,
                        ``tc5``, ``layered_jet``, ``layered_jet_balanced``.
* ``deform_wind``       time-dependent deformational flows (Nair & Lauritzen 2010,
                        Lauritzen et al. 2012) with ``deform_streamfunction`` and the
                        cases of ``deform_tracer``: ``cosine_bells``,
                        ``gaussian_hills``, ``slotted_cylinders``.
* ``lima_flag``         checkerboard heat source on the top panel (face 0) on a
                        1 K background (PDF s.12 / s.17, log scale 1..1000 K).
"""
from __future__ import annotations

import math

import numpy as np

from .geometry import DAY, EARTH_RADIUS, GRAVITY, OMEGA, lonlat_vectors, xyz_to_lonlat


def great_circle_distance(lon1, lat1, lon2, lat2, radius=EARTH_RADIUS):
    c = np.sin(lat1) * np.sin(lat2) + np.cos(lat1) * np.cos(lat2) * np.cos(lon1 - lon2)
    return radius * np.arccos(np.clip(c, -1.0, 1.0))


def solid_body_wind(p, u0=None, alpha=0.0, radius=EARTH_RADIUS):
    """Williamson TC1/TC2 wind: u = u0 (cos phi cos a + sin phi cos lam sin a),
    v = -u0 sin lam sin a.  Returned as Cartesian vectors."""
    if u0 is None:
        u0 = 2.0 * math.pi * radius / (12.0 * DAY)
    lon, lat = xyz_to_lonlat(p)
    u = u0 * (np.cos(lat) * math.cos(alpha) + np.sin(lat) * np.cos(lon) * math.sin(alpha))
    v = -u0 * np.sin(lon) * math.sin(alpha)
    e, n = lonlat_vectors(p)
    return u[..., None] * e + v[..., None] * n


def rotated_center(lon_c, lat_c, t, alpha, u0, radius=EARTH_RADIUS):
    """Position of the TC1 bell centre after time t (solid-body rotation
    about the axis tilted by alpha)."""
    w = u0 / radius
    # rotation axis: Omega_vec such that v = w x r reproduces solid_body_wind
    axis = np.array([-math.sin(alpha), 0.0, math.cos(alpha)])
    c0 = np.array([math.cos(lat_c) * math.cos(lon_c), math.cos(lat_c) * math.sin(lon_c), math.sin(lat_c)])
    th = w * t
    # Rodrigues
    c = (c0 * math.cos(th) + np.cross(axis, c0) * math.sin(th) + axis * np.dot(axis, c0) * (1 - math.cos(th)))
    return c


def cosine_bell(p, h0=1000.0, lon_c=1.5 * math.pi, lat_c=0.0, r0=None, radius=EARTH_RADIUS, center_xyz=None):
    if r0 is None:
        r0 = radius / 3.0
    lon, lat = xyz_to_lonlat(p)
    if center_xyz is not None:
        cc = np.asarray(center_xyz)
        lat_c = math.asin(max(-1.0, min(1.0, cc[2])))
        lon_c = math.atan2(cc[1], cc[0]) % (2 * math.pi)
    r = great_circle_distance(lon, lat, lon_c, lat_c, radius)
    return np.where(r < r0, 0.5 * h0 * (1.0 + np.cos(math.pi * r / r0)), 0.0)


def cosine_bell_exact(p, t, alpha=0.0, h0=1000.0, radius=EARTH_RADIUS, u0=None):
    if u0 is None:
        u0 = 2.0 * math.pi * radius / (12.0 * DAY)
    c = rotated_center(1.5 * math.pi, 0.0, t, alpha, u0, radius)
    return cosine_bell(p, h0=h0, radius=radius, center_xyz=c)


def williamson_tc2(p, alpha=0.0, gh0=2.94e4, radius=EARTH_RADIUS, omega=OMEGA, g=GRAVITY):
    """Returns (h, wind, b).  Steady state: h(t) = h(0)."""
    u0 = 2.0 * math.pi * radius / (12.0 * DAY)
    lon, lat = xyz_to_lonlat(p)
    s = -np.cos(lon) * np.cos(lat) * math.sin(alpha) + np.sin(lat) * math.cos(alpha)
    gh = gh0 - (radius * omega * u0 + 0.5 * u0 * u0) * s * s
    wind = solid_body_wind(p, u0, alpha, radius)
    return gh / g, wind, np.zeros_like(gh)


def tc5_mountain(p, hs0=2000.0, lon_c=1.5 * math.pi, lat_c=math.pi / 6.0, Rm=math.pi / 9.0):
    lon, lat = xyz_to_lonlat(p)
    dl = np.mod(lon - lon_c + math.pi, 2 * math.pi) - math.pi
    r = np.minimum(Rm, np.sqrt(dl * dl + (lat - lat_c) ** 2))
    return hs0 * (1.0 - r / Rm)


def williamson_tc5(p, h0=5960.0, u0=20.0, radius=EARTH_RADIUS, omega=OMEGA, g=GRAVITY):
    """Zonal flow over an isolated mountain.  Returns (h = fluid depth, wind, b)."""
    lon, lat = xyz_to_lonlat(p)
    b = tc5_mountain(p)
    htot = h0 - (radius * omega * u0 + 0.5 * u0 * u0) * np.sin(lat) ** 2 / g
    wind = solid_body_wind(p, u0, 0.0, radius)
    return htot - b, wind, b


def williamson_tc6(p, radius=EARTH_RADIUS, omega=OMEGA, g=GRAVITY, w=7.848e-6, K=7.848e-6, R=4, h0=8000.0):
    """Rossby-Haurwitz wave (Williamson TC6).  Returns (h, wind, b)."""
    lon, lat = xyz_to_lonlat(p)
    c, s = np.cos(lat), np.sin(lat)
    u = radius * w * c + radius * K * c ** (R - 1) * (R * s * s - c * c) * np.cos(R * lon)
    v = -radius * K * R * c ** (R - 1) * s * np.sin(R * lon)
    A = 0.5 * w * (2 * omega + w) * c ** 2 + 0.25 * K ** 2 * c ** (2 * R) * (
        (R + 1) * c ** 2 + (2 * R * R - R - 2) - 2 * R * R * c ** (-2.0))
    B = 2 * (omega + w) * K / ((R + 1) * (R + 2)) * c ** R * ((R * R + 2 * R + 2) - (R + 1) ** 2 * c ** 2)
    C = 0.25 * K ** 2 * c ** (2 * R) * ((R + 1) * c ** 2 - (R + 2))
    gh = g * h0 + radius ** 2 * (A + B * np.cos(R * lon) + C * np.cos(2 * R * lon))
    e, n = lonlat_vectors(p)
    wind = u[..., None] * e + v[..., None] * n
    return gh / g, wind, np.zeros_like(gh)


# ---- Galewsky, Scott & Polvani (2004): the barotropically unstable jet ---------------------
GALEWSKY_PHI0 = math.pi / 7.0
GALEWSKY_PHI1 = 0.5 * math.pi - GALEWSKY_PHI0
GALEWSKY_UMAX = 80.0
GALEWSKY_MEAN_DEPTH = 10000.0
GALEWSKY_PANELS = 64          # quadrature panels across the jet
GALEWSKY_NODES = 16           # Gauss-Legendre nodes per panel


def galewsky_wind(lat):
    """u(phi) = (80 / e_n) exp[1 / ((phi - phi0)(phi - phi1))] inside the jet
    phi0 < phi < phi1, 0 elsewhere; e_n = exp[-4 / (phi1 - phi0)^2]."""
    lat = np.asarray(lat, dtype=np.float64)
    p0, p1 = GALEWSKY_PHI0, GALEWSKY_PHI1
    inside = (lat > p0) & (lat < p1)
    x = np.where(inside, (lat - p0) * (lat - p1), -1.0)
    en = math.exp(-4.0 / (p1 - p0) ** 2)
    return np.where(inside, GALEWSKY_UMAX / en * np.exp(1.0 / x), 0.0)


def _galewsky_integrand(lat, radius, omega, scale=1.0):
    u = galewsky_wind(lat) if scale == 1.0 else scale * galewsky_wind(lat)
    return radius * u * (2.0 * omega * np.sin(lat) + u * np.tan(lat) / radius)


def _gauss_on(a, b, fn, nodes):
    """Gauss-Legendre quadrature of fn over [a, b] (arrays of equal shape)."""
    x, w = np.polynomial.legendre.leggauss(nodes)
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    half, mid = 0.5 * (b - a), 0.5 * (b + a)
    return half * (fn(mid[..., None] + half[..., None] * x) * w).sum(-1)


def galewsky_depth(lat, radius=EARTH_RADIUS, omega=OMEGA, g=GRAVITY, nodes=GALEWSKY_NODES, scale=1.0):
    """Balanced depth h(phi) of the jet (m), of ``scale`` times its wind:
    g h(phi) = g h0 - int_{-pi/2}^{phi} a u (f + u tan(phi') / a) dphi'
    by composite Gauss-Legendre quadrature on the host (``GALEWSKY_PANELS``
    fixed panels across the jet with ``nodes`` nodes each, and a last partial
    panel up to phi); h0 makes the analytic global mean depth 10 000 m."""
    lat = np.asarray(lat, dtype=np.float64)
    p0, p1, K = GALEWSKY_PHI0, GALEWSKY_PHI1, GALEWSKY_PANELS
    fn = lambda x: _galewsky_integrand(x, radius, omega, scale)
    edges = np.linspace(p0, p1, K + 1)
    cum = np.concatenate([[0.0], np.cumsum(_gauss_on(edges[:-1], edges[1:], fn, nodes))])
    x = np.clip(lat, p0, p1)
    k = np.minimum(((x - p0) / (p1 - p0) * K).astype(np.int64), K - 1)
    I = cum[k] + _gauss_on(edges[k], x, fn, nodes)
    # mean of I over the sphere = 1/2 int I cos = 1/2 (I(phi1) - int_jet I' sin) by parts
    mean_I = 0.5 * (cum[-1] - _gauss_on(edges[:-1], edges[1:], lambda y: fn(y) * np.sin(y), nodes).sum())
    return GALEWSKY_MEAN_DEPTH + (mean_I - I) / g


def galewsky_perturbation(lon, lat):
    """120 cos(phi) exp[-(lambda / (1/3))^2] exp[-((pi/4 - phi) / (1/15))^2] m,
    lambda in (-pi, pi]."""
    lam = np.mod(np.asarray(lon, dtype=np.float64) + math.pi, 2.0 * math.pi) - math.pi
    lat = np.asarray(lat, dtype=np.float64)
    return 120.0 * np.cos(lat) * np.exp(-(lam * 3.0) ** 2) * np.exp(-((0.25 * math.pi - lat) * 15.0) ** 2)


def galewsky(p, perturbed=True, radius=EARTH_RADIUS, omega=OMEGA, g=GRAVITY):
    """The barotropically unstable jet of Galewsky, Scott & Polvani (2004):
    the balanced zonal jet, with the depth perturbation that triggers the
    instability (``perturbed``).  Returns (h, wind, b = 0)."""
    lon, lat = xyz_to_lonlat(p)
    h = galewsky_depth(lat, radius, omega, g)
    if perturbed:
        h = h + galewsky_perturbation(lon, lat)
    e, _ = lonlat_vectors(p)
    return h, galewsky_wind(lat)[..., None] * e, np.zeros_like(h)


def lima_flag(N: int, squares: int = 8, hot: float = 1000.0, background: float = 1.0) -> np.ndarray:
    """[6, N, N] temperature: checkerboard of `hot` squares on face 0."""
    T = np.full((6, N, N), background, dtype=np.float64)
    k = max(1, N // squares)
    j, i = np.mgrid[0:N, 0:N]
    T[0] = np.where(((i // k) + (j // k)) % 2 == 0, hot, background)
    return T


def gaussian_hill(p, center=(1.0, 0.0, 0.0), width=0.3, amp=1.0):
    c = np.asarray(center, dtype=np.float64)
    c = c / np.linalg.norm(c)
    d2 = np.sum((p - c) ** 2, axis=-1)
    return amp * np.exp(-d2 / (width * width))


# ---- spherical harmonics with a closed-form heat solution (models/diffusion.py) -----
# name: (degree l, Y(p) at unit positions p[..., 3], an unnormalised harmonic of that degree)
HARMONICS = {
    "harmonic": (4, lambda p: 35.0 * p[..., 2] ** 4 - 30.0 * p[..., 2] ** 2 + 3.0),                   # zonal
    "harmonic32": (3, lambda p: p[..., 2] * (p[..., 0] ** 2 - p[..., 1] ** 2)),                       # l = 3, m = 2
}


def harmonic_decay(name, p, t, kappa, radius=EARTH_RADIUS):
    """The solution of dT/dt = kappa lap T from the harmonic ``name`` at time t:
    Y(p) exp(-l (l + 1) kappa t / R^2)."""
    l, Y = HARMONICS[name]
    return Y(np.asarray(p, dtype=np.float64)) * math.exp(-l * (l + 1) * kappa * t / (radius * radius))


# ---- shallow-water tracers (models/swe.py::ShallowWaterTracers) ------------------
# centre (lon, lat) and angular radius of the ``cap`` tracer
CAP_CENTER = (0.6, 0.3)
CAP_RADIUS = 0.5
TRACER_FIELDS = ("constant", "cosine_bell", "cap", "gradient")


def tracer_field(name, p, radius=EARTH_RADIUS):
    """Initial mixing ratio q in [0, 1] at unit positions p[..., 3]:

    * ``constant``     q = 1 (stays 1: the tracer flux is the mass flux);
    * ``cosine_bell``  the TC1 bell (270 E, 0 N, radius a/3) scaled to [0, 1];
    * ``cap``          1 inside the spherical cap of angular radius ``CAP_RADIUS``
                       about ``CAP_CENTER``, 0 outside (a discontinuity: the
                       bounds test of the limiters);
    * ``gradient``     (1 + sin lat) / 2.

    A number instead of a name gives q = that number everywhere."""
    if isinstance(name, (int, float)) and not isinstance(name, bool):
        return np.full(p.shape[:-1], float(name))
    if name == "constant":
        return np.ones(p.shape[:-1])
    if name == "cosine_bell":
        return cosine_bell(p, h0=1.0, radius=radius)
    if name == "cap":
        lon_c, lat_c = CAP_CENTER
        c = np.array([math.cos(lat_c) * math.cos(lon_c), math.cos(lat_c) * math.sin(lon_c), math.sin(lat_c)])
        return (p @ c > math.cos(CAP_RADIUS)).astype(np.float64)
    if name == "gradient":
        return 0.5 * (1.0 + p[..., 2])
    raise ValueError(f"unknown tracer initial condition {name!r}; choose from {list(TRACER_FIELDS)}")


# ---- two-layer shallow water (models/swe.py::LayeredShallowWater) -----------------
LAYER_CASES = ("tc2", "rest", "tc5", "layered_jet", "layered_jet_balanced")
LAYER_DEPTHS = {"tc2": (4000.0, 4000.0), "rest": (1000.0, 1000.0), "tc5": (2000.0, 5960.0),
                "layered_jet": (5000.0, 5000.0), "layered_jet_balanced": (5000.0, 5000.0)}
LAYER_WINDS = (0.5, 0.4)       # tc2: layer winds as fractions of TC2's u0
LAYER_JET_SCALE = 0.25         # layered_jet: the Galewsky wind times this, in the top layer


def layered_fields(case, p, depths=None, density_ratio=0.9, winds=None, jet_scale=None, alpha=0.0,
                   radius=EARTH_RADIUS, omega=OMEGA, g=GRAVITY):
    """Two layers (0 on top, r = rho_0 / rho_1 = ``density_ratio`` < 1) with
    resting depths ``depths`` = [H_0, H_1].  Returns (h [2, ...], wind
    [2, ..., 3], b).  The top layer's pressure is g (b + h_0 + h_1), the bottom
    layer's g (b + r h_0 + h_1):

    * ``tc2``   exact steady state: layer k in solid-body rotation
      U_k = winds[k] u0 (TC2's u0 and ``alpha``).  With A_k = R Omega U_k +
      U_k^2 / 2 and TC2's s:  h_0 + h_1 = H_0 + H_1 - A_0 s^2 / g  and
      r h_0 + h_1 = r H_0 + H_1 - A_1 s^2 / g,  so
      h_0 = H_0 - (A_0 - A_1) s^2 / (g (1 - r));
    * ``rest``  uniform layers, no wind;
    * ``tc5``   both layers at TC5's u0 over its mountain: h_0 = H_0 and
      h_1 = H_1 - (R Omega u0 + u0^2 / 2) sin^2(lat) / g - b;
    * ``layered_jet`` / ``layered_jet_balanced``  ``jet_scale`` times the
      Galewsky wind in the top layer, the bottom layer at rest: the free surface
      is H_0 + H_1 + d with d the balanced Galewsky depth of the scaled wind
      minus its mean, the interface makes r h_0 + h_1 constant; ``layered_jet``
      adds the Galewsky bump to h_0.

    Parameters that make a thickness non-positive are refused."""
    if case not in LAYER_CASES:
        raise ValueError(f"unknown layered shallow-water case {case!r}; choose from {list(LAYER_CASES)}")
    depths = LAYER_DEPTHS[case] if depths is None else depths
    if len(depths) != 2 or not all(float(H) > 0 for H in depths):
        raise ValueError(f"layered shallow water: depths = [H_0, H_1], both positive, expected, not {list(depths)!r}")
    H0, H1 = float(depths[0]), float(depths[1])
    r = float(density_ratio)
    if not 0.0 < r < 1.0:
        raise ValueError(f"layered shallow water: density_ratio = rho_0 / rho_1 in (0, 1) expected, not {r!r}")
    lon, lat = xyz_to_lonlat(p)
    zero = np.zeros(p.shape[:-1])
    if case == "rest":
        h = np.stack([zero + H0, zero + H1])
        wind = np.zeros((2,) + p.shape)
        b = zero
    elif case == "tc2":
        winds = LAYER_WINDS if winds is None else winds
        if len(winds) != 2:
            raise ValueError(f"layered shallow water: winds = [w_0, w_1] expected, not {list(winds)!r}")
        u0 = 2.0 * math.pi * radius / (12.0 * DAY)
        U = [float(w) * u0 for w in winds]
        A = [radius * omega * u + 0.5 * u * u for u in U]
        s = -np.cos(lon) * np.cos(lat) * math.sin(alpha) + np.sin(lat) * math.cos(alpha)
        h0 = H0 - (A[0] - A[1]) * s * s / (g * (1.0 - r))
        h1 = H0 + H1 - A[0] * s * s / g - h0
        h = np.stack([h0, h1])
        wind = np.stack([solid_body_wind(p, u, alpha, radius) for u in U])
        b = zero
    elif case == "tc5":
        u0 = 20.0
        b = tc5_mountain(p)
        h1 = H1 - (radius * omega * u0 + 0.5 * u0 * u0) * np.sin(lat) ** 2 / g - b
        h = np.stack([zero + H0, h1])
        w = solid_body_wind(p, u0, 0.0, radius)
        wind = np.stack([w, w])
    else:
        sc = LAYER_JET_SCALE if jet_scale is None else float(jet_scale)
        d = galewsky_depth(lat, radius, omega, g, scale=sc) - GALEWSKY_MEAN_DEPTH
        h0 = H0 + d / (1.0 - r)
        h1 = H1 - r * d / (1.0 - r)
        if case == "layered_jet":
            h0 = h0 + galewsky_perturbation(lon, lat)
        h = np.stack([h0, h1])
        e, _ = lonlat_vectors(p)
        wind = np.stack([(sc * galewsky_wind(lat))[..., None] * e, np.zeros(p.shape)])
        b = zero
    for k in range(2):
        if not h[k].min() > 0:
            raise ValueError(f"layered shallow water, case {case!r}: the thickness of layer {k} is not positive "
                             f"(minimum {h[k].min():.6g} m) with depths {[H0, H1]}, density_ratio {r}; "
                             f"use deeper layers, weaker winds or a smaller density_ratio")
    return h, wind, b


# ----------------------------------------------------------------------------
# Deformational flows (Nair & Lauritzen 2010; Lauritzen et al. 2012): prescribed
# winds that depend on time, reverse at t = T / 2 and return the tracer to its
# initial condition at t = T.
# ----------------------------------------------------------------------------

DEFORM_FLOWS = ("deform_nd", "deform_nd_static", "deform_div")
STREAM_FLOWS = ("deform_nd", "deform_nd_static")
DEFORM_CASES = ("cosine_bells", "gaussian_hills", "slotted_cylinders")
DEFORM_CENTERS = ((5.0 * math.pi / 6.0, 0.0), (7.0 * math.pi / 6.0, 0.0))


def deform_amplitude(flow: str, radius: float, period: float) -> float:
    """k of the flow: 10 R / T for the non-divergent flows, 5 R / T for the divergent one."""
    if flow not in DEFORM_FLOWS:
        raise ValueError(f"unknown deformational flow {flow!r}; choose from {list(DEFORM_FLOWS)}")
    return (5.0 if flow == "deform_div" else 10.0) * radius / period


def deform_rotation(flow: str, radius: float, period: float) -> float:
    """Speed 2 pi R / T of the background rotation (0 for ``deform_nd_static``)."""
    return 0.0 if flow == "deform_nd_static" else 2.0 * math.pi * radius / period


def deform_streamfunction(lon, lat, t: float, flow: str = "deform_nd", radius=EARTH_RADIUS, period=12.0 * DAY):
    """psi (m^2/s) of the non-divergent flows, v = k_hat x grad psi:
    psi = R [k sin^2(lam') cos^2(th) cos(pi t / T) - u_rot sin(th)],
    lam' = lam - 2 pi t / T with the background rotation u_rot = 2 pi R / T
    (``deform_nd``, NL2010 case 4), lam' = lam without (``deform_nd_static``, case 2)."""
    if flow not in STREAM_FLOWS:
        raise ValueError(f"{flow!r} has no streamfunction; choose from {list(STREAM_FLOWS)}")
    k = deform_amplitude(flow, radius, period)
    urot = deform_rotation(flow, radius, period)
    lp = lon - 2.0 * math.pi * t / period if urot else lon
    return radius * (k * np.sin(lp) ** 2 * np.cos(lat) ** 2 * math.cos(math.pi * t / period) - urot * np.sin(lat))


def deform_wind_uv(lon, lat, t: float, flow: str = "deform_nd", radius=EARTH_RADIUS, period=12.0 * DAY):
    """(u, v) zonal / meridional wind (m/s) of a deformational flow at time t."""
    k = deform_amplitude(flow, radius, period)
    urot = deform_rotation(flow, radius, period)
    lp = lon - 2.0 * math.pi * t / period if urot else lon
    c = math.cos(math.pi * t / period)
    if flow == "deform_div":
        u = -k * np.sin(0.5 * lp) ** 2 * np.sin(2.0 * lat) * np.cos(lat) ** 2 * c + urot * np.cos(lat)
        v = 0.5 * k * np.sin(lp) * np.cos(lat) ** 3 * c
    else:
        u = k * np.sin(lp) ** 2 * np.sin(2.0 * lat) * c + urot * np.cos(lat)
        v = k * np.sin(2.0 * lp) * np.cos(lat) * c
    return u, v


def deform_wind(p, t: float, flow: str = "deform_nd", radius=EARTH_RADIUS, period=12.0 * DAY):
    """Cartesian wind of a deformational flow at unit positions p [..., 3]."""
    lon, lat = xyz_to_lonlat(p)
    u, v = deform_wind_uv(lon, lat, t, flow, radius, period)
    e, n = lonlat_vectors(p)
    return u[..., None] * e + v[..., None] * n


def deform_tracer(p, case: str):
    """Initial mixing ratio of the deformational-flow tests at unit positions
    p [..., 3]: two ``cosine_bells`` (background 0.1, peak 1), ``gaussian_hills``
    (peak 0.95) or ``slotted_cylinders`` (0.1 / 1) centred at ``DEFORM_CENTERS``."""
    lon, lat = xyz_to_lonlat(p)
    r = [great_circle_distance(lon, lat, lc, tc, 1.0) for lc, tc in DEFORM_CENTERS]
    if case == "cosine_bells":
        q = np.full(lon.shape, 0.1)
        for ri in r:
            q = np.where(ri < 0.5, 0.1 + 0.9 * 0.5 * (1.0 + np.cos(math.pi * ri / 0.5)), q)
        return q
    if case == "gaussian_hills":
        q = np.zeros(lon.shape)
        for lc, tc in DEFORM_CENTERS:
            x = np.array([math.cos(tc) * math.cos(lc), math.cos(tc) * math.sin(lc), math.sin(tc)])
            q = q + 0.95 * np.exp(-5.0 * np.sum((p - x) ** 2, axis=-1))
        return q
    if case == "slotted_cylinders":
        (l1, t1), (l2, t2) = DEFORM_CENTERS
        d1, d2 = np.abs(lon - l1), np.abs(lon - l2)
        inside = ((r[0] <= 0.5) & (d1 >= 1.0 / 12.0)) | ((r[1] <= 0.5) & (d2 >= 1.0 / 12.0))
        inside |= (r[0] <= 0.5) & (d1 < 1.0 / 12.0) & (lat - t1 < -5.0 / 24.0)
        inside |= (r[1] <= 0.5) & (d2 < 1.0 / 12.0) & (lat - t2 > 5.0 / 24.0)
        return np.where(inside, 1.0, 0.1)
    raise ValueError(f"unknown deformational-flow case {case!r}; choose from {list(DEFORM_CASES)}")
