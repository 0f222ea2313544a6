"""Output products of the solver: derived fields, lat-lon regridding, point
sampling and particles, spherical-harmonic spectra and synthesis, invariants.

``SolverDiagnostics`` is the base class of ``driver.Solver``; it reads the
solver's ``engines``, ``layout``, ``mode``, ``rank``, ``world``, ``fields``,
``physics`` and ``grid``.  Every product goes through the same three steps:

* names      ``_resolve_names``: each name is a prognostic field, a tracer mixing
             ratio, a derived field or a wind, allowed or not for the model;
* sources    ``_source_groups``: per kind present, the partial of every
             engine of this process (``_derived_all()`` at most once);
* combine    ``_gather_tiles`` (tiles to rank 0), ``_gather_partials`` (sum on
             rank 0) or ``_sum_terms`` (sum on every rank), always in ascending
             rank order (``ops.common.add_partials``), so that the one-rank,
             virtual-rank and SPMD results are equal bit for bit.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from .engine import assemble_global
from .models.derived import FIELDS as DERIVED_FIELDS, INVARIANTS
from .models.latlon import fold_terms
from .models.spectra import check_lmax, ke_spectrum as spectra_ke, power as spectra_power
from .models.spectra import (MAX_CHANNELS as spectra_max_channels, band_factors as spectra_band,
                             helmholtz as spectra_helmholtz, scale_degrees as spectra_scale)
from .ops.common import add_partials

# zonal and meridional wind of the lat-lon output (shallow water)
LATLON_WINDS = ("u", "v")


class SolverDiagnostics:
    def __init__(self):
        # optional state: the particle replicas of this process' engines (None: no
        # particles attached), their interval in steps, and the positions a restored
        # checkpoint held (None: it held none)
        self._particles = None
        self._pinterval = 0
        self._restored_particles = None

    # ---- names, sources, rank combine -------------------------------------------------
    def layers(self) -> int:
        """Layers of a layered shallow-water run (``physics.layers``), else 0."""
        return int(self.physics.nl) if getattr(self.physics, "kernel_id", None) == 4 else 0

    def layer_names(self) -> List[str]:
        """The computed names of a layered run: the interface heights ``eta0``
        (= b + h_0 + h_1 + .., the free surface), ``eta1`` (= b + h_1 + ..), ..
        and per layer ``vorticity0``, ``divergence0``, ``pv0``, ``vorticity1``, .."""
        L = self.layers()
        return [f"eta{k}" for k in range(L)] + [f"{d}{k}" for k in range(L) for d in DERIVED_FIELDS]

    def _layer_tiles_all(self) -> List[torch.Tensor]:
        """[len(layer_names()), T, n, n] of every engine of this process.  The
        derived fields of layer k go through the existing derived path on the
        layer's rows (``DerivedFields.set_layer``): all engines start, then all
        finish, layer by layer."""
        L = self.layers()
        ds = [e.derived_fields for e in self.engines]
        per = []
        for k in range(L):
            per.append([f.clone() for f, _ in self._derived_all(layer=k)])
        for d in ds:
            d.set_layer(0)
        out = []
        for j, e in enumerate(self.engines):
            qi = e.tiles_view().detach()
            eta, acc = [], e.tens["b"]
            for k in reversed(range(L)):
                acc = acc + qi[4 * k]
                eta.insert(0, acc)
            out.append(torch.stack(eta + [per[k][j][i] for k in range(L) for i in range(len(DERIVED_FIELDS))]))
        return out

    def mix_names(self) -> List[str]:
        """The names computed from the state besides the prognostic ones: ``q0
        ..``, the mixing ratios hq_k / h of a shallow-water run with tracers;
        ``layer_names()`` of a layered run."""
        if self.layers():
            return self.layer_names()
        return [f"q{k}" for k in range(getattr(self.physics, "nq", 0))]

    def _mixing_tiles(self, e) -> torch.Tensor:
        """[NQ, T, n, n] mixing ratios of engine ``e`` (0 where h = 0); of a
        layered run its ``layer_names()`` fields."""
        if self.layers():
            return self._layer_tiles_all()[[id(x) for x in self.engines].index(id(e))]
        qi = e.tiles_view().detach()
        return torch.stack([self.physics.mixing_ratio(qi, k) for k in range(self.physics.nq)])

    def tracer(self, k: int = 0) -> Optional[np.ndarray]:
        """[6, N, N] mixing ratio q_k = hq_k / h of tracer ``k`` on rank 0 (None
        elsewhere), like ``global_field``."""
        nq = getattr(self.physics, "nq", 0)
        if not 0 <= int(k) < nq:
            raise ValueError(f"tracer({k}): this run carries {nq} tracer(s) (physics.tracers)")
        return self._gather_tiles({e.rank: self._mixing_tiles(e)[int(k)].cpu().double().numpy()
                                   for e in self.engines})

    def tracer_extrema(self) -> Dict[str, List[float]]:
        """{"tracer_min": [NQ], "tracer_max": [NQ]} of the mixing ratios over the
        sphere, on every rank."""
        nq = getattr(self.physics, "nq", 0)
        lo, hi = {}, {}
        for e in self.engines:
            q = self._mixing_tiles(e).reshape(nq, -1)
            for k in range(nq):
                a, b = float(q[k].min()), float(q[k].max())
                lo[f"{k}"] = min(lo.get(f"{k}", a), a)
                hi[f"{k}"] = max(hi.get(f"{k}", b), b)
        lo, hi = self._allreduce(lo, op="min"), self._allreduce(hi, op="max")
        return {"tracer_min": [lo[f"{k}"] for k in range(nq)], "tracer_max": [hi[f"{k}"] for k in range(nq)]}

    def _resolve_names(self, names, what: str, winds: bool = True) -> List[Tuple[str, int]]:
        """[(kind, index)] of ``names``: ``prog`` (index into ``self.fields``),
        ``mix`` (mixing ratio q_k of a tracer run), ``der`` (into the derived
        fields) or ``wind`` (u, v).  ``what`` names the product in the message
        for an unknown name; ``winds`` false: the product is a scalar spectrum,
        which has no winds."""
        out = []
        mix = self.mix_names()
        for name in names:
            if name in mix:
                out.append(("mix", mix.index(name)))
                continue
            if name in LATLON_WINDS and not winds:
                raise ValueError(f"{name!r} is a vector component, not a scalar on the sphere: it has no "
                                 f"spherical-harmonic spectrum; use ke_spectrum for the winds")
            if name in DERIVED_FIELDS or name in LATLON_WINDS:
                if self.layers():
                    raise ValueError(f"{name!r} on a layered run: derived fields are per layer "
                                     f"({name if name in DERIVED_FIELDS else 'vorticity'}0, ..); choose from "
                                     f"{self.fields + self.layer_names()}")
                if self.physics.name != "swe":
                    kind = "derived fields" if name in DERIVED_FIELDS else "winds"
                    raise ValueError(f"{kind} are defined for the shallow-water model, not {self.physics.name!r}")
            elif name not in self.fields:
                choices = self.latlon_names() if winds else self.spectrum_names()
                raise ValueError(f"unknown {what} field {name!r}; choose from {choices}")
            out.append(("prog", self.fields.index(name)) if name in self.fields else
                       ("der", DERIVED_FIELDS.index(name)) if name in DERIVED_FIELDS else
                       ("wind", LATLON_WINDS.index(name)))
        return out

    def _source_groups(self, resolved, make, der=None) -> Dict[str, list]:
        """{kind: [make(kind, j, x) of engine j]} for every kind in ``resolved``
        (prog, mix, der, wind, in that order); x: the engine's derived fields [3,
        T, n, n] for ``der``, its mixing ratios [NQ, T, n, n] for ``mix``, else None.  ``der``: ``_derived_all()`` when the
        caller has it already; it is computed here at most once."""
        out = {}
        for kind in ("prog", "mix", "der", "wind"):
            if not any(k == kind for k, _ in resolved):
                continue
            if kind == "der" and der is None:
                der = self._derived_all()
            out[kind] = [make(kind, j, der[j][0] if kind == "der" else
                              self._mixing_tiles(e) if kind == "mix" else None)
                         for j, e in enumerate(self.engines)]
        return out

    def _gather_tiles(self, vals: Dict[int, np.ndarray]) -> Optional[np.ndarray]:
        """{rank: [T, n, n] or [C, T, n, n]} of this process' engines as [6, N,
        N] or [C, 6, N, N] on rank 0 (None elsewhere).  Collective under SPMD."""
        if self.mode == "spmd":
            import torch.distributed as dist
            objs = [None] * self.world
            dist.all_gather_object(objs, vals)
            vals = {}
            for o in objs:
                vals.update(o)
            if self.rank != 0:
                return None
        C = next(iter(vals.values())).shape[:-3]
        if not C:
            return assemble_global(self.layout, vals)
        return np.stack([assemble_global(self.layout, {r: v[k] for r, v in vals.items()}) for k in range(C[0])])

    def _gather_partials(self, parts) -> Optional[torch.Tensor]:
        """The ranks' partials added in ascending rank order, on rank 0 (None
        elsewhere): virtual ranks on the device, SPMD ranks on the CPU of rank 0
        after an ``all_gather_object``.  ``parts``: one tensor per engine of
        this process.  Collective under SPMD."""
        if self.mode == "spmd":
            import torch.distributed as dist
            objs = [None] * self.world
            dist.all_gather_object(objs, (self.rank, parts[0].detach().cpu().numpy()))
            if self.rank != 0:
                return None
            parts = [torch.as_tensor(a) for _, a in sorted(objs, key=lambda o: o[0])]
        return add_partials(parts)

    def _sum_terms(self, parts):
        """The ranks' term arrays added, on every rank: virtual ranks on the
        device in ascending rank order, SPMD ranks by an all-reduce (one rank
        owns each term, the others hold 0: exact in any order)."""
        acc = add_partials(parts)
        if self.mode == "spmd":
            import torch.distributed as dist
            acc = acc.contiguous()
            if acc.is_cuda and dist.get_backend() == "gloo":
                host = acc.cpu()
                dist.all_reduce(host)
                acc = host.to(acc.device)
            else:
                dist.all_reduce(acc)
        return acc

    # ---- derived fields (models/derived.py, ops/derived.py) -------------------------
    def _derived_all(self, layer: Optional[int] = None):
        """[(fields [3, T, n, n], inv [8])] of every engine of this process.
        Ranks with remote ghosts exchange first: all engines start, then all
        finish (the virtual cluster's lockstep).  ``layer``: of that layer of a
        layered run (buffers overwritten by the next call)."""
        if self.physics.name != "swe":
            raise ValueError(f"derived fields are defined for the shallow-water model, not {self.physics.name!r}")
        if self.layers() and layer is None:
            raise ValueError(f"derived fields of a layered run are per layer: use {self.layer_names()}")
        ds = [e.derived_fields for e in self.engines]
        if layer is not None:
            for d in ds:
                d.set_layer(layer)
        for d in ds:
            d.start()
        for d in ds:
            d.finish()
        return [d.compute() for d in ds]

    def derived_field(self, name: str) -> Optional[np.ndarray]:
        """[6, N, N] of ``vorticity``, ``divergence`` or ``pv`` on rank 0 (None
        elsewhere), like ``global_field``."""
        if self.layers():
            names = self.layer_names()
            if name not in names:
                raise ValueError(f"unknown derived field {name!r} of a layered run; choose from {names}")
            tiles = self._layer_tiles_all()
            return self._gather_tiles({e.rank: x[names.index(name)].detach().cpu().double().numpy()
                                       for e, x in zip(self.engines, tiles)})
        if name not in DERIVED_FIELDS:
            raise ValueError(f"unknown derived field {name!r}; choose from {list(DERIVED_FIELDS)}")
        k = DERIVED_FIELDS.index(name)
        return self._gather_tiles({e.rank: f[k].detach().cpu().double().numpy()
                                   for e, (f, _) in zip(self.engines, self._derived_all())})

    # ---- Laplacian of a field (models/dissipation.py, ops/dissipation.py) --------------
    def laplacian(self, name: str) -> Optional[np.ndarray]:
        """[6, N, N] float64 of the consistent Laplacian (1 / m^2 times the
        field's unit) of a prognostic field, a mixing ratio, ``vorticity``,
        ``divergence``, ``pv``, ``u`` or ``v`` (the names ``latlon_field``
        takes) on rank 0 (None elsewhere); of the advection and diffusion models,
        their prognostic field (ops/heat.py).  One process."""
        from .models.geometry import lonlat_vectors
        from .models.dissipation import primitives
        from .ops.dissipation import laplacian_all
        if self.mode == "spmd":
            raise ValueError("laplacian: one process per rank (spmd) is not supported")
        if self.physics.name != "swe":
            from .ops import heat
            if name not in self.fields:
                raise ValueError(f"unknown laplacian field {name!r}; choose from {list(self.fields)}")
            Ls = heat.laplacian_all([e.heat_operator() for e in self.engines])
            return self._gather_tiles({e.rank: y.detach().cpu().numpy() for e, y in zip(self.engines, Ls)})
        (kind, k), = self._resolve_names([name], "laplacian")

        def make(kind, j, x):
            e = self.engines[j]
            if kind in ("der", "mix"):
                return x[k][None]
            if kind == "prog":
                return e.tiles_view()[k][None]
            v = primitives(e.tiles_view()[:4])[1:4]
            d = torch.as_tensor(np.moveaxis(lonlat_vectors(e.geo.center)[k], -1, 0), device=v.device)
            return ((v[0] * d[0] + v[1] * d[1]) + v[2] * d[2])[None]
        xs = self._source_groups([(kind, k)], make)[kind]
        s = getattr(self, "_dspec", None) or {"order": 1, "nu": 1.0e5, "depth": None}
        ds = [e.dissipation(s["order"], s["nu"], s["depth"]) for e in self.engines]
        return self._gather_tiles({e.rank: y[0].detach().cpu().numpy()
                                   for e, y in zip(self.engines, laplacian_all(ds, xs))})

    # ---- lat-lon output (models/latlon.py, ops/latlon.py) ---------------------------
    def latlon_names(self) -> List[str]:
        """What ``latlon_field`` / ``zonal_mean`` accept for this model."""
        swe = self.physics.name == "swe" and not self.layers()
        return list(self.fields) + self.mix_names() + (list(DERIVED_FIELDS) + list(LATLON_WINDS) if swe else [])

    def _latlon_arrays(self, names, nlat: int, nlon: int, der=None):
        """(arrays [len(names), nlat, nlon], zonal means [len(names), nlat]
        float64) of the current state on rank 0, None elsewhere: tensors on the
        device (single, virtual) or on the CPU (spmd).  Several ranks gather the
        terms of their own cells, the arrays are added (``_gather_partials``)
        and the finish step runs on the sum: the one-rank result bit for bit.
        ``der``: the engines' derived fields when the caller has them already
        (``_derived_all()``).  Collective under SPMD."""
        resolved = self._resolve_names(names, "lat-lon")
        lls = [e.latlon(nlat=nlat, nlon=nlon) for e in self.engines]
        terms = self.layout.num_ranks > 1

        def make(kind, j, x):
            return (lls[j].partial_fields(terms=terms) if kind == "prog" else
                    lls[j].partial_tiles(x, terms=terms) if kind in ("der", "mix") else
                    lls[j].partial_velocity(terms=terms))
        done = {}
        for kind, parts in self._source_groups(resolved, make, der).items():
            tot = self._gather_partials(parts)
            if tot is not None:
                done[kind] = lls[0].finish(tot.contiguous(), project=kind == "wind")
        if self.rank != 0:
            return None
        return (torch.stack([done[kind][0][k] for kind, k in resolved]),
                torch.stack([done[kind][1][k] for kind, k in resolved]))

    def latlon_field(self, name: str, nlat: int, nlon: int) -> Optional[np.ndarray]:
        """[nlat, nlon] of a prognostic field, ``vorticity``, ``divergence``,
        ``pv``, ``u`` or ``v`` on the cell-centred lat-lon grid, on rank 0 (None
        elsewhere), like ``global_field``."""
        r = self._latlon_arrays([name], nlat, nlon)
        return None if r is None else r[0][0].detach().cpu().double().numpy()

    def zonal_mean(self, name: str, nlat: int, nlon: int) -> Optional[np.ndarray]:
        """[nlat] zonal mean of ``latlon_field(name, nlat, nlon)``."""
        r = self._latlon_arrays([name], nlat, nlon)
        return None if r is None else r[1][0].detach().cpu().numpy()

    def _latlon_frame(self, names, der=None) -> Optional[torch.Tensor]:
        """The ``io.latlon`` arrays of a history frame (rank 0; None elsewhere)."""
        r = self._latlon_arrays(names, *self.cfg.io.latlon, der=der)
        return None if r is None else r[0].detach()

    # ---- point sampling and particles (models/points.py, ops/points.py) ---------------
    def _sample_arrays(self, names, p: np.ndarray, lat: np.ndarray, lon: np.ndarray, der=None) -> torch.Tensor:
        """[len(names), K] float64 of the current state at the unit vectors p
        [K, 3] (lat, lon: the same points, for the winds), on every rank.
        Several ranks sample the terms of their own cells, the arrays are added
        (``_sum_terms``) and folded: the one-rank result bit for bit.
        Collective under SPMD."""
        resolved = self._resolve_names(names, "sample")
        sms = [e.points() for e in self.engines]
        pts = [sm.points(p) for sm in sms]
        terms = self.layout.num_ranks > 1

        def make(kind, j, x):
            return (sms[j].fields(pts[j], terms=terms) if kind == "prog" else
                    sms[j].tiles(pts[j], x, terms=terms) if kind in ("der", "mix") else
                    sms[j].velocity(pts[j], terms=terms))
        done = {kind: fold_terms(self._sum_terms(parts)) if terms else parts[0]
                for kind, parts in self._source_groups(resolved, make, der).items()}
        if "wind" in done:
            v = done["wind"]
            t = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=v.device)
            e = t(np.stack([-np.sin(lon), np.cos(lon), np.zeros_like(lon)]))
            n = t(np.stack([-np.sin(lat) * np.cos(lon), -np.sin(lat) * np.sin(lon), np.cos(lat)]))
            done["wind"] = torch.stack([(v[0] * e[0] + v[1] * e[1]) + v[2] * e[2],
                                        (v[0] * n[0] + v[1] * n[1]) + v[2] * n[2]])
        return torch.stack([done[kind][k] for kind, k in resolved])

    def sample(self, names, lat, lon) -> Optional[np.ndarray]:
        """[len(names), K] float64 of prognostic fields, ``vorticity``,
        ``divergence``, ``pv``, ``u`` or ``v`` (the names ``latlon_field`` takes)
        at the points ``lat`` / ``lon`` [K] (radians), on rank 0 (None
        elsewhere).  Second order, dual-mesh interpolation (models/points.py)."""
        from .models.points import lonlat_points
        names = [names] if isinstance(names, str) else list(names)
        lat = np.asarray(lat, dtype=np.float64).reshape(-1)
        lon = np.asarray(lon, dtype=np.float64).reshape(-1)
        p = lonlat_points(lat, lon)
        if p.shape[0] < 1 or not np.isfinite(p).all():
            raise ValueError("sample: lat and lon must be finite and hold at least one point")
        r = self._sample_arrays(names, p, lat, lon)
        return r.detach().cpu().numpy() if self.rank == 0 else None

    def add_particles(self, lat, lon, interval: int = 1) -> None:
        """Attach passive particles seeded at ``lat`` / ``lon`` [K] (radians),
        advanced every ``interval`` steps by Heun's scheme in the tangent plane
        (models/points.py).  Positions are replicated: every rank advances the
        same particles from the summed velocity terms."""
        if self.physics.name != "swe":
            raise ValueError(f"particles are carried by the shallow-water model, not {self.physics.name!r}")
        if self.layers():
            raise ValueError("particles on a layered run are not supported: they follow the winds of one "
                             "shallow-water layer")
        self._particles = [e.particles(lat, lon, interval) for e in self.engines]
        self._pinterval = int(interval)
        self._particles_stage(1)

    def _init_particles(self, spec) -> None:
        """Particles of the config block ``io.particles``."""
        from .models.points import points_lonlat, random_points
        if not isinstance(spec, dict) or not (("count" in spec) ^ ("lat" in spec and "lon" in spec)):
            raise ValueError(f"io.particles: {{count, seed}} or {{lat, lon}} expected, not {spec!r}")
        unknown = set(spec) - {"count", "seed", "lat", "lon", "interval", "fields"}
        if unknown:
            raise ValueError(f"io.particles: unknown key(s) {sorted(unknown)}")
        if "count" in spec:
            if not isinstance(spec["count"], int) or spec["count"] < 1:
                raise ValueError(f"io.particles: count must be a positive integer, not {spec['count']!r}")
            lat, lon = points_lonlat(random_points(spec["count"], int(spec.get("seed", 0))))
        else:
            lat, lon = np.asarray(spec["lat"], dtype=np.float64), np.asarray(spec["lon"], dtype=np.float64)
        for f in spec.get("fields") or []:
            if f not in self.latlon_names():
                raise ValueError(f"io.particles: unknown field {f!r}; choose from {self.latlon_names()}")
        self.add_particles(lat, lon, int(spec.get("interval", 1)))
        self._restore_particles()

    def _restore_particles(self) -> None:
        """Positions of the checkpoint just restored, when it holds them for
        as many particles as are attached."""
        x, ps = self._restored_particles, self._particles
        if x is None or not ps or x.shape != (ps[0].K, 3):
            return
        for P in ps:
            P.set_positions(x)
        self._particles_stage(1)

    def _particles_stage(self, stage: int) -> None:
        """Corrector (0) or predictor (1) of every replica: sample, add, apply."""
        ps = self._particles
        terms = self.layout.num_ranks > 1
        parts = [P.sample(stage, terms=terms) for P in ps]
        tot = self._sum_terms(parts) if terms else parts[0]
        for P in ps:
            P.apply(stage, tot)

    def _particles_advance(self) -> None:
        if self.layout.num_ranks == 1:
            self._particles[0].advance()         # one fused launch
        else:
            self._particles_stage(0)
            self._particles_stage(1)

    def particle_positions(self):
        """(lat, lon) [K] numpy, radians (NaN: a lost particle)."""
        if not self._particles:
            raise ValueError("no particles attached (add_particles)")
        return self._particles[0].lonlat()

    def _particles_frame(self, names, der=None) -> torch.Tensor:
        """The particle positions [K, 3] of a history frame, flattened and
        followed by the fields ``names`` sampled there ([len(names), K]), on
        every rank.  Collective under SPMD when fields are sampled."""
        from .models.points import points_lonlat
        x = self._particles[0].st.x.detach()
        if not names:
            return x
        lat = lon = None
        if any(f in LATLON_WINDS for f in names):
            lat, lon = points_lonlat(x.cpu().numpy())
        return torch.cat([x.reshape(-1), self._sample_arrays(names, x, lat, lon, der=der).to(x.device).reshape(-1)])

    def _particles_rows(self, h: torch.Tensor) -> np.ndarray:
        """The host copy of ``_particles_frame`` as the rows of a particle frame:
        lat, lon, then the sampled fields, [2 + len(names), K]."""
        from .models.points import points_lonlat
        K = self._particles[0].K
        a = h.numpy().reshape(-1)
        la, lo = points_lonlat(a[:3 * K].reshape(K, 3))
        return np.concatenate([la[None], lo[None], a[3 * K:].reshape(-1, K)])

    # ---- spectra (models/spectra.py, ops/spectra.py) --------------------------------
    def spectrum_names(self) -> List[str]:
        """What ``sh_coefficients`` / ``spectrum`` accept for this model."""
        swe = self.physics.name == "swe" and not self.layers()
        return list(self.fields) + self.mix_names() + (list(DERIVED_FIELDS) if swe else [])

    def _spectra_coeffs(self, names, lmax: int, der=None):
        """Coefficients [len(names), 2, L+1, L+1] float64 of the current state
        on rank 0, None elsewhere: a tensor on the device (single, virtual) or
        on the CPU (spmd).  Every rank analyses its own cells and the ranks'
        arrays are added (``_gather_partials``).  ``der``: the engines' derived
        fields when the caller has them already (``_derived_all()``).
        Collective under SPMD."""
        resolved = self._resolve_names(names, "spectrum", winds=False)
        sps = [e.spectra(lmax) for e in self.engines]

        def make(kind, j, x):
            return sps[j].partial_fields() if kind == "prog" else sps[j].partial_tiles(x)
        done = {kind: self._gather_partials(parts)
                for kind, parts in self._source_groups(resolved, make, der).items()}
        if self.rank != 0:
            return None
        return torch.stack([done[kind][k] for kind, k in resolved])

    def sh_coefficients(self, name: str, lmax: int) -> Optional[np.ndarray]:
        """[2, L+1, L+1] real spherical-harmonic coefficients (cos, sin; [l, m])
        of a prognostic field, ``vorticity``, ``divergence`` or ``pv`` on rank 0
        (None elsewhere)."""
        r = self._spectra_coeffs([name], lmax)
        return None if r is None else r[0].detach().cpu().numpy()

    def spectrum(self, name: str, lmax: int) -> Optional[np.ndarray]:
        """[L+1] power per degree of ``sh_coefficients(name, lmax)``."""
        r = self._spectra_coeffs([name], lmax)
        return None if r is None else spectra_power(r)[0].detach().cpu().numpy()

    def _ke_spectrum(self, lmax: int, der=None):
        if self.physics.name != "swe" or self.layers():
            raise ValueError(f"the kinetic-energy spectrum is defined for the one-layer shallow-water model, "
                             f"not {'a layered run' if self.layers() else repr(self.physics.name)}")
        r = self._spectra_coeffs(["vorticity", "divergence"], lmax, der=der)
        return None if r is None else spectra_ke(r[0], r[1], self.grid.radius)

    def ke_spectrum(self, lmax: int) -> Optional[np.ndarray]:
        """[L+1] kinetic energy per degree (m^2 / s^2) from the vorticity and
        the divergence, on rank 0 (None elsewhere)."""
        r = self._ke_spectrum(lmax)
        return None if r is None else r.detach().cpu().numpy()

    def _spectra_frame(self, names, der=None) -> Optional[torch.Tensor]:
        """The ``io.spectra`` power per degree of a history frame, [len(names)
        (+ 1: the kinetic energy, shallow water), L+1] (rank 0; None elsewhere)."""
        L = self.cfg.io.spectra
        swe = self.physics.name == "swe" and not self.layers()
        if der is None and (swe or any(f in DERIVED_FIELDS for f in names)):
            der = self._derived_all()
        r = self._spectra_coeffs(names, L, der=der)
        ke = self._ke_spectrum(L, der=der) if swe else None
        if r is None:
            return None
        v = spectra_power(r)
        return (v if ke is None else torch.cat([v, ke[None]])).detach()

    # ---- synthesis: filters, psi and chi (models/spectra.py, ops/spectra.py) ---------------
    def _synthesise(self, coeffs, lmax: int) -> Optional[np.ndarray]:
        """[C, 6, N, N] float64 on rank 0 (None elsewhere) of the coefficients
        [C, 2, L+1, L+1] that rank 0 holds (a tensor; ignored elsewhere).  Under
        SPMD they are broadcast from rank 0; every rank synthesises its own
        cells and the tiles are gathered as ``derived_field`` gathers them.
        Collective under SPMD."""
        sps = [e.spectra(lmax) for e in self.engines]
        if self.mode == "spmd":
            import torch.distributed as dist
            box = [coeffs.detach().cpu().numpy() if self.rank == 0 else None]
            dist.broadcast_object_list(box, src=0)
            coeffs = torch.as_tensor(box[0])
        C = coeffs.shape[0]
        vals = {}
        for e, sp in zip(self.engines, sps):
            # at most 8 channels per launch
            parts = [sp.synthesise(coeffs[k:k + spectra_max_channels].contiguous())
                     for k in range(0, C, spectra_max_channels)]
            vals[e.rank] = torch.cat(parts).detach().cpu().numpy()
        return self._gather_tiles(vals)

    def synthesise(self, coeffs) -> Optional[np.ndarray]:
        """The band-limited field of given real spherical-harmonic coefficients
        on the solver's own cells: [6, N, N] for ``coeffs`` [2, L+1, L+1] (cos,
        sin; [l, m]), [C, 6, N, N] for [C, 2, L+1, L+1]; float64, on rank 0
        (None elsewhere).  Every rank passes the same array.  Entries with
        m > l and S_l0 are not read."""
        co = torch.as_tensor(np.asarray(coeffs, dtype=np.float64))
        one = co.dim() == 3
        if one:
            co = co[None]
        if co.dim() != 4 or co.shape[0] < 1 or co.shape[1] != 2 or co.shape[2] != co.shape[3]:
            raise ValueError(f"synthesise: coefficients [2, L+1, L+1] or [C, 2, L+1, L+1] expected, "
                             f"not {tuple(np.shape(coeffs))}")
        lmax = check_lmax(int(co.shape[2]) - 1, self.layout.N)
        r = self._synthesise(co.to(self.engines[0].device), lmax)
        return None if r is None else (r[0] if one else r)

    def filtered_field(self, name: str, lmax: int, factors) -> Optional[np.ndarray]:
        """[6, N, N] float64 on rank 0 (None elsewhere): the field ``name``
        (anything in ``spectrum_names()``) analysed to degree ``lmax``, its
        coefficients of degree l multiplied by ``factors[l]`` ([L+1]; see
        ``band_factors`` / ``exp_factors`` in models/spectra.py) and synthesised
        on the solver's cells."""
        f = torch.as_tensor(np.asarray(factors, dtype=np.float64))
        lmax = check_lmax(lmax, self.layout.N)
        if f.shape != (lmax + 1,):
            raise ValueError(f"filtered_field: factors [{lmax + 1}] expected, not {tuple(f.shape)}")
        r = self._spectra_coeffs([name], lmax)
        co = None if r is None else spectra_scale(r, f.to(r.device))
        r = self._synthesise(co, lmax)
        return None if r is None else r[0]

    def band_field(self, name: str, lmax: int, lmin: int = 0, lcut: Optional[int] = None) -> Optional[np.ndarray]:
        """``filtered_field`` with the degrees ``lmin .. lcut`` (default: up to
        ``lmax``) kept and the others dropped: a low-, high- or band-pass view."""
        lmax = check_lmax(lmax, self.layout.N)
        return self.filtered_field(name, lmax, spectra_band(lmax, lmin, lcut))

    def _psi_chi(self, lmax: int, which: int, what: str) -> Optional[np.ndarray]:
        if self.physics.name != "swe":
            raise ValueError(f"the {what} is defined for the shallow-water model, "
                             f"not {self.physics.name!r}")
        r = self._spectra_coeffs(["vorticity", "divergence"], lmax)
        co = None if r is None else spectra_helmholtz(r[0], r[1], self.grid.radius)[which][None]
        r = self._synthesise(co, check_lmax(lmax, self.layout.N))
        return None if r is None else r[0]

    def streamfunction(self, lmax: int) -> Optional[np.ndarray]:
        """[6, N, N] streamfunction psi (m^2 / s), psi_lm = -R^2 zeta_lm / (l (l+1))
        to degree ``lmax`` (v = k x grad psi + grad chi), on rank 0 (None
        elsewhere)."""
        return self._psi_chi(lmax, 0, "streamfunction")

    def velocity_potential(self, lmax: int) -> Optional[np.ndarray]:
        """[6, N, N] velocity potential chi (m^2 / s) from the divergence, like
        ``streamfunction``."""
        return self._psi_chi(lmax, 1, "velocity potential")

    def invariants(self) -> Dict[str, float]:
        """mass, energy, potential_enstrophy, circulation, abs_circulation
        (sums over the sphere) and max_courant (maximum) of the current state."""
        if self.layers():
            raise ValueError("invariants() is defined for one shallow-water layer; a layered run reports mass0, "
                             "mass1, .. and energy through diagnostics()")
        sums: Dict[str, float] = {}
        cmax = 0.0
        for _, inv in self._derived_all():
            for k, v in zip(INVARIANTS, inv.tolist()):
                if k == "max_courant":
                    cmax = max(cmax, v)
                else:
                    sums[k] = sums[k] + v if k in sums else v
        out = self._allreduce(sums)
        out.update(self._allreduce({"max_courant": cmax}, op="max"))
        return {k: out[k] for k in INVARIANTS}
