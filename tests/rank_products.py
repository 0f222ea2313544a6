"""The Solver on SPMD ranks against one rank: state, restart and output
products (a plain helper module: ``from rank_products import ...``).

``spmd_run`` spawns one process per rank (a gloo group; with ``share_gpu`` all
on one GPU, ``STSP_SHARE_GPU=1``).  Every rank runs ``n1`` steps, saves a
checkpoint, runs ``n2`` steps and gathers the state (``a``), restores the
checkpoint, runs ``n2`` steps again and gathers the state (``b``), then takes
the products of ``PRODUCTS[kind]`` collectively.  Rank 0 saves everything;
``reference`` does the ``n1 + n2`` steps and the products on one rank, and
``assert_equal`` compares: state, lat-lon fields, samples and derived field bit
for bit, the spectra within 1e-12 of their maximum (the bound of
tests/test_spectra.py for the same sum over ranks in another order).
"""
import os
import socket
import time

import numpy as np
import torch.multiprocessing as mp

# per physics: the names that go through latlon_field and sample, the derived field, the spectra
PRODUCTS = {"swe": (["h", "pv", "u"], "pv", ["h", "pv"]),
            "tracers": (["h", "q0", "pv", "u"], "pv", ["q0", "pv"]),
            "layers": (["h1", "eta1", "pv0", "vorticity1"], "pv0", ["eta1", "pv0"])}
NLAT, NLON, LMAX = 6, 12, 4
LAT, LON = np.linspace(-1.2, 1.2, 5), np.linspace(0.1, 6.0, 5)
SPECTRUM_BOUND = 1e-12


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def products(s, kind):
    """{name: array} on rank 0 ({name: None} elsewhere).  Collective."""
    names, der, spec = PRODUCTS[kind]
    out = {f"latlon_{nm}": s.latlon_field(nm, NLAT, NLON) for nm in names}
    out["sample"] = s.sample(names, LAT, LON)
    out[f"derived_{der}"] = s.derived_field(der)
    out.update({f"spectrum_{nm}": s.spectrum(nm, LMAX) for nm in spec})
    return out


def _worker(rank, world, port, cfg, kind, n1, n2, outdir, share_gpu, expect):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    if share_gpu:
        os.environ["STSP_SHARE_GPU"] = "1"
    import torch.distributed as dist
    from stsphere.driver import Solver
    from stsphere.utils import checkpoint as ckpt
    try:
        s = Solver(cfg, verbose=False)
        s.initialize()
        assert s.mode == "spmd" and s.world == world
        s.run(nsteps=n1)
        if expect is not None:      # the device runtime: which transport the chain landed on, and graph replay
            assert s.comm == expect["comm"], s.comm
            assert s.fused is None, s.fused
            assert s.runner.use_graph and s.runner.stats["graph_steps"] > 0, s.runner.stats
        root = s.checkpoint_root()
        s.save_checkpoint()
        s.run(nsteps=n2)
        a = s.gather_global()
        s.restore_checkpoint(ckpt.step_dir(root, n1))
        s.run(nsteps=n2)
        b = s.gather_global()
        out = products(s, kind)
        if expect is not None:
            # the derived fields' ghosts travelled outside the step loop, through the process
            # group: device rows handed to gloo go through pinned host buffers
            tr = s.engines[0].derived_fields.transport()
            assert type(tr).__name__ == "TorchDistTransport" and tr is not s.engines[0].transport
            assert tr.host_staged == (dist.get_backend() == "gloo"), tr.host_staged
        if rank == 0:
            np.savez(os.path.join(outdir, "ranks.npz"), a=a, b=b, **out)
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()


def spmd_run(cfg, kind, world, outdir, n1=3, n2=3, share_gpu=False, expect=None):
    """{name: array} of rank 0: ``a``, ``b`` and the products.  ``cfg``: the
    ranks' config (num_devices = world); its output_dir holds the checkpoint."""
    t0 = time.perf_counter()
    mp.spawn(_worker, args=(world, free_port(), cfg, kind, n1, n2, str(outdir), share_gpu, expect), nprocs=world,
             join=True)
    with np.load(os.path.join(str(outdir), "ranks.npz")) as z:
        got = {k: z[k] for k in z.files}
    got["seconds"] = time.perf_counter() - t0
    return got


def reference(cfg, kind, nsteps):
    """The one-rank Solver of ``cfg`` after ``nsteps`` steps: (state, products)."""
    from stsphere.driver import Solver
    s = Solver(cfg, verbose=False)
    s.initialize()
    assert s.mode == "single"
    s.run(nsteps=nsteps)
    r = s.gather_global(), products(s, kind)
    s.close()
    return r


def assert_equal(got, state, prods, what=""):
    """``got`` (``spmd_run``) against the one-rank state and products."""
    assert np.isfinite(state).all() and got["a"].shape == state.shape

    def rel(x):
        return max(float(np.abs(x[f] - state[f]).max() / np.abs(state[f]).max()) for f in range(state.shape[0]))
    print(f"RANKS {what}: state against one rank {rel(got['a']):.2e}, after the restart {rel(got['b']):.2e} of the "
          f"field maximum; spectra " + " ".join(
              f"{k[9:]} {float(np.abs(got[k] - v).max() / np.abs(v).max()):.2e}" for k, v in prods.items()
              if k.startswith("spectrum_")))
    for f in range(state.shape[0]):
        assert np.array_equal(got["a"][f], state[f]), f"{what}: field {f} of the ranks differs from one rank"
        assert np.array_equal(got["b"][f], state[f]), f"{what}: field {f} differs after the restart"
    for k, v in prods.items():
        assert np.isfinite(v).all(), (what, k)
        if k.startswith("spectrum_"):
            d = float(np.abs(got[k] - v).max())
            assert d <= SPECTRUM_BOUND * float(np.abs(v).max()), (what, k, d)
        else:
            assert got[k].shape == v.shape and np.array_equal(got[k], v), f"{what}: product {k} differs from one rank"
