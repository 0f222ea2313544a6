"""Tracers, layers and the output products on SPMD ranks sharing one GPU.

Two processes (``STSP_SHARE_GPU=1``, a gloo group) run the Solver with the
graph-replayed IPC copy transport under the stage kernels of shallow water with
tracers (``swe_tracer_stage.hip``, receive rows of 5 and 6 values, with PPM
mixing ratios three ghost layers) and of two-layer shallow water
(``swe_layer_stage.hip``, rows of 8): the transport chain of ``comm: auto``
(the direct xGMI exchange refuses these physics on every rank alike, the run
lands on ``ipc``), ``bd.recv = ipc.recv_slot(j)`` across processes, restart
from a checkpoint, and the output products on SPMD ranks, where the derived
fields' ghost exchange goes through ``TorchDistTransport`` (staged through the
host under gloo).  ``rank_products.py`` holds the worker and the comparison:
everything is bitwise equal to the one-GPU Solver running the same stage
kernels with the same block, the spectra within 1e-12 of their maximum.

Two ranks only: more processes on one GPU get their hardware queues
time-sliced (docs/ARCHITECTURE.md, "Shared-GPU rehearsals").  Each rank has one
peer at offset 0.  ``tracers_ppm`` sends 405 rows of 40 bytes, the one payload of
the wide-row GPU cases that is no multiple of 16 bytes: the IPC copy kernel
copies it in 4-byte words (runtime.cpp picks 16-byte words only when every
pointer and size allows); the test asserts the payload sizes on the host.
profiles/physics_ranks/README.md records what the cases printed."""
import pytest

from rank_products import assert_equal, reference, spmd_run
from stsphere.parallel.layout import TileLayout

pytestmark = pytest.mark.gpu

BLOCK = [16, 8]
LAYERS = {"depths": [2000.0, 5960.0], "density_ratio": 0.9}
#        id          products   physics keys                                                    t  comm
CASES = {"tracers": ("tracers", {"tracers": ["gradient", "cap"]}, 2, "auto"),
         "tracers_ppm": ("tracers", {"tracers": ["gradient"], "tracer_limiter": "ppm"}, 1, "ipc"),
         "layers": ("layers", {"layers": LAYERS}, 2, "auto"),
         "swe": ("swe", {}, 2, "ipc")}


def _cfg(physics, nd, t, out, comm, fused):
    return {"parallelization": {"tiles_per_edge": t, "num_devices": nd, "device_type": "gpu"},
            "grid": {"N": 24, "halo": 2, "dtype": "float64"},
            "physics": dict({"model": "swe", "case": "tc5", "limiter": "mc"}, **physics),
            "time": {"integrator": "ssprk3", "dt": 150.0},
            "io": {"output_dir": str(out)},
            "runtime": {"comm": comm, "steps_per_graph": 4, "fused": fused, "block": list(BLOCK)}}


@pytest.mark.parametrize("case", list(CASES))
def test_two_processes_one_gpu_state_restart_and_products(case, tmp_path):
    kind, physics, t, comm = CASES[case]
    # the ranks: 6 steps, checkpoint, 4 steps, restore, 4 steps, products; every rank
    # asserts comm == "ipc" (with auto: past the xGMI refusal), no fused step, graph replay
    got = spmd_run(_cfg(physics, 2, t, tmp_path / "ranks", comm, "auto"), kind, 2, tmp_path, n1=6, n2=4,
                   share_gpu=True, expect={"comm": "ipc"})
    state, prods = reference(_cfg(physics, 1, t, tmp_path / "one", comm, "off"), kind, 10)
    print(f"PHYSRANKS {case}: two processes took {got['seconds']:.1f} s (spawn, 14 steps, checkpoint, products)")
    assert state.shape[0] == {"tracers": 6, "tracers_ppm": 5, "layers": 8, "swe": 4}[case]
    assert_equal(got, state, prods, f"{case}, two processes on one GPU")
    # which word size the IPC copy kernel took, by runtime.cpp's rule (one peer, offset 0, fp64)
    plan = TileLayout(24, t, 2, ng=3 if "tracer_limiter" in physics else 2).plan(0)
    assert list(plan.send_offsets) == [0] and list(plan.recv_offsets) == [0]
    assert (plan.send_counts[0] * state.shape[0] * 8 % 16 != 0) == (case == "tracers_ppm")
