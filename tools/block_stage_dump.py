"""States of the plain block stage kernels (tracer, two-layer, layer-streaming)
after 3 SSP-RK3 steps, for a bit-for-bit comparison of two builds of the library.

    python tools/block_stage_dump.py --out a.pt        # in one tree
    python tools/block_stage_dump.py --out b.pt        # in the other
    python tools/block_stage_dump.py --compare a.pt b.pt

The library is the one of the tree the script runs in.  Cases: tracers NQ = 1
and 4 (PLR) and NQ = 3 (PPM), two layers, L = 3 and L = 8, each at C24 t = 2 and
C17 t = 1, both block shapes, fp64 and fp32, limiter 2; limiter 0 and 8 virtual
ranks once per kernel.  Starts are the analytic TC5 states, identical in both
trees.  --compare exits 1 unless every tensor is torch.equal.
"""
import argparse
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

STEPS = 3
BLOCKS = [(16, 16), (16, 8)]
SIZES = [(24, 2), (17, 1)]
TRACERS = ["cap", "cosine_bell", "gradient", "constant"]


def kinds():
    from stsphere.models.swe import LayeredShallowWater, ShallowWaterTracers
    def tr(nq, tl):
        return lambda lim: ShallowWaterTracers("tc5", tracers=TRACERS[:nq], limiter=lim, tracer_limiter=tl)
    def ly(nl):
        depths = [2000.0] * (nl - 1) + [5960.0]
        return lambda lim: LayeredShallowWater("tc5", depths=depths, density_ratio=0.9, limiter=lim)
    # name -> (physics factory, ghost layers, first of its kernel)
    return {"tracer_nq1": (tr(1, None), 2, True), "tracer_nq4": (tr(4, None), 2, False), "tracer_nq3_ppm": (tr(3, "ppm"), 3, False),
            "layers2": (ly(2), 2, True), "layers3": (ly(3), 2, True), "layers8": (ly(8), 2, False)}


def dump(path):
    import torch
    from stsphere.engine import Engine, VirtualCluster
    from stsphere.models.geometry import CubedSphereGrid
    from stsphere.parallel.layout import TileLayout
    grids = {N: CubedSphereGrid(N) for N, _ in SIZES}
    out = {}
    for name, (mk, ng, first) in kinds().items():
        cases = [(N, t, b, dt, 2, 1) for N, t in SIZES for b in BLOCKS for dt in (torch.float64, torch.float32)]
        if first:
            cases += [(24, 2, (16, 8), torch.float64, 0, 1), (24, 2, (16, 8), torch.float64, 2, 8)]
        for N, t, block, dtype, lim, ranks in cases:
            key = f"{name} C{N} t{t} {block[0]}x{block[1]} {str(dtype)[6:]} lim{lim} ranks{ranks}"
            kw = dict(grid=grids[N], dtype=dtype, device="cuda", backend="hip", block=block)
            if ranks == 1:
                e = Engine(mk(lim), TileLayout(N, t, 1, ng=ng), **kw)
                e.step(STEPS)
                torch.cuda.synchronize()
                out[key] = e.tiles_view().detach().clone().cpu()
            else:
                vc = VirtualCluster(lambda: mk(lim), TileLayout(N, t, ranks, ng=ng), **kw)
                vc.step(STEPS)
                torch.cuda.synchronize()
                nf = vc.engines[0].tiles_view().shape[0]
                out[key] = torch.stack([torch.as_tensor(vc.global_field(f)).cpu() for f in range(nf)])
            assert torch.isfinite(out[key]).all(), key
            print("dumped", key, tuple(out[key].shape), flush=True)
    torch.save(out, path)


def compare(pa, pb):
    import torch
    a, b = torch.load(pa), torch.load(pb)
    assert set(a) == set(b), sorted(set(a) ^ set(b))
    bad = 0
    for k in a:
        same = a[k].shape == b[k].shape and torch.equal(a[k], b[k])
        if not same:
            bad += 1
            d = (a[k].double() - b[k].double()).abs().max().item() if a[k].shape == b[k].shape else float("nan")
            print(f"DIFFERENT {k}: max abs diff {d:.3e}")
    print(f"{len(a)} cases, {len(a) - bad} bitwise equal, {bad} different")
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--compare", nargs=2)
    a = ap.parse_args()
    if a.compare:
        sys.exit(compare(*a.compare))
    dump(a.out)


if __name__ == "__main__":
    main()
