// Launch side shared by the plain block stage kernels (swe_tracer_stage.hip,
// swe_layer_stage.hip, swe_layers_stream.hip): the argument check and the three
// launch forms.  The maps they share are block_map.h.  Their device code stays
// in each file: moved into shared functions it cost registers and 1 to 4 % of
// their speed (profiles/block_stage).
#pragma once
#include "stage_common.h"
#include "block_map.h"

namespace {

// What every kernel of the family needs of a descriptor; ng: its ghost layers.
// -5 stays the first check: the tracer launcher puts its own -15 (three ghost
// layers for PPM) between -5 and the codes after it
inline int block_args_check(const StageDesc* d, int ng) {
  if (d->pw != d->n + 2 * d->mg || d->mg < ng) return -5;
  if (!d->pedge || !d->pe_base || !d->pe_t || d->n < 2) return -12;   // panel-edge tables
  if (!d->mx || !d->my || !d->cgeo || !d->ex || !d->ey) return -6;
  if (!d->push || (d->remote && (!d->gmap || !d->blocks || !d->recv))) return -6;
  if (d->xg) return -10;                                               // no direct xGMI halo
  return 0;
}

// One launch in the form the descriptor asks for: block list + remote ghosts,
// block list, or every block.  -13: the dynamic LDS is over what a launch gets
template <typename K, typename... A>
int block_launch(const StageDesc* d, K remote, K list, K plain, int nt, size_t lds, hipStream_t s, A... args) {
  if (lds > 65536) return -13;
  const dim3 grid(d->nblocks), block(nt);
  if (d->remote) hipLaunchKernelGGL(remote, grid, block, lds, s, args...);
  else if (d->blocks) hipLaunchKernelGGL(list, grid, block, lds, s, args...);
  else hipLaunchKernelGGL(plain, grid, block, lds, s, args...);
  return (int)hipGetLastError();
}

}  // namespace
