// Shared declarations of the gfx950 kernels and their C ABI descriptors.
//
// The descriptors are plain C structs mirrored by ctypes (ops/native.py) and
// by the C++ runtime (runtime.cpp).  Pointers are device pointers; scalars are
// carried as double and converted to the kernel's element type at launch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

extern "C" {

// One fused finite-volume RK stage (see stage_kernel.hip).
typedef struct StageDesc {
  const void* X;        // [F][S]  RK combination input, read at own cell (padded layout)
  const void* Q;        // [F][S]  stage input, read with halos (padded layout)
  const void* acc_in;   // [F][S]  RK4 accumulator in (nullable)
  void* out;            // [F][S]
  void* acc_out;        // [F][S]  (nullable)
  const void* recv;     // [R][F]  remote ghost slots (nullable when R == 0)
  const int* gmap;      // [T][4][mg][n]  ghost map (remote slots < 0)
  const int* push;      // [T][4][mg][n]  push map (same-rank ghost slot fed by a strip cell, or -1)
  const int* blocks;    // work list of linear block ids (nullable -> all blocks)
  const void* invA;     // [T][n][n]
  const void* ex;       // [T][n][n+1]  per x-edge coefficient (L, U*L or kappa L/d)
  const void* ey;       // [T][n+1][n]
  const void* mx;       // [T][3][n+1]  x-edge unit normals (SWE)
  const void* my;       // [T][3][n+1]
  const void* cgeo;     // [T][n][n][8] per-cell record (1/A, centre xyz, grad b xyz, 0) (SWE)
  int ntile, n, S, mg, pw;  // pw = n + 2 mg (padded tile width), S = ntile pw^2
  int nblocks;          // number of entries in `blocks` (or total blocks)
  int limiter;
  int remote;           // 1: read remote ghost slots from recv via gmap (boundary blocks)
  double a0, a1, a2, c0, c1, c2, dt;
  double g, omega2;
  void* stamps;         // diagnostic builds only (-DSTSP_STAMPS): [nblocks][16 waves][8] s_memtime per phase
  // ---- direct xGMI halo (xg = 1; see ops/xgmi.py) ----------------------------
  // The producing block stores remote ghost cells straight into the consumer
  // rank's receive ring (IPC-mapped, uncached, STSP_XG_SLOTS slots) as tagged
  // granules: every ghost word travels as an 8-byte {epoch tag, 32-bit payload}
  // atomic store and the consumer re-reads its granules until every tag
  // matches (no counters, no drain; the protocol is xg_ring.h).
  // `recv` is then this rank's ring base; `push` entries < -1 encode
  // -2 - (peer << 24 | slot).
  int xg;
  int ring;             // 8-byte granules per ring slot
  void* const* peer_ring;                  // [world] ring base of rank p (device array)
  const int* bmask;     // [nblocks][2] (peers read, peers fed) bit masks; the kernel reads the first
  int* epoch;           // [nblocks] stages completed
  int* err;             // set to 1 on a poll timeout (all later polls fall through)
  long long timeout_ticks;  // s_memrealtime ticks (100 MHz)
  const int* pedge;     // [T] tile sides on a panel edge (bits W, E, S, N); PLR / PPM physics
  // panel-edge ghost interpolation (models/base.py::panel_edge_tables): for tile
  // side s, ghost layer k < 3, strip cell j: ghost = x[b] + t (x[b+1] - x[b]) over
  // the raw strip x of that layer, b = pe_base[t][s][k][j] (tile-local), t = pe_t[...]
  const int* pe_base;   // [T][4][3][n]
  const void* pe_t;     // [T][4][3][n] element type
  // streaming stage only (march_kernel.hip): panel-shared geometry instead of
  // the per-tile records (cgeo, ex, ey), and the topography itself instead of
  // its gradient (ops/hip_compute.py::march_tables)
  const int* torg;      // [T][3] face, I0, J0 of each tile
  const void* crec;     // [Nf*Nf][8] 1/A, S (3), centre (3), 0 in panel-local components (ops/fused.py::kernel_geometry)
  const void* lxt;      // [Nf][Nf+1] x-edge lengths; the y-edge (J', I) has length lxt[I][J']
  const void* bpad;     // [S] topography in the padded layout, ghost ring filled (null: no topography)
  int Nf;               // cells per panel edge
  int frames[6];        // ops/fused.py::frame_code of each panel
  // carried tile-corner ghosts (parallel/layout.py::corner_sources): the strip
  // cells beyond a tile end that the panel-edge interpolation pairs reach.
  // Corner (quad, a, b): quad = (x side E) | 2 (y side N), a rows and b columns
  // beyond the tile corner.
  const int* cgmap;     // [T][4][mg][mg] RankPlan.corner_map: remote slot -1 - m where < 0, else read as stored
  const int* cpush;     // [T][4][mg][mg] slot fed by the own cell of corner block (quad, a, b): >= 0 same
                        // rank, < -1 remote code (as push), -1 none (nullable)
  int nq;               // shallow water with tracers (phys 3, swe_tracer_stage.hip): tracer fields, 1 .. 4;
                        // the state then holds F = 4 + nq fields (h, M, hq_k) and recv is [R][4 + nq]
  int tracer_limiter;   // phys 3: reconstruction of the mixing ratios, 0 = as `limiter`, 4 = monotone PPM
                        // (interface values confined between their cells; needs mg >= 3)
  double layer_r;       // two-layer shallow water (phys 4, swe_layer_stage.hip): density ratio rho_0 / rho_1
                        // in (0, 1]; the state holds F = 8 fields (h_0, M_0, h_1, M_1) and recv is [R][8]
} StageDesc;

int stsp_stage_launch(int phys, int dtype, int bx, int by, const StageDesc* d, hipStream_t stream);
// One RK stage of `members` independent states in one launch (stage_kernel.hip,
// stage_batch_kernel; ensemble.py mode="batched").  Member m works on X, Q,
// acc_in, out and acc_out advanced by m * member_stride elements (null acc_in /
// acc_out stay null); every other pointer and scalar of the descriptor is shared.
// d->nblocks is the block count of ONE member.  Physics 0, 1, 2 and the five block
// shapes of the plain stage kernel; the codes of stsp_stage_launch apply (bx == 64:
// -2, physics 3 / 4: -3, dtype: -4, ...), and nothing is launched on any of them or on
//   -20  members < 1, or more members than one launch holds
//        (8 * members * ceil(nblocks / 8) workgroups must stay below 2^31)
//   -21  member_stride < F * S (members would overlap)
//   -22  a descriptor with remote, blocks or xg set (one rank, all blocks, no exchange)
int stsp_stage_batch_launch(int phys, int dtype, int bx, int by, const StageDesc* d, int members,
                            long long member_stride, hipStream_t stream);
// Two-layer shallow water (swe_layer_stage.hip): one RK stage; stsp_stage_launch routes phys 4 here.
int stsp_swe_layer_launch(int dtype, int bx, int by, const StageDesc* d, hipStream_t stream);
// dynamic LDS bytes of one of its blocks (-1: unsupported shape); a launch over 65536 is refused with -13
int stsp_swe_layer_lds(int dtype, int bx, int by);
// Pipelined streaming SSP-RK3 step (march3_kernel.hip): one launch marches all
// three stages up each strip of a tile (stage s + 1 trails stage s by two rows),
// reading the step input d->Q once and writing the step output d->out at the
// cells at least 4 from a tile edge.  Stage s computes out = b0[s] X + b1[s] Q
// + b2[s] dt L(Q) with X = the step input.  The cells within D of a tile edge of
// the stage-1 and stage-2 results go to q1 / q2 (stage 1 also pushes its
// same-rank ghost copies into q1), so that two band launches of the stage kernel
// finish stages 2 and 3 next to the tile edges (ops/march3.py).
typedef struct March3Desc {
  void* q1;
  void* q2;
  double b0[3], b1[3], b2[3];
  int D;
} March3Desc;
int stsp_march3_launch(int dtype, int rows, const StageDesc* d, const March3Desc* m, hipStream_t stream);
int stsp_pack_launch(int dtype, const void* q, int S, int F, const int* idx, int ns, void* send, hipStream_t stream);
int stsp_copy_index_launch(int dtype, const void* src, const int* sidx, void* dst, const int* didx, int k,
                           int batch, long src_stride, long dst_stride, hipStream_t stream);
// Direct xGMI halo: write the remote ghost cells of state q (entries src[i] ->
// code[i] = peer << 24 | slot) into every peer's ring slot of stage `epoch`.
int stsp_xg_prime_launch(int dtype, const void* q, int S, int F, const int* src, const int* code, int nent,
                         void* const* peer_ring, int ring, int epoch, hipStream_t stream);
// One fused SSP-RK3 step of the shallow-water solver (fused_step.hip, ops/fused.py):
// temporal blocking over a window of the block plus a ring of 2 NS cells.
typedef struct FusedDesc {
  const void* Q;        // [F][S] step input, padded layout
  void* out;            // [F][S] step output: interior + same-rank ghost pushes
  const int* src;       // [nb][W*W] padded offset of each window cell's source, -1 = not loaded
  const int* org;       // [nb][4] X0, Y0, tile_local, xo | yo << 12 | region flags << 24 | face << 29
  // geometry (ops/fused.py::kernel_geometry): panel-independent tables, no
  // per-cell records; blocks with a side region also read their own face
  // lengths and line normals
  const void* len;      // [nb][2 H1 (H1+1)] x-faces, then y-faces
  const void* nrm;      // [nb][2][5][3][W+1] line normals per region, component-major
  const void* tane;     // [N+1]
  const void* crec;     // [N*N][8] 1/A, S (3), centre (3), 0 in panel-local components
  const void* lxt;      // [N][N+1]
  const void* gbt;      // [S (+ ring)][4] grad b, padded layout; null without topography
  int frames[6];
  const void* code;     // [nb][W*W] u64: 4 x int16 neighbour codes per window cell and side (-1, entry, -3)
  const int* gtab;      // [nb][G][2] LDS index of the interpolation pair
  const void* gw;       // [nb][G] interpolation weights
  const int* ctab;      // [nb][C][16] corner faces (ops/fused.py::corner_tables): per side q (c, d) the cell's
                        // LDS index and its across / inward stencil pairs (5 ints), face slots c, d, flags
  const void* cgf;      // [nb][C][8] normal out of c, length, the four stencil weights
  const int* ccnt;      // [nb]
  const int* push;      // [T][4][mg][n] push map (same-rank ghost slot fed by a strip cell, or -1)
  int G, C;
  int nblocks, n, N, S, mg, pw;
  int B, ns, limiter;
  double a0[4], a1[4], a2[4];
  double dt, g, omega2;
  // several ranks (xg = 1, ops/fused.py::FusedExchangePlan): window cells with
  // src <= -2 are read from this rank's receive ring, slot epoch % STSP_XG_SLOTS,
  // entry -2 - src, as tagged granules; every step stores the block's cells that
  // peers read into their rings (xpush codes peer << 24 | entry), tag epoch + 2
  int xg;
  int ring;                 // 8-byte granules per ring slot
  const void* recv;         // this rank's ring (granules)
  void* const* peer_ring;   // [world] ring bases (IPC-mapped)
  const int* xpush;         // [nb][B*B][K] destination codes, -1 none
  int K;
  int* epoch;               // [nb] steps completed
  int* err;                 // set to 1 on a wait timeout (every later wait falls through)
  long long timeout_ticks;  // s_memrealtime ticks (100 MHz)
  // nullable: [nb][16 waves][16] s_memtime of every wave at the phase boundaries
  // (prologue, then faces / updates of each stage, end); profiling only
  unsigned long long* stamps;
  // one rank holding every tile in id order: the kernel computes each window
  // cell's storage offset from the cube topology (links: per face, sides W E S
  // N, 6 bits each: nbr face | nbr edge << 3 | reversed << 5) instead of
  // loading `src` (one dependent memory round trip less in the prologue)
  int local_src;
  int links[6];
  // several steps per launch (0 / 1 = one): needs every block co-resident
  // (checked by the launcher), epoch / err, and prod [nb][PM] (producer blocks of
  // each block's window, -1 padded, symmetric)
  int nsteps;
  const int* prod;
  int PM;
  const int* cpush;     // [T][4][mg][mg] carried corner ghost pushes (StageDesc::cpush), nullable
  // face-pass schedule (ops/fused.py::pass_schedule): [nb][3 stages][20] u32:
  // per wave (16) bit p set = the wave runs pass p (faces 64 p .. 64 p + 63) of
  // the stage, balanced over the CU's four SIMDs (waves w and w + 4 share one);
  // word 16 bit p = pass p holds a face next to a panel-edge line
  const unsigned* sched;
  const void* nrmf;     // [nb][3][2 H1 (H1+1)] per-face normals of panel-edge blocks (component-major)
  // tagged in-launch hand-off of a multi-step launch, [2][W][S] u64 (W = 5 fp64, 4 fp32)
  // zero-initialised and kept with the epoch array; null = epoch hand-off
  void* hx;
  // per-cell producer polls of a one-rank epoch hand-off: [nb][W*W] int8
  // index into prod[b] of the producer of each window cell (-1: none); null =
  // wave 0 polls every producer before a barrier
  const signed char* pidx;
  // face tasks of the table-driven builds (fp32, or B <= 16): [classes][64 TCAP]
  // u16 per pass slot; sched words 17-19 say which passes are shared, where a
  // stage starts and which row a block reads (ops/fused.py::face_tables)
  const unsigned short* ftab;
} FusedDesc;
int stsp_fused_launch(int dtype, const FusedDesc* d, hipStream_t stream);
int stsp_fused_limits(int* gmax, int* cmax);
int stsp_fused_tagh(void);
int stsp_fused_table_passes(int B);
// the fused step's packed cell records (granules per cell) and their initial
// delivery into the peers' xGMI rings
int stsp_fused_record_words(int dtype);
int stsp_fused_prime_launch(int dtype, const void* q, int S, const int* src, const int* code, int nent,
                            void* const* peer_ring, int ring, int epoch, hipStream_t stream);
// Derived shallow-water fields and invariants of a state (derived_kernel.hip,
// ops/derived.py; definitions in models/derived.py): two ordinary launches, one
// workgroup per 16 x 16 cell block, then a one-workgroup fold of the block records.
typedef struct DerivedDesc {
  const void* Q;        // [4][S] state (h, M), padded layout; only interior cells are read directly
  const void* recv;     // [R][4] remote ghost slots (nullable when R == 0)
  const int* gmap;      // [T][4][mg][n] ghost map (layer 0 is read)
  const int* cgmap;     // [T][4][mg][mg] RankPlan.corner_map (entry a = b = 0 is read)
  const int* pedge;     // [T] tile sides on a panel edge (bits W, E, S, N)
  const int* pe_base;   // [T][4][3][n] panel-edge interpolation pairs (layer 0 is read)
  const void* pe_t;     // [T][4][3][n]
  const void* cdx;      // [T][3][n][n+1] x-edge chords, south to north (m)
  const void* cdy;      // [T][3][n+1][n] y-edge chords, west to east (m)
  const void* mx;       // [T][3][n+1] x-edge unit normals
  const void* my;       // [T][3][n+1]
  const void* ex;       // [T][n][n+1] x-edge lengths
  const void* ey;       // [T][n+1][n]
  const void* invA;     // [T][n][n]
  const void* area;     // [T][n][n]
  const void* idxy;     // [T][n][n] 1/dx + 1/dy
  const void* b;        // [T][n][n] topography
  const void* rz;       // [T][n][n] z of the unit cell centre
  void* fields;         // [3][T][n][n] out: zeta, delta, q
  double* partials;     // [nblocks][8] block records (5 sums, 1 max, 2 spare)
  double* inv;          // [8] out: mass, energy, potential enstrophy, circulation, |circulation|, max Courant
  int ntile, n, S, mg, pw;  // as StageDesc
  int nrecv;            // rows of recv
  int nblocks;          // ntile * ceil(n / 16)^2
  double g, omega2, dt;
} DerivedDesc;
int stsp_derived_launch(int dtype, const DerivedDesc* d, hipStream_t stream);
int stsp_derived_desc_size(void);
// Longitude-latitude regridding (latlon_kernel.hip, ops/latlon.py; definitions
// and tables in models/latlon.py): a gather launch (one thread per target
// point) and a finish launch (projection onto east / north, zonal means; one
// workgroup per latitude row).  `phases` selects them: with several ranks the
// caller adds the ranks' term arrays (`terms`) between the two.
typedef struct LatLonDesc {
  const void* Q;        // source channels [C][cs]; velocity: h, then M (3) at stride cs
  const int* idx;       // [K][4] source index inside a channel, -1 = skipped (16-byte aligned)
  const double* w;      // [K][4] weights (32-byte aligned)
  const double* east;   // [K][3] unit east vectors (project)
  const double* north;  // [K][3]
  void* partial;        // gather out / finish in, element type: [C][K], or the four terms of each sum
                        // [C][4][K] (terms); K = nlat nlon, k = j nlon + i
  void* out;            // finish out, element type: [2][K] (project) or the folded [C][K] (terms)
  double* zm;           // finish out: zonal means [C][nlat] ([2][nlat] with project; nullable then)
  long long cs;         // channel stride of Q in elements
  int K, nlat, nlon;
  int C;                // channels (3 with velocity / project)
  int velocity;         // gather: 1 = v = M / h per source cell
  int project;          // finish: 1 = (u, v) from the Cartesian triple
  int phases;           // bit 0 gather, bit 1 finish
  int terms;            // 1 = partial holds the unsummed terms (several ranks)
} LatLonDesc;
int stsp_latlon_launch(int dtype, const LatLonDesc* d, hipStream_t stream);
int stsp_latlon_desc_size(void);
// Spherical-harmonic analysis (spectra_kernel.hip, ops/spectra.py; definitions,
// tables and the twin in models/spectra.py): an analysis launch over (order m) x
// (cell slabs) that leaves one partial record per workgroup, then a fold of the
// slabs in ascending order.
typedef struct SpectraDesc {
  const void* Q;        // source channels [C][cs], element type
  const int* idx;       // [cells] position of each cell inside a channel (interior slots)
  const double* cell;   // [cells][4] mu, cos phi, lambda, w (32-byte aligned)
  const double* a;      // [L+1][L+1] recurrence factors a[l][m] (0 where l <= m)
  const double* b;      // [L+1][L+1]
  const double* c;      // [L+1] sectoral factors: P_mm = c[m] cos^m phi
  double* partial;      // [slabs][L+1][RP][16] workgroup records, row l - m, column 2 ch + (sin)
  double* out;          // [C][2][L+1][L+1] coefficients at [l][m]; the caller zero-fills it
  long long cs;         // channel stride of Q in elements
  int cells;            // cells of the rank
  int C;                // channels, 1 .. 8
  int lmax;             // L, 0 .. 1023
  int slabs;            // cell slabs (grid y), none empty
  int slab_cells;       // cells per slab, a multiple of 128
  int RP;               // rows per record: a multiple of 32, >= L + 1
} SpectraDesc;
int stsp_spectra_launch(int dtype, const SpectraDesc* d, hipStream_t stream);
int stsp_spectra_desc_size(void);
// Spherical-harmonic synthesis (synth_kernel.hip, ops/spectra.py; packing, chunk
// bounds and the twin in models/spectra.py): a launch over (cell batches of 128) x
// (order chunks); with more than one chunk every workgroup leaves a record and a
// fold adds the chunks in ascending order.
typedef struct SynthDesc {
  const double* K;        // packed coefficients [k_rows][16]: row of (m, l >= m) = m (L+1) - m (m-1) / 2 + l - m
  const int* idx;         // [cells] position of each cell inside a channel of out, all < idx_limit
  const double* cell;     // [cells][4] mu, cos phi, lambda, w (32-byte aligned)
  const double* a;        // [L+1][L+1] recurrence factors, transposed: a[m][l] (0 where l <= m)
  const double* b;        // [L+1][L+1] likewise b[m][l]
  const double* c;        // [L+1] sectoral factors: P_mm = c[m] cos^m phi
  const int* bounds;      // host: [chunks + 1] first order of each chunk, 0 = b[0] < ... < b[chunks] = L + 1
  const int* bounds_dev;  // the same numbers in device memory
  double* rec;            // [chunks][C][cells] workgroup records (unused, nullable, with one chunk)
  double* out;            // [C][cells] the field, float64
  long long k_rows;       // (L+1)(L+2)/2
  long long rec_elems;    // elements rec holds, >= chunks C cells
  int cells;              // cells of the rank
  int idx_limit;          // what the host checked idx against: must equal cells
  int C;                  // channels, 1 .. 8
  int lmax;               // L, 0 .. 1023
  int chunks;             // order chunks (grid y), 1 .. L + 1
  int pad_;
} SynthDesc;
int stsp_synth_launch(const SynthDesc* d, hipStream_t stream);
int stsp_synth_desc_size(void);
// Point sampling and Lagrangian particles (points_kernel.hip, ops/points.py;
// definitions and the twin in models/points.py): one thread per point locates
// it on the dual mesh of the cell centres and gathers four source cells.
// `mode` 0 samples at p; 1 applies the corrector (`stage` 0) or the predictor
// (`stage` 1) move from a velocity sampled before; 2 is the fused advance of one
// rank (sample at xs, corrector, sample at x, predictor in one thread).
typedef struct PointsDesc {
  const void* Q;          // source channels [C][cs], element type; velocity: h, then M (3)
  const int* cmap;        // [6 N N] global cell id -> index inside a channel, -1 = not owned
  const int* eid;         // [6][4][N-1] edge quad of panel, side, position: row of bcell
  const int* bcell;       // [nb][4] cells of the border elements: 12 (N-1) edge quads, then 8
                          // corner triangles (fourth slot -1)
  const int* ctri;        // [6][4] corner triangle of panel, quadrant: 0 .. 7
  const double* bctr;     // [nb][4][3] unit centres of the cells of bcell
  const double* p;        // mode 0: [K][3] points
  double* out;            // mode 0 out: [C][K], or the terms [C][4][K]
  int* elem;              // mode 0 out, nullable: [K] element id (-1: lost)
  const double* vel;      // mode 1 in: [3][K] velocity sampled at xs (stage 0) / x (stage 1), or terms [3][4][K]
  double* x;              // [K][3] particle positions (modes 1, 2)
  double* xs;             // [K][3] predicted positions
  double* v0;             // [K][3] V(x)
  long long cs;           // channel stride of Q in elements
  long long lim;          // elements of a channel the map may address, <= cs
  double da;              // pi / (2 N)
  double radius;          // sphere radius (m)
  double dtp;             // particle step (s)
  int K, N;
  int C;                  // channels (3 in velocity mode)
  int velocity;           // mode 0: 1 = v = M / h per source cell
  int terms;              // out / vel hold the unsummed terms
  int mode, stage;
  int pad_;
} PointsDesc;
int stsp_points_launch(int dtype, const PointsDesc* d, hipStream_t stream);
int stsp_points_desc_size(void);
// Scale-selective dissipation of the shallow-water state (dissipation_kernel.hip,
// ops/dissipation.py; the scheme, the tables and the twin in models/dissipation.py):
// one ordinary launch per pass, one workgroup per 16 x 16 cell block.  Pass 1
// writes the four scalars and their least-squares gradients to the scratch, pass
// 2 forms the corrected edge fluxes from the scratch alone and either stores L w
// or updates the state in place.  All arithmetic and every table is float64;
// `dtype` is the element type of the state.
typedef struct DissDesc {
  const void* src;      // pass 1 in: mode 1 the state [F][S] (element type), mode 0 scalars [4][S] (double)
  const void* recv;     // pass 1 in: remote ghosts of src, [R][recv_stride], type of src (nullable when R == 0)
  double* scratch;      // [16][S]: rows 0..3 scalars, row 4 + 3 c + k component k of G of scalar c
  const double* srecv;  // pass 2 in: remote ghosts of scratch [R][16] (nullable when R == 0)
  void* out;            // pass 2 out: mode 0 L w [4][S] (double), mode 1 the state [F][S] (element type)
  const int* gmap;      // [T][4][mg][n] ghost map (layer 0 is read)
  const double* W;      // [4][3][T][n][n] gradient weights of the neighbours W, E, S, N
  const double* cx;     // [T][n][n+1] L / dn of the x-edges
  const double* cy;     // [T][n+1][n]
  const double* kx;     // [3][T][n][n+1] L (m - dvec / dn)
  const double* ky;     // [3][T][n+1][n]
  const double* gb;     // [3][T][n][n] G(b)
  const double* dbx;    // [T][n][n+1] b_R - b_L
  const double* dby;    // [T][n+1][n]
  const double* invA;   // [T][n][n]
  const double* ctr;    // [3][T][n][n] unit cell centres
  int ntile, n, S, mg, pw;  // as StageDesc
  int nrecv;            // rows of recv / srecv
  int recv_stride;      // pass 1: values per row of recv (>= 4)
  int nblocks;          // ntile * ceil(n / 16)^2
  int pass_;            // 1 gradients, 2 fluxes
  int mode;             // pass 1: 1 = src is (h, M), read as (h, M / h); pass 2: 1 = update the state
  int use_b;            // add the topography terms to scalar 0
  int depth;            // update: write h
  double coef;          // update: w += coef L w
} DissDesc;
int stsp_dissipation_launch(int dtype, const DissDesc* d, hipStream_t stream);
int stsp_dissipation_desc_size(void);
// Consistent thermal diffusion (heat_kernel.hip, ops/heat.py; the twin in
// models/diffusion.py): the Laplacian of the dissipation for one scalar, fused
// with the Runge-Kutta stage combination.  One ordinary launch per pass, one
// workgroup per 16 x 16 cell block.  Pass 1 writes the scalar and its
// least-squares gradient to the scratch; pass 2 forms L from the scratch alone
// and stores L (mode 0), out = a2dt kappa L (+ a1 Q) (+ a0 X) (mode 1), or that
// and acc_out = c1 X + c2dt kappa L (+ c0 ACC) (mode 2).  All arithmetic and every
// table is float64; `dtype` is the element type of q, x, acc_in, out, acc_out.
typedef struct HeatDesc {
  const void* q;        // the stage input, one row [S] (element type); pass 2: read at the own cell only
  const void* recv;     // pass 1: remote ghosts of q, [R][recv_stride], element 0 of a row (nullable when R == 0)
  double* scratch;      // [4][S]: T, Gx, Gy, Gz
  const double* srecv;  // pass 2: remote ghosts of scratch, [R][4] (nullable when R == 0)
  const int* gmap;      // [T][4][mg][n]; layer 0 is read: >= 0 an interior cell of this rank, < 0 receive row -1 - code
  const double* W;      // [4][3][T][n][n]
  const double* cx;     // [T][n][n+1]
  const double* cy;     // [T][n+1][n]
  const double* kx;     // [3][T][n][n+1]
  const double* ky;     // [3][T][n+1][n]
  const double* invA;   // [T][n][n]
  const void* x;        // modes 1, 2: X, one row [S] (read when a0 != 0 or mode 2; may alias out)
  const void* acc_in;   // mode 2: ACC, one row [S] (nullable: no accumulator input; may alias acc_out)
  void* out;            // modes 1, 2: one row [S]
  void* acc_out;        // mode 2: one row [S]
  double* lout;         // mode 0: L, one row [S] (double)
  int ntile, n, S, mg, pw;   // S = ntile * pw * pw, pw = n + 2 mg
  int nrecv;            // R
  int recv_stride;      // elements per row of recv (pass 1)
  int nblocks;          // ntile * ceil(n / 16)^2
  int pass_;            // 1 or 2
  int mode;             // pass 2: 0, 1 or 2
  double kappa;
  double a0, a1, a2dt;  // a2dt = a2 * dt
  double c0, c1, c2dt;  // c2dt = c2 * dt
} HeatDesc;
int stsp_heat_launch(int dtype, const HeatDesc* d, hipStream_t stream);
int stsp_heat_desc_size(void);
// Ensemble statistics of one field of a batched state (ensemble_kernel.hip,
// ops/ensemble_stats.py; definitions and the twin in models/ensemble_stats.py):
// a launch with one workgroup per 16 x 16 cell block (mean and population
// variance over the members per cell, in float64, and a block record), then a
// one-workgroup fold of the records in ascending block order.
typedef struct EnsStatsDesc {
  const void* Q;        // [members][fields][S] batched state (element type), padded layout; interior cells are read
  const void* area;     // [T][n][n] cell areas (element type)
  double* mean;         // [T][n][n] out
  double* var;          // [T][n][n] out
  double* partials;     // [nblocks][4] block records: sum A mean, sum A var, sum A, max var
  double* out;          // [4] out: the records folded
  long long member_stride;  // elements between members, >= fields * S
  int members, fields, field;
  int ntile, n, S, mg, pw;  // as StageDesc
  int nblocks;          // ntile * ceil(n / 16)^2
} EnsStatsDesc;
int stsp_ensemble_stats_launch(int dtype, const EnsStatsDesc* d, hipStream_t stream);
int stsp_ensemble_stats_desc_size(void);
// Time-dependent winds of the advection model (wind_kernel.hip, ops/wind.py; the
// twin: models/advection.py): one launch before a Runge-Kutta stage refills the
// stage kernel's transport tables ex / ey in place at the stage time
// t_s = ((double)count[0] + cs) * dt.  The step count lives on the device and
// stsp_wind_tick adds one to it.  Every table and all arithmetic is float64;
// `dtype` is the element type of ex and ey.
typedef struct WindDesc {
  void* ex;             // [T][n][n+1] out (element type)
  void* ey;             // [T][n+1][n] out (element type)
  const double* vtab;   // mode 0: [4][T][n+1][n+1] vertex factors sin lam, cos lam, P, Q
  const double* xtab;   // mode 1: [5][T][n][n+1] x-edge factors sin lam, cos lam, A, B, C
  const double* ytab;   // mode 1: [5][T][n+1][n]
  const int* count;     // [1] the step count
  int ntile, n;
  int nblocks;          // mode 0: ntile * ceil(n / 16)^2; mode 1: ceil(2 ntile n (n+1) / 256)
  int mode;             // 0 streamfunction (vertex differences), 1 midpoint rule
  double dt, cs;        // the step and the stage's abscissa
  double omega;         // w of lam' = lam - w t (2 pi / T; 0 without the background rotation)
  double pi_over_T;     // c(t) = cos(pi_over_T * t)
} WindDesc;
int stsp_wind_launch(int dtype, const WindDesc* d, hipStream_t stream);
int stsp_wind_tick(int* count, hipStream_t stream);
int stsp_wind_desc_size(void);
// Direct xGMI halo build constant: ring slots.
int stsp_xg_slots(void);
}
