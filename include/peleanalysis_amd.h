/*
 * peleanalysis_amd.h -- C ABI of the MI355X-native PeleAnalysis stencil path.
 *
 * The reference (AMReX-Combustion/PeleAnalysis) has no plugin/FFI interface:
 * its boundary is (i) each tool's key=value command line + plotfile formats and
 * (ii) the per-FArrayBox call shape inside the MFIter loops of the tool mains.
 * This header is the C ABI at (ii); tools/ keeps (i).  Every entry point cites
 * the reference call site it replaces.  Plain pointers and sizes only; all
 * `double*` named dev* / stored in pa_mf are DEVICE pointers (HBM).
 *
 * Conventions: return 0 = OK, non-zero = error (text via pa_last_error); the
 * library never aborts.  All work is enqueued on the pa_ctx's HIP stream and is
 * asynchronous unless stated; pa_sync() waits.  A pa_ctx is not thread-safe;
 * use one per host thread (the reference's per-FAB loops are serial per rank).
 *
 * Array layout: AMReX FArrayBox layout -- [comp][k][j][i], i fastest, over the
 * valid box grown by ng ghost cells.  Boxes are inclusive cell-index boxes
 * {lo0,lo1,lo2,hi0,hi1,hi2}.
 */
#ifndef PELEANALYSIS_AMD_H
#define PELEANALYSIS_AMD_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pa_ctx pa_ctx;     /* device, stream, error text, scratch */
typedef struct pa_level pa_level; /* BoxArray + Geometry of one AMR level (host + device copies) */
typedef struct pa_mf pa_mf;       /* MultiFab: ncomp x (boxes grown by ng) doubles in HBM */

/* mirrors amrex::Array4 / FArrayBox: p = device pointer, lo/hi incl. ghosts, nstride = component
 * stride in doubles (Array4::nstride; 0 = contiguous nx*ny*nz like a plain FArrayBox) */
typedef struct { double* p; int32_t lo[3]; int32_t hi[3]; int32_t ncomp; int64_t nstride; } pa_fab;
typedef struct { int32_t lo[3]; int32_t hi[3]; } pa_box;

/* LinOpBCType subset used by grad.cpp:180-193 / curvature.cpp:428-441 */
enum { PA_BC_PERIODIC = 0, PA_BC_NEUMANN = 1, PA_BC_REFLECT_ODD = 2 };

/* ------------------------------------------------------------------ context */
int         pa_version(void);
pa_ctx*     pa_ctx_create(int device, void* hip_stream /* NULL: library-owned stream */);
void        pa_ctx_destroy(pa_ctx*);
const char* pa_last_error(const pa_ctx*);
int         pa_sync(pa_ctx*);
void*       pa_ctx_stream(pa_ctx*);
/* The library's environment switches (the PA_* table in peleanalysis_amd/csrc/pa_internal.h: pa_options) are read ONCE, when the
 * first context is created.  A caller that changes one afterwards -- a test, an A/B measurement inside one process -- asks for a
 * re-read with this call.  No reference counterpart (AMReX's ParmParse is read at amrex::Initialize, grad.cpp:31). */
void        pa_options_reload(void);

/* raw HBM buffers for callers without their own device allocator (vertex / triangle buffers of
 * the marching-cubes entry points, caller-owned FABs).  Copies are synchronous. */
void* pa_device_malloc(pa_ctx*, int64_t bytes);
void  pa_device_free(pa_ctx*, void* devptr);
int   pa_memcpy_h2d(pa_ctx*, void* devdst, const void* hostsrc, int64_t bytes);
int   pa_memcpy_d2h(pa_ctx*, void* hostdst, const void* devsrc, int64_t bytes);
/* device to device, also between the devices of two contexts of one process (peer copy over xGMI); synchronous */
int   pa_memcpy_d2d(pa_ctx*, void* devdst, const void* devsrc, int64_t bytes);
/* number of HIP devices visible to the process (0: none / no runtime) */
int   pa_device_count(void);

/* Per-launch timing of the library's own kernels with HIP events recorded on the
 * context's stream (what bench.py's roofline object reports).  Tags: 1 fused
 * grad->curvature, 2 its face fix-up, 3 FillBoundary, 4 applyBC, 5 grad,
 * 6 progress, 7 box filter, 8 marching cubes.  on: 0 off, 1 every tag, otherwise a bit mask (1 << tag) of the
 * tags to time.  pa_profile_read is synchronous. */
int pa_profile_enable(pa_ctx*, int on);
/* which variant of the fused grad->curvature sweep the last pa_gradcurv_* call launched, e.g.
 * "k_gradcurv_march3<MTY=13,CLIP=0,PAIR=0,CG=1>" (bench.py keys the committed PMC traffic figure on it) */
const char* pa_sweep_kernel_name(const pa_ctx*);
/* diagnostic: workgroups of the all-levels sweep kernel the runtime keeps resident per CU (which = 0: boxes wider than 32 cells,
 * 1: the narrow-box kernel); < 0: the query failed */
int pa_sweep_occupancy(pa_ctx*, int which);
/* diagnostic: cells that the clip-aware curvature fix-up of the last fused pass (threshold_prog, curvature.cpp:549-570) had to
 * recompute through its general path because a neighbour's normal was clipped; -1 if that path has never run.  Synchronous. */
int pa_last_slow_cells(pa_ctx*);
/* diagnostic: number of IRREGULAR cells of a level -- boundary cells of its local boxes next to a concave coarse-fine corner or to
 * the line where a box face changes from covered-by-a-neighbour to coarse-fine (general BoxArrays; the reference's MLPoisson /
 * FillBoundary code has no such distinction, curvature.cpp:426-546) -- whose curvature the fused grad->curvature pass recomputes
 * cell by cell after its sweep.  0 for the nested, convex hierarchies of the SURVEY's configs.  Builds the list on first use;
 * synchronous; -1 on error. */
int64_t pa_level_irregular_cells(pa_ctx*, const pa_level*);
int pa_profile_read(pa_ctx*, int tag, int64_t* nlaunch, double* total_ms, int reset);

/* ---------------------------------------------------- level = BoxArray+Geometry
 * replaces: amrData.boxArray(lev) / Geometry(ProbDomain, rb, coord, is_per)
 * (grad.cpp:160-163, curvature.cpp:287-291).  dx = (prob_hi-prob_lo)/ncells. */
pa_level* pa_level_create(pa_ctx*, int nboxes, const int32_t* boxes6, const int32_t domlo[3],
                          const int32_t domhi[3], const int32_t is_per[3], const double prob_lo[3],
                          const double prob_hi[3]);
/* ------------------------------------------------------- multi-GPU: one rank per GPU
 * The reference distributes the boxes of every level over MPI ranks with DistributionMapping(ba)
 * (grad.cpp:162, curvature.cpp:289, filterPlt.cpp:142, isosurface.cpp:1441) and moves ghost data with
 * point-to-point messages inside FillBoundary / FillPatch / the MLMG boundary registers.  Here a rank is one
 * pa_ctx (one process per GPU, or one host thread per GPU inside a tool).  A level created with
 * pa_level_create_sharded knows the whole BoxArray and its owner map; every entry point that fills ghost cells
 * (pa_fill_boundary, pa_apply_bc, pa_fillpatch_two_levels, the pa_*_run pipelines) then also performs the
 * cross-rank half -- pack kernels -> one grouped point-to-point exchange -> unpack kernels -- through the
 * context's transport, and pa_*_run reduces the progress-variable range over the ranks (curvature.cpp:147-148).
 * All ranks must make the same sequence of calls (as MPI ranks of the reference do). */
typedef struct { int32_t peer; double* sendbuf; int64_t nsend; double* recvbuf; int64_t nrecv; } pa_xfer;
typedef struct {
  void*   user;
  int32_t rank, nranks;
  /* One grouped exchange: for every i send nsend doubles from sendbuf to rank peer and receive nrecv doubles from it
   * into recvbuf (device pointers; either count may be 0).  Several entries may name the same peer: they are matched
   * in list order on both sides.  Stream-ordered: the call consumes data produced by work already enqueued on
   * hip_stream, and work enqueued on it afterwards sees the received data.
   * POINT-TO-POINT contract (like MPI_Isend/Irecv inside FillBoundary): the library calls exchange on a rank only when
   * that rank has at least one entry, so a rank without a box of the level, or without a neighbour on another rank,
   * does not call it -- an implementation must pair sends with receives per (sender, receiver) in FIFO order and must
   * never wait for ranks that are not named in x. */
  int (*exchange)(void* user, void* hip_stream, int32_t n, const pa_xfer* x);
  /* vals[i] = reduction over the ranks of vals[i] (host memory); op: 0 min, 1 max, 2 sum */
  int (*allreduce)(void* user, double* vals, int32_t n, int32_t op);
} pa_comm;
/* caller-supplied transport (tests: gloo through host memory; tools: peer copies between host threads) */
int pa_ctx_set_comm(pa_ctx*, const pa_comm*);
/* built-in transport: RCCL over xGMI (grouped ncclSend / ncclRecv on the context's stream, ncclAllReduce).
 * pa_rccl_unique_id fills 128 bytes on one rank; the caller broadcasts them; every rank then calls pa_ctx_init_rccl. */
/* diagnostic transport for PROJECTIONS of an N-rank run on one GPU (bench.py --sim-of N --xdelay-us / --xlink-GBs): moves no
 * data; every exchange enqueues on its stream a kernel that spins for fixed_us + (most bytes to or from one peer) / link_GBs,
 * the cost model of a grouped point-to-point exchange over per-peer xGMI links -- the schedule hides or exposes that time as it
 * would a real exchange.  Ghost-cell results are wrong by construction.  pa_delay_comm_stats: exchanges issued / modelled time. */
int pa_ctx_set_delay_comm(pa_ctx*, int nranks, int rank, double fixed_us, double link_GBs);
int pa_delay_comm_stats(const pa_ctx*, int64_t* calls, double* total_us);
int pa_rccl_unique_id(pa_ctx*, void* id128);
int pa_ctx_init_rccl(pa_ctx*, int nranks, int rank, const void* id128);
int pa_ctx_nranks(const pa_ctx*);
/* transport check: a ring exchange of n doubles with known contents + a max-reduction with a known answer; synchronous */
int pa_comm_selftest(pa_ctx*, int64_t n);
/* the transport's reduction over the ranks (no-op on one rank): op 0 min, 1 max, 2 sum */
int pa_allreduce(pa_ctx*, double* vals, int n, int op);
/* DistributionMapping(ba) restated: boxes in Morton order of their low corners, cut into nranks contiguous pieces of
 * (nearly) equal cell count.  Host arithmetic only.  owner[b] in [0, nranks). */
int pa_distribution_map(int nboxes, const int32_t* boxes6, int nranks, int32_t* owner);
/* This rank's share of a level: the whole BoxArray + the owner rank of every box.  The level's boxes are the ones with
 * owner == rank, in BoxArray order (pa_level_global_ids gives their indices in the BoxArray). */
pa_level* pa_level_create_sharded(pa_ctx*, int nboxes, const int32_t* boxes6, const int32_t* owner, int rank, int nranks,
                                  const int32_t domlo[3], const int32_t domhi[3], const int32_t is_per[3],
                                  const double prob_lo[3], const double prob_hi[3]);
int pa_level_global_ids(const pa_level*, int32_t* gids /* [pa_level_nboxes] */);
/* The region lists behind those exchanges, as plain host arithmetic (no GPU; what the CPU-tier tests check against the
 * undistributed answer).  Rows of 9 int32: {kind, peer, box, lo0, lo1, lo2, hi0, hi1, hi2}; returns the number of rows
 * (writes at most cap).  kind 0 = send (box = global index of a box this rank owns, region in its index space),
 * kind 1 = receive (FillBoundary: box = global index of the destination box, ghost region).
 * pa_plan_coarse_source: the coarse data rank `rank` needs under the coarse-fine faces of its fine boxes (mode 0: the
 * stencils of pa_apply_bc) or under the ng ghost layers of its fine boxes grown by `halo` coarse cells (mode 1:
 * pa_fillpatch_two_levels); kind 2 = piece (box = global coarse box it is cut from, peer = its owner; pieces are
 * disjoint and listed in the order of the rank's coarse-source BoxArray), kind 0 = what this rank sends to `peer`. */
int64_t pa_plan_fill_boundary(int nboxes, const int32_t* boxes6, const int32_t* owner, int rank, const int32_t domlo[3],
                              const int32_t domhi[3], const int32_t is_per[3], int ng, int32_t* rows9, int64_t cap);
int64_t pa_plan_coarse_source(int nfine, const int32_t* fboxes6, const int32_t* fowner, const int32_t fdomlo[3],
                              const int32_t fdomhi[3], int ncrse, const int32_t* cboxes6, const int32_t* cowner,
                              const int32_t cdomlo[3], const int32_t cdomhi[3], const int32_t is_per[3], int rank,
                              int mode, int ng, int halo, int32_t* rows9, int64_t cap);
/* pa_plan_restriction: what moves between ranks in the distributed smoothing solve (pa_smooth_solve on sharded levels; what
 * amrex::average_down and MLMG's flux register move, curvature.cpp:328-406).  which = 0: the child averages -- kind 0 = send
 * (box = global FINE box this rank owns, region = part of that box coarsened by `ratio`), kind 1 = receive (box = global COARSE
 * box, the same region: its valid cells), kinds 3 / 4 = source / destination of a same-rank copy, in pairs.  which = 1 + 2 * dir
 * + side: the flux register of that face orientation -- the source regions lie in the one-cell ghost slab behind face (dir, side)
 * of the coarsened fine box (special faces only), the destination regions are those cells folded into the coarse domain through
 * its periodic images.  Both sides of a pair of ranks list their regions in the same order. */
int64_t pa_plan_restriction(int nfine, const int32_t* fboxes6, const int32_t* fowner, const int32_t fdomlo[3],
                            const int32_t fdomhi[3], int ncrse, const int32_t* cboxes6, const int32_t* cowner,
                            const int32_t cdomlo[3], const int32_t cdomhi[3], const int32_t is_per[3], int rank, int ratio,
                            int which, int32_t* rows9, int64_t cap);
/* Internal re-tiling (host arithmetic only): another BoxArray with exactly the cells of boxes6 -- boxes at least min_thick cells
 * thick in every direction merged into the largest rectangles the cell set allows (maximal x-runs, stacked in y, then z; at
 * most max_size[d] cells per direction, cut as evenly as the input edges allow; an input box larger than that is not split),
 * thinner boxes passed through unchanged at the end of the list.  grad.cpp:158-236, curvature.cpp:283-570 and
 * Filter::apply_filter (filterPlt.cpp:206-219) are point-wise functions of the level's cell set except for the coarse-fine
 * interpolant of a box fewer than 3 cells thick (MLCellLinOp::applyBC, order min(n + 1, 4)), so with min_thick >= 3 a level
 * created on the returned boxes gives the same value in every cell -- bit for bit -- as one created on boxes6
 * (tests/test_retile.py; filterPlt.cpp:141 re-chops the file's BoxArray itself: the tiling is not part of the tools'
 * contract).  Marching cubes numbers nodes in box order and must keep the file's boxes.  The caller moves FAB data between
 * the two tilings by box intersection (tools/common/pa_plotfile.h read_comp / write_plotfile, hierarchy.regrid_copy).
 * out_boxes6: room for cap >= nboxes boxes (an L-shaped union of two boxes may come back as three rectangles); returns the
 * number of boxes written (the input itself when nothing can be merged, a piece would come out thinner than min_thick or cap
 * is too small for the result), -1 on bad arguments.  max_size NULL: 128 per direction. */
int pa_level_retile(int nboxes, const int32_t* boxes6, const int32_t max_size[3], int min_thick, int32_t* out_boxes6, int cap);
/* The max_size the tools and bench.py pass to pa_level_retile for the levels of one hierarchy (boxes6[l]: the nboxes[l] boxes of
 * level l): 512 x 256 x 256 cells where every level then consists of blocks at least 128 cells thick, else 128^3 (measured:
 * profiles/r05_retile.txt); PA_RETILE_MAX="x y z" in the environment overrides.  Host arithmetic only; 0 = OK. */
int pa_hierarchy_retile_limits(int nlev, const int32_t* nboxes, const int32_t* const* boxes6, int min_thick, int32_t max_size[3]);
/* the same for a hierarchy sharded over nranks ranks: the largest of 512 x 256 x 256 / 256^3 / 256 x 256 x 128 / 128^3 that leaves every level at least
 * 4 nranks boxes (nranks <= 1: pa_hierarchy_retile_limits) */
int pa_hierarchy_retile_limits_ranks(int nlev, const int32_t* nboxes, const int32_t* const* boxes6, int min_thick, int nranks, int32_t max_size[3]);
void      pa_level_destroy(pa_level*);
int       pa_level_nboxes(const pa_level*);

/* -------------------------------------------------------------- MultiFab
 * pa_mf_layout is pure host arithmetic (no GPU): offset (in doubles) of each box in the flat
 * buffer and its component stride (>= nx*ny*nz incl. ghosts: rounded up to 512 B and kept off
 * multiples of 16 KiB so that the components of one cell do not share an HBM channel); returns
 * the total size in doubles.  Inside a component the layout is the FArrayBox one ([k][j][i]).
 * replaces: MultiFab(ba, dm, ncomp, ngrow) (grad.cpp:164, curvature.cpp:294).
 * Output contract of every entry point: it stores EVERY valid cell of the components it owns and nothing else -- a caller's devptr
 * is never cleared, and what a call does not own (ghost cells of an ng = 0 output, components of options that are off) is left as it was. */
int64_t pa_mf_layout(int nboxes, const int32_t* boxes6, int ncomp, int ng, int64_t* off, int64_t* cstride);
pa_mf*  pa_mf_create(pa_ctx*, const pa_level*, int ncomp, int ng, double* devptr /* NULL: library allocates */);
void    pa_mf_destroy(pa_mf*);
double* pa_mf_data(pa_mf*);
int64_t pa_mf_size(const pa_mf*);
int     pa_mf_upload(pa_ctx*, pa_mf*, const double* host);  /* synchronous */
int     pa_mf_download(pa_ctx*, const pa_mf*, double* host); /* synchronous */
/* components comp .. comp + ncomp - 1 only; host is laid out like the whole multifab (pa_mf_layout), its other components are not
 * read / written (a tool's multifab that holds inputs AND outputs, grad.cpp:164: only the inputs go up, only the outputs come back) */
int     pa_mf_upload_comps(pa_ctx*, pa_mf*, const double* host, int comp, int ncomp);   /* synchronous */
int     pa_mf_download_comps(pa_ctx*, const pa_mf*, double* host, int comp, int ncomp); /* synchronous */
int     pa_mf_setval(pa_ctx*, pa_mf*, int comp, int ncomp, double v); /* whole fabs incl. ghosts */
/* MultiFab::Copy(dst, src, scomp, dcomp, ncomp, ng) -- same BoxArray */
int     pa_mf_copy(pa_ctx*, const pa_mf* src, int scomp, pa_mf* dst, int dcomp, int ncomp, int ng);

/* ------------------------------------------------------------ ghost cells
 * FabArray::FillBoundary(comp, ncomp, periodicity): grad.cpp:169,
 * curvature.cpp:322,484,488,502; isosurface.cpp:1468. */
int pa_fill_boundary(pa_ctx*, pa_mf*, int comp, int ncomp, int ng);
/* MLCellLinOp::applyBC on the ring-1 face ghosts (inside MLMG::getFluxes,
 * grad.cpp:212-213, curvature.cpp:445-457,518-531): covered cells untouched,
 * physical walls Neumann / reflect_odd, coarse-fine cells = InterpBndryData
 * (order 3, tangential) + cubic in the normal direction (setMaxOrder(4)).
 * crse may be NULL on level 0.  only_dir = -1 for all three directions. */
int pa_apply_bc(pa_ctx*, pa_mf* fine, int comp, const pa_mf* crse, int ccomp, const int32_t bc[3],
                int ratio, int only_dir);
/* coarse-fine ghost cells (since the last call) whose coarse data was missing: improper
 * nesting.  Synchronous; resets the counter.  0 = all ghost fills were well defined. */
int pa_bc_errors(pa_ctx*);

/* --------------------------------------------------- level-batched kernels
 * One launch covers every box of the level (many small FABs per launch). */
/* grad.cpp:211-236: gx,gy,gz,|g| of phi[comp] into out[ocomp..ocomp+3] */
int pa_grad_level(pa_ctx*, const pa_mf* phi, int comp, pa_mf* out, int ocomp);
/* curvature.cpp:139-149 (AmrData::MinMax of one level; valid cells) */
int pa_minmax_level(pa_ctx*, const pa_mf* s, int comp, double* mn, double* mx); /* synchronous */
/* curvature.cpp:310-321: c = (s - pmin) * (1/(pmax-pmin)), ng ghost layers too */
int pa_progress_level(pa_ctx*, const pa_mf* s, int comp, double pmin, double pmax, pa_mf* c, int ccomp, int ng);
/* curvature.cpp:451-502: G = grad c, normgrad = -max(1e-14,|G|), n = G/normgrad
 * (valid cells).  G, normgrad may be NULL (not stored). */
int pa_normal_level(pa_ctx*, const pa_mf* c, int comp, pa_mf* G, int gcomp, pa_mf* normgrad, int ngcomp,
                    pa_mf* n, int ncomp0);
/* curvature.cpp:508-546: K = scale * sum_d d n_d/dx_d  (n: 3 comps with
 * resolved face ghosts), + threshold clip :549-567 if thr >= 0 (c needed) */
int pa_div_level(pa_ctx*, pa_mf* n, int ncomp0, double scale, const pa_mf* c, int ccomp, double thr,
                 pa_mf* K, int kcomp);
/* same, only where the fused path reads a stored progress variable: for every box face that has
 * a ghost cell which is not a valid cell of the level (coarse-fine or wall), the `depth` valid
 * layers + ng ghost layers behind/beyond that face over the grown tangential extent.  Other cells
 * of c are left untouched. */
int pa_progress_shell_level(pa_ctx*, const pa_mf* s, int comp, double pmin, double pmax, pa_mf* c, int ccomp, int ng,
                            int depth);
/* fused grad->curvature (headline kernel; grad.cpp:211-236 + curvature.cpp:316-320,451-567 in
 * one sweep).  Reads phi only (ng>=2: FillBoundary(2) + applyBC'd face ghosts; 8 B/cell) and
 * writes out[ocomp..+3] = gx,gy,gz,|g|, out[ocomp+4..+6] = FlameNormal, out[ocomp+7] =
 * MeanCurvature (64 B/cell); the progress variable (phi-pmin)/(pmax-pmin) is formed on chip.
 * Cells within two layers of a coarse-fine or physical face of their box then get N and K from
 * pa_gradcurv_faces_level, which applies the reference's boundary conditions on c and n there
 * (c: ng>=2, FillBoundary(2) + applyBC on face and edge ghosts, valid within 4 cells of the faces). */
int pa_gradcurv_level(pa_ctx*, const pa_mf* phi, int pcomp, double prog_min, double prog_max, double thr,
                      pa_mf* out, int ocomp);
int pa_gradcurv_faces_level(pa_ctx*, const pa_mf* c, int ccomp, const pa_mf* crse_n /* NULL on level 0 */,
                            int cncomp0, const int32_t bc[3], int ratio, double thr, pa_mf* out, int ncomp0,
                            int kcomp);

/* -------------------------------------------------------- per-FAB entry points
 * (the body of one MFIter iteration; device pointers in pa_fab) */
/* grad.cpp:211-236 for one FAB; phi has >=1 resolved ghost layer */
int pa_grad_fab(pa_ctx*, pa_box valid, const pa_fab* phi, int comp, const double dxinv[3], pa_fab* out, int ocomp);
/* curvature.cpp:316-320 */
int pa_progress_fab(pa_ctx*, pa_box bx, const pa_fab* s, int comp, double pmin, double pmax, pa_fab* c, int ccomp);
/* curvature.cpp:451-502 */
int pa_normal_fab(pa_ctx*, pa_box valid, const pa_fab* c, int comp, const double dxinv[3], pa_fab* G, int gcomp,
                  pa_fab* normgrad, int ngcomp, pa_fab* n, int ncomp0);
/* curvature.cpp:508-546 */
int pa_div_fab(pa_ctx*, pa_box valid, const pa_fab* n, int ncomp0, const double dxinv[3], double scale,
               pa_fab* K, int kcomp);
/* fused sweep for one FAB (phi with 2 ghost layers; exact where they hold same-level data) */
int pa_gradcurv_fab(pa_ctx*, pa_box valid, const pa_fab* phi, int pcomp, double prog_min, double prog_max,
                    const double dxinv[3], double thr, pa_fab* out, int ocomp);
/* filterPlt.cpp:217 Filter::apply_filter(box, in, out) */
int pa_boxfilter_fab(pa_ctx*, pa_box valid, const pa_fab* in, pa_fab* out, int scomp, int ncomp, int ng,
                     const double* w /* host, 2ng+1 */);

/* ----------------------------------------------------------------- filterPlt
 * Filter(type=box, fgr) weights (filterPlt.cpp:136-137); returns ngrow */
int pa_box_filter_weights(int fgr, double* w);
/* filterPlt.cpp:80 filter_type -> the PelePhysics Filter weights for the types restated here: 0 none, 1 box, 3 / 7 the
 * 3-point and 4 / 8 the 5-point approximations of the box / Gaussian filter (w: at least max(fgr + 2, 5) doubles).
 * Returns ngrow, or -1 for a type that is not available (5 6 9 10 "optimized"; 2 Gaussian unless PA_ALLOW_UNVERIFIED_GAUSSIAN=1 is
 * in the environment: its weights -- the textbook kernel sampled at cell centres, cut at 4 standard deviations -- could not be
 * checked against PelePhysics, whose source is not in the reference tree) or fgr < 1.  Host only.
 * [weights re-derived from the moment conditions; PelePhysics is not part of the reference tree: parity unpinned] */
int pa_filter_weights(int type, int fgr, double* w);
/* filterPlt.cpp:206-219, all boxes of a level */
int pa_boxfilter_level(pa_ctx*, const pa_mf* in, pa_mf* out, int scomp, int ncomp, int ng, const double* w);
/* Filter::apply_filter on every level of a hierarchy in one call (the level loop of filterPlt.cpp:206-219): in[l] / out[l] / ngs[l] /
 * ws[l] as pa_boxfilter_level's arguments for level l (the levels one after the other on the context's stream). */
int pa_boxfilter_hierarchy(pa_ctx*, int nlev, const pa_mf* const* in, pa_mf* const* out, int scomp, int ncomp, const int32_t* ngs,
                           const double* const* ws);
/* the AMREX_SPACEDIM == 2 build of the same call on a level stored as one plane of cells (k = 0):
 * out(i,j,c) = sum_m sum_l (w_l w_m) in(i+l, j+m, c) */
int pa_boxfilter_level2d(pa_ctx*, const pa_mf* in, pa_mf* out, int scomp, int ncomp, int ng, const double* w);
/* which kernel the last pa_boxfilter_fab / _level / _level2d call on the context launched, and in what shape (for a hierarchy call: its
 * last level).  info = {kind, ng, threads per workgroup, rows per y strip TY, y strips, planes per z segment kseg, z segments, refused}:
 * kind 0 = none yet, 1 = separable, 2 = tap order streaming (box weights), 3 = tap order from an LDS tile, 4 = tap order for any width,
 * 5 = the 2-D kernel; strips and segments are those of the largest box, the one the launch was shaped for; refused = 1 when the
 * separable form was asked for and its shape rule declined the boxes, so a tap-order kernel ran instead.  A call that returns before its
 * launch (bad arguments, a level without boxes) leaves the record as it was.  Returns non-zero for a null argument.  Diagnostic (tests). */
int pa_filter_last_launch(const pa_ctx*, int32_t info[8]);
/* filterPlt.cpp:174-203 ghost fill pieces */
int pa_foextrap(pa_ctx*, pa_mf*, int comp, int ncomp, int ng);
int pa_fillpatch_two_levels(pa_ctx*, pa_mf* fine, const pa_mf* crse, int comp, int ncomp, int ng, int ratio,
                            int interp_type);

/* The ghost fill of a whole hierarchy in three launches: pa_fill_boundary of every level, pa_fillpatch_two_levels of every level
 * pair, and (foextrap != 0) pa_foextrap of every level -- filterPlt.cpp:159-203 with foextrap, isosurface.cpp:1468-1524 (PCInterp,
 * interp_type 0) without.  mfs[l] on level l (coarse first), ngs[l] ghost layers on level l.  Results identical to the per-level
 * calls (no step of a level reads what another level's step writes); sharded levels take the per-level calls. */
int pa_fill_ghosts_hierarchy(pa_ctx*, int nlev, pa_mf* const* mfs, int comp, int ncomp, const int32_t* ngs, int ratio, int interp_type, int foextrap);

/* ---------------------------------------------------------------- isosurface
 * isosurface.cpp:1531-1592 for one FAB: state = 3 coordinate comps + fields,
 * mask (<0 = covered by a finer level), loop = box of cube base points.
 * pa_mc_count_fab classifies and counts (wave ballot + popcount); pa_mc_emit_fab
 * writes vertices in the reference's vertCache (std::map<Edge>) order and
 * triangles in cube traversal order; both deterministic.  Synchronous. */
int pa_mc_count_fab(pa_ctx*, pa_box loop, const pa_fab* state, const pa_fab* mask, int isocomp, double isoval,
                    int64_t* nvert, int64_t* ntri);
int pa_mc_emit_fab(pa_ctx*, pa_box loop, const pa_fab* state, const pa_fab* mask, int isocomp, double isoval,
                   double* dev_verts /* [nvert][ncomp] */, int32_t* dev_vkeys /* [nvert][6] */,
                   int32_t* dev_tris /* [ntri][3] */, int64_t nvert, int64_t ntri);
/* The same for every FAB of a level in one pass (the whole MFIter loop of isosurface.cpp:1531-1592).
 * pa_iso_mask_level: mask = 1, and -1 on every cell (ghost cells included) covered by the next finer level
 * (isosurface.cpp:1540-1563; fine = NULL: nothing covered).  pa_mc_level: state and mask are multifabs of one
 * level with the same ghost width; loops[b] = cube base points of FAB b (lo > hi: FAB skipped).  Per-FAB results
 * are identical to pa_mc_count_fab / pa_mc_emit_fab and are concatenated in box order: FAB b owns vertices
 * [sum_{b'<b} nvert[b'], +nvert[b]) and its triangles hold FAB-local vertex ids.  The three output arrays are
 * parts of ONE device allocation made by the library whose base is *dev_verts (all NULL when the level has no
 * surface): release it with pa_device_free(*dev_verts) only.  Synchronous. */
int pa_iso_mask_level(pa_ctx*, pa_mf* mask, int comp, const pa_level* fine, int ratio);
/* isosurface.cpp:1458-1465: comps comp0..comp0+2 of every cell of every grown FAB = its cell-centre coordinates,
 * (index + 0.5) * dx + prob_lo in that operation order (what FillBoundary / FillPatch then overwrite in ghost cells) */
int pa_iso_coords_level(pa_ctx*, pa_mf* state, int comp0);
int pa_mc_level(pa_ctx*, const pa_mf* state, const pa_mf* mask, int mcomp, const pa_box* loops /* host [nboxes] */,
                int isocomp, double isoval, int64_t* nvert /* host [nboxes] */, int64_t* ntri /* host [nboxes] */,
                double** dev_verts /* [sum nvert][ncomp] */, int32_t** dev_vkeys /* [sum nvert][6] */,
                int32_t** dev_tris /* [sum ntri][3] */);
/* AMREX_SPACEDIM == 2 builds of the reference (Segmentise, isosurface.cpp:303-406; the loop :1574-1582): a 2-D level
 * is stored as ONE plane of cells, k = 0 (boxes lo[2] = hi[2] = 0; ghost planes in z are ignored); state = 2
 * coordinate components + fields; loops[b] = square base points, lo[2] = hi[2] = 0.  Vertices in vertCache order
 * ((j, i) of the edge's lower endpoint, x before y), segments in traversal order, as rows of THREE int32
 * (id0, id1, -1) with FAB-local vertex ids; everything else as pa_mc_level (one allocation, base *dev_verts). */
int pa_msq_level(pa_ctx*, const pa_mf* state, const pa_mf* mask, int mcomp, const pa_box* loops /* host [nboxes] */,
                 int isocomp, double isoval, int64_t* nvert /* host [nboxes] */, int64_t* nseg /* host [nboxes] */,
                 double** dev_verts /* [sum nvert][ncomp] */, int32_t** dev_vkeys /* [sum nvert][6] */,
                 int32_t** dev_segs /* [sum nseg][3] */);
/* The same two calls with the mask of isosurface.cpp:1540-1563 evaluated inside the cell pass instead of read from a
 * multifab: a cell is masked iff its refined image has an owner on `fine` (periodic images included; fine = NULL:
 * nothing is masked, as when the distance function is built).  Halves the bytes the pass reads. */
int pa_mc_level_fine(pa_ctx*, const pa_mf* state, const pa_level* fine, int ratio, const pa_box* loops, int isocomp,
                     double isoval, int64_t* nvert, int64_t* ntri, double** dev_verts, int32_t** dev_vkeys,
                     int32_t** dev_tris);
int pa_msq_level_fine(pa_ctx*, const pa_mf* state, const pa_level* fine, int ratio, const pa_box* loops, int isocomp,
                      double isoval, int64_t* nvert, int64_t* nseg, double** dev_verts, int32_t** dev_vkeys,
                      int32_t** dev_segs);
/* The level loop of isosurface.cpp:1434-1728 as ONE call: pa_mc_level_fine on every level of the hierarchy, with the cell
 * passes and counts of all levels enqueued back to back, ONE read-back of the per-FAB counts and ONE pooled allocation for
 * the surfaces of all levels, whatever nlev is (per level the reference pays an MFIter loop; here a level costs no host
 * round trip of its own).  The call does NOT wait for the surfaces: it returns with them complete in stream order, so
 * pa_memcpy_d2h and every later call on the context see them; the single-level calls above return after a synchronisation.
 * states[l] lives on level l; fine_mask[l] != 0: cells covered by level l + 1 are masked (isosurface.cpp:1540-1563; null:
 * nothing is masked); loops[l] / nvert[l] / ntri[l]: host arrays over the FABs of level l.  dev_verts[l] / dev_vkeys[l] /
 * dev_tris[l] (host arrays of nlev pointers) point into *block (null for a level without surface); free *block with
 * pa_device_free.  Per-level results are identical to pa_mc_level_fine's. */
int pa_mc_hierarchy_fine(pa_ctx*, int nlev, const pa_mf* const* states, const int32_t* fine_mask, int ratio,
                         const pa_box* const* loops, int isocomp, double isoval, int64_t* const* nvert, int64_t* const* ntri,
                         double** dev_verts, int32_t** dev_vkeys, int32_t** dev_tris, void** block);
/* pa_mc_hierarchy_fine WITHOUT the three coordinate components: fields[l] holds only the plotfile components (the iso field at
 * isocomp + the mapped ones, ghost cells filled by pa_fill_ghosts_hierarchy with PCInterp).  The coordinates isosurface.cpp:1458-1465
 * stores per cell and :1468-1478 FillBoundaries / FillPatches in ghost cells are a function of the cell index and of which level
 * covers the cell -- (i + 0.5) dx + plo where the level itself covers it (through periodic images too), the coarse parent's centre
 * in every other ghost cell -- so the vertex kernels form them in registers, with the operations of pa_iso_coords_level: vertices
 * ([nvert][3 + ncomp]), keys and triangles are bit-identical to pa_mc_hierarchy_fine's on the reference-shaped state, and 24 B
 * per cell (+ their ghost fills) are never written.  3-D levels; level l must be the `ratio` refinement of level l - 1. */
int pa_mc_hierarchy_xyz(pa_ctx*, int nlev, const pa_mf* const* fields, const int32_t* fine_mask, int ratio, const pa_box* const* loops,
                        int isocomp, double isoval, int64_t* const* nvert, int64_t* const* ntri, double** dev_verts, int32_t** dev_vkeys,
                        int32_t** dev_tris, void** block);
/* isosurface.cpp:1687-1726 + 1751-1812 on the device: the global node / element sets from the per-FAB fragments, in
 * insertion order (level by level, FAB by FAB: exactly the fragments whose ntri > 0, as the reference skips the others).
 * A vertex within 1e-15 (Euclidean) of an earlier node IS that node (Node::operator<, :834-873), otherwise a new node
 * numbered by insertion rank; elements = node-id triples rotated so the smallest id leads, degenerate ones dropped,
 * unique, sorted (std::set<Element>, :877-927).  verts / tris are DEVICE pointers ([nvert][ncomp] with the position in
 * the first three components; [ntri][3] fragment-local vertex ids) -- e.g. slices of what pa_mc_level* returned.
 * Outputs: two device allocations ([nnodes][ncomp], [nelts][3]; release each with pa_device_free; NULL when empty).
 * Returns 0, or 1 on error, or 2 when some cluster of nearby vertices is not transitive under the tolerance (a ~ b,
 * b ~ c, a !~ c): the reference's answer then depends on the insertion chain, nothing is returned, and the caller runs
 * the sequential merge (tools/common/pa_isomerge.h).  Synchronous. */
typedef struct { const double* verts; int64_t nvert; const int32_t* tris; int64_t ntri; } pa_iso_frag;
int pa_iso_merge(pa_ctx*, int nfrag, const pa_iso_frag* frags /* host array */, int ncomp, int64_t* nnodes,
                 double** dev_nodes, int64_t* nelts, int32_t** dev_elts);
const uint16_t* pa_mc_edge_table(void); /* [256] host */
const int8_t*   pa_mc_tri_table(void);  /* [256][16] host */

/* ----------------------------------------------- isosurface: distance function
 * isosurface.cpp:1595-1655 (build_distance_function).  One pa_sdf_grid = one call of
 * make_level_set3(faceList, vertList, local_origin, dx, ni, nj, nk, phi_grid) (isosurface.cpp:1625,
 * Tools/SDFGen/makelevelset3.cpp:118-185): unsigned distance, in the reference's float arithmetic and
 * visiting order, from grid point (i,j,k) = origin + (i,j,k)*dx to the triangle mesh; phi is
 * [k][j][i] with i fastest (Array3f order), ni*nj*nk floats.  All pointers are DEVICE pointers; tri
 * holds 3 vertex indices per triangle, x 3 floats per vertex.  A batch of grids runs concurrently
 * (one workgroup per grid for the sweeps).  Asynchronous on the context's stream. */
typedef struct {
  int64_t ntri;  const uint32_t* tri;
  int64_t nvert; const float* x;
  float origin[3]; float dx;
  int32_t n[3];
  float* phi;
} pa_sdf_grid;
int pa_sdf_level_set3(pa_ctx*, int ngrids, const pa_sdf_grid* grids /* host array */, int exact_band /* reference default 1 */);
/* isosurface.cpp:1637-1650: dist(i,j,k,dcomp) = sgn * min(dmax, phi(i-lo,j-lo,k-lo)) over vbox (the
 * distance FAB's box incl. ghosts), sgn = state(i,j,k,isocomp) < isoval ? -1 : +1 */
int pa_sdf_signed_fab(pa_ctx*, pa_box vbox, const float* dev_phi, const pa_fab* state, int isocomp, double isoval,
                      double dmax, pa_fab* dist, int dcomp);

/* ------------------------------------------------------------- streamlines
 * partStream.cpp:121-207 / StreamPC.cpp: two lines per seed (line 2s forward, 2s+1 backward) of nsteps
 * points each, RK4 with step dt (= hRK * finest dx in the tool) through the trilinear interpolant of
 * vfield[lev] comps vcomp..vcomp+2, whose nGrow ghost layers the caller has filled (FillPatch with
 * piecewise-constant interpolation + FillBoundary, partStream.cpp:160-177).  A line interpolates from the
 * grid it was last assigned to; all lines are re-assigned to the finest level containing them whenever one
 * leaves its grid grown by nGrow-1 (StreamPC.cpp:88-141).  seeds: host [nseed][3]; dev_pos: device
 * [2*nseed][nsteps][3].  Returns non-zero where the reference aborts with "bad RK".  Synchronous. */
int pa_stream_trace(pa_ctx*, int nlev, pa_mf* const* vfield, int vcomp, int64_t nseed, const double* seeds, int nsteps,
                    double dt, double* dev_pos, int32_t* nredist /* may be NULL */);
/* The same with the lines dealt to the ranks of the context's transport (partStream.cpp under MPI: the particles live on
 * the ranks, StreamPC.cpp:88-141 Redistribute is collective): every rank holds the WHOLE vector field (levels created
 * unsharded) and traces its own seeds; with share_flags != 0 the per-step "a line has left its grid" flag is max-reduced
 * over the ranks, so every line equals the one-rank run's.  Every rank must call it, also with nseed = 0. */
int pa_stream_trace_ranks(pa_ctx*, int nlev, pa_mf* const* vfield, int vcomp, int64_t nseed, const double* seeds, int nsteps,
                          double dt, double* dev_pos, int32_t* nredist /* may be NULL */, int share_flags);

/* ------------------------------------------------------------- gradient streamlines (stream.cpp / stream_nd.f90)
 * Lines of the progress variable's gradient (or of the velocity, traceAlongV) seeded on isosurface nodes, one
 * (level, file box) per seed; each line only reads its own box's FAB.  The arithmetic is stream_nd.f90's:
 * ntrpv (closed [plo, phi] test, trilinear sum in the Fortran's term order), vnrml (normalise only if
 * |v|^2 > (double)1.e-12f, divide by the square root), RK4 ending x + (k1+k4)/6 + (k2+k3)/3.
 *
 * One MFIter iteration of stream.cpp:920-925, vtrace(...) with device pointers: T holds nT components
 * (progress first) on T->lo..T->hi; loc: nloc node coordinates, component-major (loc[c * nloc + j]); ids:
 * n_ids 1-based node ids (device); g: 3 components, WRITTEN with g = T(i+1) - T(i-1) per direction over
 * g->lo..g->hi when computeVec = 1, read as the vector field when 0 (g may then alias components of T);
 * strm: ncs = 3 + nT components on (0, -nRKh, 0)..(n_ids-1, nRKsteps-1-nRKh, 0) = strm->lo..strm->hi;
 * dx / plo / phi / hRK: host values as vtrace gets them.  *errFlag: vtrace's final errFlag (0, 1 "Problem
 * with interpolation", 2 / 4 a backward / forward line was cut short -- the LAST such event of the box, as
 * the Fortran assigns it).  Synchronous. */
int pa_vtrace_fab(pa_ctx*, const pa_fab* T, int32_t nT, const double* loc, int64_t nloc, const int32_t* ids, int32_t n_ids,
                  pa_fab* g, int32_t computeVec, pa_fab* strm, int32_t ncs, const double dx[3], const double plo[3],
                  const double phi[3], double hRK, int32_t* errFlag);
/* State of stream.cpp:796-884 for the whole hierarchy, in place, levels coarse to fine: state[l] holds the
 * plotfile's data in the valid cells (components 0..ncomp-1, nGrow = state[l]'s ghost width) and gets every
 * ghost cell set as FillBoundary -> FillCFgrowCells (piecewise-constant copy of the PREPARED coarse level,
 * its ghost cells included) -> FillBoundary -> FixOOB leave it: cells outside the index domain 0 (periodic
 * images too: is_per has no effect), cells of another box of the level its valid value, other cells the
 * coarse value of their parent (0 on level 0).  The refinement ratio of each level pair is taken from the
 * domains.  Returns non-zero where the reference would read a coarse value it never set (a parent cell that
 * no coarse FAB holds, or that a fine box partly covers).  Asynchronous on the context's stream. */
int pa_streamgrad_prepare(pa_ctx*, int nlev, pa_mf* const* state);
/* vtrace of every (level, box) that holds seeds, in ONE launch, two threads per seed (backward, forward).
 * state: pa_streamgrad_prepare's result, nT = its component count, vcomp: first velocity component
 * (traceAlongV) or -1 (the gradient of component 0, formed on the fly = the reference's g); nodes: device,
 * component-major [3][nnodes]; boxes of all levels numbered globally (level 0's first, file order);
 * box_start: host CSR [nbox_total + 1] of the lines per box; ids: device, 1-based node id per line in that
 * order; strm: device, the Str FABs of the boxes with lines back to back (box g at box_start[g] * nRKsteps *
 * (3 + nT) doubles, i fastest, then n + nRKh, component outermost).  box_flag: host [nbox_total], vtrace's
 * final errFlag per box (0 for boxes without lines).  Synchronous. */
int pa_streamgrad_trace(pa_ctx*, int nlev, pa_mf* const* state, int vcomp, int64_t nnodes, const double* nodes,
                        const int64_t* box_start, const int32_t* ids, int nRKsteps, double hRK, double* strm,
                        int32_t* box_flag);
/* The alternate surface of stream.cpp (buildAltSurf): build_surface_at_isoVal (:1841-2074), add_thermal_thickness_to_surf
 * (:1554-1838), add_cold_strain_to_surf (:1369-1552) and add_angle_to_surf (:1211-1367) for every line of the trace, one launch.
 * A line is column i of a Str box, j = lo .. hi with lo = -nRKh, hi = nRKsteps - 1 - nRKh, nRKh = (nRKsteps - 1) / 2.
 * locate(c, val) -> (lIdx, rIdx, frac): (lo, lo + 1, 0) when val <= v(lo) or a comparison meets a NaN [branch 0]; (hi - 1, hi, 1)
 * when val > v(hi) [3]; else the first j with val >= v(j) && val < v(j + 1) and frac = (val - v(j)) / (v(j + 1) - v(j)), 0 when
 * the two are equal [1]; (hi, hi, 0) when no segment qualifies [2].  lerp(c) = xL + (xR - xL) * frac; arc = the signed distance
 * along the line from j = 0, summed in increasing j with the located segment weighted by frac (or 1 - frac below j = 0).
 * strm, box_start, ids: as pa_streamgrad_trace takes and writes them (strm and ids on the device, box_start on the host, nbox
 * boxes of all levels), ncs components per point.  out: device [nout][nNodes], node id - 1 of the line decides the column:
 *   X Y Z and the ncarry components `carry` = lerp at locate(isoComp, altVal); then arc there;
 *   thickComp >= 0: arc(locate(thickComp, thickHi)) - arc(locate(thickComp, thickLo));
 *   TComp >= 0: lerp(strainComp) at locate(TComp, TVal);
 *   addAngle: dx[2] / |dx| with dx = x(h - 1) - x(h + 1), h = (int)(0.5 * (lo + hi)) -- the COSINE: the caller applies acos.
 * branch: device int8 [nquery][nNodes] or NULL: the branch 0 .. 3 above of the queries alt, thickLo, thickHi, T (those asked for,
 * in this order).  Every operation is an IEEE add, multiply, divide or sqrt in the reference's association: the serial code's bits.
 * Fails (pa_last_error) on a component outside 0 .. ncs - 1, nRKsteps < 3, more than 8 carried components, a box_start that
 * does not ascend from 0, and a node id outside 1 .. nNodes (checked on the device before anything is written).  Synchronous. */
typedef struct {
  int32_t isoComp;            /* the progress variable among the line's components */
  double  altVal;
  int32_t ncarry, carry[8];
  int32_t thickComp;          /* < 0: no thickness */
  double  thickLo, thickHi;
  int32_t TComp, strainComp;  /* TComp < 0: no cold strain */
  double  TVal;
  int32_t addAngle;
} pa_streamalt_params;
int pa_streamalt_run(pa_ctx*, int32_t nbox, const int64_t* box_start, const int32_t* ids, const double* strm, int32_t ncs,
                     int32_t nRKsteps, int64_t nNodes, const pa_streamalt_params* p, double* out, int8_t* branch);

/* ------------------------------------------------------------- sampling along streamlines (sampleStreamlines.cpp / _nd.f90)
 * The arithmetic is sampleStreamlines_nd.f90's: ntrpv WITHOUT the [plo, phi] test (b = FLOOR((x-plo)/dx - 0.5), n clamped
 * to [0, 1], the trilinear sum in the Fortran's term order); a point fails when b is outside [lo, hi - 1] of the data
 * (the Fortran's b > hi test reads b + 1 outside the FAB at b == hi: a failure here).
 *
 * One MFIter iteration of sampleStreamlines.cpp:745-748, interpstream(...) with device pointers: loc = the path FAB (nl >= 3
 * components, X / Y / Z first; its box holds j = 0, the seeds), fab = the staged data (np components), strm = np components
 * on loc's box (the caller points it at component dComp of the sample FAB).  *status: 0, 1 "Seed not in valid region for
 * interp", 2 "Interp bad, increase nGrow" -- the FIRST failing point in the Fortran's loop order decides (k, then j = 0 down
 * to lo, then j = 1 .. hi, i innermost); failing points write nothing.  Synchronous. */
int pa_interpstream_fab(pa_ctx*, const pa_fab* loc, int32_t nl, const pa_fab* fab, int32_t np, pa_fab* strm, const double dx[3],
                        const double plo[3], int32_t* status);
/* set_distance (sampleStreamlines.cpp:772): res(i, j, k) = the arc length from the seed along line i, negative for j < 0;
 * res(i, 0, 0) = 0 (k = 0 hard-coded as in the Fortran: the box must hold j = 0 and k = 0).  res on loc's box.  Synchronous. */
int pa_set_distance_fab(pa_ctx*, const pa_fab* loc, pa_fab* res);
/* sample_pathlines + set_sample_location + set_sample_distance (sampleStreamlines.cpp:176-194) for the whole hierarchy, without
 * the staged FABs: data[l] = components 0..K-1 of the plotfile on level l (any ghost width; only FABs that some grown seed box
 * can reach need to hold data); file_dx: host [nlev][3], the plotfile header's dx; nbox: host [nlev] Str boxes per level;
 * str_boxes: host [nbt][6] (lo, hi), each (ilo, jlo, 0)..(ihi, jhi, 0) with jlo <= 0 <= jhi; has_lines: host [nbt], non-zero
 * for the boxes with inside_nodes (only those are sampled); bbox: host [nbt][6], the grown seed box of find_containing_box
 * (:503-536, :620-621); xyz: device, X / Y / Z of box g at 3 * o_g doubles (component-major, i fastest, then j), o_g = the
 * points of the boxes before g; out: device, ncout components of box g at ncout * o_g.  Writes components dcomp .. dcomp+K-1
 * (0 in boxes without lines) and, with with_xyzd != 0, components 0..2 = X / Y / Z and 3 = distance_from_seed of every box.
 * A corner cell of level lev inside the domain takes the value of the finest level <= lev that holds it (FillVar,
 * piecewise-constant); outside, its periodic image's (one domain length at most, is_per directions) or -20000.
 * box_fail: host [nbt], 0 or the status of pa_interpstream_fab for that box.  Synchronous. */
int pa_streamsample_run(pa_ctx*, int nlev, pa_mf* const* data, int32_t K, const double* file_dx, const double plo[3],
                        const int32_t is_per[3], const int32_t* nbox, const int32_t* str_boxes, const int32_t* has_lines,
                        const int32_t* bbox, const double* xyz, double* out, int32_t ncout, int32_t dcomp, int32_t with_xyzd,
                        int32_t* box_fail);
/* hipMemGetInfo of the context's device: the tools size their passes by it */
int pa_device_mem_info(pa_ctx*, int64_t* free_bytes, int64_t* total_bytes);

/* ------------------------------------------------------------- binned statistics (jpdf.cpp / conditionalMean.cpp)
 * One accumulator object (pa_hist) lives across the levels of a plotfile; the add_level calls take ONE level at a time -- its data,
 * the next finer level (boxes only; NULL: nothing is covered) and the refinement ratio -- so only one level's components have to be
 * resident.  A cell counts when its refined image has no owner on `finer` (jpdf.cpp:373-387, :472; conditionalMean.cpp:246-258, :267).
 * NUMERICS: the reference adds cell after cell in double precision; here every sum is a 192-bit fixed-point integer (quantum
 * 2^-157 x the power of two above the magnitude declared at begin) added with 64-bit integer atomics and rounded ONCE when read.
 * Bin indices, counts, hits, minima and maxima are exact; a sum S of n terms t satisfies |S - sum t| <= 2^-53 |sum t| (+ n quanta
 * for terms below 2^-105 of the declared magnitude), the same bits on every run and for every tiling or box order of the level.
 * A term larger than twice the declared magnitude, or not finite, makes the read call fail.  One rank; 3-D levels.
 * add_level is asynchronous on the context's stream unless it returns counts; begin and read are synchronous. */
#define PA_STATS_MAXV 8
typedef struct pa_hist pa_hist;
typedef struct {
  int32_t nload;            /* loaded variables: components 0 .. nload-1 of the multifab */
  int32_t do_stoichiometry; /* one more variable, index nload: 0.5 * sumH / sumO over the loaded ones (jpdf.cpp:410-418) */
  double  hlist[PA_STATS_MAXV], olist[PA_STATS_MAXV];
  double  vmin[PA_STATS_MAXV], vmax[PA_STATS_MAXV]; /* axis of every variable (jpdf.cpp:297-326); vmax == vmin is refused */
  int32_t do_conditioning;  /* 0, 1: c, 2: c (1 - c) (jpdf.cpp:476-487) */
  int32_t cvar, norm_cval;
  double  cnorm_min, cnorm_max, cmin, cmax;
  int32_t uncombined;       /* 1: the plain kernel, one set of global atomics per cell (measurement; identical bits) */
} pa_jpdf_params;
/* AmrData::MinMax of several components of one level in one launch (jpdf.cpp:297-306): every valid cell, cells covered by a finer
 * level included.  ncomps <= 16.  Synchronous. */
int pa_minmax_comps_level(pa_ctx*, const pa_mf* s, int ncomps, const int32_t* comps, double* mn, double* mx);
/* jpdf.cpp:328-337: the three accumulators bin / binX1 / binX2 of all nvars (nvars - 1) / 2 pairs, pair order as the loops at :427-428 */
pa_hist* pa_jpdf_create(pa_ctx*, int nvars, int nbins);
/* zero the accumulators for a new plotfile and fix their scales: vol_max = the largest cell volume that will be added (level 0's),
 * vabs[v] >= |value| of variable v (max(|vMin|, |vMax|) of the data; 2 for the stoichiometry) */
int pa_jpdf_begin(pa_ctx*, pa_hist*, double vol_max, const double* vabs /* [nvars] */);
/* jpdf.cpp:440-522 for one level: ONE pass over the cells bins all pairs (up to 6 per pass).  Bin index (int)(nBins*(v-vMin)/(vMax-vMin));
 * a quotient >= nBins (+inf too) clamps high and counts, <= -1 clamps low and counts, NaN skips the cell for that pair and counts.
 * outside: host [npairs][4] = v1l v1g v2l v2g of THIS level (:516-521), nan_cells: host [npairs]; either may be NULL. */
int pa_jpdf_add_level(pa_ctx*, pa_hist*, const pa_mf* vars, const pa_level* finer, int ratio, double vol, const pa_jpdf_params*,
                      int64_t* outside, int64_t* nan_cells);
/* raw sums (before jpdf.cpp:571-589), [npairs][nbins * nbins] each, bin v1i * nbins + v2i */
int pa_jpdf_read(pa_ctx*, const pa_hist*, double* bin, double* binx1, double* binx2);
/* conditionalMean.cpp:97-106: binHits (64-bit here), binVals, binValsSq and, with_minmax, binMinVals / binMaxVals; navg <= 8 per object */
pa_hist* pa_condmean_create(pa_ctx*, int navg, int nbins, int with_minmax);
/* zero + scales: weight_max = the largest cell weight (level 0's), vabs[a] >= |value| of averaged component a */
int pa_condmean_begin(pa_ctx*, pa_hist*, int64_t weight_max, const double* vabs /* [navg] */);
/* conditionalMean.cpp:260-296 for one level: comps holds the bin component first, then the navg averaged ones; domain = the bounds
 * box in this level's index space (:183-191, :226); a cell with binMin <= binVal < binMax goes to bin (int)(nBins*(binVal-binMin)/
 * (binMax-binMin)) with sums weight*val and (weight*val)*val; an index outside [0, nBins) is the reference's "Bad bin" abort: the
 * read call fails.  uncombined != 0: the plain kernel (measurement; identical bits). */
int pa_condmean_add_level(pa_ctx*, pa_hist*, const pa_mf* comps, const pa_level* finer, int ratio, const pa_box* domain,
                          int64_t weight, double bin_min, double bin_max, int uncombined);
/* hits [nbins]; sum, sumsq, mn, mx [nbins][navg] (mn / mx may be NULL without with_minmax; 0 in empty bins) */
int pa_condmean_read(pa_ctx*, const pa_hist*, int64_t* hits, double* sum, double* sumsq, double* mn, double* mx);
void pa_hist_destroy(pa_hist*);

/* ------------------------------------------------------------- composite integrals (integral.cpp / rmsVel.cpp)
 * One accumulator object (pa_integral) lives across the levels of a plotfile, as pa_hist does.  It projects the uncovered cells of
 * every level onto a point (kind 3: volume integral), a line along `dir` (kind 2: plane integrals) or the plane normal to `dir`
 * (kind 1: line integrals), at the resolution of the FINEST level that is integrated: 1, ldir or ldir1 x ldir2 slots, dir1 = (dir+1)%3
 * the rows and dir2 = (dir+2)%3 the columns of the plane.  It holds nvars + 1 rows: row 0 the measure (volume, area, length), rows
 * 1 .. nvars the sums of w * v_n and, with `squares`, rows nvars+1 .. 2 nvars the sums of (v_n * v_n) * w.  A cell of a level whose
 * cells are R_l fine cells wide adds to the R_l (kind 2) or R_l x R_l (kind 1) fine slots under it.
 * NUMERICS: the contract of the binned statistics above -- 192-bit fixed-point sums scaled from the magnitudes declared at begin,
 * integer atomics, ONE rounding at read, the same bits for every run, tiling, box order and kernel variant; |S - sum t| <= 2^-53
 * |sum t| (+ n quanta).  Row 0 is a cell count per level times the level's weight, summed exactly and rounded once.  A term that is
 * not finite sets a sticky flag of its slot and row; read returns what IEEE addition gives in any order: NaN if a NaN or both
 * infinities were seen, else the infinity that was seen, else the finite sum.  A finite term larger than twice the declared
 * magnitude makes read fail.  One rank; 3-D levels.  add_level is asynchronous on the context's stream; begin and read are synchronous. */
typedef struct pa_integral pa_integral;
/* integral.cpp:442-449, :497-501, :520 (outdata) and rmsVel.cpp:82 (the seven sums): nvars <= 8, kind 1..3, dir 0..2 (unused by kind 3),
 * domain = the index box of the finest level's problem domain (AmrData::ProbDomain()[finestLevel]) */
pa_integral* pa_integral_create(pa_ctx*, int nvars, int kind, int dir, const pa_box* domain, int squares);
/* zero + scales: w_max = the largest weight that will be added (level 0's), vabs[n] >= |value| of variable n */
int pa_integral_begin(pa_ctx*, pa_integral*, double w_max, const double* vabs /* [nvars] */);
/* integrate1d / 2d / 3d for one level (integral.cpp:24-44, :85-101, :129-140) and rmsVel.cpp:83-115: vars holds the nvars variables as
 * components 0 .. nvars-1; a cell counts when its refined image has no owner on `finer` (integral.cpp:425-436; NULL: every cell) and,
 * with ccomp >= 0, when cmin <= v_ccomp < cmax (a NaN fails).  R_l = the product of the refinement ratios from this level to the
 * finest one: the level's domain times R_l must be the domain given at create.  w = dx*dy*dz (kind 3), dx[dir1]*dx[dir2] (kind 2) or
 * dx[dir] (kind 1) of this level.  uncombined != 0: one set of global atomics per cell (measurement; identical bits). */
int pa_integral_add_level(pa_ctx*, pa_integral*, const pa_mf* vars, const pa_level* finer, int ratio, int R_l, double w, int ccomp,
                          double cmin, double cmax, int uncombined);
/* the number of output slots per row */
int64_t pa_integral_slots(const pa_integral*);
/* the raw sums, before the avg division (integral.cpp:51-58, :107-112, :143-147; rmsVel.cpp:116-122): out[rows][slots] */
int pa_integral_read(pa_ctx*, const pa_integral*, double* out);
void pa_integral_destroy(pa_integral*);

/* ------------------------------------------------------------- surface PDFs (binMEF.cpp)
 * The area-weighted PDF (one binned component) or joint PDF (up to 4) of node fields over a triangulated surface.  Every triangle is
 * clipped against the bin edges of each binned component (processTriangle, binMEF.cpp:231-331); each piece adds its area to the bin
 * it lies in.  The pieces are the reference's, operation for operation; the sums are 192-bit fixed-point integers scaled from the
 * largest element area and rounded once at read: the same bits for every order of the elements, every list capacity and with
 * uncombined.  An element with a value that is not finite in x, y, z, a binned component or (condApply) the condition component is
 * skipped and counted.  A split fraction outside [0, 1] (the reference's AMREX_ALWAYS_ASSERT, :121 / :159) makes read fail.
 * One GPU.  All arrays are HOST memory; add_surface uploads what it needs and returns when the surface has been binned. */
typedef struct pa_surfbin pa_surfbin;
/* binMEF.cpp:417-458, :477-489: nc <= 4 binned components with nbins[j] bins over [bin_min[j], bin_max[j]]; at most 2^24 bins in all.
 * work_items: the capacity of the work list in triangles (248 bytes each, two lists); 0 = the default (2^19).  A small value forces the
 * list to be worked off in slices (same bits).  4 R^2 / 3 with R = the sum of nbins[j] + 3 suffices (in exact arithmetic; DESIGN.md 3.9 names the rounding
 * case the proof leaves open); a smaller list works while the triangles span few bins, and add_surface fails with a message, never
 * with a write out of bounds, only when the children of one work item do not fit. */
pa_surfbin* pa_surfbin_create(pa_ctx*, int nc, const int32_t* nbins, const double* bin_min, const double* bin_max, int64_t work_items);
/* zero the table and fix the scale: area_max >= the area of every element that will be added until read (pa_surfbin_max_area of
 * each surface, the largest).  The scale cannot change once a sum has begun and a table may take several surfaces, so the CALLER
 * computes the magnitude and passes it here; add_surface does not.  A larger area sets the overflow flag, and read fails. */
int pa_surfbin_begin(pa_ctx*, pa_surfbin*, double area_max);
/* triangleArea (binMEF.cpp:46-60) of every element, the largest finite one; -1 when an element names a node outside 1 .. nnodes */
double pa_surfbin_max_area(int64_t nnodes, const double* x, const double* y, const double* z, int64_t nelts, const int32_t* elts);
/* the element loop (binMEF.cpp:522-540): comps[j] = the node values [nnodes] of binned component j, cond = those of condComp (NULL
 * without cond_apply), elts = [nelts][3] node numbers, 1-based.  cond_apply / cond_sgn / cond_val: :206-226, :465-475; area_eps: :244, :504.
 * uncombined != 0: one set of global atomics per leaf (measurement; identical bits). */
int pa_surfbin_add_surface(pa_ctx*, pa_surfbin*, int64_t nnodes, const double* x, const double* y, const double* z, const double* const* comps,
                           const double* cond, int64_t nelts, const int32_t* elts, int cond_apply, int cond_sgn, double cond_val, double area_eps,
                           int uncombined);
/* the table the output of binMEF.cpp:594-670 is made from: area, hits [prod nbins], first component slowest (the order of the
 * reference's map); a bin is nonempty when hits > 0.  total_area: the sum of :535; outside_area: areaOutsideCondition (:265).
 * counters [8] (may be NULL): NmyTriangles (:257), skipped elements, rounds, peak list occupancy, sliced rounds, work items walked,
 * elements, list capacity. */
int pa_surfbin_read(pa_ctx*, const pa_surfbin*, double* area, int64_t* hits, double* total_area, double* outside_area, int64_t* counters);
void pa_surfbin_destroy(pa_surfbin*);

/* ------------------------------------------------------------- hex-element mesh of a hierarchy (amrToFE.cpp)
 * The centres of all uncovered cells of the levels become nodes, every 2 x 2 x 2 block of them an 8-node brick; at a coarse-fine
 * interface the ghost corners of the fine bricks collapse onto coarse cell centres.  Node ids, element order and connectivity are the
 * reference's (std::map<Node,int> filled level -> grid -> cell, std::set<Element> in Element::operator< order), built by compaction
 * and radix sorts; the same input gives the same bytes.  One GPU, 3-D levels, nGrowPer = 0.  The calls are
 * synchronous except pa_fe_gather, which is asynchronous on the context's stream. */
typedef struct pa_fe pa_fe;
/* amrToFE.cpp:374-452 and :465-633.  levels: the file's BoxArrays (up to 8); ratios [nlev - 1]; subbox: the box key in level-0 indices
 * (NULL: the domain; it is intersected with the domain, and refined level by level); a level no box of which touches its subbox ends the
 * hierarchy (:445-451; *nlev_used).  connect_cc = 0: one flat brick per node (:603, :626-633, :775-813), nnodes = 8 * nelts.
 * Fails (NULL, pa_last_error) where the reference misnumbers or writes out of bounds: a fine box that is not aligned to its ratio
 * (:499-507), a corner that lies in no grid ("Node not found in node map", :615-619), counts beyond int. */
pa_fe* pa_fe_build(pa_ctx*, int nlev, const pa_level* const* levels, const int32_t* ratios, const pa_box* subbox, int connect_cc,
                   int32_t* nlev_used, int64_t* nnodes, int64_t* nelts);
/* amrToFE.cpp:608-633: connData, [nelts][8] node numbers, 1-based, corners in the order of :585-592; a DEVICE array owned by the mesh */
int pa_fe_connectivity(pa_ctx*, const pa_fe*, const int32_t** dev_conn);
/* amrToFE.cpp:638-646: nodeVect, (level, i, j, k) of every node id, [*nids][4]; a DEVICE array owned by the mesh.  *nids is the number
 * of uncovered cells (= nelts without connect_cc) */
int pa_fe_nodes(pa_ctx*, const pa_fe*, int64_t* nids, const int32_t** dev_nodes);
/* amrToFE.cpp:711-814: tmpData in block ordering, dev_out [3 + ncomp][nnodes] (device): x, y, z = plo + (iv + 0.5) * dx with dx =
 * ProbSize / domain length of the node's level (:718-724), then components comps[0 .. ncomp-1] of the node's cell.  mfs[l]: a multifab
 * on levels[l] of the build (any ghost width), l < nlev_used. */
int pa_fe_gather(pa_ctx*, pa_fe*, int nlev, const pa_mf* const* mfs, int ncomp, const int32_t* comps, double* dev_out);
/* HIP-event times in ms of the build's stages -- number, tag, cubes, order -- and of the last gather; ncubes (may be NULL): cubes kept
 * before duplicate removal (tools/amrtofe_bench.py) */
int pa_fe_stage_times(pa_ctx*, const pa_fe*, double ms[5], int64_t* ncubes);
void pa_fe_destroy(pa_fe*);

/* ------------------------------------------------------------- stream tubes (streamTubeStats.cpp)
 * The three lines through the nodes of a surface triangle bound a stream tube; between consecutive line points it is a wedge.
 * DATA LAYOUT: the Str FABs of a streamSampleFile, all levels and boxes back to back (box g after the boxes before it): a buffer of
 * ncomp components holds box g at ncomp * off_g doubles, component-major, i (line in box) fastest, then j -- what
 * pa_streamsample_run takes for xyz.  xyz = such a buffer of the 3 coordinates; data = one of the components the call names.
 * NUMERICS: a thread owns a triangle or a line from its first point to its last; every expression keeps the reference's association
 * and every sum its order (j, then the CSR's column order), without floating-point atomics: the results are the serial code's bits
 * for any grouping of the components.  All calls are synchronous; arrays are device memory unless called "host".
 *
 * The tables of one stream directory: box_desc host [nbt][4] = (ni, nj, jlo, off_g) of every Str box of every level (build_nodeMap
 * :1256-1281 needs them flat); node_table host [nNodes][2] = (box g, line i) of node id n + 1; faceData host [nElts][3], 1-based.
 * Node ids outside 1 .. nNodes, boxes or lines out of range: NULL with pa_last_error set (the reference asserts in debug builds). */
typedef struct pa_tube pa_tube;
pa_tube* pa_tube_create(pa_ctx*, int32_t nbt, const int64_t* box_desc, int64_t nNodes, const int32_t* node_table, int64_t nElts,
                        const int32_t* faceData);
void pa_tube_destroy(pa_tube*);
/* The element loop of streamTubeStats.cpp:650-699 with wedge_volume_int / tetVol / wedge_surf_area (:850-873, :1003-1254): for every
 * triangle the wedges j = jlo .. jlo + nPtsOnStr - 2 in order; components 0 .. K-1 of data are integrated.  ints_raw [K][nElts] =
 * the sums (what :693-694 totals), ints_per_area [K][nElts] = the sums / area (:696-699).  with_geom != 0 also writes vol, area (the
 * triangle at j = 0) and wa [nElts] (:663-685; wa = area_wtAvg of component 0 of THIS call, 0 when K == 0): a caller that passes the
 * components in groups asks for them with the first group.  Every box with lines must hold j = 0 and the swept range (the reference
 * indexes without a check): checked on the host before any launch. */
int pa_tube_wedges(pa_ctx*, pa_tube*, const double* xyz, const double* data, int32_t K, int32_t jlo, int32_t nPtsOnStr,
                   int32_t with_geom, double* vol, double* area, double* wa, double* ints_raw, double* ints_per_area);
/* max_grad (:876-952) of component comp of data (ncomp components) along every line, over the box's whole j range: gradmax [nNodes].
 * use_eps == 0: a gradient counts across segments with L > maxs, the longest segment (the reference's test); != 0: L > 1.e-4 * maxs. */
int pa_tube_lines(pa_ctx*, pa_tube*, const double* xyz, const double* data, int32_t ncomp, int32_t comp, int32_t use_eps,
                  double* gradmax);
/* peak_val (:955-1001): the first maximum (strict >) of component pcomp along every line; peak_samples [nsample][nNodes] = the
 * components sample_comps (host, nsample <= 32) there; ok [nNodes] int32 = 0 when it sits at the first or last point of the line */
int pa_tube_peaks(pa_ctx*, pa_tube*, const double* data, int32_t ncomp, int32_t pcomp, int32_t nsample, const int32_t* sample_comps,
                  double* peak_samples, int32_t* ok);
/* node values to elements (:724-753): out [nv][nElts] = (a + b + c) / 3. of vals [nv][nNodes] at the element's nodes in order */
int pa_tube_node_means(pa_ctx*, pa_tube*, int32_t nv, const double* vals, double* out);
/* :739-742: out [nElts] = 1.0 where ok (int32 [nNodes]) holds at all three nodes, else 0.0 */
int pa_tube_node_all(pa_ctx*, pa_tube*, const int32_t* ok, double* out);
/* :703-713: out [nElts] = the values of component comp at the surface (j = 0) of the three nodes, summed from 0 in node order, / 3 */
int pa_tube_node_avg(pa_ctx*, pa_tube*, const double* data, int32_t ncomp, int32_t comp, double* out);
/* smoothVals (:274-298) nSmooth times over ping-pong buffers, neighbours from buildNodeNeighbors (:196-235): every other element that
 * shares a node, ascending, built on the device at the first call and kept with the tube.  nSmooth <= 0 copies vals.  out != vals. */
int pa_tube_smooth(pa_ctx*, pa_tube*, const double* vals, const double* area, int32_t nSmooth, double* out);
/* the neighbour lists as CSR, to the host: *nnz always; rowptr [nElts + 1] and cols [*nnz] where not NULL (tests) */
int pa_tube_neighbors(pa_ctx*, pa_tube*, int64_t* nnz, int64_t* rowptr, int32_t* cols);

/* ------------------------------------------------------------- selecting streamlines (streamScatter.cpp, stream2plt.cpp)
 * DATA LAYOUT and tables: those of the stream tubes above -- box_desc host [nbt][4] = (ni, nj, jlo, off_g), node_table host [nNodes][2] =
 * (box g, line i) of node id n + 1 (box -1: no box lists the id -- refused), data buffers flat, component-major, i fastest, then j.
 * The dense array of stream2plt ("final", finalMF of stream2plt.cpp:498-502) is device [component][point][line], line fastest.
 * NUMERICS: a thread owns a line from its first point to its last; every expression keeps the reference's association, every sum
 * its order in j, every comparison its literal form (>, <, std::max, std::min: NaN goes the serial code's way); no floating-point
 * atomics.  The results are the serial code's bits.  All calls are synchronous; arrays are device memory unless called "host".
 * Boxes, lines and components out of range fail on the host, before any launch, with pa_last_error set. */
typedef struct pa_ssel pa_ssel;
pa_ssel* pa_ssel_create(pa_ctx*, int32_t nbt, const int64_t* box_desc, int64_t nNodes, const int32_t* node_table);
void pa_ssel_destroy(pa_ssel*);
/* streamScatter.cpp:129-143: along every node's line, over its box's own j range lo .. hi, the peak of component comp of data (ncomp
 * components): the scan starts at ptOnStr = (int)(0.5 * (lo + hi)) -- truncated toward zero -- with the value there, runs j = lo .. hi
 * ascending and replaces on strict >.  jpeak, hival [nNodes], by node id. */
int pa_ssel_peaks(pa_ctx*, pa_ssel*, const double* data, int32_t ncomp, int32_t comp, int32_t* jpeak, double* hival);
/* streamScatter.cpp:145-154: the nodes with hival >= moreThan && hival < lessThan, compacted in node-id order (an integer scan, no
 * atomic counter); components comps (host, nvars <= 64) of data at (line, jpeak) go to columns col0 .. col0 + nvars - 1 of the kept
 * node's row of out [*nkept][stride] -- a caller short of memory passes the variables in groups.  nvars == 0 only counts (jpeak, data
 * and out may be NULL): size out with it.  *nkept is host. */
int pa_ssel_scatter(pa_ctx*, pa_ssel*, const double* data, int32_t ncomp, int32_t nvars, const int32_t* comps, const int32_t* jpeak, const double* hival,
                    double moreThan, double lessThan, int32_t stride, int32_t col0, double* out, int64_t* nkept);
/* stream2plt.cpp:504-547: the selected lines sel host [nSel][2] = (box g, line i), in level -> box -> line order, as the dense array
 * final [ncompSel][shi - slo + 1][nSel] of components comps (host) of data.  Every selected box must span exactly j = slo .. shi
 * (the reference copies that range without a check, :529-540). */
int pa_ssel_gather_lines(pa_ctx*, pa_ssel*, const double* data, int32_t ncomp, int32_t ncompSel, const int32_t* comps, int64_t nSel, const int32_t* sel,
                         int32_t slo, int32_t shi, double* final);
/* one condition of stream2plt.cpp:568-651.  MAX / MIN (:569-600): the running std::max / std::min of selected component comp along the
 * line, STARTED FROM THE FIRST POINT OF LINE 0 (:574, :591), tested `sgn val`; a failed test clears the line.  RXY (:604-619): the radius
 * sqrt(c0^2 + c1^2) of selected components 0 and 1 at point (int)(0.5 * (slo + shi)), tested `sgn val`.  AT (:622-651): at the first
 * segment where comp strictly brackets val2, comp2 interpolated there is tested `sgn val` and the result is ASSIGNED to the line (:646).
 * sgn: 0 ge, 1 gt, 2 lt, 3 le, 4 eq, 5 ne; any other value is an unknown string and tests false (do_test, :732-751). */
enum { PA_SSEL_MAX = 0, PA_SSEL_MIN = 1, PA_SSEL_RXY = 2, PA_SSEL_AT = 3 };
typedef struct { int32_t kind, comp, comp2, sgn; double val, val2; } pa_ssel_cond;
/* stream2plt.cpp:556-651 in one launch: write_lines [nSel] int32 = 1, then the conditions conds (host) in order -- the kinds must not
 * descend: max-tests, min-tests, RXY, at-tests, the reference's order.  final holds at least ncompSel components. */
int pa_ssel_filter(pa_ctx*, const double* final, int32_t ncompSel, int32_t slo, int32_t shi, int64_t nSel, int32_t ncond, const pa_ssel_cond* conds,
                   int32_t* write_lines);
/* stream2plt.cpp:654-713: component ncompSel of final [ncompSel + 1][npts][nSel] = the signed arc length: 0 at the first point, the serial
 * running sum of sqrt(dx^2 + dy^2 + dz^2) over selected components 0 .. 2 after it, minus its value interpolated where distComp first
 * strictly brackets distVal; without a crossing every point gets 2 * the line's last running sum (:702-709). */
int pa_ssel_arclength(pa_ctx*, double* final, int32_t ncompSel, int32_t npts, int64_t nSel, int32_t distComp, double distVal);

/* ------------------------------------------------------------- subsetting a stream directory by elements (streamSub.cpp)
 * The streamlines of a few surface elements cut out of a stream directory: the selected connectivity, the Str boxes it needs -- kept
 * WHOLE, in the file's order --, new consecutive node numbers over them, and their data copied to a compact buffer.
 * DATA LAYOUT and tables: those of pa_ssel above (box_desc, node_table, flat buffers: box g at ncomp * off_g doubles, component-major,
 * i fastest, then j).  face: device int32 [nElts][npe], 1-based node ids, npe >= 1.  The compact buffer has the same layout over the
 * kept boxes: kept box b' at ncompOut * off'_b'.
 * INTENT, NOT TEXT: streamSub.cpp:337-343 writes EVERY selected element over slots 0 .. nodesPerElt-1 of faceData (the last one wins,
 * the other slots stay zero) and :380-388 then reads that shrunken array at the FILE's element offset, so the reference is defined for
 * sElt=0 nElt=1 only.  Built here: faceSel[j * npe + i] = fileFace[E[j] * npe + i], and a box is needed iff it lists a node of faceSel.
 * DETERMINISM: no atomics.  Every count and position comes from an integer scan; boxes are flagged by plain stores of the value 1.
 * The copy moves 64-bit patterns (NaN payloads survive).  Two runs give the same bytes.  All calls are synchronous.
 * The handle's tables must put the ids of every box on its lines 0 .. n-1, one id a line (what build_nodeMap, :228-250, produces from
 * inside_nodes lists no longer than their boxes): checked on the host at the first call, refused with pa_last_error set otherwise. */
typedef struct pa_ssub pa_ssub;
/* NEW (Docs/source/streamSub.rst: "by physical location of the streamline seed point"; no line of streamSub.cpp does it): element e is
 * kept iff for each of its npe nodes the seed point x = components 0, 1, 2 of data (ncomp >= 3 components) at j = 0 of the node's line
 * has lo[d] <= x[d] && x[d] <= hi[d] for d = 0, 1, 2 -- literal comparisons, a NaN fails.  elts device [nElts] receives the kept
 * element indices (0-based) ascending: a count per 256 elements, a scan of the counts, a scatter that recomputes the flag.  *nsel (host)
 * = their number.  A box with lines whose j range lacks 0 is refused on the host; a node id outside 1 .. nNodes in face is found by the
 * count pass (nothing is read through it), the scatter then stores nothing and the call fails with elts as it was.  launch (host, may be NULL) = elements, count blocks,
 * passes of the one-workgroup scan over them, kept elements. */
int pa_ssub_select_seedbox(pa_ctx*, pa_ssel*, const double* data, int32_t ncomp, int64_t nElts, int32_t npe, const int32_t* face, const double lo[3], const double hi[3],
                           int32_t* elts, int64_t* nsel, int64_t launch[4]);
/* streamSub.cpp:337-343 (as intended), :375-395, :417-425, :439-441 for the element list elts device [nSel] (0-based file indices, any
 * order, duplicates repeat the element): gathers faceSel, flags the needed boxes, scans flag / listed lines / points / copy chunks over
 * the boxes in int64 (one workgroup up to 256 boxes, block sums beyond), numbers the nodes of the kept boxes 1 .. in level -> box ->
 * position order, maps faceSel through them and builds the chunk table of the copy.  NULL with pa_last_error set when nSel == 0, an
 * element id lies outside 0 .. nElts-1, face names an id outside 1 .. nNodes (nothing is read through a bad id), or the new node count
 * does not fit int32.  The plan refers to the pa_ssel: destroy it first. */
pa_ssub* pa_ssub_plan(pa_ctx*, pa_ssel*, int64_t nElts, int32_t npe, const int32_t* face, int64_t nSel, const int32_t* elts);
void pa_ssub_destroy(pa_ssub*);
/* counts host [3] = kept boxes, new nodes (:411-416 `tot`), points of the kept boxes */
int pa_ssub_counts(const pa_ssub*, int64_t counts[3]);
/* ReadMF (:267-304) for the kept boxes: components comps (host, ncompSel <= 64 a call) of data (ncomp components) become components
 * c0 .. c0 + ncompSel - 1 of out (ncompOut components of counts[2] points) -- a caller short of memory passes the components in groups,
 * holding only a group's in data.  A segmented copy from chunk records (at most 2048 doubles of one (box, component) run each), 16-byte
 * accesses where source and destination share the alignment, 8-byte ones otherwise.  out must not overlap data. */
int pa_ssub_gather(pa_ctx*, pa_ssub*, const double* data, int32_t ncomp, int32_t ncompSel, const int32_t* comps, double* out, int32_t ncompOut, int32_t c0);
/* to the host, each where not NULL: kept [counts[0]] = the old flat index g of every kept box (ascending: the std::set order of :392 within
 * a level); box_desc [counts[0]][4] = (ni, nj, jlo, off') of the kept boxes; newNum [nNodes] = the new number of node id n + 1 (the map of
 * :417-425), 0 where its box is not kept; faceSel [nSel][npe] in the new numbers (:439-441) */
int pa_ssub_read(pa_ctx*, pa_ssub*, int32_t* kept, int64_t* box_desc, int32_t* newNum, int32_t* faceSel);
/* what the plan launched: rec = nElts, nSel, boxes, kept boxes, copy chunks, box-scan path (1 one workgroup, 2 block sums), box-scan
 * workgroups, workgroups of the last pa_ssub_gather (chunks * components; 0 before the first) */
int pa_ssub_last_launch(const pa_ssub*, int64_t rec[8]);

/* ------------------------------------------------------------ tool pipelines
 * The level loops of the tool mains, operating on device-resident MultiFabs.
 * levels/state/out are arrays of nlev pointers, coarse first. */
/* grad.cpp:158-236.  state[lev]: comp = gradVar, ng >= 1.  out[lev][ocomp..+3]. */
int pa_grad_run(pa_ctx*, int nlev, pa_mf* const* state, int comp, const int32_t bc[3], pa_mf* const* out, int ocomp);

typedef struct {
  double  prog_min, prog_max; /* if prog_min > prog_max: use file min/max over the levels */
  int32_t do_threshold;       /* threshold_prog */
  double  threshold;          /* threshold_value */
  int32_t fused;              /* 1: fused grad->curvature kernels, 0: pass-by-pass */
  /* options of curvature.cpp:575-789 (pa_curvature_run only) */
  int32_t do_gauss_curv;      /* do_gaussCurv  (:575-677) */
  int32_t do_strain;          /* do_strain     (:679-749), keeps the reference's result = div u (quirk Q3) */
  int32_t get_strain_tensor;  /* getStrainTensor (:755-757): the 9 components of grad u */
  int32_t do_velnormal;       /* do_velnormal  (:765-787) */
  int32_t vel_comp;           /* first of the 3 consecutive velocity components in state */
  /* do_smooth (:328-406, pa_curvature_run only): one implicit diffusion step of the progress variable,
   * composite over the levels; everything downstream (curvature, threshold) then uses the smoothed field */
  int32_t do_smooth;
  double  smoothing_time;     /* smoothing_time (reference default 1e-7) */
  /* 0 or 3: the 3-D build.  2: the AMREX_SPACEDIM == 2 build on a level stored as ONE plane of cells (boxes with
   * lo[2] = hi[2] = 0, z a non-periodic direction: the homogeneous-Neumann wall makes every z difference an exact
   * zero, and adding exact zeros changes no sum of the path): MeanCurvature = sum_d d(n_d)/dx_d WITHOUT the 0.5 of
   * the 3-D build (curvature.cpp:542-546); pass-by-pass kernels (the fused sweep has the 0.5 built in); do_strain /
   * do_velnormal need a zero third velocity component at vel_comp + 2; do_gauss_curv and do_smooth are refused. */
  int32_t spacedim;
} pa_curv_params;
/* curvature.cpp:283-326 + 408-570 (core) + 575-789 (options).  state[lev][comp] = progress source
 * (ng>=2; with do_strain the velocity components get their ghost cells filled in place).
 * out[lev] comps: ocomp+0 Progress, +1 MeanCurvature, +2..4 FlameNormal, and when requested
 * +5 GaussianCurvature, +6 StrainRate, +7 VelFlameNormal, +8..16 ROST_dU?d? (row-major grad u), and with
 * do_smooth +17 SmoothedProgress.
 * Two implementations with identical results (bit for bit; both tested against the oracle): fused != 0, 3-D, boxes >= 3 cells thick
 * (one rank or a sharded hierarchy; with do_smooth the smoothed field is the pipeline's progress source with range [0, 1]): Progress / MeanCurvature / FlameNormal from the exact-normal pipeline of pa_gradcurv_run, whose
 * sweeps leave the cell-centred gradient of c (curvature.cpp:457-490, what do_gaussCurv differentiates again at :582-613) in a work
 * multifab of the level (3 components + 1 ghost layer, kept for the level's lifetime) instead of grad phi, then one pass per level
 * for the options; otherwise (or with params.fused = 0) one pass per AMReX call of the reference. */
int pa_curvature_run(pa_ctx*, int nlev, pa_mf* const* state, int comp, const int32_t bc[3],
                     const pa_curv_params*, pa_mf* const* out, int ocomp);
/* curvature.cpp:328-406: (I - dt Lap) sol = rhs[rcomp] as a composite solve over the levels (periodic /
 * homogeneous Neumann walls from bc, fine ghosts by applyBC, refluxed coarse-fine fluxes, covered coarse
 * cells = child averages), BiCGStab to ||b - A x||_inf <= tol ||b||_inf (the reference: 1e-12).  sol[lev]
 * comp scomp receives the solution on valid cells.  Refinement ratio 2.  Synchronous.
 * dt / dx^2 > 8 on the finest level (PA_SMOOTH_MG=1 / 0 in the environment: always / never; one rank or sharded): right-preconditioned with
 * one multigrid V(2,4) cycle per application (damped Jacobi on the AMR levels and on coarsened copies of level 0) -- the reference
 * solves with MLMG, whose iteration count does not grow with dt either; same solution to the tolerance.  The work vectors stay with
 * the levels (pa_level_destroy frees them).
 * Levels from pa_level_create_sharded: the solve is DISTRIBUTED over the context's ranks -- every rank iterates on its own boxes,
 * the restriction / ghost fills / flux register of one operator application cross ranks in nlev + 1 grouped exchanges
 * (pa_plan_restriction lists two of them), every dot product is one allreduce of the transport -- and returns the one-rank field
 * to the tolerance, not bit for bit; all ranks must call it together.  PA_SMOOTH_REPLICATED=1 in the environment: every rank
 * gathers the right-hand side of the whole hierarchy and runs the one-rank solve (its bits; no speed-up). */
int pa_smooth_solve(pa_ctx*, int nlev, pa_mf* const* rhs, int rcomp, pa_mf* const* sol, int scomp, double dt,
                    const int32_t bc[3], double tol, int maxiter, int* iters, double* rel_residual);
/* what the do_smooth solve of the last pa_curvature_run took: iterations and ||b - A x||_inf / ||b||_inf (the reference runs MLMG
 * with setVerbose(1), curvature.cpp:396-399, which prints its iteration count and residuals; the tool prints these).  Non-zero
 * when no such solve has run on the context. */
int pa_smooth_last(const pa_ctx*, int* iters, double* rel_residual);
/* which implementation the last pa_curvature_run on the context took: 1 = the exact-normal pipeline's G-output sweeps + one options
 * pass per level, 2 = the same with the Gaussian curvature formed inside the sweeps (one rank, every box wider than 32 cells and at
 * least 16 rows tall; only its first layer behind special faces is recomputed from the stored G), 0 = one kernel per AMReX call (fused = 0, 2-D levels, boxes thinner than 3 cells, or a hierarchy the
 * all-levels sweeps do not take; on a sharded hierarchy the ranks agree on one answer), -1 = none yet.  Diagnostic (tests, bench.py). */
int pa_curvature_last_path(const pa_ctx*);
/* Work multifabs the library keeps with a level between calls (pa_curvature_run: the gradient of c, 3 components, or the pass-by-pass
 * path's 8; pa_smooth_solve: its 8-13 vectors) -- kept because a multi-GB hipMalloc + hipFree per call cost more than the kernels they
 * served.  pa_level_destroy frees them; this frees them now (after a synchronisation of the context's stream) and returns the bytes
 * released.  The next call that needs them allocates again. */
int64_t pa_level_free_scratch(pa_level*);
/* fused grad+curvature of one variable: out[lev] comps ocomp+0..3 = gx,gy,gz,|g|,
 * +4..6 FlameNormal, +7 MeanCurvature.  work[lev]: scratch mf, 1 comp, ng=2. */
int pa_gradcurv_run(pa_ctx*, int nlev, pa_mf* const* state, int comp, const int32_t bc[3],
                    const pa_curv_params*, pa_mf* const* work, pa_mf* const* out, int ocomp);

/* Components comp0 .. comp0+ncomps-1 of state, one after the other into the SAME output buffers (what a tool does with the
 * variables of a plotfile).  done(user, comp) is called when a component's results are complete in `out` -- stream-ordered:
 * pa_sync before reading them on the host -- and before the next component overwrites them (NULL: no callback).  Ghost
 * fills that do not depend on results are done once for all components: FillBoundary of every component in one launch
 * and, on a sharded hierarchy, the first cross-rank exchange. */
int pa_gradcurv_run_comps(pa_ctx*, int nlev, pa_mf* const* state, int comp0, int ncomps, const int32_t bc[3],
                          const pa_curv_params*, pa_mf* const* work, pa_mf* const* out, int ocomp,
                          int (*done)(void* user, int comp), void* user);
/* The same in batches of nbatch components (1 .. 16): out[lev] holds nbatch SLOTS of 8 components from ocomp, component
 * comp0 + i of a batch goes to slot i % nbatch, and done(user, comp, ocomp_of_its_slot) is called for every component of a
 * batch once the batch is complete (stream-ordered, as above).  The boundary kernels of the exact-normal pipeline -- resolved
 * ghost values, coarse-patch gathers, curvature fix-up, and on a sharded hierarchy the exchange of the coarse normals --
 * then run once per BATCH instead of once per component; the sweeps stay component by component.  nbatch = 1 is
 * pa_gradcurv_run_comps.  (curvature.cpp:126-330 applied to each variable of a plotfile in turn.) */
int pa_gradcurv_run_comps2(pa_ctx*, int nlev, pa_mf* const* state, int comp0, int ncomps, const int32_t bc[3],
                           const pa_curv_params*, pa_mf* const* work, pa_mf* const* out, int ocomp, int nbatch,
                           int (*done)(void* user, int comp, int ocomp), void* user);

/* ------------------------------------------------- resampling onto a foreign BoxArray + running sum (avgPlotfiles.cpp)
 * One object (pa_resample) lives across the files of an average.  The caller owns the multifabs: per output level l a running
 * multifab on the output BoxArray U_l (avgPlotfiles.cpp:157-167) and, for every level but the finest, a work multifab T_l on the
 * same pa_level with g_l ghost layers, g = 0 on the finest level and one more per level down (with interp_type 0 none are needed).
 * For file f and level l, V(f, l) is defined over the whole level-l domain: the file's own value where one of its level-l boxes
 * holds the cell, elsewhere -- also when the file has no level l -- the interpolant of V(f, l-1): interp_type 0 the parent,
 * 1 the cell-conservative linear rule of pa_fillpatch_two_levels (same operations, same operands; coarse neighbours beyond a wall
 * are the nearest cell inside, beyond a periodic face the wrapped one; periodicity is the output level's is_per).  This is
 * FillPatchTwoLevels of the file's levels l-1, l wherever the parent's 27 neighbours are data of the file's level l-1 (properly
 * nested files) and its recursive extension elsewhere (PltFileManager::fillPatchFromPlt is recalled, not restated: DESIGN.md 1).
 * The output is (((0.0 + V(1,l)) + V(2,l)) + ... + V(nf,l)) * (1.0 / nf) in call order, each cell summed by one thread: the bits
 * do not depend on the tiling of U_l, the order of the file's boxes or how the variables are split into passes.
 * One rank; 3-D levels; ratio 2 or 4.  add_file_level is asynchronous on the context's stream; finish is synchronous. */
typedef struct pa_resample pa_resample;
pa_resample* pa_resample_create(pa_ctx*);
/* running_data[lev].define + setVal(0.0) (avgPlotfiles.cpp:156-167): the nlev running multifabs (coarsest first, at least nvar
 * components each, 1 <= nvar <= 16; the first nvar components are zeroed) of one pass over the files; clears the counter */
int pa_resample_begin(pa_ctx*, pa_resample*, int nlev, pa_mf* const* running, int nvar);
/* fillPatchFromPlt + MultiFab::Add for one file and level (avgPlotfiles.cpp:178-186), levels coarse first within a file: the valid
 * cells of V(f, lev) are added to running[lev]; work (NULL: not needed by a finer level) receives V(f, lev) in its valid and
 * ghost cells.  file: the file's level-lev data on its own pa_level (same domain; NULL: the file has no such level); comp_map[v] =
 * component of `file` that holds variable v (variables= resolved per file, :101-115, :183).  crse_work: work of level lev - 1
 * filled by the previous call for this file (NULL on level 0), with at least ceil(g / ratio) + interp_type ghost layers. */
int pa_resample_add_file_level(pa_ctx*, pa_resample*, int lev, const pa_mf* file, const int32_t* comp_map, const pa_mf* crse_work,
                               int ratio, int interp_type, pa_mf* work);
/* running_data[lev].mult(1.0 / nf) (avgPlotfiles.cpp:191-195) on every level; waits; nosrc (may be NULL) = cells, ghost cells of the
 * work multifabs included, for which neither the file nor the coarser work multifab had data (they hold NaN): 0 whenever the
 * file's level 0 covers the domain and the output levels are nested */
int pa_resample_finish(pa_ctx*, pa_resample*, int nfiles, int64_t* nosrc);
void pa_resample_destroy(pa_resample*);

/* ------------------------------------------------- one level of one file on a uniform BoxArray, by slabs (flattenAMRFile.cpp)
 * flattenAMRFile.cpp:77-89 (geom, grid.maxSize, fillPatchFromPlt) for ONE level of ONE file: every valid and ghost cell of
 * `out` receives V(f, l) as pa_resample defines it; no running sum.  file / comp_map / crse / ratio / interp_type as in
 * pa_resample_add_file_level; out: nvar (1..16) components on ANY list of disjoint boxes of the level's domain (a slab), any ng.
 * Asynchronous on the context's stream; *nosrc (device-counted, valid after pa_sync) as in pa_resample_finish.
 * file may be NULL (no box of the file's level meets the slab), crse is NULL on level 0 only; crse lives on any tiling of the coarser
 * domain with at least ceil(ng / ratio) + interp_type ghost layers that hold their canonical cells' values.  The file's own cells are
 * copied as 8 bytes each: a -0.0 and a NaN's payload survive (the running sum's 0.0 + v does not keep them).  Boxes without ghost cells
 * whose rows start and end on a parent's edge take a kernel that stores whole rows of children as 16-byte vectors, the others the
 * per-parent code of pa_resample_add_file_level; the bits do not depend on the route, the slab, the order of the boxes or crse's tiling.
 * (PltFileManager::fillPatchFromPlt is recalled, not restated: semantics stated by this project) */
int pa_flatten_level(pa_ctx*, const pa_mf* file, const int32_t* comp_map, const pa_mf* crse, int ratio, int interp_type,
                     pa_mf* out, int nvar, int64_t* nosrc);
/* what the last call launched, for tests (flattenAMRFile.cpp:89 has no counterpart): boxes on the wide route / on the general route /
 * skipped as fully covered, overlay rectangles.  The record is ONE per process, not per context (the entry has no context argument):
 * a hook for single-threaded tests, racy where several contexts or threads flatten at once -- pa_filter_last_launch's lives in its context */
void pa_flatten_last_launch(int64_t counts[4]);

/* ------------------------------------------------- plane sums and slices as images (avgToPlane.cpp / slicePlot.cpp)
 * One object (pa_plane) reduces a hierarchy to ONE plane normal to `dir` at the resolution of the finest level given to run: width =
 * length(d0), height = length(d1) with d0 < d1 the two directions other than dir, pixel (i', j') at i' + width * j'.
 * Composite value F of a cell of that level inside its domain: the value of the finest level <= it whose grids hold the cell's
 * coarsened image (AmrData::FillVar, piecewise-constant injection; recalled, not restated: DESIGN.md 1).  A cell no level holds is
 * counted (nosrc) and reads as NaN.  Every level's grids are whole refined cells of the next coarser level's (any AMR plotfile).
 * Sum (max_grid_size > 0): the sub-box is chopped along dir as BoxArray::maxSize does (even split) into chunks c = 0 .. C-1; per pixel
 * s_c = (((0.0 + F(a_c)) + F(a_c + 1)) + ... + F(b_c)) over the chunk's cells, ascending, and S = (((0.0 + s_0) + s_1) + ... + s_{C-1}):
 * plain IEEE additions in that order (a coarse cell R fine cells wide adds its value R times; -0.0 alone gives +0.0); the bits do not
 * depend on the tiling or the box order of the levels, nor on how the components are grouped.  Slice (max_grid_size == 0): S = F, bits kept.
 * The hierarchy is walked in place: device memory beyond the levels is the plane (ncomp doubles + 1 byte per pixel) and the chunk table.
 * One rank; 3-D levels; at most 8 levels.  run is asynchronous on the context's stream; read, minmax and pixelize are synchronous. */
typedef struct pa_plane pa_plane;
/* avgToPlane.cpp:93-104, :118-123 (subbox, dir, ba_sub.maxSize) / slicePlot.cpp:51-54 (the domain flattened at sliceloc): ncomp >= 1
 * rows of the plane; subbox in the finest level's indices; max_grid_size 0 = a slice, subbox one cell thick along dir.  NULL (and
 * pa_last_error) for dir outside 0..2, an empty sub-box, a slice box thicker than one cell or a plane of more than 2^31 - 1 pixels */
pa_plane* pa_plane_create(pa_ctx*, int ncomp, int dir, const pa_box* subbox, int max_grid_size);
/* avgToPlane.cpp:142-202 for every component at once (GetGrids + ParallelCopy, the MFIter loop, ParallelAdd) / slicePlot.cpp:55 (FillVar):
 * levels[0 .. nlev-1] = level 0 .. finestLevel, ratios[l] = refinement ratio between levels l and l + 1, comps[c] = the component of the
 * levels' multifabs that becomes row c of the plane.  Fails, launching nothing, for more than 8 levels, a component out of range on any
 * level, domains that are not each the coarser one refined by the ratio, a sub-box outside the finest domain, sharded levels. */
int pa_plane_run(pa_ctx*, pa_plane*, int nlev, const pa_mf* const* levels, const int32_t* ratios, const int32_t* comps /* [ncomp] */);
/* res_mf (avgToPlane.cpp:140, :201) / data (slicePlot.cpp:54): out[ncomp][height][width]; nosrc (may be NULL) = cells of the sub-box no
 * level holds.  Fails, leaving out alone, without a completed run. */
int pa_plane_read(pa_ctx*, const pa_plane*, double* out, int64_t* nosrc);
/* data.min() / data.max() (avgToPlane.cpp:206-207, slicePlot.cpp:56, :61-62) of row comp over the values that are not NaN (FArrayBox's
 * min / max on a NaN depend on its position); fails when there is none */
int pa_plane_minmax(pa_ctx*, const pa_plane*, int comp, double* mn, double* mx);
/* pixelizeData (avgToPlane.cpp:233-270, slicePlot.cpp:95-132) of row comp: t = (v - mn) / (mx - mn); level 0 if !(t > 0) -- a NaN t
 * included, where the reference's cast is undefined -- else (int)(255 * (t < 1 ? t : 1)).  levels[height][width], host memory. */
int pa_plane_pixelize(pa_ctx*, const pa_plane*, int comp, double mn, double mx, uint8_t* levels);
void pa_plane_destroy(pa_plane*);

/* ------------------------------------------------------------- quadric edge-collapse decimation of a surface (decimateMEF.cpp)
 * The job of the reference's qslim wrapper (Tools/qslim/main.cpp: read_mef :323-359, slim_init :92-136, output_mef :214-263; slim->decimate, Tools/qslim/qslim.cpp:58)
 * with an algorithm of our own (mixkit is not part of the reference tree): rounds that contract an independent set of
 * the cheapest edges at once.  Positions stay double (the reference casts to float) and the contraction order is not qslim's.
 * NUMERICS: every floating-point value is computed by one thread in a written order, without fused multiply-adds; lane groups and
 * atomics only combine flags, integer counts and minima of unique 64-bit integer keys.  The same input gives the same bytes, and
 * they are the bytes of the restatement tests/decimate_ref.py after every round.  One GPU.  All arrays are HOST memory; every call
 * is synchronous. */
typedef struct pa_decimate pa_decimate;
/* decimateMEF.cpp (Tools/qslim/main.cpp:323-359 read_mef, :92-136 slim_init): xyz [nnodes][3]; elts [nelts][3], 1-based.
 * boundary_weight / weighting (0 uniform, 1 area) / placement (0 endpoints, 1 endpoints or midpoint, 3 optimal): -B, -W, -O of
 * Tools/qslim/cmdline.cpp:23-45.  NULL (and pa_last_error) for a node id outside 1 .. nnodes, an element that names a node twice, any
 * other weighting or placement, or more than 2^31 - 1 nodes or 3 * nelts (the bound on the edges) */
pa_decimate* pa_decimate_create(pa_ctx*, int64_t nnodes, const double* xyz, int64_t nelts, const int32_t* elts, double boundary_weight, int weighting,
                                int placement);
/* decimateMEF.cpp: ONE round towards face_target (part of slim->decimate(face_target), Tools/qslim/qslim.cpp:58).  1 = a round was
 * applied; 0 = nothing left to do (the target is reached, or no edge passes the tests: pa_decimate_last_round says which); -1 = error */
int pa_decimate_round(pa_ctx*, pa_decimate*, int64_t face_target);
/* decimateMEF.cpp: rounds until one returns 0, at most max_rounds of them (slim->decimate, Tools/qslim/qslim.cpp:58); the number of
 * rounds applied, or -1.  The surface ends with face_target or face_target - 1 faces unless no valid contraction is left. */
int pa_decimate_run(pa_ctx*, pa_decimate*, int64_t face_target, int max_rounds);
/* decimateMEF.cpp (one record per round; the reference reports nothing between Tools/qslim/qslim.cpp:49 and :60): edges, locked edges,
 * candidates, budget = ceil((valid faces - target) / 2), selected, applied, faces removed, valid faces afterwards */
int pa_decimate_last_round(const pa_decimate*, int64_t rec[8]);
/* decimateMEF.cpp (the "(<v>v/<f>f)" of Tools/qslim/qslim.cpp:49-61): vertices the valid faces use, valid faces, rounds applied */
int pa_decimate_counts(const pa_decimate*, int64_t* nverts, int64_t* nfaces, int64_t* rounds);
/* decimateMEF.cpp (output_mef, Tools/qslim/main.cpp:214-263): xyz [nverts][3] of the used vertices and elts [nfaces][3], 1-based, of the
 * valid faces, both in input order */
int pa_decimate_read(pa_ctx*, const pa_decimate*, double* xyz, int32_t* elts);
/* decimateMEF.cpp: the whole state, for comparing a round on its own: xyz_all [nnodes][3], faces_all [nelts][3] 0-based (a dead face
 * keeps its slot and its last vertices), face_valid [nelts], quadrics [10][nnodes] (q11 q12 q13 q14 q22 q23 q24 q33 q34 q44).  Any
 * pointer may be NULL. */
int pa_decimate_read_state(pa_ctx*, const pa_decimate*, double* xyz_all, int32_t* faces_all, uint8_t* face_valid, double* quadrics);
void pa_decimate_destroy(pa_decimate*);

/* ------------------------------------------------------------- cutting and trimming a surface (sliceMEF.cpp, trimMEFgen.cpp)
 * A pa_surf is a triangulated surface with its node fields that stays in device memory between steps (component-major columns,
 * 0-based triples: DESIGN.md 3.15), so trim -> area -> slice -> slice runs without an upload in between.
 * NUMERICS: every floating-point value is computed by one thread in a written order, without fused multiply-adds; atomics and lane
 * groups combine only flags, integer counts, minima / maxima of bit patterns and fixed-point limbs.  The same input gives the same
 * bytes, and they are the bytes of the restatement tests/surfcut_ref.py.  The one value that is not the reference's: the area TOTAL is
 * the exactly rounded 192-bit fixed-point sum of the triangle areas (scaled from the largest, rounded once), where the reference adds
 * serially in element order (trimMEFgen.cpp:64-85).  One GPU.  All arrays are HOST memory; every call is synchronous. */
typedef struct pa_surf pa_surf;
/* sliceMEF.cpp:204-237 / trimMEFgen.cpp:423-429 (read_iso and the copy into GridPts): nodes [nnodes][ncomp] node-major as the file
 * stores them, elts [nelts][3] 1-based, triangles only.  NULL (and pa_last_error) for a node id outside 1 .. nnodes ("element <n>
 * names a node that does not exist"), ncomp < 3, or more than 2^31 - 1 nodes or 3 * nelts */
pa_surf* pa_surf_create(pa_ctx*, int64_t nnodes, int ncomp, const double* nodes, int64_t nelts, const int32_t* elts);
/* nodes.box().length(0), nElts, nodes.nComp() (sliceMEF.cpp:212-213, :230) of the surface as it stands (after a trim: the trimmed one) */
int pa_surf_counts(const pa_surf*, int64_t* nnodes, int64_t* nelts, int* ncomp);
/* write_iso's arguments (trimMEFgen.cpp:526): nodes [nnodes][ncomp], elts [nelts][3] 1-based.  Either pointer may be NULL.  The
 * surface is not changed, but the handle's scratch buffers are used (hence no const): one call at a time per handle. */
int pa_surf_read(pa_ctx*, pa_surf*, double* nodes, int32_t* elts);
/* sliceMEF.cpp:239-256 (the element loop), :637-681 (Segmentise), :607-630 (VertexInterp), :581-605 (VI_doIt), :260-268 (numbering):
 * the contour value[comp] == val.  Bit q of an element's case is set where node q has value[comp] < val (strict); cases 0 and 7 give
 * nothing, every other case ONE segment whose ends lie on the edges (apex, other) -- 1/6: (p0,p1),(p0,p2); 2/5: (p1,p0),(p1,p2);
 * 3/4: (p2,p0),(p2,p1) -- in element order.  A vertex lives under the DIRECTED pair of the first request for it (requests ordered by
 * element, then first or second end: the reference's map orders by std::pair's <, and the reverse lookup of :614 joins (a,b) and
 * (b,a)); its value is VI_doIt in that direction; vertices are numbered in lexicographic order of that pair.  The surface is not
 * changed and nothing is uploaded; the result stays on the device until the next slice or trim of this handle. */
int pa_surf_slice(pa_ctx*, pa_surf*, int comp, double val, int64_t* nverts, int64_t* nsegs);
/* the last slice (sliceMEF.cpp:260-268 vertVec, :429-436 slice_segs): verts [nverts][ncomp]; pairs [nverts][2] the directed node pair
 * (0-based) of each vertex; segs [nsegs][2] vertex ids (0-based; the file adds 1); src_elt [nsegs] the element (0-based) of each
 * segment; the incidence CSR the line assembly needs (:270-309, FindMySeg :537-546): csr_off [nverts + 1], csr_adj [2 * nsegs] = the
 * segments of each vertex in ascending segment index.  Any pointer may be NULL. */
int pa_surf_slice_read(pa_ctx*, const pa_surf*, double* verts, int32_t* pairs, int32_t* segs, int32_t* src_elt, int32_t* csr_off, int32_t* csr_adj);
/* trimMEFgen.cpp:90-192 (trim_surface), :195-294 (trim_surface_RXY), :297-372 (remove_unused_nodes) in one step: a node is removed if
 * ANY of the ncond conditions value[comps[i]] <ops[i]> vals[i] holds (ops: 0 lt, 1 le, 2 gt, 3 ge, 4 eq), or, when rxy >= 0, if
 * sqrt(x*x + y*y) <rxy_op> rxy holds; an element survives only if all three of its nodes do; nodes that no surviving element uses are
 * removed as well (*nodes_unused: how many of those the conditions had kept, the "Removed <n> unusued nodes" of :370).  Nodes and
 * elements keep their input order; ids are renumbered.  The handle is replaced in place; a slice it held is dropped. */
int pa_surf_trim(pa_ctx*, pa_surf*, int ncond, const int32_t* comps, const int32_t* ops, const double* vals, double rxy, int rxy_op, int64_t* nodes_unused);
/* trimMEFgen.cpp:53-87 (surface_area), :375-409 (triangle_area), :511-518 (min, max): every triangle's area by the written expression
 * 0.5 * sqrt(t0*t0 + t1*t1 + t2*t2); *total = their exactly rounded sum (see NUMERICS), *amin / *amax the smallest / largest (all 0 for
 * a surface without elements).  Fails when an area is not finite.  Any pointer may be NULL.  The surface and a slice it holds are
 * not changed, but the handle's scratch and launch record are written (hence no const): one call at a time per handle. */
int pa_surf_area(pa_ctx*, pa_surf*, double* total, double* amin, double* amax);
/* what the last slice, trim or area call of this handle launched, for tests (the reference has no counterpart; sliceMEF.cpp:257 and
 * trimMEFgen.cpp:370 are its only reports).  rec[0] = 1 slice / 2 trim / 3 area, rec[7] = kernels launched (scans and sorts not counted).
 * slice: [1] elements classified, [2] segments, [3] requests sorted, [4] vertices, [5] values interpolated, [6] CSR entries;
 * trim: [1] nodes flagged, [2] elements flagged, [3] nodes the conditions kept, [4] nodes out, [5] elements out, [6] values gathered;
 * area: [1] elements, [2] terms added in fixed point.
 * rec[0] = 4 merge / 5 scale / 6 product / 7 select (below).  merge: [1] nodes of S, [2] nodes of M entered in the table (0 off the grid
 * path), [3] path taken: 0 append, 1 grid, 2 brute force, [4] duplicates found, [5] nodes appended, [6] elements appended;
 * scale, product, select: [1] values written.
 * rec[0] = 8 smooth (below): [1] elements, [2] incidence entries sorted (3 * nelts), [3] neighbour entries (the sum of |N(e)|),
 * [4] iterations run, [5] nodes written, [6] the largest |N(e)|, [7] kernels launched (scans and sorts not counted, as for every op). */
int pa_surf_last_launch(const pa_surf*, int64_t rec[8]);
void pa_surf_destroy(pa_surf*);

/* ------------------------------------------------------------- joining surfaces (mergeMEF.cpp, scaleMEF.cpp, multMEF.cpp, combineMEF.cpp)
 * The same handle: merge -> scale -> select -> trim -> slice runs without leaving the device.  NUMERICS as above: one
 * thread per value in a written order, no fused multiply-adds; atomics combine only integer counts, minima and maxima.  The bytes are
 * those of the restatement tests/surfjoin_ref.py.  Handles from product and select may have fewer than three components: they can be
 * read, sliced, scaled, selected from and trimmed by conditions, while pa_surf_area, pa_surf_trim with rxy >= 0 and pa_surfjoin_merge
 * with rem_dup_nodes refuse them. */
/* mergeMEF.cpp:138-244 (merge_iso): S is merged into M.  With rem_dup_nodes = 0 (the reference's default, :74) nothing is compared and
 * node i of S becomes node nN_M + i.  With rem_dup_nodes = 1 node i of S becomes the SMALLEST j < nN_M (the count before this call:
 * nodes of S are never compared with each other) for which ((dx0*dx0) + dx1*dx1) + dx2*dx2 <= eps*eps holds (:186-208; dx = S minus M,
 * eps*eps formed once, :184); a comparison with a NaN is false, so NaN and +-inf coordinates never match; a node without such a j gets
 * the next new id in order of i.  If no node of S is new (cnt == nNodesM, :210) NOTHING is appended -- the reference drops the elements
 * of S as well, and so does this call -- and *appended = 0; otherwise the new nodes are appended with all their components in S's
 * order (M's own values win at a duplicate), all elements of S are appended after M's, renumbered, degenerate and repeated ones as they
 * are (:229-242), and *appended = 1.  method: 0 auto, 1 the hashed cell grid, 2 brute force (the reference's loop); both give the same
 * bytes.  The grid is taken only where it is provably conservative (pa_surfjoin.hip): auto takes brute force, and method = 1 refuses,
 * where a cell coordinate of M or S reaches 2^51 or is not finite, where M has no finite node, or where fewer than 2 cells span M (eps
 * at or above its extent).  M is replaced in place; a call that succeeds drops a slice M held (also where nothing was appended).
 * Refused: different component counts, eps*eps not finite, a result of more than 2^31 - 1 nodes or 3 * nelts, S == M, rem_dup_nodes
 * with fewer than three components, method = 1 where the grid cannot be taken.  A refused or failed call leaves M as it was: nodes,
 * elements, the slice it held and its launch record. */
int pa_surfjoin_merge(pa_ctx*, pa_surf* M, const pa_surf* S, double eps, int rem_dup_nodes, int method, int* appended);
/* scaleMEF.cpp:101-108: value[comps[k]] = value[comps[k]] * vals[k] at every node, for k = 0 .. n - 1 in list order; a component named
 * twice is scaled twice, (d * v0) * v1.  In place; a slice the handle held is dropped. */
int pa_surfjoin_scale(pa_ctx*, pa_surf*, int n, const int32_t* comps, const double* vals);
/* multMEF.cpp:135-148: a NEW handle of one component, ((1.0 * d[comps[0]]) * d[comps[1]]) * ..., with the elements of the surface;
 * n = 1 .. 32, repeats allowed.  NULL (and pa_last_error) on a component out of range.  Destroy it with pa_surf_destroy.  The launch
 * record is the NEW handle's; the source is not touched. */
pa_surf* pa_surfjoin_product(pa_ctx*, const pa_surf*, int n, const int32_t* comps);
/* combineMEF.cpp:165-181: a NEW handle of nsel components, column k a copy of component comps[k] of L (which[k] = 0) or of R
 * (which[k] = 1), in the given order, repeats allowed, with the elements of L.  R may be NULL when every which[k] is 0.  NULL (and
 * pa_last_error) where the element counts differ ("MEF files not compible", :117-120) and -- a deviation: the reference copies over the
 * intersection of the two boxes and leaves the rest uninitialised -- where the node counts differ.  The launch record is the NEW
 * handle's; L and R are not touched. */
pa_surf* pa_surfjoin_select(pa_ctx*, const pa_surf* L, const pa_surf* R_or_null, int nsel, const int32_t* which, const int32_t* comps);

/* ------------------------------------------------------------- smoothing a node field over a surface (smoothMEF.cpp)
 * The same handle: merge -> smooth -> trim -> slice runs without leaving the device.  NUMERICS as above; the bytes are
 * those of the restatement tests/surfsmooth_ref.py.  The two entries are named after their file (pa_surfsmooth.hip), as the
 * pa_surfjoin_* ones are; they take the pa_surf handle of pa_surf_create. */
/* smoothMEF.cpp:224-273 as it is evidently meant, with d = component comp and (n0, n1, n2) the nodes of element e in file order:
 *   weights   0 <= area_comp < ncomp: w_e = ((A[n0] + A[n1]) + A[n2]) * (1./3) with A that component (:249-256); otherwise w_e = the area of
 *             triangle e by the written expression of triangle_area (:160-194): R1 = pb - pa, R2 = pc - pa, R3 = R1 x R2 as written there,
 *             res = ((0 + R3x*R3x) + R3y*R3y) + R3z*R3z, 0.5 * sqrt(res).  The coordinates are read before anything is written, so
 *             comp < 3 (smoothing a coordinate) is well defined
 *   values    q_e = ((d[n0] + d[n1]) + d[n2]) * (1./3)
 *   N(e)      buildNodeNeighbors (:94-131): the elements other than e that share at least one node with e, each once, ascending
 *   iterate   W_e = w_e + sum of w_nb, nb ascending, added one by one; each of the nsmooth Jacobi iterations sets
 *             q'_e = ((w_e*q_e) + sum of (w_nb*q_nb)) / W_e in the same order from the previous iteration's q only (smoothVals, :134-157);
 *             where !(W_e > 0), q'_e = q_e
 *   nodes     node n with incident elements E(n), ascending, each once: Wn = sum of w_e, Sn = sum of (w_e*q_e), d[n] = Sn / Wn where
 *             Wn > 0; a node with !(Wn > 0), or one that no element uses, keeps its value.  No other component is touched.
 *             nsmooth = 0 still averages to the elements and back.
 * Deviations from the letter of smoothMEF.cpp, whose output is meaningless or undefined: without areaComp it indexes an array of
 * element areas by node id (:241-242, :252); it weights each node value by the running partial area sum (:253), feeds the intensive
 * result of smoothVals back in as value * area (:155, :267-269) and divides by the area once more (:273); and it writes the nElts
 * element values over the first nElts slots of the nNodes node values (:272-273), a heap overrun for nElts > nNodes.
 * In place; a slice the handle held is dropped.  Refused, with the handle left as it was (nodes, elements, slice, launch record):
 * comp out of range, nsmooth < 0, fewer than three components when area_comp is out of range, a sum of |N(e)| beyond 2^31 - 1. */
int pa_surfsmooth_run(pa_ctx*, pa_surf*, int comp, int area_comp, int nsmooth);
/* the last smooth of this handle: the neighbour lists as a CSR (nbr_off [nelts + 1], nbr_adj [nbr_off[nelts]], element ids 0-based),
 * w [nelts], and q [nelts] after the last iteration; valid until the next operation on the handle.  Any pointer may be NULL.  The
 * sizes are those of the launch record: nelts = rec[1], nbr_off[nelts] = rec[3].  Fails where the handle has not been smoothed. */
int pa_surfsmooth_read(pa_ctx*, const pa_surf*, int32_t* nbr_off, int32_t* nbr_adj, double* w, double* q);

#ifdef __cplusplus
}
#endif
#endif
