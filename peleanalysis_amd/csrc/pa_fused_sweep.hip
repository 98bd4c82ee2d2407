// pa_fused_sweep.hip -- fused grad -> curvature, stage 2 of 3: the launchers of the sweep kernels (gfx950).
//
// The sweep reads phi once per box and writes gx,gy,gz,|g|,Nx,Ny,Nz,K; the flame normal at the neighbours is recomputed on chip
// instead of being stored, ghost-exchanged and re-read (curvature.cpp:451-546 makes ~10 passes over memory).  The kernels
// themselves are in pa_fused_march3.h (boxes wider than 32 cells) and pa_fused_march3n.h (narrower ones); this is the only unit
// that includes them.
//   first fused pipeline (PA_FUSED2=0, level 0 with boxes thinner than three cells): pa_gradcurv_level, one launch per level;
//     the two layers behind special faces are recomputed afterwards (pa_fused_fix.hip: pa_gradcurv_faces_phase)
//   exact-normal pipeline (default): pa_gradcurv_levels_cg, the CG variants of all levels in one launch per tile height, after
//     pa_gradcurv_prep_levels (pa_fused_prep.hip) and before pa_gradcurv_fix_levels (pa_fused_fix.hip)
// Entry points: pa_gradcurv_level, pa_gradcurv_fab, pa_sweep_occupancy (C ABI); pa_gradcurv_levels_cg, pa_gradcurv_gout_ok,
// pa_gradcurv_parts_ok, pa_gradcurv_kg_ok (pa_internal.h).
#include "pa_fused.h"
#include "pa_dist.h"
#include "pa_fabview.h"
#include "pa_fused_march3.h"
#include "pa_fused_march3n.h"
#include <cstdlib>

// planes per workgroup: 64 vs 128 measured 1.91 vs 1.94 ms with the burst schedule (within noise; more, shorter workgroups; not
// re-measured after round 11 took the junk stores and the drain out of a segment's prologue).  The tile
// heights (13 / 8 / 4 rows by the boxes' height), the XCD-aware workgroup order (2) and 8-byte stores are what the measurements of
// rounds 1-5 left standing; the 16-byte paired stores, the first marching kernel, tiles of 9-12 rows and the diagnostic builds of the
// sweep went with their switches in round 6 (DESIGN_HISTORY.md lists what each measured).
constexpr int FUSED_KSEG = 64;
static dim3 march_grid(int nx, int ny, int nz, int kseg, int mty, unsigned nboxes) {
  const unsigned tx = (nx + 63) / 64, ty = (ny + mty - 1) / mty, tz = (nz + kseg - 1) / kseg;
  return dim3(tx * ty * tz, nboxes);
}
constexpr int FUSED_ORDER = 2;
// kname: receives the variant that was launched (what bench.py matches the committed PMC traffic figure against)
template <typename BP>
static void march_launch(hipStream_t st, const BP& bp, int nx, int ny, int nz, unsigned nboxes, const MarchArgs& A0, std::string* kname = nullptr) {
  MarchArgs A = A0;
  // Small levels: a 256^3 level of 64^3 boxes is 320 workgroups at 64 planes each -- 1.25 rounds on 256 CUs -- and
  // ran at 50 % of the HBM figure; shorter z segments give the chip enough workgroups to balance (64 / 32 /
  // 16 / 8 planes on that level: 0.305 / 0.280 / 0.267 / 0.269 ms per launch; on the 512^3 headline level 64 stays best).
  // Round 2: the segment length is chosen from a small model instead of halved -- one workgroup per CU (LDS), so a launch
  // takes about ceil(workgroups / 256) rounds of (planes per segment + ~4 planes of pipeline fill); measured on rank 0's
  // share of the headline (8 boxes of 128^3 per level = 160 tiles): 16 / 22 / 32 / 43 / 64 planes -> 0.266 / 0.272 / 0.280 /
  // 0.254 / 0.309 ms per launch (model: 100 / 104 / 108 / 94 / 136), 16 boxes: 32 planes best (model and measurement).
  {
    const long long per_seg = (long long)((nx + 63) / 64) * ((ny + 12) / 13) * nboxes;
    if (per_seg * ((nz + A.kseg - 1) / A.kseg) < 2048) {
      long long best = -1;
      int best_k = A.kseg;
      for (int tz = 1; tz <= std::max(1, nz / 8); ++tz) {
        const int k = (nz + tz - 1) / tz;
        const long long rounds = (per_seg * ((nz + k - 1) / k) + 255) / 256, cost = rounds * (k + 4);
        if (best < 0 || cost < best) { best = cost; best_k = k; }
      }
      A.kseg = std::max(best_k, 4);
    }
  }
  A.order = FUSED_ORDER;
  A.nboxes = (int)nboxes;
  const bool clip = A.thr >= 0.0;
  if (nx <= 32) {  // boxes at most 32 cells wide: two rows per wavefront (pa_fused_march3n.h)
    constexpr int NRW = 8;
    const unsigned tiles = (unsigned)(((nx + 31) / 32) * ((ny + 2 * NRW - 1) / (2 * NRW)) * ((nz + A.kseg - 1) / A.kseg));
    A.tiles_max = (int)tiles;
    const dim3 g(tiles * 8u * ((nboxes + 7u) / 8u), 1);
    if (A.cg && clip) hipLaunchKernelGGL((k_gradcurv_march3n<BP, NRW, true, true>), g, dim3(64 * (NRW + 2)), 0, st, bp, A);
    else if (A.cg) hipLaunchKernelGGL((k_gradcurv_march3n<BP, NRW, false, true>), g, dim3(64 * (NRW + 2)), 0, st, bp, A);
    else if (clip) hipLaunchKernelGGL((k_gradcurv_march3n<BP, NRW, true>), g, dim3(64 * (NRW + 2)), 0, st, bp, A);
    else hipLaunchKernelGGL((k_gradcurv_march3n<BP, NRW, false>), g, dim3(64 * (NRW + 2)), 0, st, bp, A);
    if (kname) *kname = std::string("k_gradcurv_march3n<NRW=8,CLIP=") + (clip ? "1" : "0") + ",CG=" + (A.cg ? "1>" : "0>");
    return;
  }
  auto go = [&](auto mc) {  // short boxes do not fill a 13-row tile
    constexpr int M = decltype(mc)::value;
    dim3 g = march_grid(nx, ny, nz, A.kseg, M, nboxes);
    A.txy_max = ((nx + 63) / 64) * ((ny + M - 1) / M);
    A.tiles_max = (int)g.x;
    g = dim3(g.x * 8u * ((nboxes + 7u) / 8u), 1);
    if (kname) *kname = "k_gradcurv_march3<MTY=" + std::to_string(M) + ",CLIP=" + std::to_string((int)clip) + ",PAIR=0,CG=" + std::to_string((int)(A.cg != 0)) + ">";
    if (A.cg && !clip) hipLaunchKernelGGL((k_gradcurv_march3<BP, M, false, true>), g, dim3(64 * (M + 3)), 0, st, bp, A);
    else if (A.cg) hipLaunchKernelGGL((k_gradcurv_march3<BP, M, true, true>), g, dim3(64 * (M + 3)), 0, st, bp, A);
    else if (clip) hipLaunchKernelGGL((k_gradcurv_march3<BP, M, true>), g, dim3(64 * (M + 3)), 0, st, bp, A);
    else hipLaunchKernelGGL((k_gradcurv_march3<BP, M, false>), g, dim3(64 * (M + 3)), 0, st, bp, A);
  };
  if (ny >= 52) go(std::integral_constant<int, 13>{});
  else if (ny >= 16) go(std::integral_constant<int, 8>{});
  else go(std::integral_constant<int, 4>{});
}

// diagnostic: workgroups of a sweep kernel the runtime's occupancy query admits per CU (which = 0: the wide all-levels sweep, 13 rows;
// 1: the narrow all-levels sweep, 2 x 8 rows).  < 0: the query failed.  NOTE (profiles/r04_wg_residency.txt): the query says 2 for the
// narrow kernel (640 threads, 56 KB of LDS, 80 VGPRs) but per-workgroup clocks show exactly ONE resident per CU; 512-thread variants
// of the same kernel are admitted two per CU.
extern "C" int pa_sweep_occupancy(pa_ctx* ctx, int which) {
  PaBind bind_(ctx);
  if (!ctx) return -1;
  int nb = -1;
  hipError_t e = which == 0 ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k_gradcurv_march3_levels<13, false>, 64 * 16, 0)
                            : hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k_gradcurv_march3n_levels<8, false>, 64 * 10, 0);
  if (e != hipSuccess) { (void)hipGetLastError(); return -1; }
  return nb;
}

extern "C" int pa_gradcurv_level(pa_ctx* ctx, const pa_mf* phi, int pcomp, double pmin, double pmax, double thr, pa_mf* out, int ocomp) {
  PaBind bind_(ctx);
  if (!ctx || !phi || !out) return pa_fail(ctx, "pa_gradcurv_level: null argument");
  if (phi->lev != out->lev) return pa_fail(ctx, "pa_gradcurv_level: different levels");
  if (phi->ng < 2) return pa_fail(ctx, "pa_gradcurv_level: phi needs >= 2 ghost layers");
  if (pcomp < 0 || pcomp >= phi->ncomp || ocomp < 0 || ocomp + 8 > out->ncomp) return pa_fail(ctx, "pa_gradcurv_level: component range");
  if (!(pmax > pmin)) return pa_fail(ctx, "pa_gradcurv_level: progress variable has no range");
  const pa_level* L = phi->lev;
  if (phi->lev->boxes.empty()) return 0;  // a rank that owns no box of this level
  LevelBP2 bp{L->view, phi->view, out->view};
  MarchArgs A{pcomp, ocomp, FUSED_KSEG, pmin, 1.0 / (pmax - pmin), thr, 0, 1, 1, 1};
  ProfScope prof(ctx, PA_TAG_GRADCURV);
  march_launch(ctx->stream, bp, L->maxn[0], L->maxn[1], L->maxn[2], (unsigned)L->boxes.size(), A, &ctx->sweep_kernel);
  PA_HIP(hipGetLastError());
  return 0;
}

extern "C" int pa_gradcurv_fab(pa_ctx* ctx, pa_box valid, const pa_fab* phi, int pcomp, double pmin, double pmax, const double dxinv[3],
                               double thr, pa_fab* out, int ocomp) {
  PaBind bind_(ctx);
  if (!ctx || !phi || !out || !dxinv) return pa_fail(ctx, "pa_gradcurv_fab: null argument");
  std::string why;
  if (!fab_covers(*phi, valid, 2, pcomp, 1, why) || !fab_covers(*out, valid, 0, ocomp, 8, why)) return pa_fail(ctx, "pa_gradcurv_fab: " + why);
  if (!(pmax > pmin)) return pa_fail(ctx, "pa_gradcurv_fab: progress variable has no range");
  FabBP2 bp{fab_view(*phi), fab_view(*out), to_dbox(valid), {dxinv[0], dxinv[1], dxinv[2]}};
  MarchArgs A{pcomp, ocomp, FUSED_KSEG, pmin, 1.0 / (pmax - pmin), thr, 0, 1, 1, 1};
  march_launch(ctx->stream, bp, valid.hi[0] - valid.lo[0] + 1, valid.hi[1] - valid.lo[1] + 1, valid.hi[2] - valid.lo[2] + 1, 1, A);
  PA_HIP(hipGetLastError());
  return 0;
}

// NCG arrays of a level (MarchArgs::ncg): three arrays of pairs, each shaped like one set of the compact ghost arrays, allocated on first use
static int level_ncg(pa_ctx* ctx, const pa_level* Lc) {
  pa_level* L = const_cast<pa_level*>(Lc);
  if (L->d_ncg) return 0;
  const size_t n = 6 * (size_t)std::max<long long>(L->cg_total, 8);  // three arrays of pairs
  if (hipMalloc(&L->d_ncg, sizeof(double) * n) != hipSuccess) { L->d_ncg = nullptr; return pa_fail(ctx, "compact first-layer arrays: device allocation failed"); }
  PA_HIP(hipMemsetAsync(L->d_ncg, pa_opt().scratch_poison ? 0xFF : 0, sizeof(double) * n, ctx->stream));
  return 0;
}

// A sweep group: the boxes of one level that one kernel variant covers (all of them, or -- a level with boxes both wider and
// not wider than 32 cells -- its wide or its narrow ones through an index list)
struct SweepGroup { int lev; const int* list; int n; int dims[3]; };
static void sweep_groups(int l, const pa_level* L, std::vector<SweepGroup>& out) {
  if (L->boxes.empty()) return;
  if (!L->d_blist) { out.push_back({l, nullptr, (int)L->boxes.size(), {L->maxn[0], L->maxn[1], L->maxn[2]}}); return; }
  out.push_back({l, L->d_blist, L->nwide, {L->wmax[0], L->wmax[1], L->wmax[2]}});
  out.push_back({l, L->d_blist + L->nwide, L->nnarrow, {L->nmax[0], L->nmax[1], L->nmax[2]}});
}

static const WgTab* sweep_wgtab(const pa_level* L, const SweepGroup& g, int tw, int mty, int kseg, int part = 0, bool force = false) {
  if (!part && g.n <= 0) return nullptr;
  return pa_sweep_wgtab(L, !g.list ? 2 : (g.list == L->d_blist ? 0 : 1), tw, mty, kseg, force, part);
}

// the sweep with exact normals (the level's compact ghost arrays must be current: pa_gradcurv_prep_levels)
static int sweep_group_cg(pa_ctx* ctx, const SweepGroup& g, const pa_mf* phi, int pcomp, double pmin, double pmax, pa_mf* out, int ocomp, double thr, int slot) {
  const pa_level* L = phi->lev;
  if (pa_level_cg(ctx, L, slot + 1)) return 1;
  LevelBP2 bp{L->view, phi->view, out->view};
  bp.L.cg += slot * pa_cg_stride(L);  // the component slot's set of compact arrays
  MarchArgs A{pcomp, ocomp, FUSED_KSEG, pmin, 1.0 / (pmax - pmin), thr >= 0.0 ? thr : -1.0, 0, 1, 1, 1};
  A.cg = 1;
  A.boxlist = g.list;
  ProfScope prof(ctx, PA_TAG_GRADCURV);
  march_launch(ctx->stream, bp, g.dims[0], g.dims[1], g.dims[2], (unsigned)g.n, A, &ctx->sweep_kernel);
  PA_HIP(hipGetLastError());
  return 0;
}

// the CG sweeps of all levels: the groups of boxes wider than 32 cells in one launch (k_gradcurv_march3_levels) when they agree
// on the tile variant, else group by group (PA_FORCE_FALLBACKS=1: always); narrow groups one launch each.
// nslots > 1 (slot must be 0): components pcomp .. pcomp + nslots - 1 in ONE launch per kernel variant (blockIdx.y = slot: outputs at
// ocomp + 8 z, compact arrays of slot z, progress range prog[2 z], prog[2 z + 1] on the device); groups that do not take a batched
// launch run slot by slot with the host's ranges pmins / pmaxs
// gout (pa_curvature_run with options): the GOUT variants of the sweeps -- Progress, K, N at out components ocomp .. ocomp + 4, the
// cell-centred gradient of c at components 0 .. 2 of gout[l] (any ghost width).  Only as all-levels launches:
// pa_gradcurv_gout_ok says whether this hierarchy takes them (else the caller runs pass by pass).
// the sweeps of this hierarchy can be split into early and late tiles: every group of wide boxes goes through the all-levels launches
bool pa_gradcurv_parts_ok(int nlev, pa_mf* const* phi) { return pa_gradcurv_gout_ok(nlev, phi); }
// the G-output sweeps of this hierarchy can form the Gaussian curvature themselves (GOUT == 2, pa_fused_march3.h): every box wider
// than 32 cells (the narrow sweep has no such variant) and at least 16 rows tall (tiles of 13 or 8 rows)
bool pa_gradcurv_kg_ok(int nlev, pa_mf* const* phi) {
  if (!pa_gradcurv_gout_ok(nlev, phi)) return false;
  for (int l = 0; l < nlev; ++l) {
    const pa_level* L = phi[l]->lev;
    if (L->boxes.empty()) continue;
    if (L->nnarrow > 0 || L->maxn[1] < 16) return false;
    for (const DBox& B : L->boxes)
      if (B.hi[0] - B.lo[0] + 1 <= 32) return false;
  }
  return true;
}
bool pa_gradcurv_gout_ok(int nlev, pa_mf* const* phi) {
  if (pa_opt().force_fallbacks) return false;
  std::vector<SweepGroup> all;
  for (int l = 0; l < nlev; ++l) sweep_groups(l, phi[l]->lev, all);
  return all.size() <= 8 * PA_MAXB;  // (the launches come in chunks of PA_MAXB groups)
}

// part (a sharded hierarchy's pass, pa_pipeline.hip): 1 = only the EARLY tiles of the wide boxes (pa_sweep_wgtab: their input is
// complete after the local FillBoundary), 2 = the other tiles and every narrow box; 0 = everything
int pa_gradcurv_levels_cg(pa_ctx* ctx, int nlev, pa_mf* const* phi, int pcomp, double pmin, double pmax, pa_mf* const* out, int ocomp, double thr, int slot,
                          int nslots, const double* prog, const double* pmins, const double* pmaxs, pa_mf* const* gout, int part, int kg) {
  const bool clip = thr >= 0.0;
  if (kg && (!gout || !pa_gradcurv_kg_ok(nlev, phi))) return pa_fail(ctx, "pa_gradcurv_levels_cg: the Gaussian curvature inside the sweep needs the G-output sweeps of wide boxes");
  if (part && !pa_gradcurv_parts_ok(nlev, phi)) return pa_fail(ctx, "pa_gradcurv_levels_cg: this hierarchy's sweeps cannot be split into early and late tiles");
  if (nslots > 1 && (slot != 0 || !prog || !pmins || !pmaxs)) return pa_fail(ctx, "pa_gradcurv_levels_cg: component slots need slot 0 and the progress ranges");
  if (gout && (nslots != 1 || slot != 0 || !pa_gradcurv_gout_ok(nlev, phi))) return pa_fail(ctx, "pa_gradcurv_levels_cg: the G-output sweeps take one component of a hierarchy pa_gradcurv_gout_ok accepts");
  std::vector<SweepGroup> all, lv, rest;
  for (int l = 0; l < nlev; ++l) sweep_groups(l, phi[l]->lev, all);
  for (int l = 0; l < nlev; ++l) const_cast<pa_level*>(phi[l]->lev)->ncg_live = false;  // (set again below by the launches that mirror the x faces' first layer)
  bool any_ncg = false;
  int mty = 0;
  bool same = true;
  for (const SweepGroup& g : all) {
    if (g.dims[0] <= 32) { rest.push_back(g); continue; }
    const int m = g.dims[1] >= 52 ? 13 : (g.dims[1] >= 16 ? 8 : 4);  // as march_launch (tools/ab_driver.py, 13 against 12 / 11 / 10 / 9 rows: +0.058 / +0.041 / +0.31 / +0.97 ms per pass)
    same = same && (mty == 0 || m == mty);
    mty = m;
    lv.push_back(g);
  }
  // (Round 5, measured and not kept: tiles of 11 or 12 rows on BoxArrays whose boxes are 32 or 96 rows tall -- 13 + 13 + 6 rows
  // leave a fifth of the row slots idle -- took 7.52 against 7.41 ms per pass on the re-tiled irregular hierarchy: idle ROWS cost
  // nothing, a partly filled 64-cell tile in x does; profiles/r05_retile.txt.)
  // groups of different tile heights (a level of flat boxes next to one of tall ones): one launch per tile height (until round 5's
  // second session such a hierarchy went group by group, a launch each)
  (void)same;
  const bool ok = !lv.empty() && lv.size() <= 8u * PA_MAXB && !pa_opt().force_fallbacks;  // more than PA_MAXB groups (a hierarchy of 5+ levels): several launches
  if (!ok) {
    rest.insert(rest.begin(), lv.begin(), lv.end());
    lv.clear();
  }
  const std::vector<SweepGroup> lv_all = lv;
  // Round 6: a hierarchy with wide AND narrow boxes -- the narrow-box launch goes to the side stream and runs BESIDE the wide one (both
  // are sweeps: its workgroups fill the CUs the wide launch's tail leaves idle; 6.213 -> 6.167 ms per pass on the irregular hierarchy,
  // tools/ab_driver.py, profiles/r06_narrow_side_ab.txt).  One rank only: a sharded pass uses the side stream for its exchanges.
  bool nar_side = false;
  for (const SweepGroup& g : rest) nar_side = nar_side || g.dims[0] <= 32;
  nar_side = nar_side && !lv_all.empty() && part == 0 && !pa_opt().force_fallbacks && phi[0]->lev->nranks == 1;
  if (nar_side) {
    if (!ctx->stream2) PA_HIP(hipStreamCreateWithFlags(&ctx->stream2, hipStreamNonBlocking));
    while (ctx->sync_evs.size() < 5) {
      hipEvent_t e;
      PA_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
      ctx->sync_evs.push_back(e);
    }
    PA_HIP(hipEventRecord(ctx->sync_evs[3], ctx->stream));  // the ghost cells and compact arrays the sweeps read are complete
    PA_HIP(hipStreamWaitEvent(ctx->stream2, ctx->sync_evs[3], 0));
  }
  for (int pass_i = 0; pass_i < 3 * 8; ++pass_i) {  // (tile height) x (chunk of PA_MAXB groups)
    const int mty_pass = pass_i / 8 == 0 ? 13 : (pass_i / 8 == 1 ? 8 : 4), chunk = pass_i % 8;
    std::vector<SweepGroup> lvm, lv;
    for (const SweepGroup& g : lv_all)
      if ((g.dims[1] >= 52 ? 13 : (g.dims[1] >= 16 ? 8 : 4)) == mty_pass) lvm.push_back(g);
    for (size_t q = (size_t)chunk * PA_MAXB; q < lvm.size() && q < (size_t)(chunk + 1) * PA_MAXB; ++q) lv.push_back(lvm[q]);
    if (lv.empty()) continue;
    const int mty = mty_pass;
    SweepBatch S;
    S.n = (int)lv.size();
    S.wg0[0] = 0;
    // planes per workgroup: the model of march_launch on the whole launch (workgroups of all levels share the rounds)
    std::vector<long long> per_seg(lv.size());
    long long wgs = 0;
    const int kdef = FUSED_KSEG;
    for (size_t q = 0; q < lv.size(); ++q) {
      per_seg[q] = (long long)((lv[q].dims[0] + 63) / 64) * ((lv[q].dims[1] + mty - 1) / mty) * (long long)lv[q].n;
      wgs += per_seg[q] * ((lv[q].dims[2] + kdef - 1) / kdef);
    }
    int tz_best = 0;
    if (wgs < 2048) {
      long long best = -1;
      int nzmax = 0;
      for (const SweepGroup& g : lv) nzmax = std::max(nzmax, g.dims[2]);
      for (int tz = 1; tz <= std::max(1, nzmax / 8); ++tz) {
        long long w = 0;
        int kmax = 0;
        for (size_t q = 0; q < lv.size(); ++q) {
          const int nz = lv[q].dims[2], k = std::max(4, (nz + tz - 1) / tz);
          w += per_seg[q] * ((nz + k - 1) / k);
          kmax = std::max(kmax, k);
        }
        const long long cost = ((w + 255) / 256) * (kmax + 4);
        if (best < 0 || cost < best) { best = cost; tz_best = tz; }
      }
    }
    for (size_t q = 0; q < lv.size(); ++q) {
      const int l = lv[q].lev;
      const pa_level* L = phi[l]->lev;
      if (pa_level_cg(ctx, L, slot + nslots)) return 1;
      S.bp[q] = LevelBP2{L->view, phi[l]->view, out[l]->view};
      S.bp[q].L.cg += slot * pa_cg_stride(L);
      S.cgs[q] = pa_cg_stride(L);
      MarchArgs A{pcomp, ocomp, kdef, pmin, 1.0 / (pmax - pmin), clip ? thr : -1.0, 2, 1, 1, 1};
      A.cg = 1;
      {  // NCG: the first-layer data of the special x faces for the fix-up (PA_NCG=0: off)
        if (pa_opt().ncg && !clip && nslots == 1 && slot == 0 && !L->sfaces.empty()) {
          if (level_ncg(ctx, L)) return 1;
          pa_level* Lm = const_cast<pa_level*>(L);
          A.ncg = L->d_ncg; A.ncgs = pa_cg_stride(L);
          Lm->ncg_live = true;
          any_ncg = true;
          Lm->ncg_minw = lv[q].list ? 33 : 1;  // a list: the level's boxes wider than 32 cells; none: every box of the level is in this group
        }
      }
      A.boxlist = lv[q].list;
      if (tz_best) A.kseg = std::max(4, (lv[q].dims[2] + tz_best - 1) / tz_best);
      const unsigned nb = (unsigned)lv[q].n;
      const dim3 g = march_grid(lv[q].dims[0], lv[q].dims[1], lv[q].dims[2], A.kseg, mty, nb);
      A.nboxes = (int)nb;
      A.txy_max = ((lv[q].dims[0] + 63) / 64) * ((lv[q].dims[1] + mty - 1) / mty);
      A.tiles_max = (int)g.x;
      const WgTab* wt = sweep_wgtab(L, lv[q], 64, mty, A.kseg, part, kg == 2);
      if (wt) A.wgtab = wt->d;
      if (gout) { A.gdata = gout[l]->data; A.goff = gout[l]->d_off; A.gng = gout[l]->ng; }
      if (kg == 2 && wt && wt->d) {  // G only where something reads it (null: everywhere)
        const pa_level* F = l + 1 < nlev ? phi[l + 1]->lev : nullptr;
        const CpPlan* cp = (F && !F->boxes.empty()) ? pa_cp_plan(ctx, F, L) : nullptr;
        const bool no_patches = F && !F->boxes.empty() && F->cp_total > 0 && !(cp && cp->ok);  // the finer level reads the coarse G through the owner map: anywhere
        if (!no_patches) A.gneed = pa_sweep_gneed(L, wt, 64, mty, A.kseg, F ? F->serial : 0, cp && cp->ok ? &cp->hregs : nullptr);
      }
      S.A[q] = A;
      S.wg0[q + 1] = S.wg0[q] + (wt ? wt->n : (part ? 0u : g.x * 8u * ((nb + 7u) / 8u)));  // (a part's table may be empty)
    }
    if (S.wg0[S.n] == 0) continue;
    ProfScope prof(ctx, PA_TAG_GRADCURV);
    S.prog = nslots > 1 ? prog : nullptr;
    const dim3 grid(S.wg0[S.n], (unsigned)nslots);
    if (gout && kg) {  // GOUT == 2: + the Gaussian curvature at out component ocomp + 5
      if (clip) {
        if (mty == 13) hipLaunchKernelGGL((k_gradcurv_march3_levels<13, true, 2>), grid, dim3(64 * 16), 0, ctx->stream, S);
        else hipLaunchKernelGGL((k_gradcurv_march3_levels<8, true, 2>), grid, dim3(64 * 11), 0, ctx->stream, S);
      } else {
        if (mty == 13) hipLaunchKernelGGL((k_gradcurv_march3_levels<13, false, 2>), grid, dim3(64 * 16), 0, ctx->stream, S);
        else hipLaunchKernelGGL((k_gradcurv_march3_levels<8, false, 2>), grid, dim3(64 * 11), 0, ctx->stream, S);
      }
    } else if (gout) {
      if (clip) {
        if (mty == 13) hipLaunchKernelGGL((k_gradcurv_march3_levels<13, true, true>), grid, dim3(64 * 16), 0, ctx->stream, S);
        else if (mty == 8) hipLaunchKernelGGL((k_gradcurv_march3_levels<8, true, true>), grid, dim3(64 * 11), 0, ctx->stream, S);
        else hipLaunchKernelGGL((k_gradcurv_march3_levels<4, true, true>), grid, dim3(64 * 7), 0, ctx->stream, S);
      } else {
        if (mty == 13) hipLaunchKernelGGL((k_gradcurv_march3_levels<13, false, true>), grid, dim3(64 * 16), 0, ctx->stream, S);
        else if (mty == 8) hipLaunchKernelGGL((k_gradcurv_march3_levels<8, false, true>), grid, dim3(64 * 11), 0, ctx->stream, S);
        else hipLaunchKernelGGL((k_gradcurv_march3_levels<4, false, true>), grid, dim3(64 * 7), 0, ctx->stream, S);
      }
    } else if (clip) {
      if (mty == 13) hipLaunchKernelGGL((k_gradcurv_march3_levels<13, true>), grid, dim3(64 * 16), 0, ctx->stream, S);
      else if (mty == 8) hipLaunchKernelGGL((k_gradcurv_march3_levels<8, true>), grid, dim3(64 * 11), 0, ctx->stream, S);
      else hipLaunchKernelGGL((k_gradcurv_march3_levels<4, true>), grid, dim3(64 * 7), 0, ctx->stream, S);
    } else {
      if (mty == 13) hipLaunchKernelGGL(k_gradcurv_march3_levels<13>, grid, dim3(64 * 16), 0, ctx->stream, S);
      else if (mty == 8) hipLaunchKernelGGL(k_gradcurv_march3_levels<8>, grid, dim3(64 * 11), 0, ctx->stream, S);
      else hipLaunchKernelGGL(k_gradcurv_march3_levels<4>, grid, dim3(64 * 7), 0, ctx->stream, S);
    }
    PA_HIP(hipGetLastError());
  }
  if (part == 1) return 0;  // the narrow boxes and the groups outside the all-levels launches go with the late tiles
  // the narrow groups (boxes at most 32 cells wide) of all levels in one launch too
  std::vector<SweepGroup> nar;
  {
    std::vector<SweepGroup> keep;
    for (const SweepGroup& g : rest) (g.dims[0] <= 32 ? nar : keep).push_back(g);
    if (!nar.empty() && !pa_opt().force_fallbacks) rest.swap(keep);
    else nar.clear();
  }
  const std::vector<SweepGroup> nar_all = nar;
  for (size_t n0 = 0; n0 < nar_all.size(); n0 += PA_MAXB) {  // chunks of PA_MAXB groups
    const std::vector<SweepGroup> nar(nar_all.begin() + (long)n0, nar_all.begin() + (long)std::min(nar_all.size(), n0 + PA_MAXB));
    constexpr int NRW = 8;
    SweepBatch S;
    S.n = (int)nar.size();
    S.wg0[0] = 0;
    for (size_t q = 0; q < nar.size(); ++q) {
      const int l = nar[q].lev;
      const pa_level* L = phi[l]->lev;
      if (pa_level_cg(ctx, L, slot + nslots)) return 1;
      S.bp[q] = LevelBP2{L->view, phi[l]->view, out[l]->view};
      S.bp[q].L.cg += slot * pa_cg_stride(L);
      S.cgs[q] = pa_cg_stride(L);
      MarchArgs A{pcomp, ocomp, FUSED_KSEG, pmin, 1.0 / (pmax - pmin), clip ? thr : -1.0, 2, 1, 1, 1};
      A.cg = 1;
      A.boxlist = nar[q].list;
      A.nboxes = nar[q].n;
      // planes per workgroup as march_launch chooses them for one level
      const int nx = nar[q].dims[0], ny = nar[q].dims[1], nz = nar[q].dims[2];
      {
        const long long per_seg = (long long)((nx + 63) / 64) * ((ny + 12) / 13) * nar[q].n;
        if (per_seg * ((nz + A.kseg - 1) / A.kseg) < 2048) {
          long long best = -1;
          int best_k = A.kseg;
          for (int tz = 1; tz <= std::max(1, nz / 8); ++tz) {
            const int k = (nz + tz - 1) / tz;
            const long long rounds = (per_seg * ((nz + k - 1) / k) + 255) / 256, cost = rounds * (k + 4);
            if (best < 0 || cost < best) { best = cost; best_k = k; }
          }
          A.kseg = std::max(best_k, 4);
        }
      }
      const unsigned tiles = (unsigned)(((nx + 31) / 32) * ((ny + 2 * NRW - 1) / (2 * NRW)) * ((nz + A.kseg - 1) / A.kseg));
      A.tiles_max = (int)tiles;
      const WgTab* wt = sweep_wgtab(L, nar[q], 32, 2 * NRW, A.kseg);
      if (wt) A.wgtab = wt->d;
      if (gout) { A.gdata = gout[l]->data; A.goff = gout[l]->d_off; A.gng = gout[l]->ng; }
      S.A[q] = A;
      S.wg0[q + 1] = S.wg0[q] + (wt ? wt->n : tiles * 8u * (((unsigned)nar[q].n + 7u) / 8u));
    }
    ProfScope prof(ctx, PA_TAG_GRADCURV);
    S.prog = nslots > 1 ? prog : nullptr;
    hipStream_t ns = nar_side ? ctx->stream2 : ctx->stream;
    if (gout && clip) hipLaunchKernelGGL((k_gradcurv_march3n_levels<NRW, true, true>), dim3(S.wg0[S.n], 1u), dim3(64 * (NRW + 2)), 0, ns, S);
    else if (gout) hipLaunchKernelGGL((k_gradcurv_march3n_levels<NRW, false, true>), dim3(S.wg0[S.n], 1u), dim3(64 * (NRW + 2)), 0, ns, S);
    else if (clip) hipLaunchKernelGGL((k_gradcurv_march3n_levels<NRW, true>), dim3(S.wg0[S.n], (unsigned)nslots), dim3(64 * (NRW + 2)), 0, ns, S);
    else hipLaunchKernelGGL((k_gradcurv_march3n_levels<NRW, false>), dim3(S.wg0[S.n], (unsigned)nslots), dim3(64 * (NRW + 2)), 0, ns, S);
    PA_HIP(hipGetLastError());
    if (lv.empty()) ctx->sweep_kernel = "k_gradcurv_march3n_levels<NRW=8" + std::string(clip ? ",CLIP" : "") + ">[" + std::to_string(S.n) + " levels per launch]";
  }
  if (nar_side) {  // later work on the caller's stream sees the narrow boxes swept
    PA_HIP(hipEventRecord(ctx->sync_evs[4], ctx->stream2));
    PA_HIP(hipStreamWaitEvent(ctx->stream, ctx->sync_evs[4], 0));
  }
  if (gout && !rest.empty()) return pa_fail(ctx, "pa_gradcurv_levels_cg: a sweep group outside the all-levels launches (G-output variant)");
  for (const SweepGroup& g : rest)
    for (int z = 0; z < nslots; ++z)
      if (sweep_group_cg(ctx, g, phi[g.lev], pcomp + z, nslots > 1 ? pmins[z] : pmin, nslots > 1 ? pmaxs[z] : pmax, out[g.lev], ocomp + 8 * z, thr, slot + z)) return 1;
  if (!lv.empty())
    ctx->sweep_kernel = "k_gradcurv_march3_levels<MTY=" + std::to_string(mty) + (clip ? ",CLIP" : "") + ">[" + std::to_string(lv.size()) + " levels per launch" + (any_ncg ? "; x faces mirrored" : "") + "]" +
                        ((rest.empty() && nar.empty()) ? "" : " + narrow-box launch(es)");
  return 0;
}
