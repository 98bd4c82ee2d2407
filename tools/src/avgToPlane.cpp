// avgToPlane3d -- drop-in for PeleAnalysis Src/avgToPlane.cpp (the sum of plotfile components along one direction -- line-of-sight
// sums -- over a sub-box of the composite hierarchy, at the finest level's resolution, as a PPM image) on MI355X.
//   avgToPlane3d.ex infile=<plt> palette=<file> [comps="<c> ..." | sComp=<c> nComp=<n>] [finestLevel=<n>] [box="lo0 lo1 lo2 hi0 hi1 hi2"]
//       [dir=0] [max_grid_size=32] [min=<v>] [max=<v>] [sumfile=<path>] [help=1]
// Host side (this file and ../common/pa_image.h): the keys (:58-123, :204-223), the palette, pixelizeData's box print, the PPM.
// Device side (pa_plane.hip): every pixel's column is walked through the hierarchy in place, in the reference's order of additions;
// the reference's mf_full -- the finest level over the whole sub-box, 68 GB per component on a 2048^3 domain -- is never built.
// Only levels 0 .. finestLevel, the selected components and the FABs under the sub-box are read.  The components are worked off in
// groups of 4 (all levels of a group are resident on the device); the bits of a sum do not depend on the grouping.
// Kept: the image is <last piece of infile>.ppm in the working directory, from the FIRST selected component (res_mf[0], :205);
// "Filling <name> on level <n>" per component; an existing image is overwritten.
// Added: sumfile=<path> writes every component's sums ("ncomp height width\n", then little-endian doubles
// [ncomp][height][width]).  Deviations, all aborts where the reference is undefined or silent: see ../common/pa_image.h; also a
// sub-box cell no level holds, a first component without a value that is not NaN, ngpus > 1.
#include "../common/pa_device.h"
#include "../common/pa_image.h"

static void print_usage(char** argv) {  // :22-30
  std::cerr << "usage:\n";
  std::cerr << argv[0] << " infile=f1 [options] \n\tOptions:\n";
  std::exit(1);
}

int main(int argc, char** argv) {
  if (argc < 2) print_usage(argv);
  pa::ParmParse pp(argc, argv);
  if (pp.contains("help")) print_usage(argv);
  int ngpus = 1;
  pp.query("ngpus", ngpus);
  if (ngpus > 1) pa::Abort("ngpus > 1 is not supported by avgToPlane3d (one GPU)");
  std::string infile;
  pp.get("infile", infile);
  const pa::PlotfileHeader H = pa::read_header(infile, 3, true);
  pa::PlaneFileInfo I;
  I.names = H.names;
  for (const pa::LevelMeta& L : H.lev) I.domains.push_back({L.domain.lo[0], L.domain.lo[1], L.domain.lo[2], L.domain.hi[0], L.domain.hi[1], L.domain.hi[2]});
  const pa::AvgToPlaneArgs A = pa::parse_avgtoplane(pp, infile, I);  // every key, the palette included, before anything is computed or written
  const int nlev = A.finestLevel + 1, ncomp = (int)A.comps.size(), dir = A.dir;
  const int d0 = dir == 0 ? 1 : 0, d1 = dir == 2 ? 1 : 2;
  const int width = A.box[3 + d0] - A.box[d0] + 1, height = A.box[3 + d1] - A.box[d1] + 1;
  const size_t np = (size_t)width * (size_t)height;

  pa::AsyncCtx actx;
  // the FABs of every level under the sub-box: the others are not read
  std::vector<std::vector<char>> only((size_t)nlev);
  for (int l = 0; l < nlev; ++l) {
    int R = 1;
    for (int q = l; q < A.finestLevel; ++q) R *= H.ref_ratio[(size_t)q];
    only[(size_t)l].resize(H.lev[(size_t)l].boxes.size());
    for (size_t b = 0; b < only[(size_t)l].size(); ++b) {
      const pa::Box3& B = H.lev[(size_t)l].boxes[b];
      bool in = true;
      for (int d = 0; d < 3; ++d) {
        auto fl = [R](int i) { return i >= 0 ? i / R : -((-i + R - 1) / R); };
        in = in && B.hi[d] >= fl(A.box[d]) && B.lo[d] <= fl(A.box[3 + d]);
      }
      only[(size_t)l][b] = in ? 1 : 0;
    }
  }
  pa::Ctx& ctx = actx.get();
  const int per[3] = {0, 0, 0};
  std::vector<std::unique_ptr<pa::DevLevel>> dl;
  for (int l = 0; l < nlev; ++l) dl.emplace_back(new pa::DevLevel(ctx, H.lev[(size_t)l].boxes, H.lev[(size_t)l].domain, per, H.prob_lo, H.prob_hi));
  pa_box sub;
  for (int d = 0; d < 3; ++d) { sub.lo[d] = A.box[d]; sub.hi[d] = A.box[3 + d]; }
  std::vector<int32_t> ratios(H.ref_ratio.begin(), H.ref_ratio.end());
  ratios.push_back(0);

  std::vector<double> sums((size_t)ncomp * np);
  std::vector<uint8_t> image(np);
  for (int c0 = 0; c0 < ncomp; c0 += 4) {
    const int nc = std::min(4, ncomp - c0);
    for (int c = 0; c < nc; ++c) std::cout << "Filling " << H.names[(size_t)A.comps[(size_t)(c0 + c)]] << " on level " << A.finestLevel << std::endl;  // :144-146
    std::vector<std::unique_ptr<pa::DevMF>> mfs;
    std::vector<const pa_mf*> handles;
    for (int l = 0; l < nlev; ++l) {
      pa::HostMF h;
      h.define(H.lev[(size_t)l].boxes, nc, 0);
      for (int c = 0; c < nc; ++c) pa::read_comp(H, l, A.comps[(size_t)(c0 + c)], h, c, &only[(size_t)l]);
      mfs.emplace_back(new pa::DevMF(ctx, *dl[(size_t)l], nc, 0));
      ctx.check(pa_mf_upload(ctx.h, mfs.back()->h, h.data.data()));
      handles.push_back(mfs.back()->h);
    }
    pa_plane* P = pa_plane_create(ctx.h, nc, dir, &sub, A.max_grid_size);
    if (!P) pa::Abort(pa_last_error(ctx.h));
    const int32_t map[4] = {0, 1, 2, 3};
    ctx.check(pa_plane_run(ctx.h, P, nlev, handles.data(), ratios.data(), map));
    int64_t nosrc = 0;
    ctx.check(pa_plane_read(ctx.h, P, sums.data() + (size_t)c0 * np, &nosrc));
    if (nosrc != 0) pa::Abort(std::to_string(nosrc) + " cells of the box are held by no level of the plotfile");
    if (c0 == 0) {  // :204-213: the image comes from the first component
      double data_min = 0.0, data_max = 0.0;
      ctx.check(pa_plane_minmax(ctx.h, P, 0, &data_min, &data_max));
      if (A.have_min) data_min = A.vmin;
      if (A.have_max) data_max = A.vmax;
      pa::Box3 rb;
      for (int d = 0; d < 3; ++d) { rb.lo[d] = A.box[d]; rb.hi[d] = A.box[3 + d]; }
      rb.lo[dir] = rb.hi[dir] = 0;  // ProjectBox(subbox, dir, loc = 0), :137
      std::cout << pa::box_str(rb) << std::endl;  // pixelizeData, :249
      ctx.check(pa_plane_pixelize(ctx.h, P, 0, data_min, data_max, image.data()));
    }
    pa_plane_destroy(P);
  }
  pa::store_ppm(A.outfile, width, height, image.data(), A.palette);
  if (!A.sumfile.empty()) {
    FILE* fp = std::fopen(A.sumfile.c_str(), "w");
    if (!fp) pa::Abort("cannot open output file " + A.sumfile);
    std::fprintf(fp, "%d %d %d\n", ncomp, height, width);
    const size_t w = std::fwrite(sums.data(), sizeof(double), sums.size(), fp);
    if (std::fclose(fp) != 0 || w != sums.size()) pa::Abort("short write to " + A.sumfile);
  }
  pa::Finish();
}
