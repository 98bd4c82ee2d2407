// slicePlot3d -- drop-in for PeleAnalysis Src/slicePlot.cpp (one slice of one plotfile variable through the composite hierarchy, at the
// finest level's resolution, as a PPM or PGM image) on MI355X.
//   slicePlot3d.ex file=<plt> slicedir=<d> sliceloc=<index> varname=<name> [finestLevel=<n>] [outtype=image|gray] [palette=<file>]
//       [min=<v>] [max=<v>] [outfile=<path>]
// Host side (this file and ../common/pa_image.h): the keys (:28-48, :58-88), the "min,max:" line (:56), the image file.  Device side
// (pa_plane.hip): FillVar's rule per pixel (the reference fills the slice serially on one rank), min / max, pixelizeData.
// Only levels 0 .. finestLevel, the one variable and the FABs the slice cuts are read.
// Kept: the key is `file`, not `infile`; the default output is <last piece of file>.ppm / .pgm in the working directory; an outtype
// other than image or gray writes nothing and exits 0; palette is required for image only; an existing image is overwritten.
// Deviations, all aborts where the reference is undefined or silent: see ../common/pa_image.h; also a cell of the
// slice no level holds, a slice without a value that is not NaN, ngpus > 1.  min / max are those of the values that are not NaN.
#include "../common/pa_device.h"
#include "../common/pa_image.h"

int main(int argc, char** argv) {
  pa::ParmParse pp(argc, argv);
  int ngpus = 1;
  pp.query("ngpus", ngpus);
  if (ngpus > 1) pa::Abort("ngpus > 1 is not supported by slicePlot3d (one GPU)");
  std::string file;
  pp.get("file", file);
  const pa::PlotfileHeader H = pa::read_header(file, 3, true);
  pa::PlaneFileInfo I;
  I.names = H.names;
  for (const pa::LevelMeta& L : H.lev) I.domains.push_back({L.domain.lo[0], L.domain.lo[1], L.domain.lo[2], L.domain.hi[0], L.domain.hi[1], L.domain.hi[2]});
  const pa::SlicePlotArgs A = pa::parse_sliceplot(pp, file, I);  // every key, the palette included, before anything is computed or written
  const int nlev = A.finestLevel + 1, dir = A.slicedir;
  const int d0 = dir == 0 ? 1 : 0, d1 = dir == 2 ? 1 : 2;
  const int width = A.box[3 + d0] - A.box[d0] + 1, height = A.box[3 + d1] - A.box[d1] + 1;

  pa::AsyncCtx actx;
  pa::Ctx& ctx = actx.get();
  const int per[3] = {0, 0, 0};
  std::vector<std::unique_ptr<pa::DevLevel>> dl;
  std::vector<std::unique_ptr<pa::DevMF>> mfs;
  std::vector<const pa_mf*> handles;
  for (int l = 0; l < nlev; ++l) {
    int R = 1;
    for (int q = l; q < A.finestLevel; ++q) R *= H.ref_ratio[(size_t)q];
    const int cl = A.sliceloc >= 0 ? A.sliceloc / R : -((-A.sliceloc + R - 1) / R);
    const std::vector<pa::Box3>& boxes = H.lev[(size_t)l].boxes;
    std::vector<char> only(boxes.size());
    for (size_t b = 0; b < boxes.size(); ++b) only[b] = boxes[b].lo[dir] <= cl && cl <= boxes[b].hi[dir];
    pa::HostMF h;
    h.define(boxes, 1, 0);
    pa::read_comp(H, l, A.comp, h, 0, &only);
    dl.emplace_back(new pa::DevLevel(ctx, boxes, H.lev[(size_t)l].domain, per, H.prob_lo, H.prob_hi));
    mfs.emplace_back(new pa::DevMF(ctx, *dl.back(), 1, 0));
    ctx.check(pa_mf_upload(ctx.h, mfs.back()->h, h.data.data()));
    handles.push_back(mfs.back()->h);
  }
  pa_box sub;
  for (int d = 0; d < 3; ++d) { sub.lo[d] = A.box[d]; sub.hi[d] = A.box[3 + d]; }
  std::vector<int32_t> ratios(H.ref_ratio.begin(), H.ref_ratio.end());
  ratios.push_back(0);
  pa_plane* P = pa_plane_create(ctx.h, 1, dir, &sub, 0);
  if (!P) pa::Abort(pa_last_error(ctx.h));
  const int32_t map[1] = {0};
  ctx.check(pa_plane_run(ctx.h, P, nlev, handles.data(), ratios.data(), map));
  std::vector<double> data((size_t)width * (size_t)height);
  int64_t nosrc = 0;
  ctx.check(pa_plane_read(ctx.h, P, data.data(), &nosrc));
  if (nosrc != 0) pa::Abort(std::to_string(nosrc) + " cells of the slice are held by no level of the plotfile");
  double data_min = 0.0, data_max = 0.0;
  ctx.check(pa_plane_minmax(ctx.h, P, 0, &data_min, &data_max));
  std::cout << "min,max: " << data_min << ", " << data_max << std::endl;  // :56
  if (A.writes) {
    if (A.have_min) data_min = A.vmin;
    if (A.have_max) data_max = A.vmax;
    pa::Box3 rb;
    for (int d = 0; d < 3; ++d) { rb.lo[d] = A.box[d]; rb.hi[d] = A.box[3 + d]; }
    std::cout << pa::box_str(rb) << std::endl;  // pixelizeData, :111
    std::vector<uint8_t> image(data.size());
    ctx.check(pa_plane_pixelize(ctx.h, P, 0, data_min, data_max, image.data()));
    if (A.outtype == "image") pa::store_ppm(A.outfile, width, height, image.data(), A.palette);
    else pa::store_pgm(A.outfile, width, height, image.data());
  }
  pa_plane_destroy(P);
  pa::Finish();
}
