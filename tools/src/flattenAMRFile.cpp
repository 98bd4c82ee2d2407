// flattenAMRFile3d -- drop-in for PeleAnalysis Src/flattenAMRFile.cpp (one level of an AMR plotfile on the whole domain as a
// single-level plotfile: the file's cells where it has them, interpolated from its coarser levels elsewhere) on MI355X.
//   flattenAMRFile3d.ex infile=<plt> [output_file=<root>_flatten] [output_level=0] [output_max_grid_size=64] [verbose=0]
//       [interp_type=1] [is_per="0 0 0"] [comp_batch=<n>] [slab_boxes=<n>] [stream_write=1] [help=1]
// Host side (this file): the keys and defaults (:47-56), the check (:69), the output grids (:77-80), the writer (:97;
// tools/common/pa_flatten_plan.h).  Device side (pa_flatten.hip): pa_flatten_level per level -- the levels below output_level once
// per component batch as ghosted work multifabs on the whole domain, the output level in slabs of consecutive output boxes, each
// computed, downloaded and handed to a writer thread while the next one is computed: the flattened level (68.7 GB per variable for
// a 2048^3 output) is never resident, on the device or on the host.
// Deviations, all stated in INTEGRATION.md: fillPatchFromPlt is recalled, semantics stated by this project (the recursive rule of
// include/peleanalysis_amd.h: V(f, l) = the file's value where it holds the cell, else the interpolant of V(f, l-1)); interp_type
// (the default of PelePhysics' six-argument call is recalled, not verifiable here); periodicity from is_per /
// geometry.is_periodic (the Header holds none); abort on ngpus > 1, a 2-D file, a ratio other than 2 or 4 or ratios that differ
// between levels, an output path that is or contains the input, and on cells without source data.
#include "../common/pa_device.h"
#include "../common/pa_flatten_plan.h"

namespace {

[[noreturn]] void print_usage(const char* argv0) {  // :10-20
  std::cerr << "usage:\n";
  std::cerr << argv0 << " infile=<s> [options] \n\tOptions:\n";
  std::cerr << "\t     infile=<s> where <s> is a pltfile\n";
  std::cerr << "\t     output_file=<s> where <s> is the flatten pltfile\n";
  std::cerr << "\t     output_level=<s> where <s> is the level of infile kept in output_file [DEF->0]\n";
  std::cerr << "\t     output_max_grid_size=<s> where <s> is the flatten max_grid_size [DEF->64]\n";
  std::cerr << "\t     interp_type=<int> 0 -> piecewise constant, 1 -> cell cons linear [DEF->1]\n";
  std::cerr << "\t     is_per=<i j k> periodic directions (the plotfile Header holds none) [DEF->0 0 0]\n";
  std::cerr << "\t     comp_batch=<n> variables per pass, slab_boxes=<n> output boxes per slab [DEF-> what fits the device]\n";
  std::cerr << "\t     stream_write=<0|1> write slab by slab while computing [DEF->1]\n";
  std::exit(1);
}

std::string file_root(const std::string& infile) {  // getFileRoot, :22-27: the last token between slashes
  std::string last, cur;
  for (char ch : infile) {
    if (ch == '/') { if (!cur.empty()) last = cur; cur.clear(); }
    else cur += ch;
  }
  return cur.empty() ? last : cur;
}

std::string real_path(const std::string& p) {
  char r[PATH_MAX];
  return ::realpath(p.c_str(), r) ? std::string(r) : std::string();
}

double fab_bytes(const pa::Box3& B, int g) {
  return 8.0 * (double)(B.hi[0] - B.lo[0] + 1 + 2 * g) * (double)(B.hi[1] - B.lo[1] + 1 + 2 * g) * (double)(B.hi[2] - B.lo[2] + 1 + 2 * g);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) print_usage(argv[0]);
  pa::ParmParse pp(argc, argv);
  if (pp.contains("help")) print_usage(argv[0]);
  int ngpus = 1;
  pp.query("ngpus", ngpus);
  if (ngpus > 1) pa::Abort("ngpus > 1 is not supported by flattenAMRFile3d (one GPU)");

  int verbose = 0;
  pp.query("verbose", verbose);
  std::string plotFileName;
  if (!pp.query("infile", plotFileName)) pa::Abort("ParmParse::get: infile not found");  // pp.get, :50
  std::string outfile(file_root(plotFileName) + "_flatten");
  pp.query("output_file", outfile);
  int output_level = 0;
  pp.query("output_level", output_level);
  int output_mgs = 64;
  pp.query("output_max_grid_size", output_mgs);
  if (output_mgs < 1) pa::Abort("output_max_grid_size must be positive");
  int interp_type = 1;
  pp.query("interp_type", interp_type);
  if (interp_type != 0 && interp_type != 1) pa::Abort("interp_type must be 0 (piecewise constant) or 1 (cell cons linear)");
  std::vector<int> is_per(3, 0);
  if (!pp.queryarr("is_per", is_per, 0, 3)) pp.queryarr("geometry.is_periodic", is_per, 0, 3);
  int stream_write = 1;
  pp.query("stream_write", stream_write);
  int comp_batch = 0, slab_boxes = 0;
  if (pp.query("comp_batch", comp_batch) && (comp_batch < 1 || comp_batch > 16)) pa::Abort("comp_batch must be 1 .. 16");
  if (pp.query("slab_boxes", slab_boxes) && slab_boxes < 1) pa::Abort("slab_boxes must be positive");

  pa::AsyncCtx actx;
  if (verbose) std::cout << " Reading data from pltfile " << plotFileName << "\n";
  const pa::PlotfileHeader P = pa::read_header(plotFileName, 3, true);  // a 2-D file aborts here
  const std::vector<std::string>& plt_vars = P.names;
  const int nvars = (int)plt_vars.size();
  if (output_level < 0 || output_level >= P.nlev) pa::Abort("Assertion `output_level < pltData.getNlev()' failed (the file has " + std::to_string(P.nlev) + " levels)");  // :69
  const int L = output_level;
  int ratio = 2;
  for (int lev = 1; lev <= L; ++lev) {  // (levels finer than output_level are ignored, as in the reference)
    const int rr = P.ref_ratio[(size_t)lev - 1];
    if (rr != 2 && rr != 4) pa::Abort("only refinement ratios 2 and 4 are supported (level " + std::to_string(lev) + " has " + std::to_string(rr) + ")");
    if (lev > 1 && rr != ratio) pa::Abort("levels with different refinement ratios are not supported");
    ratio = rr;
    const pa::Box3 &D = P.lev[(size_t)lev].domain, &C = P.lev[(size_t)lev - 1].domain;
    for (int d = 0; d < 3; ++d)
      if (D.lo[d] != C.lo[d] * rr || D.hi[d] + 1 != (C.hi[d] + 1) * rr) pa::Abort("the domain of level " + std::to_string(lev) + " is not the coarser one refined by the ratio");
  }
  {  // the output must not be (or hold) the input: the input is read slab by slab while the output is written
    const std::string out = real_path(outfile), I = real_path(plotFileName);
    if (!out.empty() && (I == out || (I.size() > out.size() && I.compare(0, out.size(), out) == 0 && I[out.size()] == '/')))
      pa::Abort("the output path " + outfile + " is or contains the input plotfile " + plotFileName);
  }

  if (verbose) std::cout << " Setting outgoing container \n";
  // grid.maxSize(output_mgs) of the domain on every level up to the output level (:77-80); ghost layers of the work multifabs as
  // in avgPlotfiles3d: none on the output level, ceil(g / ratio) + interp_type one level further down
  std::vector<std::vector<pa::Box3>> grids((size_t)L + 1);
  for (int lev = 0; lev <= L; ++lev) grids[(size_t)lev] = pa::max_size({P.lev[(size_t)lev].domain}, output_mgs);
  std::vector<int> ghosts((size_t)L + 1, 0);
  for (int lev = L - 1; lev >= 0; --lev) ghosts[(size_t)lev] = (ghosts[(size_t)lev + 1] + ratio - 1) / ratio + interp_type;
  const std::vector<pa::Box3>& obx = grids[(size_t)L];
  const int nob = (int)obx.size();

  pa::Ctx& ctx = actx.get();
  // components per pass and boxes per slab: the work multifabs with the largest coarser level of the file next to them, then a
  // slab's output boxes and the file's level-L FABs that meet it (whole FABs go up, also where they merely touch the slab: FABs
  // larger than the output boxes can outweigh them), counted slab by slab
  int nb = std::min(nvars, 16);
  {
    const std::vector<pa::Box3>& fboxes = P.lev[(size_t)L].boxes;
    double work = 0.0, largest = 0.0, obox = 0.0;
    for (int lev = 0; lev < L; ++lev) {
      for (const pa::Box3& B : grids[(size_t)lev]) work += fab_bytes(B, ghosts[(size_t)lev]);
      double n = 0.0;
      for (const pa::Box3& B : P.lev[(size_t)lev].boxes) n += fab_bytes(B, 0);
      largest = std::max(largest, n);
    }
    for (const pa::Box3& B : obx) obox = std::max(obox, fab_bytes(B, 0));
    int64_t free_b = 0, total_b = 0;
    ctx.check(pa_device_mem_info(ctx.h, &free_b, &total_b));
    const double avail = 0.9 * (double)free_b;
    if (comp_batch > 0) nb = std::min(nb, comp_batch);
    const bool slab_given = slab_boxes >= 1;
    auto largest_slab = [&](int sb) {  // bytes per variable of the heaviest slab: its output boxes + the file FABs that meet it
      double worst = 0.0;
      for (const auto& s : pa::flat_slabs(nob, sb)) {
        const std::vector<pa::Box3> slab(obx.begin() + s.first, obx.begin() + s.second);
        double n = 0.0;
        for (const pa::Box3& B : slab) n += fab_bytes(B, 0);
        for (int id : pa::flat_file_boxes(fboxes, slab)) n += fab_bytes(fboxes[(size_t)id], 0);
        worst = std::max(worst, n);
      }
      return worst;
    };
    for (;;) {
      const double left = avail - 1.05 * (work + largest) * nb;  // (1.05: padding of the component strides)
      if (!slab_given)  // a first guess from the output boxes alone, at most 2 GiB per host buffer
        slab_boxes = (int)std::max(1.0, std::min({left / (1.05 * 2.0 * obox * nb), 2147483648.0 / (obox * nb), (double)nob}));
      bool fits = left > 0.0 && 1.05 * nb * largest_slab(slab_boxes) <= left;
      while (!fits && !slab_given && left > 0.0 && slab_boxes > 1) {
        slab_boxes /= 2;
        fits = 1.05 * nb * largest_slab(slab_boxes) <= left;
      }
      if (fits) break;
      if (nb == 1) pa::Abort("the work multifabs of one variable and one slab of the output do not fit the device memory");
      nb /= 2;
    }
  }
  const std::vector<std::pair<int, int>> slabs = pa::flat_slabs(nob, slab_boxes);
  if (verbose) std::cout << " -> " << nob << " boxes on level " << L << " in " << slabs.size() << " slabs, " << nb << " variables per pass\n";

  // everything is validated: the first byte is written from here on
  pa::OldOutput old_out;
  old_out.move_away(outfile, "", pp);  // UtilCreateCleanDirectory inside WriteSingleLevelPlotfile (:97)
  std::unique_ptr<pa::FlatWriter> writer;
  std::vector<pa::HostMF> whole(1);  // stream_write=0: the level as one multifab, written by pa::write_plotfile
  if (stream_write) {
    writer.reset(new pa::FlatWriter(outfile, plt_vars, P.lev[(size_t)L].domain, P.prob_lo, P.prob_hi, obx, P.time));
    writer->open();
  } else {
    whole[0].define(obx, nvars, 0);
  }

  if (verbose) std::cout << " Interpolate data \n";
  int64_t nosrc_total = 0;
  std::vector<int32_t> ident(16);
  for (int a = 0; a < 16; ++a) ident[(size_t)a] = a;
  for (int v0 = 0; v0 < nvars; v0 += nb) {
    const int n = std::min(nb, nvars - v0);
    int64_t pass_nosrc = 0;  // cells, not cells x variables: every pass finds the same ones
    // levels below the output level: V(f, l) on the whole domain, valid and ghost cells
    std::vector<std::unique_ptr<pa::DevLevel>> dl;
    std::vector<std::unique_ptr<pa::DevMF>> work;
    for (int lev = 0; lev < L; ++lev) {
      dl.emplace_back(new pa::DevLevel(ctx, grids[(size_t)lev], P.lev[(size_t)lev].domain, is_per.data(), P.prob_lo, P.prob_hi));
      work.emplace_back(new pa::DevMF(ctx, *dl.back(), n, ghosts[(size_t)lev]));
      pa::HostMF h;
      h.define(P.lev[(size_t)lev].boxes, n, 0);
      for (int a = 0; a < n; ++a) pa::read_comp(P, lev, v0 + a, h, a);
      pa::DevLevel fl(ctx, P.lev[(size_t)lev].boxes, P.lev[(size_t)lev].domain, is_per.data(), P.prob_lo, P.prob_hi);
      pa::DevMF fm(ctx, fl, n, 0);
      ctx.check(pa_mf_upload(ctx.h, fm.h, h.data.data()));
      int64_t nosrc = 0;
      ctx.check(pa_flatten_level(ctx.h, fm.h, ident.data(), lev > 0 ? work[(size_t)lev - 1]->h : nullptr, ratio, interp_type, work.back()->h, n, &nosrc));
      ctx.check(pa_sync(ctx.h));  // the file's level is released here
      pass_nosrc += nosrc;
    }
    // the output level, slab by slab: two host buffers, the writer thread works on one while the other is filled
    pa::HostMF hbuf[2];
    std::future<void> pending[2];
    const std::vector<pa::Box3>& fboxes = P.lev[(size_t)L].boxes;
    for (size_t s = 0; s < slabs.size(); ++s) {
      const int b0 = slabs[s].first, b1 = slabs[s].second;
      const std::vector<pa::Box3> sb(obx.begin() + b0, obx.begin() + b1);
      pa::DevLevel sl(ctx, sb, P.lev[(size_t)L].domain, is_per.data(), P.prob_lo, P.prob_hi);
      pa::DevMF out(ctx, sl, n, 0);
      // only the file's boxes that meet the slab go up
      const std::vector<int> ids = pa::flat_file_boxes(fboxes, sb);
      std::unique_ptr<pa::DevLevel> fl;
      std::unique_ptr<pa::DevMF> fm;
      if (!ids.empty()) {
        std::vector<pa::Box3> fb;
        std::vector<char> only(fboxes.size(), 0);
        for (int id : ids) { fb.push_back(fboxes[(size_t)id]); only[(size_t)id] = 1; }
        pa::HostMF h;
        h.define(fb, n, 0);
        for (int a = 0; a < n; ++a) pa::read_comp(P, L, v0 + a, h, a, &only);
        fl.reset(new pa::DevLevel(ctx, fb, P.lev[(size_t)L].domain, is_per.data(), P.prob_lo, P.prob_hi));
        fm.reset(new pa::DevMF(ctx, *fl, n, 0));
        ctx.check(pa_mf_upload(ctx.h, fm->h, h.data.data()));
      }
      int64_t nosrc = 0;
      ctx.check(pa_flatten_level(ctx.h, fm ? fm->h : nullptr, ident.data(), L > 0 ? work[(size_t)L - 1]->h : nullptr, ratio, interp_type, out.h, n, &nosrc));
      pa::HostMF& H = hbuf[s & 1];
      if (pending[s & 1].valid()) pending[s & 1].get();  // the writer is done with this buffer
      H.define(sb, n, 0);
      ctx.check(pa_mf_download(ctx.h, out.h, H.data.data()));  // (waits for the kernels: nosrc is valid)
      pass_nosrc += nosrc;
      if (writer) {
        pa::FlatWriter* W = writer.get();
        pending[s & 1] = std::async(std::launch::async, [W, b0, v0, n, &H] { W->put_slab(b0, v0, n, H); });
      } else {
        pa::HostMF& O = whole[0];
        for (size_t b = 0; b < sb.size(); ++b)
          for (int a = 0; a < n; ++a)
            std::memcpy(O.data.data() + O.off[(size_t)b0 + b] + (long long)(v0 + a) * O.cs[(size_t)b0 + b], H.data.data() + H.off[b] + (long long)a * H.cs[b], sizeof(double) * (size_t)sb[b].numPts());
      }
    }
    for (auto& p : pending)
      if (p.valid()) p.get();
    nosrc_total = std::max(nosrc_total, pass_nosrc);
  }
  if (nosrc_total != 0) {  // nothing useful can be written: what this run created is removed (stream_write=0 has created nothing)
    if (writer) writer->abandon();
    pa::Abort(std::to_string(nosrc_total) + " cells found no source data (level 0 of the file does not cover the domain)");
  }

  if (verbose) std::cout << " Writting data \n";
  if (writer) writer->finish();
  else pa::write_plotfile(outfile, plt_vars, {P.lev[(size_t)L].domain}, P.prob_lo, P.prob_hi, whole, P.time, {0});
  old_out.finish();
  pa::Finish();
}
