// avgPlotfiles3d -- drop-in for PeleAnalysis Src/avgPlotfiles.cpp (the average of N plotfiles on one domain whose refined
// regions differ) on MI355X.
//   avgPlotfiles3d.ex infiles="<plt1> <plt2> ..." [outfile=plt_averaged] [variables="a b"] [output_max_level=1000]
//       [output_max_grid_size=32] [interp_type=1] [is_per="0 0 0"] [comp_batch=<n>] [help=1]
// Host side (this file): the keys and defaults (:37-70), the variable lists (:85-116), the geometry checks (:131-138), the output
// grids (:141-152, :161-163; tools/common/pa_avggrids.h), the ratios (:169), the progress lines and the writer (:199-200).
// Device side (pa_resample.hip): per file and level one launch that puts the file's data on the output BoxArray -- its own
// value where the file has the cell, the interpolant of its coarser level elsewhere -- and adds it to the running sum
// (:178-186); a last pass scales (:191-195).  One level of one file is resident on the device at a time, next to the running
// sums and the work multifabs; variables go in batches when they do not all fit (the result does not depend on the batch).
// Deviations, all stated in INTEGRATION.md: fillPatchFromPlt where a file lacks the level or the parent's neighbourhood is not
// the file's data (the recursive rule of include/peleanalysis_amd.h); the decomposition of a union level (any disjoint cover);
// periodicity from is_per / geometry.is_periodic (the Header holds none); abort on ngpus > 1, a 2-D file, a ratio other than
// 2 or 4, files or levels that disagree in ratio, and an outfile that is one of the infiles.
#include "../common/pa_avggrids.h"
#include "../common/pa_device.h"

#include <cfloat>
#include <cmath>

namespace {

[[noreturn]] void print_usage(const char* argv0) {  // :8-23
  std::cerr << "Utility to average pltfiles on same domain but with non-matching AMR";
  std::cerr << "usage:\n";
  std::cerr << argv0 << "infiles=<s1 s2 s3> [options] \n\tOptions:\n";
  std::cerr << "\t     infiles=<s1 s2 s3> where <s1> <s2> amnd <s3> are pltfiles\n";
  std::cerr << "\t     outfile=<s> where <s> is the output pltfile\n";
  std::cerr << "\t     variables=<s1 s2 s3> where <s1> <s2> and <s3> are variable names to select for combined pltfile [DEF-> all possible]\n";
  std::cerr << "\t     output_max_level=<s> where <s> is the max refinement level to combine, zero-indexed [DEF->1000]\n";
  std::cerr << "\t     output_max_grid_size=<s> where <s> is the output max_grid_size. If all BoxArrays are the same, this is ignored. [DEF->32]\n";
  std::cerr << "\t     interp_type=<int> where this determines the type of interpolation when FillPatching: 0 -> piecewise constant, 1 -> cell cons linear [DEF->1]\n";
  std::cerr << "\t     is_per=<i j k> periodic directions (the plotfile Header holds none) [DEF->0 0 0]\n";
  std::exit(1);
}

bool almost_equal(double x, double y) {  // amrex::almostEqual with ulp = 2, as AlmostEqual(RealBox, RealBox) applies it (:134)
  const double d = std::fabs(x - y);
  return d <= DBL_EPSILON * std::fabs(x + y) * 2 || d < DBL_MIN;
}

std::string real_path(const std::string& p) {
  char r[PATH_MAX];
  return ::realpath(p.c_str(), r) ? std::string(r) : std::string();
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) print_usage(argv[0]);
  pa::ParmParse pp(argc, argv);
  if (pp.contains("help")) print_usage(argv[0]);
  int ngpus = 1;
  pp.query("ngpus", ngpus);
  if (ngpus > 1) pa::Abort("ngpus > 1 is not supported by avgPlotfiles3d (one GPU)");

  const int nf = pp.countval("infiles");
  if (nf <= 0) pa::Abort("Assertion `nf>0' failed");  // :45
  std::vector<std::string> plotFileNames;
  pp.getarr("infiles", plotFileNames);
  std::string outfile("plt_averaged");
  pp.query("outfile", outfile);
  int nvar = pp.countval("variables");
  std::vector<std::string> variableNames;
  if (nvar > 0) pp.getarr("variables", variableNames);
  const bool all_vars = nvar <= 0;
  int output_max_level = 1000;
  pp.query("output_max_level", output_max_level);
  output_max_level += 1;  // account for base level
  int output_max_grid_size = 32;
  pp.query("output_max_grid_size", output_max_grid_size);
  if (output_max_grid_size < 1) pa::Abort("output_max_grid_size must be positive");
  int interp_type = 1;
  pp.query("interp_type", interp_type);
  if (interp_type != 0 && interp_type != 1) pa::Abort("interp_type must be 0 (piecewise constant) or 1 (cell cons linear)");
  std::vector<int> is_per(3, 0);
  if (!pp.queryarr("is_per", is_per, 0, 3)) pp.queryarr("geometry.is_periodic", is_per, 0, 3);

  pa::AsyncCtx actx;
  std::cout << "Loading plt file metadata..." << std::endl;
  std::vector<pa::PlotfileHeader> plt((size_t)nf);
  std::vector<std::vector<int>> var_idxs((size_t)nf);
  int nlevels = 0;
  for (int i = 0; i < nf; ++i) {
    plt[(size_t)i] = pa::read_header(plotFileNames[(size_t)i], 3, true);  // a 2-D file aborts here
    const pa::PlotfileHeader& P = plt[(size_t)i];
    nlevels = std::max(nlevels, P.nlev);
    if (all_vars) {  // :85-99
      if (i == 0) {
        variableNames = P.names;
        nvar = (int)variableNames.size();
      } else {
        if ((int)P.names.size() != nvar) pa::Abort("All plt files must have same number of variables unless variable list is specified. File: " + plotFileNames[(size_t)i]);
        for (int var = 0; var < nvar; ++var)
          if (variableNames[(size_t)var] != P.names[(size_t)var]) pa::Abort("All plt files must have same variables unless variable list is specified. File: " + plotFileNames[(size_t)i]);
      }
      for (int var = 0; var < nvar; ++var) var_idxs[(size_t)i].push_back(var);
    } else {  // :101-115
      for (int var = 0; var < nvar; ++var) {
        const int pvar = P.comp(variableNames[(size_t)var]);
        if (pvar < 0) pa::Abort("Variable '" + variableNames[(size_t)var] + "' not found in file: " + plotFileNames[(size_t)i]);
        var_idxs[(size_t)i].push_back(pvar);
      }
    }
  }
  nlevels = std::min(nlevels, output_max_level);
  if (nlevels < 1) pa::Abort("output_max_level must not be negative");
  std::cout << " -> Combining " << nf << " files across " << nlevels << " levels" << std::endl;

  std::cout << "Finding the combined grids..." << std::endl;
  std::vector<pa::Box3> domains;
  std::vector<std::array<double, 3>> cell_size;  // of the first file that has the level (level_geometries, :132)
  std::vector<std::vector<std::vector<pa::Box3>>> lists((size_t)nlevels);
  for (int i = 0; i < nf; ++i) {
    const pa::PlotfileHeader& P = plt[(size_t)i];
    for (int lev = 0; lev < std::min(nlevels, P.nlev); ++lev) {
      if ((int)domains.size() <= lev) {
        domains.push_back(P.lev[(size_t)lev].domain);
        cell_size.push_back(P.file_dx[(size_t)lev]);
      } else {  // :134-138
        bool same = true;
        for (int d = 0; d < 3; ++d) {
          same = same && almost_equal(P.prob_lo[d], plt[0].prob_lo[d]) && almost_equal(P.prob_hi[d], plt[0].prob_hi[d]);
          same = same && P.lev[(size_t)lev].domain.lo[d] == domains[(size_t)lev].lo[d] && P.lev[(size_t)lev].domain.hi[d] == domains[(size_t)lev].hi[d];
        }
        if (!same) pa::Abort("All plt files must have the same geometry");
      }
      lists[(size_t)lev].push_back(P.lev[(size_t)lev].boxes);
    }
  }
  std::vector<std::vector<pa::Box3>> combined((size_t)nlevels);
  for (int lev = 0; lev < nlevels; ++lev) combined[(size_t)lev] = pa::avg_level_grids(lists[(size_t)lev], output_max_grid_size);
  int ratio = 2;
  for (int lev = 1; lev < nlevels; ++lev) {  // :169
    const int rr = (int)(cell_size[(size_t)lev - 1][0] / cell_size[(size_t)lev][0]);
    if (rr != 2 && rr != 4) pa::Abort("only refinement ratios 2 and 4 are supported (level " + std::to_string(lev) + " has " + std::to_string(rr) + ")");
    if (lev > 1 && rr != ratio) pa::Abort("levels with different refinement ratios are not supported");
    ratio = rr;
    for (int d = 0; d < 3; ++d)
      if (domains[(size_t)lev].lo[d] != domains[(size_t)lev - 1].lo[d] * rr || domains[(size_t)lev].hi[d] + 1 != (domains[(size_t)lev - 1].hi[d] + 1) * rr)
        pa::Abort("the domain of level " + std::to_string(lev) + " is not the coarser one refined by the ratio");
    for (int i = 0; i < nf; ++i)
      if (plt[(size_t)i].nlev > lev && plt[(size_t)i].ref_ratio[(size_t)lev - 1] != rr) pa::Abort("All plt files must have the same refinement ratios. File: " + plotFileNames[(size_t)i]);
  }
  {  // the output must not be (or hold) an input: one file is read at a time, the last after the old output is moved away
    const std::string out = real_path(outfile);
    for (const std::string& in : plotFileNames) {
      const std::string I = real_path(in);
      if (!out.empty() && (I == out || (I.size() > out.size() && I.compare(0, out.size(), out) == 0 && I[out.size()] == '/')))
        pa::Abort("the output path " + outfile + " is or contains the input plotfile " + in);
    }
  }

  // ghost layers of the work multifabs: none on the finest level, ceil(g / ratio) + interp_type one level further down
  std::vector<int> ghosts((size_t)nlevels, 0);
  for (int lev = nlevels - 2; lev >= 0; --lev) ghosts[(size_t)lev] = (ghosts[(size_t)lev + 1] + ratio - 1) / ratio + interp_type;

  pa::Ctx& ctx = actx.get();
  std::vector<std::unique_ptr<pa::DevLevel>> dl;
  for (int lev = 0; lev < nlevels; ++lev)
    dl.emplace_back(new pa::DevLevel(ctx, combined[(size_t)lev], domains[(size_t)lev], is_per.data(), plt[0].prob_lo, plt[0].prob_hi));

  // components per pass: the running sums, the work multifabs and the largest level of a file have to fit
  int nb = std::min(nvar, 16);
  {
    double per_comp = 0.0, largest = 0.0;
    for (int lev = 0; lev < nlevels; ++lev) {
      for (const pa::Box3& B : combined[(size_t)lev]) {
        per_comp += 8.0 * (double)B.numPts();
        if (lev < nlevels - 1) {
          const int g = ghosts[(size_t)lev];
          per_comp += 8.0 * (double)(B.hi[0] - B.lo[0] + 1 + 2 * g) * (double)(B.hi[1] - B.lo[1] + 1 + 2 * g) * (double)(B.hi[2] - B.lo[2] + 1 + 2 * g);
        }
      }
      for (const auto& l : lists[(size_t)lev]) {
        double n = 0.0;
        for (const pa::Box3& B : l) n += 8.0 * (double)B.numPts();
        largest = std::max(largest, n);
      }
    }
    per_comp = 1.05 * (per_comp + largest);  // (padding of the component strides)
    int64_t free_b = 0, total_b = 0;
    ctx.check(pa_device_mem_info(ctx.h, &free_b, &total_b));
    const double fit = 0.9 * (double)free_b / per_comp;
    if (fit < 1.0) pa::Abort("the running sums of one variable do not fit the device memory");
    if (fit < (double)nb) nb = (int)fit;
    int cb = 0;
    if (pp.query("comp_batch", cb)) {
      if (cb < 1 || cb > 16) pa::Abort("comp_batch must be 1 .. 16");
      nb = std::min(nb, cb);
    }
  }

  std::vector<pa::HostMF> out((size_t)nlevels);
  for (int lev = 0; lev < nlevels; ++lev) out[(size_t)lev].define(combined[(size_t)lev], nvar, 0);
  pa_resample* rs = pa_resample_create(ctx.h);
  if (!rs) pa::Abort(pa_last_error(ctx.h));
  std::cout << "Fillpatching and combining..." << std::endl;
  for (int v0 = 0; v0 < nvar; v0 += nb) {
    const int n = std::min(nb, nvar - v0);
    std::vector<std::unique_ptr<pa::DevMF>> run, work;
    std::vector<pa_mf*> runh;
    for (int lev = 0; lev < nlevels; ++lev) {
      run.emplace_back(new pa::DevMF(ctx, *dl[(size_t)lev], n, 0));
      runh.push_back(run.back()->h);
      work.emplace_back(lev < nlevels - 1 ? new pa::DevMF(ctx, *dl[(size_t)lev], n, ghosts[(size_t)lev]) : nullptr);
    }
    ctx.check(pa_resample_begin(ctx.h, rs, nlevels, runh.data(), n));
    std::vector<int32_t> ident((size_t)n);
    for (int a = 0; a < n; ++a) ident[(size_t)a] = a;
    for (int i = 0; i < nf; ++i) {
      if (v0 == 0) std::cout << "   working on file " << plotFileNames[(size_t)i] << " (" << i + 1 << "/" << nf << ")" << std::endl;
      const pa::PlotfileHeader& P = plt[(size_t)i];
      for (int lev = 0; lev < nlevels; ++lev) {
        pa_mf* crse = lev > 0 ? work[(size_t)lev - 1]->h : nullptr;
        pa_mf* wk = work[(size_t)lev] ? work[(size_t)lev]->h : nullptr;
        if (lev < P.nlev) {
          pa::HostMF h;
          h.define(P.lev[(size_t)lev].boxes, n, 0);
          for (int a = 0; a < n; ++a) pa::read_comp(P, lev, var_idxs[(size_t)i][(size_t)(v0 + a)], h, a);
          pa::DevLevel fl(ctx, P.lev[(size_t)lev].boxes, domains[(size_t)lev], is_per.data(), plt[0].prob_lo, plt[0].prob_hi);
          pa::DevMF fm(ctx, fl, n, 0);
          ctx.check(pa_mf_upload(ctx.h, fm.h, h.data.data()));
          ctx.check(pa_resample_add_file_level(ctx.h, rs, lev, fm.h, ident.data(), crse, ratio, interp_type, wk));
          ctx.check(pa_sync(ctx.h));  // the file's level is released here
        } else {
          ctx.check(pa_resample_add_file_level(ctx.h, rs, lev, nullptr, nullptr, crse, ratio, interp_type, wk));
        }
      }
    }
    int64_t nosrc = 0;
    ctx.check(pa_resample_finish(ctx.h, rs, nf, &nosrc));
    if (nosrc != 0) pa::Abort(std::to_string(nosrc) + " cells found no source data (level 0 of a file does not cover the domain, or its levels are not nested)");
    for (int lev = 0; lev < nlevels; ++lev) {
      pa::HostMF h;
      h.define(combined[(size_t)lev], n, 0);
      ctx.check(pa_mf_download(ctx.h, run[(size_t)lev]->h, h.data.data()));
      pa::HostMF& O = out[(size_t)lev];
      for (size_t b = 0; b < h.boxes.size(); ++b)
        for (int a = 0; a < n; ++a)
          std::memcpy(O.data.data() + O.off[b] + (long long)(v0 + a) * O.cs[b], h.data.data() + h.off[b] + (long long)a * h.cs[b], sizeof(double) * (size_t)h.boxes[b].numPts());
    }
  }
  pa_resample_destroy(rs);

  std::cout << "Saving final plt file..." << std::endl;
  pa::OldOutput old_out;
  old_out.move_away(outfile, "", pp);  // UtilCreateCleanDirectory inside WriteMultiLevelPlotfile (:200)
  const std::vector<int> stepidx((size_t)nlevels, 0);
  pa::write_plotfile(outfile, variableNames, domains, plt[0].prob_lo, plt[0].prob_hi, out, 0.0, stepidx, ratio);
  old_out.finish();
  std::cout << "Done." << std::endl;
  pa::Finish();
}
