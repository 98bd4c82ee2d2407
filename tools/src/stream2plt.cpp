// stream2plt3d -- drop-in for PeleAnalysis Src/stream2plt.cpp (pick up to 32700 lines of a stream directory, filter them by
// conditions along the line, optionally add a signed arc-length coordinate, write one Tecplot zone per kept line) on MI355X.
//   stream2plt3d.ex infile=<stream dir> outfile=<file.dat> nLines=<n> [comps="c ..." | sComp=<c> nComp=<n>] [no_filter=0]
//       [maxComps="c ..." maxVals="v ..." maxSgns="s ..."] [minComps= minVals= minSgns=]
//       [atComps="c ..." compAt="c ..." valAt="v ..." atVal="v ..." atSgns="s ..."] [RXY=<r> RXYsgn=<s>]
//       [distComp=<c> distVal=<v>] [finestLevel=<l>] [verbose=0]
// Host side (this file): the keys (:335-439), the verbose text (:442-483), downsampleStreamData (:31-126) with the recalled random
// draw, and write_tec_ascii (:269-318).  Device side (pa_streamsel.hip): the dense array of the selected lines (:504-547), the
// filters (:556-651) and the arc length (:654-713).
// Deviations and kept quirks, all stated in INTEGRATION.md: the running max / min of every line starts from the first point of
// line 0; an at-test that finds a crossing assigns the flag; compAt is read as a real and truncated; an unknown sign tests false;
// (int)(0.5 * (slo + shi)) truncates.  amrex::Random() is RECALLED as std::uniform_real_distribution<double>(0, 1) over a
// std::mt19937 seeded with 987654321 (AMReX is not in the reference tree): with nLines >= the file's every line is taken whatever
// the generator.  nLines <= 0, finestLevel other than the file's, distComp with no_filter = 1, arrays of one condition with
// different counts, components out of range and a selected box that does not span the directory's j range abort; the TECIO
// binary writer is not built; ngpus > 1 aborts.
#include <random>

#include "../common/pa_device.h"

using pa::DBuf;

namespace {

const int NLINESMAX = 32700;

std::string g_str(double v) {
  char buf[64];
  std::snprintf(buf, sizeof buf, "%g", v);
  return buf;
}

int sgn_code(const std::string& s) {  // do_test (:732-751); an unknown string tests false
  const char* k[] = {"ge", "gt", "lt", "le", "eq", "ne"};
  for (int i = 0; i < 6; ++i)
    if (s == k[i]) return i;
  return -1;
}

// the arrays of one condition: all as long as the first (the reference's getarr aborts on a short one and ignores a long one's tail)
template <typename T>
void cond_arr(const pa::ParmParse& pp, const char* first, int n, const char* key, std::vector<T>& v) {
  if (pp.countval(key) != n)
    pa::Abort(std::string(key) + " has " + std::to_string(pp.countval(key)) + " values, " + first + " has " + std::to_string(n) + ": the arrays of one condition must have the same count");
  pp.queryarr(key, v, 0, n);
}

}  // namespace

int main(int argc, char** argv) {
  pa::ParmParse pp(argc, argv);
  int ngpus = 1;
  pp.query("ngpus", ngpus);
  if (ngpus > 1) pa::Abort("ngpus > 1 is not supported by stream2plt3d (one GPU; the reference filters on one rank)");
  std::mt19937 gen(987654321);  // InitRandom(987654321) (:333), recalled
  std::uniform_real_distribution<double> draw(0.0, 1.0);

  std::string infile, outfile;
  pp.get("infile", infile);
  pp.get("outfile", outfile);
  int verbose = 0;
  pp.query("verbose", verbose);

  const pa::StreamDir P = pa::read_stream_dir(infile);
  const int Nlev = (int)P.boxes.size(), nCompPath = (int)P.names.size();
  int finestLevel = Nlev - 1;
  pp.query("finestLevel", finestLevel);
  if (finestLevel < Nlev - 1) pa::Abort("finestLevel = " + std::to_string(finestLevel) + " is below the file's " + std::to_string(Nlev - 1) + ": the lines of the skipped levels would stay uninitialised (as in the reference)");
  if (finestLevel > Nlev - 1) pa::Abort("finestLevel = " + std::to_string(finestLevel) + " is above the file's " + std::to_string(Nlev - 1));

  // the flat box table; NLines and the j range of the lines (StreamData.cpp:207-217, :263-284: the first box that is not the zero box)
  std::vector<int64_t> box_desc;
  std::vector<const double*> fab;
  long long npts_all = 0, NLines = 0;
  bool found_extent = false;
  int slo = 0, shi = 0;
  for (int l = 0; l < Nlev; ++l)
    for (size_t b = 0; b < P.boxes[(size_t)l].size(); ++b) {
      const pa::Box3& B = P.boxes[(size_t)l][b];
      if (B.lo[0] != 0 || B.lo[2] != 0 || B.hi[2] != 0) pa::Abort("Str box " + pa::box_str(B) + " of level " + std::to_string(l) + " is not (0,jlo,0)..(n-1,jhi,0)");
      const long long ni = B.hi[0] + 1, nj = B.hi[1] - B.lo[1] + 1;
      const bool zbox = B.lo[1] == 0 && B.hi[0] == 0 && B.hi[1] == 0;
      if (!found_extent && !zbox) { slo = B.lo[1]; shi = B.hi[1]; found_extent = true; }
      if ((long long)P.inside[(size_t)l][b].size() > ni) pa::Abort("Str box " + std::to_string(b) + " of level " + std::to_string(l) + " has more inside_nodes than lines");
      box_desc.insert(box_desc.end(), {(int64_t)ni, (int64_t)nj, (int64_t)B.lo[1], (int64_t)npts_all});
      fab.push_back(P.data[(size_t)l][b].data());
      npts_all += ni * nj;
      NLines += (long long)P.inside[(size_t)l][b].size();
    }
  const int nbt = (int)fab.size();
  if (!found_extent || NLines < 1) pa::Abort("the stream file has no lines");
  if (verbose) std::cerr << "Found " << NLines << " streamlines in this file." << std::endl;

  std::vector<int> comps;  // :349-369
  if (const int nc = pp.countval("comps")) pp.queryarr("comps", comps, 0, nc);
  else {
    int sComp = 0, nComp = nCompPath;
    pp.query("sComp", sComp);
    pp.query("nComp", nComp);
    for (int i = 0; i < nComp; ++i) comps.push_back(sComp + i);
  }
  const int ncompSel = (int)comps.size();
  if (ncompSel < 1) pa::Abort("no component selected");
  for (int c : comps)
    if (c < 0 || c >= nCompPath) pa::Abort("component " + std::to_string(c) + " out of range (the stream file has " + std::to_string(nCompPath) + ")");
  std::vector<std::string> selectedNames;
  for (int c : comps) selectedNames.push_back(P.names[(size_t)c]);
  auto sel_ok = [&](int c, const char* key) {
    if (c < 0 || c >= ncompSel) pa::Abort(std::string(key) + ": component " + std::to_string(c) + " out of range (" + std::to_string(ncompSel) + " components are selected)");
  };

  int distComp = -1;  // :371-380
  pp.query("distComp", distComp);
  double distVal = 0;
  if (distComp >= 0) {
    pp.get("distVal", distVal);
    sel_ok(distComp, "distComp");
    if (ncompSel < 3) pa::Abort("distComp needs the selected components 0, 1 and 2 as coordinates");
    selectedNames.push_back("distance_from_" + P.names[(size_t)comps[(size_t)distComp]] + "_eq_" + g_str(distVal));
  }
  bool no_filter = false;
  pp.query("no_filter", no_filter);
  if (distComp >= 0 && no_filter) pa::Abort("distComp with no_filter = 1: the reference never fills the distance component in that case");

  int nLines = 0;
  pp.query("nLines", nLines);
  nLines = std::min(nLines, NLINESMAX);
  if (nLines <= 0) pa::Abort("nLines = " + std::to_string(nLines) + ": give a positive nLines (the reference builds an empty box)");
  if (verbose) std::cerr << "  Looking to extract approximately " << nLines << " of them." << std::endl;

  double RXY = -1;
  pp.query("RXY", RXY);
  std::string RXYsgn;
  pp.query("RXYsgn", RXYsgn);
  if (RXY > 0 && ncompSel < 2) pa::Abort("RXY needs the selected components 0 and 1");

  std::vector<double> maxVals, minVals, compAt, valAt, atVal;
  std::vector<std::string> maxSgns, minSgns, atSgns;
  std::vector<int> maxComps, minComps, atComps;
  if (const int nmax = pp.countval("maxComps")) {
    pp.queryarr("maxComps", maxComps, 0, nmax);
    cond_arr(pp, "maxComps", nmax, "maxVals", maxVals);
    cond_arr(pp, "maxComps", nmax, "maxSgns", maxSgns);
  }
  if (const int nmin = pp.countval("minComps")) {
    pp.queryarr("minComps", minComps, 0, nmin);
    cond_arr(pp, "minComps", nmin, "minVals", minVals);
    cond_arr(pp, "minComps", nmin, "minSgns", minSgns);
  }
  if (const int nat = pp.countval("atComps")) {  // where fab(atComp) = atVal: fab(compAt) atSgn valAt
    cond_arr(pp, "atComps", nat, "compAt", compAt);
    pp.queryarr("atComps", atComps, 0, nat);
    cond_arr(pp, "atComps", nat, "valAt", valAt);
    cond_arr(pp, "atComps", nat, "atVal", atVal);
    cond_arr(pp, "atComps", nat, "atSgns", atSgns);
  }
  std::vector<pa_ssel_cond> conds;  // the reference's order: max-tests, min-tests, RXY, at-tests
  for (size_t i = 0; i < maxComps.size(); ++i) {
    sel_ok(maxComps[i], "maxComps");
    conds.push_back({PA_SSEL_MAX, maxComps[i], 0, sgn_code(maxSgns[i]), maxVals[i], 0.0});
  }
  for (size_t i = 0; i < minComps.size(); ++i) {
    sel_ok(minComps[i], "minComps");
    conds.push_back({PA_SSEL_MIN, minComps[i], 0, sgn_code(minSgns[i]), minVals[i], 0.0});
  }
  if (RXY > 0) conds.push_back({PA_SSEL_RXY, 0, 0, sgn_code(RXYsgn), RXY, 0.0});
  for (size_t i = 0; i < atComps.size(); ++i) {
    if (!(compAt[i] > -2147483648.0 && compAt[i] < 2147483648.0)) pa::Abort("compAt: not a component");
    const int test_comp = (int)compAt[i];  // :626: a Real, truncated
    sel_ok(atComps[i], "atComps");
    sel_ok(test_comp, "compAt");
    conds.push_back({PA_SSEL_AT, atComps[i], test_comp, sgn_code(atSgns[i]), valAt[i], atVal[i]});
  }

  std::string condStr;
  if (verbose) {  // :442-483
    std::cout << "Preparing to extract/write the following components (i,idx,name): " << std::endl;
    for (int i = 0; i < ncompSel; ++i) std::cout << "(" << i << "," << comps[(size_t)i] << "," << P.names[(size_t)comps[(size_t)i]] << ") ";
    std::cout << std::endl;
    if ((int)selectedNames.size() > ncompSel) {
      std::cout << "....appending the following component(s): ";
      for (size_t i = (size_t)ncompSel; i < selectedNames.size(); ++i) std::cout << selectedNames[i] << std::endl;
    }
    auto nm = [&](int c) { return P.names[(size_t)comps[(size_t)c]]; };
    for (size_t i = 0; i < maxComps.size(); ++i) condStr += "Max(" + nm(maxComps[i]) + ") " + maxSgns[i] + " " + g_str(maxVals[i]) + "; ";
    for (size_t i = 0; i < minComps.size(); ++i) condStr += "Min(" + nm(minComps[i]) + ") " + minSgns[i] + " " + g_str(minVals[i]) + "; ";
    for (size_t i = 0; i < atComps.size(); ++i)
      condStr += nm((int)compAt[i]) + "(" + nm(atComps[i]) + " = " + g_str(atVal[i]) + ") " + atSgns[i] + " " + g_str(valAt[i]) + "; ";
    if (RXY > 0) condStr += "radiusXY " + RXYsgn + " " + g_str(RXY) + " ";
    if (condStr != "") std::cout << " ...subject to: " << condStr << std::endl;
  }

  // downsampleStreamData (:31-126): one draw per line in level -> box -> line order
  const double rval = (double)nLines / (double)NLines;
  std::vector<int32_t> sel;  // (flat box, line) of every selected line; its position is the line's new index
  std::vector<int> nSelBoxes((size_t)Nlev, 0);
  {
    int g = 0;
    for (int l = 0; l < Nlev; ++l) {
      std::vector<std::pair<int, size_t>> grids;  // (box of the level, first selected line in sel) of every box with selected lines
      for (size_t b = 0; b < P.boxes[(size_t)l].size(); ++b, ++g) {
        const size_t before = sel.size() / 2;
        for (size_t i = 0; i < P.inside[(size_t)l][b].size(); ++i) {
          const double doit = draw(gen);
          if (doit < rval) {
            sel.push_back(g);
            sel.push_back((int32_t)i);
          }
        }
        if (sel.size() / 2 > before) grids.emplace_back((int)b, before);
      }
      nSelBoxes[(size_t)l] = (int)grids.size();
      if (verbose)
        for (size_t k = 0; k < grids.size(); ++k) {
          const size_t end = k + 1 < grids.size() ? grids[k + 1].second : sel.size() / 2;
          std::cout << k << " (" << end - grids[k].second << "): ";
          for (size_t q = grids[k].second; q < end; ++q) std::cout << " ( " << q << " from " << sel[2 * q + 1] << " ) ";
          std::cout << " src data has " << P.boxes[(size_t)l][(size_t)grids[k].first].hi[0] + 1 << " particles" << std::endl;
        }
    }
  }
  const long long nSel = (long long)(sel.size() / 2);
  std::cout << "Reduced dataset has " << nSel << " lines " << std::endl;
  if (nSel < 1) pa::Abort("no line was selected (the reference builds an empty box)");
  if (verbose)
    for (int l = 0; l <= finestLevel; ++l)
      std::cout << "Reduced  dataset has " << nSelBoxes[(size_t)l] << " boxes (original has " << P.boxes[(size_t)l].size() << ") at level = " << l << std::endl;

  // the selected components of every box, flat: box g at ncompSel * off_g, component-major
  const int npts = shi - slo + 1, ncompTot = (int)selectedNames.size();
  std::vector<double> final((size_t)ncompTot * (size_t)npts * (size_t)nSel);
  std::vector<int32_t> write_lines((size_t)nSel, 1);
  {
    std::vector<double> h((size_t)((long long)ncompSel * npts_all));
    for (int g = 0; g < nbt; ++g) {
      const long long np = box_desc[4 * (size_t)g] * box_desc[4 * (size_t)g + 1], off = box_desc[4 * (size_t)g + 3];
      for (int c = 0; c < ncompSel; ++c)
        std::copy(fab[(size_t)g] + (size_t)comps[(size_t)c] * np, fab[(size_t)g] + (size_t)(comps[(size_t)c] + 1) * np, h.begin() + (size_t)((long long)ncompSel * off + (long long)c * np));
    }
    std::vector<int32_t> local((size_t)ncompSel);
    for (int c = 0; c < ncompSel; ++c) local[(size_t)c] = c;
    pa::Ctx ctx;
    pa_ssel* S = pa_ssel_create(ctx.h, nbt, box_desc.data(), 0, nullptr);
    if (!S) pa::Abort(pa_last_error(ctx.h));
    DBuf d(ctx, h.size() * 8), dfinal(ctx, final.size() * 8), dw(ctx, sizeof(int32_t) * (size_t)nSel);
    d.up(h.data(), h.size() * 8);
    dfinal.up(final.data(), final.size() * 8);  // zeros: a component the kernels do not write is never uninitialised
    ctx.check(pa_ssel_gather_lines(ctx.h, S, d.d(), ncompSel, ncompSel, local.data(), nSel, sel.data(), slo, shi, dfinal.d()));
    if (!no_filter) {
      ctx.check(pa_ssel_filter(ctx.h, dfinal.d(), ncompSel, slo, shi, nSel, (int32_t)conds.size(), conds.data(), (int32_t*)dw.p));
      dw.down(write_lines.data(), sizeof(int32_t) * (size_t)nSel);
      if (distComp >= 0) ctx.check(pa_ssel_arclength(ctx.h, dfinal.d(), ncompSel, npts, nSel, distComp, distVal));
    }
    dfinal.down(final.data(), final.size() * 8);
    pa_ssel_destroy(S);
  }

  // write_tec_ascii (:269-318)
  std::ofstream osf(outfile.c_str(), std::ios::out);
  if (!osf) pa::Abort("Unable to create " + outfile);
  osf << "VARIABLES = ";
  for (auto& n : selectedNames) osf << n << " ";
  osf << '\n';
  for (long long i = 0; i < nSel; ++i) {
    if (write_lines[(size_t)i] <= 0) continue;
    osf << "ZONE T=id" << i << " I=" << npts << " F=POINT" << std::endl;
    for (int j = 0; j < npts; ++j) {
      for (int n = 0; n < ncompTot; ++n) osf << final[((size_t)n * (size_t)npts + (size_t)j) * (size_t)nSel + (size_t)i] << " ";
      osf << '\n';
    }
  }
  osf.close();
  if (!osf) pa::Abort("short write to " + outfile);
  pa::Finish();
}
