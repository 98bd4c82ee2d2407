// jpdf3d -- drop-in for PeleAnalysis Src/jpdf.cpp (joint PDFs of every pair of a list of plotfile variables, volume weighted, with the
// bin-averaged values of both variables; optional conditioning on a progress variable and a stoichiometry variable) on MI355X.
//   jpdf3d.ex infile="<plt> ..." vars="<name> <name> ..." [nBins=64] [finestLevel=<n>] [outSuffix=<s>] [useminmax<i>="min max"]
//       [do_conditioning=0|1|2 cVar=<i> norm_cVal=0|1 cNormMin= cNormMax= cMin= cMax=] [do_average=0] [do_stoichiometry=0 Hlist= Olist=]
//       [output_gnuplot=0 output_matlab=0 output_tecplot=0 output_fab=0 output_plotfile=1 output_scatter=0]
// Host side (this file): the keys (:82-243), vMin / vMax of every variable over levels 0 .. finestLevel with the useminmax overrides
// (:297-326), jpdf.cpp:571-589 on the raw sums, every writer (:595-870) and the average over the plotfiles (:875-1070).  Device side
// (pa_stats.hip): one min / max launch per level, then ONE accumulate launch per level and group of 6 pairs; a level's variables are
// uploaded, used and released, so a file larger than device memory streams through (everything stays resident when it fits).
// NUMERICS: axes, bin indices, the out-of-range counters and everything derived from them are exact; bin / binX1 /
// binX2 are fixed-point sums rounded once per plotfile -- not the reference's cell-after-cell additions; the average adds the files'
// sums in infile order.
// Deviations, all stated in INTEGRATION.md: vMax == vMin aborts (the reference divides by zero); a quotient that is NaN or outside
// int is defined (NaN skips the cell for the pair, one warning line with the count); at most 8 variables; ngpus > 1 and 2-D
// plotfiles abort; the out-of-range counters are 64-bit.
#include "../common/pa_device.h"

#include <cmath>
#include <sys/stat.h>

namespace {

std::string ProtectSlashes(std::string s) {  // :27-42
  for (char& c : s)
    if (c == '/') c = '_';
  return s;
}

void make_dir(const std::string& d) {
  if (mkdir(d.c_str(), 0755) != 0 && errno != EEXIST) pa::Abort("Couldn't create directory: " + d);
}

struct Outputs { int gnuplot = 0, matlab = 0, tecplot = 0, fab = 0, plotfile = 1, scatter = 0; };

// jpdf.cpp:556-738 (and :893-1066 for the average): finish the raw sums of every pair and write the text / fab outputs into `dir`
void write_pairs(const std::string& dir, const Outputs& O, int nVars, int nBins, const std::vector<std::string>& whichVar, const std::vector<std::string>& whichVarOut,
                 const std::vector<double>& vMin, const std::vector<double>& vMax, std::vector<double>& binA, std::vector<double>& binX1A,
                 std::vector<double>& binX2A, double divisor, bool print_box) {
  const double small = 1.e-7;
  const size_t nb2 = (size_t)nBins * nBins;
  int iPair = 0;
  for (int var1 = 0; var1 < nVars; var1++) {
    const double dv1 = (vMax[var1] - vMin[var1]) / (double)nBins;
    for (int var2 = var1 + 1; var2 < nVars; var2++, iPair++) {
      const double dv2 = (vMax[var2] - vMin[var2]) / (double)nBins;
      double* bin = binA.data() + (size_t)iPair * nb2;
      double* binX1 = binX1A.data() + (size_t)iPair * nb2;
      double* binX2 = binX2A.data() + (size_t)iPair * nb2;
      for (int v1i = 0, i = 0; v1i < nBins; v1i++) {  // :571-585
        const double v1 = vMin[var1] + dv1 * (0.5 + (double)v1i);
        for (int v2i = 0; v2i < nBins; v2i++, i++) {
          const double v2 = vMin[var2] + dv2 * (0.5 + (double)v2i);
          const double div = bin[i];
          if (div > 0) { binX1[i] /= div; binX2[i] /= div; }
          else { binX1[i] = v1; binX2[i] = v2; }
        }
      }
      for (size_t i = 0; i < nb2; i++) bin[i] /= divisor;  // :588-589
      const std::string base = dir + "/", pn = whichVarOut[var1] + "_" + whichVarOut[var2];
      std::string filename;
      auto open = [&](const std::string& name) {
        filename = base + name;
        std::cout << "Opening file " << filename << std::endl;
        FILE* f = fopen(filename.c_str(), "w");
        if (!f) pa::Abort("Unable to create " + filename);
        return f;
      };
      auto matrix = [&](const std::string& name, const double* a) {
        FILE* file = open(name);
        for (int v1i = 0; v1i < nBins; v1i++) {
          for (int v2i = 0; v2i < nBins; v2i++) fprintf(file, "%e ", a[v1i * nBins + v2i]);
          fprintf(file, "\n");
        }
        fclose(file);
      };
      if (O.gnuplot) {
        FILE* file = open("Pdf_" + pn + ".gpd");
        for (int v1i = 0; v1i < nBins; v1i++) {
          const double v1 = vMin[var1] + dv1 * (0.5 + (double)v1i);
          for (int v2i = 0; v2i < nBins; v2i++) fprintf(file, "%e %e %e\n", v1, vMin[var2] + dv2 * (0.5 + (double)v2i), bin[v1i * nBins + v2i]);
        }
        fclose(file);
      }
      if (O.matlab) {
        matrix("Pdf_" + pn + ".dat", bin);
        FILE* file = open("Pdf_" + whichVarOut[var1] + "_x.dat");
        for (int v1i = 0; v1i < nBins; v1i++) fprintf(file, "%e\n", vMin[var1] + dv1 * (0.5 + (double)v1i));
        fclose(file);
        file = open("Pdf_" + whichVarOut[var2] + "_x.dat");
        for (int v2i = 0; v2i < nBins; v2i++) fprintf(file, "%e\n", vMin[var2] + dv2 * (0.5 + (double)v2i));
        fclose(file);
        matrix("PdfX1_" + pn + ".dat", binX1);
        matrix("PdfX2_" + pn + ".dat", binX2);
      }
      if (O.tecplot) {
        FILE* file = open("Pdf_" + pn + ".tpd");
        fprintf(file, "VARIABLES = %s %s logpdf pdf\n", whichVar[var1].c_str(), whichVar[var2].c_str());
        fprintf(file, "ZONE N=%i E=%i F=FEPOINT ET=QUADRILATERAL\n", nBins * nBins, (nBins - 1) * (nBins - 1));
        for (int v1i = 0; v1i < nBins; v1i++) {
          const double v1 = vMin[var1] + dv1 * (0.5 + (double)v1i);
          for (int v2i = 0; v2i < nBins; v2i++) {
            const double p = bin[v1i * nBins + v2i];
            fprintf(file, "%e %e %e %e\n", v1, vMin[var2] + dv2 * (0.5 + (double)v2i), log(p + small), p);
          }
        }
        for (int v1i = 0; v1i < nBins - 1; v1i++)
          for (int v2i = 0; v2i < nBins - 1; v2i++)
            fprintf(file, "%i %i %i %i\n", v1i * nBins + v2i + 1, (v1i + 1) * nBins + v2i + 1, (v1i + 1) * nBins + (v2i + 1) + 1, v1i * nBins + (v2i + 1) + 1);
        fclose(file);
      }
      if (O.fab) {  // a 4-component FAB on ((0,0,0) (nBins-1,nBins-1,0)): index (v1i, v2i), v1i fastest
        filename = base + "Pdf_" + pn + ".fab";
        std::cout << "Opening file " << filename << std::endl;
        std::ofstream os(filename.c_str(), std::ios::binary);
        if (!os) pa::Abort("Unable to create " + filename);
        const pa::Box3 bx{{0, 0, 0}, {nBins - 1, nBins - 1, 0}};
        if (print_box) std::cout << "box: ((0,0,0) (" << nBins - 1 << "," << nBins - 1 << ",0) (0,0,0))" << std::endl;
        std::vector<double> d(4 * nb2);
        for (int v1i = 0; v1i < nBins; v1i++)
          for (int v2i = 0; v2i < nBins; v2i++) {
            const double p = bin[v1i * nBins + v2i];
            const size_t o = (size_t)v2i * nBins + v1i;
            d[o] = vMin[var1] + dv1 * (0.5 + (double)v1i);
            d[nb2 + o] = vMin[var2] + dv2 * (0.5 + (double)v2i);
            d[2 * nb2 + o] = log(p + small);
            d[3 * nb2 + o] = p;
          }
        pa::write_fab(os, bx, 4, d.data());
      }
      if (O.scatter) {
        FILE* file = open("Scatter_" + pn + ".dat");
        for (int v1i = 0; v1i < nBins; v1i++)
          for (int v2i = 0; v2i < nBins; v2i++)
            if (bin[v1i * nBins + v2i] > 0) fprintf(file, "%e %e\n", vMin[var1] + dv1 * (0.5 + (double)v1i), vMin[var2] + dv2 * (0.5 + (double)v2i));
        fclose(file);
      }
    }
  }
}

}  // namespace

int main(int argc, char** argv) {
  pa::ParmParse pp(argc, argv);
  int ngpus = 1;
  pp.query("ngpus", ngpus);
  if (ngpus > 1) pa::Abort("ngpus > 1 is not supported by jpdf3d (one GPU)");
  Outputs O;
  std::cout << "Output types:" << std::endl;
  pp.query("output_gnuplot", O.gnuplot);
  if (O.gnuplot) std::cout << "   + gnuplot" << std::endl;
  pp.query("output_matlab", O.matlab);
  if (O.matlab) std::cout << "   + matlab" << std::endl;
  pp.query("output_tecplot", O.tecplot);
  if (O.tecplot) std::cout << "   + tecplot" << std::endl;
  pp.query("output_fab", O.fab);
  if (O.fab) std::cout << "   + fab" << std::endl;
  pp.query("output_plotfile", O.plotfile);
  if (O.plotfile) std::cout << "   + plotfile" << std::endl;
  pp.query("output_scatter", O.scatter);
  if (O.scatter) std::cout << "   + scatter" << std::endl;

  pa_jpdf_params P{};
  P.cmax = 1.0;
  P.cnorm_max = 1.0;
  pp.query("do_conditioning", P.do_conditioning);
  std::cout << "do_conditioning = " << P.do_conditioning << std::endl;
  if (P.do_conditioning > 0) {
    pp.query("cVar", P.cvar);
    std::cout << "cVar = " << P.cvar << std::endl;
    pp.query("norm_cVal", P.norm_cval);
    std::cout << "norm_cVal = " << P.norm_cval << std::endl;
    if (P.do_conditioning == 2) P.norm_cval = 1;
    if (P.norm_cval == 1) {
      pp.query("cNormMin", P.cnorm_min);
      std::cout << "cNormMin = " << P.cnorm_min << std::endl;
      pp.query("cNormMax", P.cnorm_max);
      std::cout << "cNormMax = " << P.cnorm_max << std::endl;
    }
    pp.query("cMin", P.cmin);
    std::cout << "cMin = " << P.cmin << std::endl;
    pp.query("cMax", P.cmax);
    std::cout << "cMax = " << P.cmax << std::endl;
  }
  if (P.do_conditioning < 0 || P.do_conditioning > 2) pa::Abort("do_conditioning must be 0, 1 or 2");
  int do_average = 0;
  pp.query("do_average", do_average);
  if (do_average) std::cout << "   + forming average" << std::endl;

  const int nPlotFiles = pp.countval("infile");
  if (nPlotFiles <= 0) {
    std::cerr << "Bad nPlotFiles:  " << nPlotFiles << std::endl;
    std::cerr << "Exiting." << std::endl;
    return 1;
  }
  std::cout << "Processing " << nPlotFiles << " plotfiles..." << std::endl;
  std::string outSuffix = "";
  pp.query("outSuffix", outSuffix);
  std::vector<std::string> plotFileNames((size_t)nPlotFiles);
  for (int i = 0; i < nPlotFiles; ++i) {
    pp.get("infile", plotFileNames[(size_t)i], i);
    std::cout << "   " << plotFileNames[(size_t)i] << std::endl;
  }
  int inFinestLevel = -1;
  pp.query("finestLevel", inFinestLevel);
  int nBins = 64;
  pp.query("nBins", nBins);
  if (nBins < 1 || nBins > 4096) pa::Abort("nBins must be 1 .. 4096");
  int nVars = pp.countval("vars");
  const int lVars = nVars;
  if (nVars < 2) pa::Abort("Need to specify at least two variables.");
  int do_stoichiometry = 0;
  pp.query("do_stoichiometry", do_stoichiometry);
  int sVar = -1;
  if (do_stoichiometry) { do_stoichiometry = 1; sVar = nVars; nVars++; }
  if (nVars > PA_STATS_MAXV) pa::Abort("at most " + std::to_string(PA_STATS_MAXV) + " variables (stoichiometry included)");
  if (P.do_conditioning > 0 && (P.cvar < 0 || P.cvar >= nVars)) pa::Abort("cVar out of range");
  std::vector<std::string> whichVar((size_t)nVars);
  std::cout << "Variable list:" << std::endl;
  for (int v = 0; v < lVars; v++) {
    pp.get("vars", whichVar[(size_t)v], v);
    std::cout << "   " << whichVar[(size_t)v] << std::endl;
  }
  if (do_stoichiometry) whichVar[(size_t)sVar] = "Stoichiometry";
  std::vector<std::string> whichVarOut((size_t)nVars);
  for (int i = 0; i < nVars; i++) {
    whichVarOut[(size_t)i] = ProtectSlashes(whichVar[(size_t)i]);
    std::cout << whichVar[(size_t)i] << " -> " << whichVarOut[(size_t)i] << std::endl;
  }
  P.nload = lVars;
  P.do_stoichiometry = do_stoichiometry;
  if (do_stoichiometry) {
    if (pp.countval("Hlist") != lVars) pa::Abort("Need to specify one Hlist entry per variable");
    if (pp.countval("Olist") != lVars) pa::Abort("Need to specify one Olist entry per variable");
    std::cout << "Doing stoichiometry:" << std::endl;
    for (int v = 0; v < lVars; v++) {
      int h = 0, o = 0;
      pp.get("Hlist", h, v);
      pp.get("Olist", o, v);
      P.hlist[v] = (double)h;
      P.olist[v] = (double)o;
      std::cout << "   " << whichVar[(size_t)v] << " : #H=" << h << " : #O=" << o << std::endl;
    }
  }
  const int nPairs = nVars * (nVars - 1) / 2;
  const size_t nb2 = (size_t)nBins * nBins, nAll = (size_t)nPairs * nb2;
  double domainVol = 1;
  std::vector<double> binAv, binAvX1, binAvX2, vMin((size_t)nVars), vMax((size_t)nVars);
  pa::AsyncCtx actx;

  for (int iPlot = 0; iPlot < nPlotFiles; iPlot++) {
    const std::string infile = plotFileNames[(size_t)iPlot];
    std::cout << "\nOpening " << infile << "..." << std::endl;
    const pa::PlotfileHeader H = pa::read_header(infile, 3, true);
    std::cout << "   ...done." << std::endl;
    std::vector<int> fileComp;
    for (int v = 0; v < lVars; v++) {
      const int c = H.comp(whichVar[(size_t)v]);
      if (c < 0) pa::Abort("Bad variable name (" + whichVar[(size_t)v] + ")");
      fileComp.push_back(c);
    }
    int finestLevel = H.nlev - 1;
    if (inFinestLevel > -1 && inFinestLevel < finestLevel) {
      finestLevel = inFinestLevel;
      std::cout << "Finest level: " << finestLevel << std::endl;
    }
    const int nLevels = finestLevel + 1;

    pa::Ctx& ctx = actx.get();
    const int per[3] = {0, 0, 0};
    std::vector<std::unique_ptr<pa::DevLevel>> dl;
    for (int l = 0; l < nLevels; ++l) dl.emplace_back(new pa::DevLevel(ctx, H.lev[l].boxes, H.lev[l].domain, per, H.prob_lo, H.prob_hi));
    int64_t freeB = 0, totalB = 0, needB = 0;
    ctx.check(pa_device_mem_info(ctx.h, &freeB, &totalB));
    for (int l = 0; l < nLevels; ++l) {
      pa::HostMF probe;
      std::vector<int32_t> b6(6 * H.lev[l].boxes.size());
      for (size_t i = 0; i < H.lev[l].boxes.size(); ++i)
        for (int d = 0; d < 3; ++d) { b6[6 * i + d] = H.lev[l].boxes[i].lo[d]; b6[6 * i + 3 + d] = H.lev[l].boxes[i].hi[d]; }
      std::vector<int64_t> off(H.lev[l].boxes.size()), cs(H.lev[l].boxes.size());
      needB += 8 * pa_mf_layout((int)H.lev[l].boxes.size(), b6.data(), lVars, 0, off.data(), cs.data());
    }
    const bool resident = needB < freeB / 10 * 8;
    std::vector<std::unique_ptr<pa::DevMF>> kept((size_t)nLevels);
    auto load = [&](int l) -> std::unique_ptr<pa::DevMF> {
      pa::HostMF h;
      h.define(H.lev[l].boxes, lVars, 0);
      for (int v = 0; v < lVars; ++v) pa::read_comp(H, l, fileComp[(size_t)v], h, v);
      std::unique_ptr<pa::DevMF> m(new pa::DevMF(ctx, *dl[(size_t)l], lVars, 0));
      ctx.check(pa_mf_upload(ctx.h, m->h, h.data.data()));
      return m;
    };
    // :297-326: exact minimum / maximum of every loaded variable over EVERY valid cell of levels 0 .. finestLevel
    std::cout << "Loading data..." << std::endl;
    std::vector<int32_t> cl((size_t)lVars);
    for (int v = 0; v < lVars; ++v) { cl[(size_t)v] = v; vMin[(size_t)v] = 1e100; vMax[(size_t)v] = -1e100; }
    for (int l = 0; l < nLevels; ++l) {
      std::cout << "   Level " << l << "..." << std::endl;
      std::unique_ptr<pa::DevMF> m = load(l);
      std::vector<double> mn((size_t)lVars), mx((size_t)lVars);
      ctx.check(pa_minmax_comps_level(ctx.h, m->h, lVars, cl.data(), mn.data(), mx.data()));
      for (int v = 0; v < lVars; ++v) {
        if (vMin[(size_t)v] > mn[(size_t)v]) vMin[(size_t)v] = mn[(size_t)v];
        if (vMax[(size_t)v] < mx[(size_t)v]) vMax[(size_t)v] = mx[(size_t)v];
      }
      if (resident) kept[(size_t)l] = std::move(m);
    }
    std::cout << "      ...done." << std::endl;
    std::vector<double> vabs((size_t)nVars);
    for (int v = 0; v < lVars; ++v) {
      vabs[(size_t)v] = std::max(std::fabs(vMin[(size_t)v]), std::fabs(vMax[(size_t)v]));
      if (!std::isfinite(vabs[(size_t)v])) pa::Abort("variable " + whichVar[(size_t)v] + " of " + infile + " holds values that are not finite");
    }
    if (do_stoichiometry) { vMin[(size_t)sVar] = 0.0; vMax[(size_t)sVar] = 2.0; vabs[(size_t)sVar] = std::ldexp(1.0, 40); }
    for (int iVar = 0; iVar < nVars; iVar++) {
      const std::string argName = "useminmax" + std::to_string(iVar + 1);
      const int nMinMax = pp.countval(argName);
      if (nMinMax > 0) {
        if (nMinMax != 2) pa::Abort("Need to specify 2 values for useMinMax");
        pp.get(argName, vMin[(size_t)iVar], 0);
        pp.get(argName, vMax[(size_t)iVar], 1);
        std::cout << "Var" << iVar + 1 << " (" << whichVar[(size_t)iVar] << ") using min/max: " << vMin[(size_t)iVar] << " / " << vMax[(size_t)iVar] << std::endl;
      }
    }
    for (int v = 0; v < nVars; ++v) {
      if (!(vMax[(size_t)v] != vMin[(size_t)v])) pa::Abort("vMax == vMin for variable " + whichVar[(size_t)v] + ": no bins");
      P.vmin[v] = vMin[(size_t)v];
      P.vmax[v] = vMax[(size_t)v];
    }
    if (do_stoichiometry)
      for (int l = 0; l < nLevels; ++l) std::cout << "      Level " << l << std::endl;

    // :423-527
    pa_hist* acc = pa_jpdf_create(ctx.h, nVars, nBins);
    if (!acc) pa::Abort(pa_last_error(ctx.h));
    const double vol0 = H.file_dx[0][0] * H.file_dx[0][1] * H.file_dx[0][2];
    ctx.check(pa_jpdf_begin(ctx.h, acc, vol0, vabs.data()));
    std::vector<int64_t> outside((size_t)nLevels * (size_t)nPairs * 4), nanc((size_t)nPairs, 0);
    for (int l = 0; l < nLevels; ++l) {
      std::unique_ptr<pa::DevMF> m = resident ? std::move(kept[(size_t)l]) : load(l);
      double Vol = H.file_dx[(size_t)l][0] * H.file_dx[(size_t)l][1];
      Vol *= H.file_dx[(size_t)l][2];
      std::vector<int64_t> nn((size_t)nPairs);
      ctx.check(pa_jpdf_add_level(ctx.h, acc, m->h, l < finestLevel ? dl[(size_t)l + 1]->h : nullptr, l < finestLevel ? H.ref_ratio[(size_t)l] : 1, Vol, &P,
                                  outside.data() + (size_t)l * (size_t)nPairs * 4, nn.data()));
      for (int p = 0; p < nPairs; ++p) nanc[(size_t)p] += nn[(size_t)p];
    }
    std::cout << "Evaluating pdfs..." << std::endl;
    {
      int iPair = 0;
      int64_t nans = 0;
      for (int var1 = 0; var1 < nVars; var1++)
        for (int var2 = var1 + 1; var2 < nVars; var2++, iPair++) {
          std::cout << "   + " << whichVar[(size_t)var1] << "-" << whichVar[(size_t)var2] << std::endl;
          for (int l = 0; l < nLevels; ++l) {
            std::cout << "      Level " << l << std::endl;
            const int64_t* c = outside.data() + ((size_t)l * (size_t)nPairs + (size_t)iPair) * 4;
            if (c[0]) std::cout << "v1i<0:      " << c[0] << std::endl;
            if (c[1]) std::cout << "v1i>=nBins: " << c[1] << std::endl;
            if (c[2]) std::cout << "v2i<0:      " << c[2] << std::endl;
            if (c[3]) std::cout << "v2i>=nBins: " << c[3] << std::endl;
          }
          nans += nanc[(size_t)iPair];
        }
      if (nans) std::cout << "Warning: " << nans << " (cell, pair) contributions skipped: the bin quotient is NaN" << std::endl;
    }
    std::cout << "   ...done." << std::endl;
    std::vector<double> bin(nAll), binX1(nAll), binX2(nAll);
    ctx.check(pa_jpdf_read(ctx.h, acc, bin.data(), binX1.data(), binX2.data()));
    pa_hist_destroy(acc);
    if (do_average) {  // :499-503: the files' sums, added in infile order
      if (iPlot == 0) { binAv.assign(nAll, 0.0); binAvX1.assign(nAll, 0.0); binAvX2.assign(nAll, 0.0); }
      for (size_t i = 0; i < nAll; ++i) { binAv[i] += bin[i]; binAvX1[i] += binX1[i]; binAvX2[i] += binX2[i]; }
    }

    if (outSuffix != "") make_dir(infile + outSuffix);
    domainVol = 1;
    for (int dd = 0; dd < 3; ++dd) domainVol *= H.prob_hi[dd] - H.prob_lo[dd];
    write_pairs(infile + outSuffix, O, nVars, nBins, whichVar, whichVarOut, vMin, vMax, bin, binX1, binX2, domainVol, true);

    if (O.plotfile) {  // :742-870: the bins transposed, then their log(small + bin), on one 2-D grid
      const double small = 1.e-7;
      const std::string pltfile = outSuffix != "" ? infile + outSuffix : infile + "jpdf";
      make_dir(pltfile);
      std::vector<std::string> pairNames;
      for (int var1 = 0; var1 < nVars; var1++)
        for (int var2 = var1 + 1; var2 < nVars; var2++) pairNames.push_back("Pdf_" + whichVar[(size_t)var1] + "_" + whichVar[(size_t)var2]);
      pa::write_jpdf_header(pltfile + "/Header", pairNames, H.time, nBins, vMin, vMax);
      make_dir(pltfile + "/Level_0");
      std::vector<double> d(2 * nAll);
      std::vector<std::vector<double>> mins(1, std::vector<double>(2 * (size_t)nPairs, 1e300)), maxs(1, std::vector<double>(2 * (size_t)nPairs, -1e300));
      for (int p = 0; p < nPairs; ++p)
        for (int v1i = 0; v1i < nBins; v1i++)
          for (int v2i = 0; v2i < nBins; v2i++) {
            const double b = bin[(size_t)p * nb2 + (size_t)v1i * nBins + v2i];
            d[(size_t)p * nb2 + (size_t)v2i * nBins + v1i] = b;
            d[((size_t)p + nPairs) * nb2 + (size_t)v2i * nBins + v1i] = log(small + b);
          }
      for (size_t c = 0; c < 2 * (size_t)nPairs; ++c) pa::minmax_run(d.data() + c * nb2, (long long)nb2, mins[0][c], maxs[0][c]);
      const pa::Box3 bx{{0, 0, 0}, {nBins - 1, nBins - 1, 0}};
      std::ofstream os(pltfile + "/Level_0/Cell_D_00000", std::ios::binary);
      if (!os) pa::Abort("Unable to create " + pltfile + "/Level_0/Cell_D_00000");
      pa::write_fab(os, bx, 2 * nPairs, d.data());
      pa::write_vismf_header(pltfile + "/Level_0/Cell_H", "Cell_D_00000", 2 * nPairs, {pa::box_str(bx)}, {0}, mins, maxs);
    }
  }

  if (do_average) {  // :875-1070, axes = the LAST plotfile's vMin / vMax
    const std::string oFile = "JPDFAverage" + outSuffix;
    make_dir(oFile);
    write_pairs(oFile, O, nVars, nBins, whichVar, whichVarOut, vMin, vMax, binAv, binAvX1, binAvX2, domainVol * (double)nPlotFiles, false);
  }
  pa::Finish();
}
