// rmsVel3d -- drop-in for PeleAnalysis Src/rmsVel.cpp (the u_rms time series over a list of plotfiles) on MI355X.
//   rmsVel3d.ex infiles="<plt> ..." [finestLevel=<n>]
// The variables are fixed: x_velocity, y_velocity, z_velocity.  For each file the boxes of finestLevel ONLY are summed -- no composite
// and no mask of covered cells: that is the reference's behaviour (:72-78) -- with weight dx*dy*dz of that level (:68).  Device side
// (pa_integral.hip): kind 3 with squares and no finer level gives the seven sums vol, uxb, uyb, uzb, ux2, uy2, uz2 (:82-122) as
// fixed-point sums rounded once; the host arithmetic of :123-125 is kept in its order.  Output: RmsVel.dat in the working directory,
// "%e %e\n" = time, urms per file (:130-135).
// Deviations: ngpus > 1, a 2-D plotfile, a file without the three velocities and an output file that cannot be
// opened abort with a message.
#include "../common/pa_device.h"

#include <cmath>
#include <cstdio>

int main(int argc, char** argv) {
  pa::ParmParse pp(argc, argv);
  int ngpus = 1;
  pp.query("ngpus", ngpus);
  if (ngpus > 1) pa::Abort("ngpus > 1 is not supported by rmsVel3d (one GPU)");
  const int nPlotFiles = pp.countval("infiles");
  if (nPlotFiles <= 0) pa::Abort("need to specify infiles");
  std::vector<std::string> plotFileNames;
  pp.getarr("infiles", plotFileNames);
  const int nVars = 3;
  const std::string whichVar[3] = {"x_velocity", "y_velocity", "z_velocity"};

  std::vector<pa::PlotfileHeader> headers;
  std::vector<double> time((size_t)nPlotFiles), urms((size_t)nPlotFiles);
  for (int iPlot = 0; iPlot < nPlotFiles; ++iPlot) {
    std::cout << "Loading " << plotFileNames[(size_t)iPlot] << std::endl;
    headers.push_back(pa::read_header(plotFileNames[(size_t)iPlot], 3, true));
    time[(size_t)iPlot] = headers.back().time;
  }
  pa::AsyncCtx actx;
  for (int iPlot = 0; iPlot < nPlotFiles; iPlot++) {
    const pa::PlotfileHeader& H = headers[(size_t)iPlot];
    int finestLevel = H.nlev - 1;
    int inFinestLevel = -1;
    pp.query("finestLevel", inFinestLevel);
    if (inFinestLevel > -1 && inFinestLevel < finestLevel) {
      finestLevel = inFinestLevel;
      std::cout << "Finest level: " << finestLevel << std::endl;
    }
    int comp[3];
    for (int v = 0; v < nVars; v++) {
      comp[v] = H.comp(whichVar[v]);
      if (comp[v] < 0) pa::Abort("variable " + whichVar[v] + " is not in " + plotFileNames[(size_t)iPlot]);
    }
    const std::array<double, 3>& dx = H.file_dx[(size_t)finestLevel];
    const double dxyz = dx[0] * dx[1] * dx[2];
    std::cout << "Processing " << iPlot << "/" << nPlotFiles << std::endl;
    const pa::LevelMeta& L = H.lev[(size_t)finestLevel];
    pa::HostMF h;
    h.define(L.boxes, nVars, 0);
    double vabs[3] = {0.0, 0.0, 0.0};
    for (int v = 0; v < nVars; v++) pa::read_comp(H, finestLevel, comp[v], h, v);
    for (size_t b = 0; b < h.boxes.size(); ++b)  // the magnitude of the finite values: the scale of the fixed-point sums
      for (int v = 0; v < nVars; v++) {
        const double* p = h.data.data() + h.off[b] + (long long)v * h.cs[b];
        for (long long q = 0, nq = h.boxes[b].numPts(); q < nq; ++q) {
          const double a = std::fabs(p[q]);
          if (a > vabs[v] && std::isfinite(a)) vabs[v] = a;
        }
      }
    pa::Ctx& ctx = actx.get();
    const int per[3] = {0, 0, 0};
    pa::DevLevel dl(ctx, L.boxes, L.domain, per, H.prob_lo, H.prob_hi);
    pa::DevMF m(ctx, dl, nVars, 0);
    ctx.check(pa_mf_upload(ctx.h, m.h, h.data.data()));
    pa_box dom;
    for (int d = 0; d < 3; ++d) { dom.lo[d] = L.domain.lo[d]; dom.hi[d] = L.domain.hi[d]; }
    pa_integral* acc = pa_integral_create(ctx.h, nVars, 3, 0, &dom, 1);
    if (!acc) pa::Abort(pa_last_error(ctx.h));
    ctx.check(pa_integral_begin(ctx.h, acc, dxyz, vabs));
    ctx.check(pa_integral_add_level(ctx.h, acc, m.h, nullptr, 1, 1, dxyz, -1, 0.0, 0.0, 0));
    double s[7];
    ctx.check(pa_integral_read(ctx.h, acc, s));
    pa_integral_destroy(acc);
    double vol = s[0], uxb = s[1], uyb = s[2], uzb = s[3], ux2 = s[4], uy2 = s[5], uz2 = s[6];
    uxb /= vol; uyb /= vol; uzb /= vol;  // :123-125
    ux2 /= vol; uy2 /= vol; uz2 /= vol;
    urms[(size_t)iPlot] = std::sqrt(((ux2 - uxb * uxb) + (uy2 - uyb * uyb) + (uz2 - uzb * uzb)) / 3.);
  }
  std::cout << "   ...done." << std::endl;
  FILE* file = std::fopen("RmsVel.dat", "w");
  if (!file) pa::Abort("Unable to create RmsVel.dat");
  for (int iPlot = 0; iPlot < nPlotFiles; iPlot++) std::fprintf(file, "%e %e\n", time[(size_t)iPlot], urms[(size_t)iPlot]);
  std::fclose(file);
  pa::Finish();
}
