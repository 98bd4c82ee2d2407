// integral3d -- drop-in for PeleAnalysis Src/integral.cpp (line, plane and volume integrals or averages of plotfile variables over the
// composite AMR hierarchy, optionally restricted to the cells where one variable lies in a window) on MI355X.
//   integral3d.ex infile=<plt> vars="<name> ..." integralDimension=<1|2|3> [finestLevel=<n>] [cVar=<name> cMin=<v> cMax=<v>] [avg=0]
//       integralDimension=1: dir=<d> [format=dat|ppm] [goPastMax=1] [useminmaxN="<min> <max>"]      integralDimension=2: dir1=<d> dir2=<d>
// Host side (this file): the keys (:318-412), the output names (:403-412), avg (:51-58, :107-112, :143-147), the coordinates and the
// writers (:226-316, :453-529).  Device side (pa_integral.hip): one accumulate launch per level; the variables of a group are read
// once, kept on the host, and every level is uploaded, integrated and released, so only one level is resident on the device.
// NUMERICS: the measure is exact; every other sum is a fixed-point sum rounded once -- not the reference's
// cell-after-cell additions -- and a sum that met a NaN or an infinite term is what IEEE addition gives in any order.
// Kept: the output name is built from the infile string as given; writeDat1D ends without a newline; rows dir1, columns dir2;
// writePPM's colour map, row flip and defaults; vMax == vMin gives the 1.5 colour; stdout lines in the reference's order.
// Deviations, all stated in INTEGRATION.md (each aborts where the reference has undefined behaviour or silently does nothing):
//   cVar without both cMin and cMax; integralDimension outside 1..3; dir / dir1 / dir2 out of range or dir1 == dir2; empty vars or a
//   name that is not in the plotfile; a format other than dat or ppm; an output file that cannot be opened; ngpus > 1; a 2-D plotfile.
//   More than 8 variables are integrated in groups of 8 (the levels are read once per group).
#include "../common/pa_device.h"

#include <cmath>
#include <cstdio>

namespace {

FILE* open_out(const std::string& filename) {
  FILE* file = std::fopen(filename.c_str(), "w");
  if (!file) pa::Abort("Unable to create " + filename);
  return file;
}

void writeDat1D(const std::vector<double>& vect, const std::string& filename, int dim) {  // :226-233
  FILE* file = open_out(filename);
  for (int i = 0; i < dim; i++) std::fprintf(file, "%e ", vect[(size_t)i]);
  std::fclose(file);
}

void writeDat2D(const double* vect, const std::string& filename, int dim1, int dim2) {  // :235-245, vect[i][j] = vect[i * dim2 + j]
  FILE* file = open_out(filename);
  for (int i = 0; i < dim1; i++) {
    for (int j = 0; j < dim2; j++) std::fprintf(file, "%e ", vect[(size_t)i * dim2 + j]);
    std::fprintf(file, "\n");
  }
  std::fclose(file);
}

// the colour map of :253-296: blue - cyan - green - yellow - red - dark red up to 1, then (goPastMax == 1) magenta to white up to 1.5
void colour_rgb(double colour, int goPastMax, unsigned char* px) {
  auto ramp = [](double x) { return (unsigned char)(int)(x * 1020.); };
  unsigned char r, g, b;
  if (colour < 0.125) { r = 0; g = 0; b = ramp(colour + 0.125); }
  else if (colour < 0.375) { r = 0; g = ramp(colour - 0.125); b = 255; }
  else if (colour < 0.625) { r = ramp(colour - 0.375); g = 255; b = ramp(0.625 - colour); }
  else if (colour < 0.875) { r = 255; g = ramp(0.875 - colour); b = 0; }
  else if (colour < 1.000) { r = ramp(1.125 - colour); g = 0; b = 0; }
  else if (goPastMax != 1) { r = 128; g = 0; b = 0; }  // above the maximum, not going past it
  else if (colour < 1.125) { r = ramp(colour - 0.875); g = 0; b = ramp(colour - 1.000); }
  else if (colour < 1.250) { r = 255; g = 0; b = ramp(colour - 1.000); }
  else if (colour < 1.500) { r = 255; g = ramp(colour - 1.250); b = 255; }
  else { r = 255; g = 255; b = 255; }  // 1.5: the clamp's ceiling, and what a NaN quotient (vMax == vMin) becomes
  px[0] = r; px[1] = g; px[2] = b;
}

void writePPM(const double* vect, const std::string& filename, int dim1, int dim2, int goPastMax, double vMin, double vMax) {  // :247-304
  std::vector<unsigned char> buff((size_t)3 * dim1 * dim2);
  for (int i = 0; i < dim1; i++)
    for (int j = 0; j < dim2; j++) {  // row i of the array is image row dim1 - i - 1 (:251)
      const double val = vect[(size_t)i * dim2 + j];
      const double colour = std::fmax(0., std::fmin(1.5, (val - vMin) / (vMax - vMin)));  // fmin / fmax drop a NaN
      colour_rgb(colour, goPastMax, buff.data() + ((size_t)(dim1 - i - 1) * dim2 + j) * 3);
    }
  FILE* file = open_out(filename);
  std::fprintf(file, "P6\n%i %i\n255\n", dim2, dim1);
  std::fwrite(buff.data(), (size_t)dim1 * dim2 * 3, sizeof(unsigned char), file);
  std::fclose(file);
}

void findMinMax(const double* vect, int dim1, int dim2, double& min, double& max) {  // :306-316
  min = vect[0];
  max = vect[0];
  for (size_t q = 0; q < (size_t)dim1 * dim2; ++q) {
    if (vect[q] < min) min = vect[q];
    if (vect[q] > max) max = vect[q];
  }
}

}  // namespace

int main(int argc, char** argv) {
  pa::ParmParse pp(argc, argv);
  int ngpus = 1;
  pp.query("ngpus", ngpus);
  if (ngpus > 1) pa::Abort("ngpus > 1 is not supported by integral3d (one GPU)");

  std::string infile;
  pp.get("infile", infile);
  std::cout << "infile = " << infile << std::endl;
  const pa::PlotfileHeader H = pa::read_header(infile, 3, true);

  const int nVars = pp.countval("vars");
  if (nVars < 1) pa::Abort("need to specify vars");
  std::vector<std::string> vars;
  pp.getarr("vars", vars);
  std::cout << "nVars= " << nVars << std::endl;
  for (int n = 0; n < nVars; n++) std::cout << "var[" << n << "]= " << vars[(size_t)n] << std::endl;
  std::vector<int> fileComp((size_t)nVars);
  for (int n = 0; n < nVars; n++) {
    fileComp[(size_t)n] = H.comp(vars[(size_t)n]);
    if (fileComp[(size_t)n] < 0) pa::Abort("variable " + vars[(size_t)n] + " is not in " + infile);
  }

  int integralDimension = 0;
  pp.get("integralDimension", integralDimension);
  if (integralDimension < 1 || integralDimension > 3) pa::Abort("integralDimension must be 1, 2 or 3");
  int finestLevel = H.nlev - 1;
  pp.query("finestLevel", finestLevel);
  if (finestLevel < 0 || finestLevel >= H.nlev) pa::Abort("finestLevel out of range");
  const int Nlev = finestLevel + 1;
  std::string cVar;
  double cMin = 0, cMax = 0;
  int cComp = -1;
  pp.query("cVar", cVar);
  const bool haveMin = pp.query("cMin", cMin), haveMax = pp.query("cMax", cMax);
  if (!cVar.empty()) {
    if (!haveMin || !haveMax) pa::Abort("cVar needs both cMin and cMax");
    for (int n = 0; n < nVars; n++) {
      if (vars[(size_t)n] == cVar) {
        cComp = n;
        break;
      }
    }
    if (cComp < 0) pa::Abort("cVar not in list of vars!");
  }
  int avg = 0;
  pp.query("avg", avg);
  int dir = 0, dir1 = 1, dir2 = 2;
  std::string format = "dat";
  std::cout << "integralDimension = " << integralDimension << std::endl;
  switch (integralDimension) {
    case 1: {
      pp.get("dir", dir);
      if (dir < 0 || dir > 2) pa::Abort("dir must be 0, 1 or 2");
      dir1 = (dir + 1) % 3;
      dir2 = (dir + 2) % 3;
      pp.query("format", format);
      if (format != "ppm" && format != "dat") pa::Abort("format must be dat or ppm");
      break;
    }
    case 2: {
      pp.get("dir1", dir1);
      pp.get("dir2", dir2);
      if (dir1 < 0 || dir1 > 2 || dir2 < 0 || dir2 > 2 || dir1 == dir2) pa::Abort("dir1 and dir2 must be two different directions out of 0, 1, 2");
      dir = 3 - dir1 - dir2;
      break;
    }
    default: break;  // case 3 doesn't care about directions
  }
  std::string outfile = infile + "_integral";
  if (integralDimension < 3) outfile += "_dir" + std::to_string(dir);
  if (!cVar.empty()) outfile += "_c" + cVar + "_" + std::to_string(cMin) + "_" + std::to_string(cMax);
  if (avg) outfile += "_avg";

  // the output at the finest level's resolution (:442-449, :497-501, :520)
  const pa::Box3& probDomain = H.lev[(size_t)finestLevel].domain;
  const int ldir = probDomain.hi[dir] - probDomain.lo[dir] + 1, ldir1 = probDomain.hi[dir1] - probDomain.lo[dir1] + 1,
            ldir2 = probDomain.hi[dir2] - probDomain.lo[dir2] + 1;
  const size_t nslots = integralDimension == 3 ? 1 : (integralDimension == 2 ? (size_t)ldir : (size_t)ldir1 * (size_t)ldir2);
  std::vector<double> outdata(((size_t)nVars + 1) * nslots, 0.0);
  // refRatio (:20-22, :79-83) and the weight of a cell of every level (:21, :80-82, :124-127)
  std::vector<int> R((size_t)Nlev, 1);
  for (int lev = finestLevel - 1; lev >= 0; lev--) R[(size_t)lev] = R[(size_t)lev + 1] * H.ref_ratio[(size_t)lev];
  std::vector<double> w((size_t)Nlev);
  double wmax = 0.0;
  for (int lev = 0; lev < Nlev; lev++) {
    const std::array<double, 3>& dx = H.file_dx[(size_t)lev];
    w[(size_t)lev] = integralDimension == 3 ? dx[0] * dx[1] * dx[2] : (integralDimension == 2 ? dx[(size_t)dir1] * dx[(size_t)dir2] : dx[(size_t)dir]);
    wmax = std::max(wmax, w[(size_t)lev]);
  }
  for (int lev = 0; lev < Nlev; lev++) std::cout << "Loading data on level " << lev << std::endl << "Data loaded" << std::endl;
  std::cout << "Determining intersects..." << std::endl;
  std::cout << "Intersects determined" << std::endl;

  pa::AsyncCtx actx;
  pa::Ctx& ctx = actx.get();
  const int per[3] = {0, 0, 0};
  std::vector<std::unique_ptr<pa::DevLevel>> dl;
  for (int lev = 0; lev < Nlev; lev++) dl.emplace_back(new pa::DevLevel(ctx, H.lev[(size_t)lev].boxes, H.lev[(size_t)lev].domain, per, H.prob_lo, H.prob_hi));
  pa_box dom;
  for (int d = 0; d < 3; ++d) { dom.lo[d] = probDomain.lo[d]; dom.hi[d] = probDomain.hi[d]; }

  for (int n0 = 0, nload = 0; n0 < nVars; n0 += nload) {  // groups of at most 8 variables per accumulator
    const int ng = std::min(8, nVars - n0);
    const bool extra = cComp >= 0 && (cComp < n0 || cComp >= n0 + ng);  // the condition variable is not one of the group's: it rides behind them
    nload = (extra && ng == 8) ? 7 : ng;
    const int nacc = nload + (extra ? 1 : 0);
    const int ccomp = cComp < 0 ? -1 : (extra ? nload : cComp - n0);
    std::vector<pa::HostMF> host((size_t)Nlev);
    std::vector<double> vabs((size_t)nacc, 0.0);
    for (int lev = 0; lev < Nlev; lev++) {
      pa::HostMF& h = host[(size_t)lev];
      h.define(H.lev[(size_t)lev].boxes, nacc, 0);
      for (int a = 0; a < nload; ++a) pa::read_comp(H, lev, fileComp[(size_t)(n0 + a)], h, a);
      if (extra) pa::read_comp(H, lev, fileComp[(size_t)cComp], h, nload);
      for (size_t b = 0; b < h.boxes.size(); ++b)  // the magnitude of the finite values: the scale of the fixed-point sums
        for (int a = 0; a < nacc; ++a) {
          const double* p = h.data.data() + h.off[b] + (long long)a * h.cs[b];
          double m = vabs[(size_t)a];
          for (long long q = 0, nq = h.boxes[b].numPts(); q < nq; ++q) {
            const double v = std::fabs(p[q]);
            if (v > m && std::isfinite(v)) m = v;
          }
          vabs[(size_t)a] = m;
        }
    }
    pa_integral* acc = pa_integral_create(ctx.h, nacc, integralDimension, dir, &dom, 0);
    if (!acc) pa::Abort(pa_last_error(ctx.h));
    ctx.check(pa_integral_begin(ctx.h, acc, wmax, vabs.data()));
    for (int q = 0; q < Nlev; ++q) {
      const int lev = integralDimension == 3 ? q : finestLevel - q;  // :123 against :20, :79
      if (n0 == 0) std::cout << "Integrating level " << lev << std::endl;
      pa::DevMF m(ctx, *dl[(size_t)lev], nacc, 0);
      ctx.check(pa_mf_upload(ctx.h, m.h, host[(size_t)lev].data.data()));
      ctx.check(pa_integral_add_level(ctx.h, acc, m.h, lev < finestLevel ? dl[(size_t)lev + 1]->h : nullptr, lev < finestLevel ? H.ref_ratio[(size_t)lev] : 1,
                                      R[(size_t)lev], w[(size_t)lev], ccomp, cMin, cMax, 0));
      ctx.check(pa_sync(ctx.h));  // the level's data are released when m goes out of scope
      host[(size_t)lev] = pa::HostMF();
    }
    std::vector<double> got(((size_t)nacc + 1) * nslots);
    ctx.check(pa_integral_read(ctx.h, acc, got.data()));
    pa_integral_destroy(acc);
    if (n0 == 0) std::copy(got.begin(), got.begin() + (long)nslots, outdata.begin());
    for (int a = 0; a < nload; ++a) std::copy(got.begin() + (long)((size_t)(1 + a) * nslots), got.begin() + (long)((size_t)(2 + a) * nslots), outdata.begin() + (long)((size_t)(1 + n0 + a) * nslots));
  }
  if (avg) {  // :51-58, :107-112, :143-147
    for (int n = 1; n < nVars + 1; n++)
      for (size_t i = 0; i < nslots; i++)
        if (outdata[i] > 0.0) outdata[(size_t)n * nslots + i] /= outdata[i];
  }
  std::cout << "Integration completed" << std::endl;
  if (integralDimension == 3) format = "dat";
  std::cout << "Writing data as " + format << std::endl;
  auto coords = [&](int d, int n) {  // :60-70, :114-118
    std::vector<double> x((size_t)n);
    const double dxFine = H.file_dx[(size_t)finestLevel][(size_t)d];
    for (int i = 0; i < n; i++) x[(size_t)i] = H.prob_lo[d] + (i + 0.5) * dxFine;
    return x;
  };
  switch (integralDimension) {
    case 1: {
      if (format == "dat") {
        writeDat1D(coords(dir1, ldir1), outfile + "_x.dat", ldir1);
        writeDat1D(coords(dir2, ldir2), outfile + "_y.dat", ldir2);
        writeDat2D(outdata.data(), outfile + "_length.dat", ldir1, ldir2);
        for (int n = 1; n < nVars + 1; n++) writeDat2D(outdata.data() + (size_t)n * nslots, outfile + "_" + vars[(size_t)n - 1] + ".dat", ldir1, ldir2);
      } else if (format == "ppm") {
        int goPastMax = 1;
        pp.query("goPastMax", goPastMax);
        std::vector<double> vMin((size_t)nVars + 1), vMax((size_t)nVars + 1);
        findMinMax(outdata.data(), ldir1, ldir2, vMin[0], vMax[0]);
        for (int n = 1; n < nVars + 1; n++) {
          const std::string argName = "useminmax" + std::to_string(n);
          const int nMinMax = pp.countval(argName);
          if (nMinMax > 0) {
            std::cout << "Reading min/max from command line" << std::endl;
            if (nMinMax != 2) pa::Abort("Need to specify 2 values for useMinMax");
            pp.get(argName, vMin[(size_t)n], 0);
            pp.get(argName, vMax[(size_t)n], 1);
          } else {
            std::cout << "Using file values for min/max" << std::endl;
            findMinMax(outdata.data() + (size_t)n * nslots, ldir1, ldir2, vMin[(size_t)n], vMax[(size_t)n]);
          }
        }
        writePPM(outdata.data(), outfile + "_length.ppm", ldir1, ldir2, goPastMax, vMin[0], vMax[0]);
        for (int n = 1; n < nVars + 1; n++)
          writePPM(outdata.data() + (size_t)n * nslots, outfile + "_" + vars[(size_t)n - 1] + ".ppm", ldir1, ldir2, goPastMax, vMin[(size_t)n], vMax[(size_t)n]);
      }
      break;
    }
    case 2: {
      writeDat1D(coords(dir, ldir), outfile + "_x.dat", ldir);
      writeDat2D(outdata.data(), outfile + "_allVars.dat", nVars + 1, ldir);
      break;
    }
    default: {
      writeDat1D(outdata, outfile + "_allVars.dat", nVars + 1);
      break;
    }
  }
  pa::Finish();
}
