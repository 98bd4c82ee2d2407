// binMEF3d -- drop-in for PeleAnalysis Src/binMEF.cpp: the area-weighted PDF / joint PDF of node fields over a MEF surface on MI355X.
//   binMEF3d.ex infile=<file.mef> binComps="c ..." binMin="v ..." binMax="v ..." nBins="n ..."
//               [condApply=0 condComp=<c> condVal=<v> condSgn=<-1|0|1>] [areaEps=1e-20] [dumpBins=0]
//               [dumpFab=0 fabFileBase=bin normalize=0]
// Every triangle is clipped against the bin edges of each binned component (:231-331) and its pieces add their area to their bins:
// pa_binmef.hip.  Output as the reference's: the progress lines and the two (three with condApply) summary lines on stderr; on
// stdout one line per nonempty bin, in the order of the reference's map -- the bin centres, then the area -- or, with dumpFab and at
// most two components, <fabFileBase>.fab (divided by the sum of the bins with normalize).
// Deviations: the bin sums are rounded once from exact sums (the reference adds in element order); an element with
// a value that is not finite is skipped and reported on stderr; more than 4 binned components, more than 2^24 bins, elements that
// are not triangles and a component out of range abort with a message; a split fraction outside [0, 1] -- the reference's
// AMREX_ALWAYS_ASSERT (:121, :159) -- exits non-zero with that text.  One GPU.
#include "../common/pa_device.h"

#include <cmath>

int main(int argc, char** argv) {
  pa::ParmParse pp(argc, argv);
  bool dumpFab = false;
  pp.query("dumpFab", dumpFab);
  std::string fabFileBase = "bin";
  pp.query("fabFileBase", fabFileBase);
  int ngpus = 1;
  pp.query("ngpus", ngpus);
  if (ngpus > 1) pa::Abort("ngpus > 1 is not supported by binMEF3d (one GPU)");
  pa::AsyncCtx actx;  // the device comes up while the file is read

  std::string infile;
  pp.get("infile", infile);
  const pa::MefSurface S = pa::read_mef(infile);
  const int nComp = (int)S.names.size();
  std::cerr << "...finished reading data header" << std::endl;
  std::cerr << "..." << S.nNodes << " nodes read from data file (nComp=" << nComp << ")" << std::endl;
  std::cerr << "..." << S.nElts << " elements read from data file" << std::endl;
  std::cerr << "...finished reading data" << std::endl;
  if (S.nodesPerElt != 3) pa::Abort("binMEF3d needs 3 nodes per element, " + infile + " has " + std::to_string(S.nodesPerElt));
  if (nComp < 3) pa::Abort("binMEF3d needs the node coordinates x, y, z as the first three components");

  std::vector<int> binComps;
  const int nc = pp.countval("binComps");
  if (nc) {  // :417-428
    pp.getarr("binComps", binComps);
    for (int i = 0; i < nc; ++i)
      if (binComps[(size_t)i] >= nComp || binComps[(size_t)i] < 0) pa::Abort("At least one element in binComps out of range");
  } else {
    pa::Abort("Need to specify binComps array");
  }
  if (nc > 4) pa::Abort("binMEF3d bins at most 4 components");
  std::vector<double> binMin, binMax;
  std::vector<int> nBins;
  if (pp.countval("binMin") == nc) pp.getarr("binMin", binMin);
  else pa::Abort("Number of binMin components must match number of binComps components");
  if (pp.countval("binMax") == nc) pp.getarr("binMax", binMax);
  else pa::Abort("Number of binMax components must match number of binComps components");
  if (pp.countval("nBins") == nc) pp.getarr("nBins", nBins);
  else pa::Abort("Number of nBins components must match number of binComps components");
  long long nTot = 1;
  for (int j = 0; j < nc; ++j) {
    if (nBins[(size_t)j] <= 0) pa::Abort("nBins must be positive");  // BL_ASSERT(nBins[j]>0), :486
    nTot *= nBins[(size_t)j];
    if (nTot > (1LL << 24)) pa::Abort("binMEF3d holds at most 2^24 bins");
  }

  bool condApply = false;  // :465-475
  pp.query("condApply", condApply);
  int condComp = 0, condSgn = 0;
  double condVal = 0.;
  if (condApply) {
    pp.get("condComp", condComp);
    pp.get("condVal", condVal);
    pp.get("condSgn", condSgn);
    if (condComp < 0 || condComp >= nComp) pa::Abort("condComp out of range");
  }

  bool dumpBins = false;
  pp.query("dumpBins", dumpBins);
  std::vector<std::vector<double>> binLO((size_t)nc);
  for (int j = 0; j < nc; ++j) {  // :477-502
    const double dBin = (binMax[(size_t)j] - binMin[(size_t)j]) / nBins[(size_t)j];
    binLO[(size_t)j].resize((size_t)nBins[(size_t)j]);
    for (int i = 0; i < nBins[(size_t)j]; ++i) binLO[(size_t)j][(size_t)i] = binMin[(size_t)j] + i * dBin;
    if (dumpBins) {
      std::cout << "bin: " << binComps[(size_t)j] << " bounds: " << std::endl;
      for (int i = 0; i < nBins[(size_t)j]; ++i) {
        const double lo = binLO[(size_t)j][(size_t)i];
        const double hi = (i == nBins[(size_t)j] - 1 ? binMax[(size_t)j] : binLO[(size_t)j][(size_t)i + 1]);
        std::cout << "         bin: [" << lo << "," << hi << "]" << std::endl;
      }
      std::cout << std::endl;
    }
  }
  double areaEps = 1.e-20;
  pp.query("areaEps", areaEps);
  int uncombined = 0;
  long long workItems = 0;
  {
    double wi = 0;  // a count that may exceed an int: read as a real
    pp.query("uncombined", uncombined);
    if (pp.query("workItems", wi)) {
      if (!(wi >= 0) || wi > 9.0e15 || wi != std::floor(wi)) pa::Abort("workItems must be a whole number that is not negative");
      workItems = (long long)wi;
    }
  }

  // node-major -> one array per component (only x, y, z, the binned and the condition component are uploaded)
  const size_t N = (size_t)S.nNodes;
  std::vector<std::vector<double>> col((size_t)nComp);
  auto column = [&](int c) -> const double* {
    std::vector<double>& v = col[(size_t)c];
    if (v.empty() && N) {
      v.resize(N);
      for (size_t i = 0; i < N; ++i) v[i] = S.nodes[i * (size_t)nComp + (size_t)c];
    }
    return v.data();
  };
  const double *x = column(0), *y = column(1), *z = column(2);
  std::vector<const double*> comps;
  for (int j = 0; j < nc; ++j) comps.push_back(column(binComps[(size_t)j]));
  const double* cond = condApply ? column(condComp) : nullptr;
  const double areaMax = pa_surfbin_max_area(S.nNodes, x, y, z, S.nElts, S.conn.data());
  if (areaMax < 0) pa::Abort("an element of " + infile + " names a node that does not exist");

  pa::Ctx& ctx = actx.get();
  pa_surfbin* sb = pa_surfbin_create(ctx.h, nc, nBins.data(), binMin.data(), binMax.data(), workItems);
  if (!sb) pa::Abort(pa_last_error(ctx.h));
  ctx.check(pa_surfbin_begin(ctx.h, sb, areaMax));
  ctx.check(pa_surfbin_add_surface(ctx.h, sb, S.nNodes, x, y, z, comps.data(), cond, S.nElts, S.conn.data(), condApply ? 1 : 0, condSgn, condVal, areaEps,
                                   uncombined));
  std::vector<double> binArea((size_t)nTot);
  std::vector<int64_t> binHits((size_t)nTot);
  double area = 0, areaOutsideCondition = 0;
  int64_t counters[8];
  ctx.check(pa_surfbin_read(ctx.h, sb, binArea.data(), binHits.data(), &area, &areaOutsideCondition, counters));
  pa_surfbin_destroy(sb);

  // :594-670.  The table is in the order of the reference's map; a bin it would hold is one that was touched.
  long long nonempty = 0;
  double binSum = 0;
  for (long long k = 0; k < nTot; ++k)
    if (binHits[(size_t)k] > 0) {
      ++nonempty;
      binSum += binArea[(size_t)k];
    }
  std::cerr << "number of nonempty bins: " << nonempty << std::endl;
  if (dumpFab && nc <= 2) {
    const int n0 = nBins[0], n1 = nc == 2 ? nBins[1] : 1;
    std::vector<double> fab((size_t)n0 * (size_t)n1, 0.0);
    for (long long k = 0; k < nTot; ++k)
      if (binHits[(size_t)k] > 0) fab[(size_t)(k % n1) * (size_t)n0 + (size_t)(k / n1)] = binArea[(size_t)k];  // component 0 is the FAB's x
    bool normalize = false;
    pp.query("normalize", normalize);
    if (normalize) {
      const double r = 1. / binSum;  // :637
      for (double& v : fab) v *= r;
    }
    const std::string outFabFile = fabFileBase + ".fab";
    std::ofstream ofs(outFabFile.c_str(), std::ios::out | std::ios::trunc | std::ios::binary);
    if (!ofs) pa::Abort("Unable to create " + outFabFile);
    const pa::Box3 box{{0, 0, 0}, {n0 - 1, n1 - 1, 0}};
    pa::write_fab(ofs, box, 1, fab.data());
  } else {
    for (long long k = 0; k < nTot; ++k) {
      if (binHits[(size_t)k] <= 0) continue;
      long long r = k;
      int idx[4] = {0, 0, 0, 0};
      for (int j = nc - 1; j >= 0; --j) { idx[j] = (int)(r % nBins[(size_t)j]); r /= nBins[(size_t)j]; }
      for (int j = 0; j < nc; ++j) {
        const double lo = binLO[(size_t)j][(size_t)idx[j]];
        const double hi = (idx[j] == nBins[(size_t)j] - 1 ? binMax[(size_t)j] : binLO[(size_t)j][(size_t)idx[j] + 1]);
        std::cout << 0.5 * (lo + hi) << " ";
      }
      std::cout << binArea[(size_t)k] << std::endl;
    }
  }
  std::cerr << "Total area of this surface: " << area << " (sum of bins: " << binSum << ")" << std::endl;
  if (condApply)
    std::cerr << "   area outside condition: " << areaOutsideCondition << " (total: " << areaOutsideCondition + binSum << ")" << std::endl;
  if (counters[1] > 0) std::cerr << "skipped " << counters[1] << " elements with a value that is not finite" << std::endl;
  pa::Finish();
}
