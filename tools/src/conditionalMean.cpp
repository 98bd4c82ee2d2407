// conditionalMean3d -- drop-in for PeleAnalysis Src/conditionalMean.cpp (means, sums of squares and optionally minima / maxima of plotfile
// components conditioned on the bins of one component, over one or several plotfiles) on MI355X.
//   conditionalMean3d.ex infile="<plt> ..." binComp=<n> avgComps="<n> ..." binMin=<v> binMax=<v> [nBins=64] [finestLevel=<n>]
//       [bounds="xlo ylo zlo xhi yhi zhi"] [writeBinMinMax=0] [aja=0] [outSuffix=<s>] [verbose=0]   (floor / ceiling are read and unused, :115-116)
// Host side (this file): the keys (:58-147), the domain cut to `bounds` and refined level by level, the levels that hold cells of it
// (:178-233), the integer weights from the FIRST plotfile (:198-205), the writer (:311-400).  Device side (pa_stats.hip): one min / max
// launch per level for the magnitudes of the averaged components, then one accumulate launch per level; a level's components are
// uploaded, used and released, so a file larger than device memory streams through (everything stays resident when it fits).
// NUMERICS: binHits, bin indices, minima and maxima are exact; the sums are fixed-point sums rounded once per plotfile
// -- not the reference's cell-after-cell additions -- and are added over the plotfiles in infile order.
// Deviations, all stated in INTEGRATION.md:
//   - binHits and the total are 64-bit (the reference's int overflows at 2^31 weighted hits).
//   - The reference declares the domain inside its file loop and sets it for the first file only, so later files meet an empty box
//     and add nothing; here every file is binned over the first file's domain.
//   - A bounds box that empties a middle level: the level below it has no finer level (the reference indexes bas[iLevel+1] out of range, :249).
//   - "Bad comp" names the number (:174 is pointer arithmetic); more than 6 values in bounds, ngpus > 1 and 2-D plotfiles abort.
//   - More than 8 averaged components are binned in groups of 8 (one more pass over the bin component per group).
#include "../common/pa_device.h"

#include <cmath>

namespace {

struct LevPlan {
  int level;
  pa::Box3 dom;
  int finer;  // plan entry of the next finer level, or -1
  int ratio;
  int64_t weight;
};

bool meets(const pa::Box3& a, const pa::Box3& b) {
  for (int d = 0; d < 3; ++d)
    if (a.lo[d] > b.hi[d] || a.hi[d] < b.lo[d]) return false;
  return true;
}

}  // namespace

int main(int argc, char** argv) {
  pa::ParmParse pp(argc, argv);
  int ngpus = 1;
  pp.query("ngpus", ngpus);
  if (ngpus > 1) pa::Abort("ngpus > 1 is not supported by conditionalMean3d (one GPU)");
  int verbose = 0;
  pp.query("verbose", verbose);

  const int nPlotFiles = pp.countval("infile");
  if (nPlotFiles <= 0) {
    std::cerr << "Bad nPlotFiles:  " << nPlotFiles << std::endl;
    std::cerr << "Exiting." << std::endl;
    return 1;
  }
  if (verbose) std::cout << "Processing " << nPlotFiles << " plotfiles..." << std::endl;
  std::string outSuffix = "";
  pp.query("outSuffix", outSuffix);
  std::vector<std::string> plotFileNames((size_t)nPlotFiles);
  for (int i = 0; i < nPlotFiles; ++i) {
    pp.get("infile", plotFileNames[(size_t)i], i);
    if (verbose) std::cout << "   " << plotFileNames[(size_t)i] << std::endl;
  }
  int finestLevel = -1;
  pp.query("finestLevel", finestLevel);
  int nBins = 64;
  pp.query("nBins", nBins);
  if (nBins < 1) pa::Abort("nBins must be at least 1");
  int binComp = -1;
  pp.get("binComp", binComp);
  const int nAvgComps = pp.countval("avgComps");
  std::vector<int> avgComps;
  if (nAvgComps > 0) pp.queryarr("avgComps", avgComps, 0, nAvgComps);
  else pa::Abort("need to specify avgComps");
  bool writeBinMinMax = false;
  pp.query("writeBinMinMax", writeBinMinMax);
  double binMin = 0, binMax = 1;
  pp.get("binMin", binMin);
  pp.get("binMax", binMax);
  if (binMax <= binMin) pa::Abort("Bad bin min,max");
  bool floor_ = false, ceiling_ = false;
  pp.query("floor", floor_);
  pp.query("ceiling", ceiling_);
  std::vector<double> bbll, bbur;
  if (const int nx = pp.countval("bounds")) {
    if (nx != 6) pa::Abort("bounds needs 6 values (lo then hi), got " + std::to_string(nx));
    std::vector<double> barr;
    pp.queryarr("bounds", barr, 0, nx);
    bbll.assign(barr.begin(), barr.begin() + 3);
    bbur.assign(barr.begin() + 3, barr.end());
  }
  bool aja = false;
  pp.query("aja", aja);
  if (aja) std::cout << "Output for aja" << std::endl;

  const size_t nA = (size_t)nAvgComps, nB = (size_t)nBins;
  std::vector<int64_t> binHits(nB, 0);
  std::vector<double> binVals(nB * nA, 0.0), binValsSq(nB * nA, 0.0), binMinVals, binMaxVals;
  if (writeBinMinMax) { binMinVals.assign(nB * nA, 0.0); binMaxVals.assign(nB * nA, 0.0); }

  std::vector<std::string> compNames;
  std::vector<int64_t> weights;
  pa::Box3 domain0{{0, 0, 0}, {-1, -1, -1}};
  pa::AsyncCtx actx;

  for (int iPlot = 0; iPlot < nPlotFiles; ++iPlot) {
    const std::string& infile = plotFileNames[(size_t)iPlot];
    if (verbose) std::cout << "\nOpening " << infile << "..." << std::endl;
    const pa::PlotfileHeader H = pa::read_header(infile, 3, true);
    const int ncp = (int)H.names.size();
    if (iPlot == 0) {  // :166-206
      if (binComp < 0 || binComp >= ncp) pa::Abort("Bad comp: " + std::to_string(binComp));
      compNames.push_back(H.names[(size_t)binComp]);
      for (int c : avgComps) {
        if (c < 0 || c >= ncp) pa::Abort("Bad comp: " + std::to_string(c));
        compNames.push_back(H.names[(size_t)c]);
      }
      domain0 = H.lev[0].domain;
      if (!bbll.empty()) {  // coarse-grid coordinates of the bounding box, rounded outwards (:183-191)
        for (int i = 0; i < 3; ++i) {
          const double dx = (H.prob_hi[i] - H.prob_lo[i]) / (double)(H.lev[0].domain.hi[i] - H.lev[0].domain.lo[i] + 1);
          domain0.lo[i] = std::max(domain0.lo[i], (int)((bbll[(size_t)i] - H.prob_lo[i] + .0001 * dx) / dx));
          domain0.hi[i] = std::min(domain0.hi[i], (int)((bbur[(size_t)i] - H.prob_lo[i] - .0001 * dx) / dx));
        }
      }
      if (finestLevel < 0) finestLevel = H.nlev - 1;
      if (finestLevel >= H.nlev) pa::Abort("finestLevel out of range");
      weights.assign((size_t)finestLevel + 1, 1);
      for (int i = finestLevel - 1; i >= 0; --i) {
        const int64_t rat = H.ref_ratio[(size_t)i];
        weights[(size_t)i] = weights[(size_t)i + 1] * rat * rat * rat;
      }
    }
    // the components of THIS file by name (AmrData::FillVar takes names, :242)
    std::vector<int> fileComp;
    for (const std::string& n : compNames) {
      const int c = H.comp(n);
      if (c < 0) pa::Abort("component " + n + " is not in " + infile);
      fileComp.push_back(c);
    }
    // the levels that hold cells of the domain (:209-233)
    const int thisFinest = std::min(finestLevel, H.nlev - 1);
    std::vector<LevPlan> plan;
    {
      pa::Box3 dom = domain0;
      for (int l = 0; l <= thisFinest; ++l) {
        bool any = false;
        for (const pa::Box3& B : H.lev[l].boxes) any = any || meets(B, dom);
        if (!any) break;
        plan.push_back({l, dom, -1, 1, weights[(size_t)l]});
        if (l < thisFinest) {
          const int r = H.ref_ratio[(size_t)l];
          for (int d = 0; d < 3; ++d) { dom.lo[d] *= r; dom.hi[d] = (dom.hi[d] + 1) * r - 1; }
        }
      }
      for (size_t q = 0; q + 1 < plan.size(); ++q) { plan[q].finer = (int)q + 1; plan[q].ratio = H.ref_ratio[(size_t)plan[q].level]; }
    }
    if (plan.empty()) continue;

    pa::Ctx& ctx = actx.get();
    const int per[3] = {0, 0, 0};
    std::vector<std::unique_ptr<pa::DevLevel>> dl;
    for (const LevPlan& P : plan) dl.emplace_back(new pa::DevLevel(ctx, H.lev[P.level].boxes, H.lev[P.level].domain, per, H.prob_lo, H.prob_hi));

    for (int a0 = 0; a0 < nAvgComps; a0 += 8) {  // groups of at most 8 averaged components per accumulator
      const int na = std::min(8, nAvgComps - a0);
      // do all levels of this group fit on the device at once?  Otherwise every level is read and uploaded twice (min / max, then bins)
      int64_t freeB = 0, totalB = 0, needB = 0;
      ctx.check(pa_device_mem_info(ctx.h, &freeB, &totalB));
      for (const LevPlan& P : plan) {
        const std::vector<pa::Box3>& bx = H.lev[P.level].boxes;
        std::vector<int32_t> b6(6 * bx.size());
        for (size_t i = 0; i < bx.size(); ++i)
          for (int d = 0; d < 3; ++d) { b6[6 * i + d] = bx[i].lo[d]; b6[6 * i + 3 + d] = bx[i].hi[d]; }
        std::vector<int64_t> off(bx.size()), cs(bx.size());
        needB += 8 * pa_mf_layout((int)bx.size(), b6.data(), 1 + na, 0, off.data(), cs.data());
      }
      const bool resident = needB < freeB / 10 * 8;
      std::vector<std::unique_ptr<pa::DevMF>> kept(plan.size());
      auto load = [&](size_t q) -> std::unique_ptr<pa::DevMF> {
        const LevPlan& P = plan[q];
        const pa::LevelMeta& L = H.lev[P.level];
        std::vector<char> only(L.boxes.size());
        for (size_t b = 0; b < L.boxes.size(); ++b) only[b] = meets(L.boxes[b], P.dom) ? 1 : 0;  // FABs outside the domain stay 0
        pa::HostMF h;
        h.define(L.boxes, 1 + na, 0);
        pa::read_comp(H, P.level, fileComp[0], h, 0, &only);
        for (int a = 0; a < na; ++a) pa::read_comp(H, P.level, fileComp[(size_t)(1 + a0 + a)], h, 1 + a, &only);
        std::unique_ptr<pa::DevMF> m(new pa::DevMF(ctx, *dl[q], 1 + na, 0));
        ctx.check(pa_mf_upload(ctx.h, m->h, h.data.data()));
        return m;
      };
      // magnitudes of the averaged components: the scale of the fixed-point sums
      std::vector<double> vabs((size_t)na, 0.0);
      std::vector<int32_t> cl((size_t)na);
      for (int a = 0; a < na; ++a) cl[(size_t)a] = 1 + a;
      for (size_t q = 0; q < plan.size(); ++q) {
        std::unique_ptr<pa::DevMF> m = load(q);
        std::vector<double> mn((size_t)na), mx((size_t)na);
        ctx.check(pa_minmax_comps_level(ctx.h, m->h, na, cl.data(), mn.data(), mx.data()));
        for (int a = 0; a < na; ++a) {
          if (!std::isfinite(mn[(size_t)a]) || !std::isfinite(mx[(size_t)a]))
            pa::Abort("component " + compNames[(size_t)(1 + a0 + a)] + " of " + infile + " holds values that are not finite");
          vabs[(size_t)a] = std::max(vabs[(size_t)a], std::max(std::fabs(mn[(size_t)a]), std::fabs(mx[(size_t)a])));
        }
        if (resident) kept[q] = std::move(m);
      }
      pa_hist* acc = pa_condmean_create(ctx.h, na, nBins, writeBinMinMax ? 1 : 0);
      if (!acc) pa::Abort(pa_last_error(ctx.h));
      ctx.check(pa_condmean_begin(ctx.h, acc, plan[0].weight, vabs.data()));
      for (size_t q = 0; q < plan.size(); ++q) {
        std::unique_ptr<pa::DevMF> m = resident ? std::move(kept[q]) : load(q);
        const LevPlan& P = plan[q];
        pa_box dom;
        for (int d = 0; d < 3; ++d) { dom.lo[d] = P.dom.lo[d]; dom.hi[d] = P.dom.hi[d]; }
        ctx.check(pa_condmean_add_level(ctx.h, acc, m->h, P.finer >= 0 ? dl[(size_t)P.finer]->h : nullptr, P.ratio, &dom, P.weight, binMin, binMax, 0));
        ctx.check(pa_sync(ctx.h));  // the level's data are released when m goes out of scope
      }
      std::vector<int64_t> hits(nB);
      std::vector<double> s(nB * (size_t)na), s2(nB * (size_t)na), mn, mx;
      if (writeBinMinMax) { mn.resize(nB * (size_t)na); mx.resize(nB * (size_t)na); }
      ctx.check(pa_condmean_read(ctx.h, acc, hits.data(), s.data(), s2.data(), writeBinMinMax ? mn.data() : nullptr, writeBinMinMax ? mx.data() : nullptr));
      pa_hist_destroy(acc);
      for (size_t b = 0; b < nB; ++b) {
        for (int a = 0; a < na; ++a) {
          const size_t o = b * nA + (size_t)(a0 + a), i = b * (size_t)na + (size_t)a;
          binVals[o] += s[i];  // in infile order: a fixed order
          binValsSq[o] += s2[i];
          if (writeBinMinMax && hits[b] > 0) {  // :284-289: the first hit of a bin sets both (binHits: the hits of EARLIER files here)
            if (binHits[b] == 0) { binMinVals[o] = mn[i]; binMaxVals[o] = mx[i]; }
            else { binMinVals[o] = std::min(mn[i], binMinVals[o]); binMaxVals[o] = std::max(mx[i], binMaxVals[o]); }
          }
        }
      }
      if (a0 + 8 >= nAvgComps)
        for (size_t b = 0; b < nB; ++b) binHits[b] += hits[b];  // once per file, after its last group
    }
  }

  // :311-400
  std::string filename;
  if (aja) filename = plotFileNames[0] + "/CM_" + compNames[0] + ".key";
  else filename = "CM_" + compNames[0] + ".dat";
  std::cout << "Opening file " << filename << std::endl;
  std::ofstream ofs(filename.c_str());
  std::string variables = "VARIABLES = " + compNames[0];
  for (size_t i = 1; i < compNames.size(); ++i) variables += " " + compNames[i] + "_sum";
  for (size_t i = 1; i < compNames.size(); ++i) variables += " " + compNames[i] + "_sumSq";
  for (size_t i = 1; i < compNames.size(); ++i) variables += " " + compNames[i] + "_avg";
  for (size_t i = 1; i < compNames.size(); ++i) variables += " " + compNames[i] + "_std";
  if (writeBinMinMax) {
    for (size_t i = 1; i < compNames.size(); ++i) variables += " " + compNames[i] + "_min";
    for (size_t i = 1; i < compNames.size(); ++i) variables += " " + compNames[i] + "_max";
  }
  variables += " N ";
  variables += " p ";
  variables += '\n';
  ofs << variables.c_str();
  ofs << "ZONE I=" << nBins << " DATAPACKING=POINT\n";
  if (aja) {
    ofs.close();
    filename = plotFileNames[0] + "/CM_" + compNames[0] + ".dat";
    std::cout << "Opening file " << filename << std::endl;
    ofs.open(filename.c_str());
  }
  if (!ofs) pa::Abort("Unable to create " + filename);
  const double dv = (binMax - binMin) / nBins;
  int64_t ntot = 0;
  for (size_t i = 0; i < nB; ++i) ntot += binHits[i];
  for (size_t i = 0; i < nB; ++i) {
    const double v = binMin + dv * (0.5 + (double)i);
    ofs << v << " ";
    for (size_t j = 0; j < nA; ++j) ofs << binVals[i * nA + j] << " ";
    for (size_t j = 0; j < nA; ++j) ofs << binValsSq[i * nA + j] << " ";
    if (binHits[i] > 0) {
      for (size_t j = 0; j < nA; ++j) ofs << binVals[i * nA + j] / (double)binHits[i] << " ";
      for (size_t j = 0; j < nA; ++j) {
        const size_t idx = i * nA + j;
        const double bh = (double)binHits[i];
        ofs << std::sqrt((binValsSq[idx] / bh) - (binVals[idx] / bh) * (binVals[idx] / bh)) << " ";
      }
    } else {
      for (size_t j = 0; j < nA * 2; ++j) ofs << "0.0 ";
    }
    if (writeBinMinMax) {
      for (size_t j = 0; j < nA; ++j) ofs << binMinVals[i * nA + j] << " ";
      for (size_t j = 0; j < nA; ++j) ofs << binMaxVals[i * nA + j] << " ";
    }
    ofs << (double)binHits[i] << " ";
    ofs << (double)binHits[i] / (double)ntot << '\n';
  }
  std::cout << "total bins: " << ntot << std::endl;
  ofs.close();
  (void)floor_; (void)ceiling_; (void)outSuffix;
  pa::Finish();
}
