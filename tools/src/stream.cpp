// stream3d -- drop-in for PeleAnalysis Src/stream.cpp (lines of the progress variable's gradient -- or of the velocity,
// traceAlongV -- seeded on the nodes of an isosurface, traced with stream_nd.f90's RK4 inside each seed's own FAB) on MI355X.
//   stream3d.ex plotfile=<plt> (isoFile=<mef> | seedLoc="x y z" | seedRakeL="x y z" seedRakeR="x y z" [seedRakeNum=2])
//       (streamFile=<dir> | outFile=<dir>) [progressName=temp] [finestLevel=<n>] [nRKsteps=51] [hRK=0.1] [nGrow=(int)(hRK*nRKh)+2]
//       [is_per="0 0 0"] [bounds="xlo ylo zlo xhi yhi zhi"] [aux_comps="c ..." | aux_sComp=<c> aux_nComp=<n>] [traceAlongV=0] [verbose=0]
// Host side (this file): the keys, the seeds (push_nodes_inside with the file's finest dx, bounds -> trim_surface), the box
// membership of every seed in the FILE's boxes (setInsideNodes: half-open tests with the recomputed dx, coarsened finer boxes
// excluded), the upload, and both writers -- streamFile: Header (OLDFORMAT) + Elements + Level_<l>/Str_H + Str_D_00000 (VisMF),
// outFile: <dir>/str_00000.dat (Tecplot points, stream.cpp:2228-2302).  Device side (pa_streamgrad.hip): the state of
// stream.cpp:796-884 (FillBoundary -> FillCFgrowCells -> FillBoundary -> FixOOB) for all levels, then every line in one launch.
//       [buildAltSurf=1 altVal=<v> [advectColdIso=0] [dt=0] [thickCompName=<c> thickLo=<v> thickHi=<v>]
//        [strainCompName=<c> TCompName=<c> TVal=<v>] [addAngle=0] [altIsoFile=surf_new_flame.mef | surf_alt.mef]]
// buildAltSurf (stream.cpp:973-1107): where every line meets altVal, with the seed surface's connectivity -- X Y Z, the progress
// variable (advectColdIso: the velocities, then the progress variable) and the distance along the line there, the thermal
// thickness, the cold-side strain and the angle to the vertical -- by pa_streamalt.hip from the lines while they are in device
// memory; the host takes the acos of the angle's cosine, adds the input surface's distance_iso_to_alt (the reference ADDS) and
// renames the distance to delta, or, advectColdIso, moves X by v * dt, and writes the MEF.  The mode puts the velocities among the
// line components (needV), so into streamFile / outFile too, also when the trace follows the gradient.
// Deviations, all stated:
//   - buildAltSurf=1 needs isoFile=: with seedLoc / seedRake* it aborts (a one-node "surface" is no surface).  The reference sizes
//     the new node array by the count of lines and indexes it by node id: here every node of the trimmed surface must carry exactly
//     one line, else the tool aborts with both counts.  nRKsteps < 3 aborts (the search and the angle index outside the line).
//     strainCompName with TCompName found but the strain component not among the line components aborts (the reference reads
//     component -1).  thickCompName / TCompName not among the line components: the quantity is skipped as in the reference, and one
//     stderr line names the component.  Missing velocity components abort at once.  The reference's "Path oriented backwards" test
//     compares a value with itself and is not built.  The other keys of the mode without buildAltSurf=1 are read by nobody, here
//     as there.  The MEF writer takes triangles: another nodesPerElt aborts.
//   - ngpus > 1, the USE_PF variant (not compiled in the reference either) and 2-D plotfiles abort.
//   - A progressName that is not in the plotfile aborts at once (the reference prints "Cannot find required data in pltfile"
//     and fails later inside FillVar).  So do a missing or doubled streamFile / outFile (the reference asserts after tracing).
//   - Where the reference would copy an unset coarse value into a coarse-fine ghost cell inside the domain (a fine level not
//     properly nested, a fine box not aligned to the ratio), the tool aborts.
//   - bounds= that removes every element aborts (the reference divides by nElts = 0 in write_ml_streamline_data).
//   - One process: the Str data file is Str_D_00000 and the Tecplot file str_00000.dat, as one MPI rank writes them.
//   - is_per is read and printed; it cannot change any output (FixOOB zeroes every periodic ghost cell before the trace).
#include "../common/pa_device.h"

#include <sys/stat.h>

namespace {

void usage(const char* argv0) {  // stream.cpp:41-59
  std::cerr << "usage:\n";
  std::cerr << argv0 << " infile plotfile=<string> [options] \n\tOptions:\n";
  std::cerr << " isoFile=<string>  OR  seedLoc=<real real [real]  OR  seedRakeL=<real real [real]> seedRakeR=<real real [real] seedRakeNum=<int>>\n";
  std::cerr << " streamFile=<string>  OR  outFile=<string>\n";
  std::cerr << " is_per=<int int int> (DEF=1 1 1)\n";
  std::cerr << " finestLevel=<int> (DEF=finest level in plotfile)\n";
  std::cerr << " progressName=<string> (DEF=temp)\n";
  std::cerr << " traceAlongV=<bool> (DEF=0)\n";
  std::cerr << " buildAltSurf=<bool> (DEF=0)\n";
  std::cerr << "     (if true, requires altVal=<real>, also takes dt=<real> (DEF=0) and altIsoFile=<string>)\n";
  std::cerr << " nRKsteps=<int> (DEF=51)\n";
  std::cerr << " hRK=<real> (DEF=.1 (*dx_finest in plotfile)\n";
  std::cerr << " nGrow=<int> (DEF=4)\n";
  std::cerr << " bounds=<float * 4> (DEF=NULL)\n";
  std::exit(1);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) usage(argv[0]);
  pa::ParmParse pp(argc, argv);
  if (pp.contains("help")) usage(argv[0]);
  int ngpus = 1;
  pp.query("ngpus", ngpus);
  if (ngpus > 1) pa::Abort("ngpus > 1 is not supported by stream3d (one GPU)");
  int verbose = 0;
  pp.query("verbose", verbose);

  std::string plotfile;
  pp.get("plotfile", plotfile);
  const pa::PlotfileHeader H = pa::read_header(plotfile, 3, true);
  int finestLevel = H.nlev - 1;
  pp.query("finestLevel", finestLevel);
  if (finestLevel < 0 || finestLevel >= H.nlev) pa::Abort("finestLevel out of range");
  const int Nlev = finestLevel + 1;
  std::string progressName = "temp";
  pp.query("progressName", progressName);
  const int idC = H.comp(progressName);
  if (idC < 0) pa::Abort("Cannot find required data in pltfile: progressName=" + progressName);

  // seeds (stream.cpp:440-560), component-major [3][N] like the node FAB
  std::vector<double> nodes;
  std::vector<int32_t> faceData;
  long long nElts = 0, nodesPerElt = 0, nSeed = 0;
  std::vector<std::string> surfNames;
  std::vector<double> isoDist;  // the input surface's distance_iso_to_alt (buildAltSurf adds it to the new one, stream.cpp:1046-1056)
  const std::string distanceVarName = "distance_iso_to_alt";
  bool buildAltSurf = false;
  pp.query("buildAltSurf", buildAltSurf);
  const int ni = pp.countval("isoFile"), ns = pp.countval("seedLoc"), nrL = pp.countval("seedRakeL"), nrR = pp.countval("seedRakeR");
  if (!((ni > 0) ^ (ns > 0) ^ ((nrL > 0) && (nrR > 0)))) pa::Abort("Assertion `ni>0 ^ ns>0 ^ (nrL>0 && nrR>0)' failed");
  if (buildAltSurf && ni == 0) pa::Abort("buildAltSurf=1 needs isoFile=: the alternate surface takes the connectivity of a seed surface (seedLoc / seedRake* give none)");
  if (ni > 0) {
    std::string isoFile;
    pp.get("isoFile", isoFile);
    std::cerr << "Reading isoFile... " << isoFile << std::endl;
    pa::MefSurface S = pa::read_mef(isoFile);
    const size_t nc = S.names.size();
    if (nc < 3) pa::Abort("isoFile: fewer than 3 node components");
    nSeed = S.nNodes;
    nElts = S.nElts;
    nodesPerElt = S.nodesPerElt;
    surfNames = S.names;
    nodes.resize(3 * (size_t)nSeed);
    for (long long i = 0; i < nSeed; ++i)
      for (int d = 0; d < 3; ++d) nodes[(size_t)d * nSeed + i] = S.nodes[(size_t)i * nc + d];
    for (size_t c = 0; c < nc; ++c) {  // the last component of that name, as the reference's loop leaves it
      if (S.names[c] != distanceVarName) continue;
      isoDist.resize((size_t)nSeed);
      for (long long i = 0; i < nSeed; ++i) isoDist[(size_t)i] = S.nodes[(size_t)i * nc + c];
    }
    faceData = S.conn;
  } else if (ns > 0) {
    std::vector<double> loc;
    if (!pp.queryarr("seedLoc", loc, 0, 3)) pa::Abort("seedLoc needs 3 values");
    nSeed = 1; nElts = 1; nodesPerElt = 1;
    faceData.assign(1, 1);
    nodes = loc;
    surfNames = {"X", "Y", "Z"};
  } else {
    int num = 2;
    pp.query("seedRakeNum", num);
    std::vector<double> L, R;
    if (!pp.queryarr("seedRakeL", L, 0, 3) || !pp.queryarr("seedRakeR", R, 0, 3)) pa::Abort("seedRakeL / seedRakeR need 3 values");
    nSeed = num; nElts = 1; nodesPerElt = 1;
    faceData.assign(1, 1);
    nodes.resize(3 * (size_t)num);
    for (int i = 0; i < num; ++i)
      for (int d = 0; d < 3; ++d) nodes[(size_t)d * num + i] = L[d] + (i / double(num - 1)) * (R[d] - L[d]);
    surfNames = {"X", "Y", "Z"};
  }
  // push_nodes_inside with 1e-4 x the file's dx of the finest level (stream.cpp:562-566)
  const double epsPush = 1.e-4 * H.file_dx[finestLevel][0];
  for (int d = 0; d < 3; ++d)
    for (long long i = 0; i < nSeed; ++i) {
      double& x = nodes[(size_t)d * nSeed + i];
      x = std::max(H.prob_lo[d] + epsPush, std::min(H.prob_hi[d] - epsPush, x));
    }
  if (const int nx = pp.countval("bounds")) {  // trim_surface (stream.cpp:218-290)
    std::vector<double> bb;
    if (nx != 6 || !pp.queryarr("bounds", bb, 0, 6)) pa::Abort("bounds needs 6 values");
    std::vector<long long> idx((size_t)nSeed);
    long long nn = 0;
    for (long long i = 0; i < nSeed; ++i) {
      bool rm = false;
      for (int d = 0; d < 3; ++d) { const double x = nodes[(size_t)d * nSeed + i]; rm = rm || x < bb[d] || x > bb[3 + d]; }
      idx[(size_t)i] = rm ? -1 : nn++;
    }
    std::vector<double> nw(3 * (size_t)nn);
    for (long long i = 0; i < nSeed; ++i)
      if (idx[(size_t)i] >= 0)
        for (int d = 0; d < 3; ++d) nw[(size_t)d * nn + idx[(size_t)i]] = nodes[(size_t)d * nSeed + i];
    if (!isoDist.empty()) {  // trim_surface keeps every component of the node FAB
      std::vector<double> nd((size_t)nn);
      for (long long i = 0; i < nSeed; ++i)
        if (idx[(size_t)i] >= 0) nd[(size_t)idx[(size_t)i]] = isoDist[(size_t)i];
      isoDist.swap(nd);
    }
    std::vector<int32_t> nf;
    long long ne = 0;
    for (long long e = 0; e < nElts; ++e) {
      bool good = true;
      for (long long j = 0; j < nodesPerElt; ++j) good = good && idx[(size_t)faceData[(size_t)(e * nodesPerElt + j)] - 1] >= 0;
      if (!good) continue;
      for (long long j = 0; j < nodesPerElt; ++j) nf.push_back((int32_t)(idx[(size_t)faceData[(size_t)(e * nodesPerElt + j)] - 1] + 1));
      ++ne;
    }
    nodes.swap(nw);
    faceData.swap(nf);
    nSeed = nn;
    nElts = ne;
  }
  if (nElts <= 0) pa::Abort("no element left to write (nElts = 0)");
  if (buildAltSurf && nodesPerElt != 3) pa::Abort("buildAltSurf: the surface writer takes triangles (nodesPerElt = " + std::to_string(nodesPerElt) + ")");

  // components of the state (stream.cpp:594-690)
  bool traceAlongV = false;
  pp.query("traceAlongV", traceAlongV);
  bool needV = traceAlongV;  // the velocities among the line components; the trace follows them only with traceAlongV
  double altVal = -1, dt = 0., thickLo = 0, thickHi = 0, TVal = 0;
  std::string thickCompName = "null", strainCompName = "null", TCompName = "null";
  bool addAngle = false;
  if (buildAltSurf) {  // stream.cpp:589-610
    pp.get("altVal", altVal);
    pp.query("dt", dt);
    needV = true;
    pp.query("thickCompName", thickCompName);
    if (thickCompName != "null") {
      pp.get("thickLo", thickLo);
      pp.get("thickHi", thickHi);
    }
    pp.query("strainCompName", strainCompName);
    if (strainCompName != "null") {
      pp.get("TCompName", TCompName);
      pp.get("TVal", TVal);
    }
    pp.query("addAngle", addAngle);
  }
  std::vector<std::string> inVarNames = {progressName};
  if (needV) for (const char* v : {"x_velocity", "y_velocity", "z_velocity"}) inVarNames.push_back(v);
  std::vector<int> auxComps;
  if (const int nc = pp.countval("aux_comps")) {
    pp.queryarr("aux_comps", auxComps, 0, nc);
  } else {
    int s = 0, n = 0;
    pp.query("aux_sComp", s);
    pp.query("aux_nComp", n);
    for (int i = 0; i < n; ++i) auxComps.push_back(s + i);
  }
  std::vector<int> fileComp;
  for (auto& n : inVarNames) {
    const int c = H.comp(n);
    if (c < 0) pa::Abort("Variable not found in the plotfile: " + n);
    fileComp.push_back(c);
  }
  for (int c : auxComps) {
    if (c < 0 || c >= (int)H.names.size()) pa::Abort("aux component out of range: " + std::to_string(c));
    inVarNames.push_back(H.names[(size_t)c]);
    fileComp.push_back(c);
  }
  const int nCompSt = (int)inVarNames.size(), nCompStr = 3 + nCompSt;
  std::vector<std::string> strNames(surfNames.begin(), surfNames.begin() + 3);
  for (auto& n : inVarNames) strNames.push_back(n);
  const int isoCompStr = 3, vCompStr = needV ? 4 : -1;
  int thickComp = -1, strainComp = -1, TComp = -1;  // stream.cpp:673-698: the last line component of each name
  for (int i = 0; i < nCompStr; ++i) {
    if (strNames[(size_t)i] == thickCompName) thickComp = i;
    if (strNames[(size_t)i] == strainCompName) strainComp = i;
    if (strNames[(size_t)i] == TCompName) TComp = i;
  }
  if (thickComp >= 0) std::cout << "Thermal thickness component id: " << thickComp << std::endl;
  if (strainComp >= 0) {
    std::cout << "Strain component id: " << strainComp << std::endl;
    std::cout << "   T component for strain eval at id: " << TComp << std::endl;
  }
  if (buildAltSurf) {
    if (thickCompName != "null" && thickComp < 0) std::cerr << "thickCompName=" << thickCompName << " is not among the line components: no thermal thickness" << std::endl;
    if (TCompName != "null" && TComp < 0) std::cerr << "TCompName=" << TCompName << " is not among the line components: no cold strain" << std::endl;
    if (TComp >= 0 && strainComp < 0) pa::Abort("strainCompName=" + strainCompName + " is not among the line components (TCompName=" + TCompName + " is)");
  }

  // trace parameters (stream.cpp:693-716)
  int nRKsteps = 51;
  pp.query("nRKsteps", nRKsteps);
  if (nRKsteps < 1) pa::Abort("nRKsteps must be at least 1");
  if (buildAltSurf && nRKsteps < 3) pa::Abort("buildAltSurf=1 needs nRKsteps >= 3: the search and the angle index the points j = -1 .. 1 of every line");
  const int nRKh = (nRKsteps - 1) / 2;
  double hRK = 0.1;
  pp.query("hRK", hRK);
  int nGrow = (int)(hRK * nRKh) + 2;
  pp.query("nGrow", nGrow);
  if (nGrow < 1) pa::Abort("nGrow must be at least 1");
  std::cout << "nGrow = " << nGrow << std::endl;
  std::vector<int> is_per(3, 0);
  pp.queryarr("is_per", is_per, 0, 3);
  std::cout << "Periodicity assumed for this case: ";
  for (int d = 0; d < 3; ++d) std::cout << is_per[d] << " ";
  std::cout << std::endl;
  const pa::Box3& fdom = H.lev[finestLevel].domain;
  hRK = hRK * (H.prob_hi[0] - H.prob_lo[0]) / (double)(fdom.hi[0] - fdom.lo[0] + 1);

  // box membership (stream.cpp:710-766, setInsideNodes :141-216): 1-based ids per (level, file box), CSR over all boxes
  std::vector<int64_t> box_start(1, 0);
  std::vector<int32_t> ids;
  for (int lev = 0; lev < Nlev; ++lev) {
    const pa::LevelMeta& L = H.lev[lev];
    double delta[3];
    for (int d = 0; d < 3; ++d) delta[d] = (H.prob_hi[d] - H.prob_lo[d]) / (double)(L.domain.hi[d] - L.domain.lo[d] + 1);
    std::vector<pa::Box3> fc;  // coarsened finer boxes
    if (lev < finestLevel) {
      const int r = H.ref_ratio[(size_t)lev];
      auto cdiv = [r](int a) { return a >= 0 ? a / r : -((-a + r - 1) / r); };
      for (const pa::Box3& F : H.lev[lev + 1].boxes) {
        pa::Box3 c;
        for (int d = 0; d < 3; ++d) { c.lo[d] = cdiv(F.lo[d]); c.hi[d] = cdiv(F.hi[d]); }
        fc.push_back(c);
      }
    }
    for (const pa::Box3& B : L.boxes) {
      double lo[3], hi[3];
      for (int d = 0; d < 3; ++d) { lo[d] = H.prob_lo[d] + B.lo[d] * delta[d]; hi[d] = H.prob_lo[d] + (B.hi[d] + 1.) * delta[d]; }
      std::vector<std::array<double, 6>> fr;  // the intersections with this box
      for (const pa::Box3& c : fc) {
        int a[3], e[3];
        bool meet = true;
        for (int d = 0; d < 3; ++d) { a[d] = std::max(c.lo[d], B.lo[d]); e[d] = std::min(c.hi[d], B.hi[d]); meet = meet && a[d] <= e[d]; }
        if (!meet) continue;
        std::array<double, 6> q;
        for (int d = 0; d < 3; ++d) { q[(size_t)d] = H.prob_lo[d] + a[d] * delta[d]; q[(size_t)(3 + d)] = H.prob_lo[d] + (e[d] + 1.) * delta[d]; }
        fr.push_back(q);
      }
      for (long long i = 0; i < nSeed; ++i) {
        bool isIn = true;
        for (int d = 0; d < 3; ++d) { const double x = nodes[(size_t)d * nSeed + i]; isIn = isIn && x >= lo[d] && x < hi[d]; }
        for (size_t n = 0; n < fr.size() && isIn; ++n) {
          bool inThis = true;
          for (int d = 0; d < 3; ++d) { const double x = nodes[(size_t)d * nSeed + i]; inThis = inThis && x >= fr[n][(size_t)d] && x < fr[n][(size_t)(3 + d)]; }
          isIn = !inThis;
        }
        if (isIn) ids.push_back((int32_t)(i + 1));
      }
      box_start.push_back((int64_t)ids.size());
    }
  }
  const long long nlines = (long long)ids.size();

  // state data: the file's valid cells, nGrow ghost layers (prepared on the device)
  std::vector<pa::HostMF> hs((size_t)Nlev);
  for (int lev = 0; lev < Nlev; ++lev) {
    hs[(size_t)lev].define(H.lev[lev].boxes, nCompSt, nGrow);
    for (int c = 0; c < nCompSt; ++c) pa::read_comp(H, lev, fileComp[(size_t)c], hs[(size_t)lev], c);
  }
  std::vector<double> strm((size_t)nlines * nRKsteps * nCompStr);
  std::vector<int32_t> box_flag(box_start.size() - 1, 0);

  // the alternate surface (stream.cpp:973-1035): its components, and the check that the node array the reference sizes by the
  // count of lines and indexes by node id is the trimmed surface's
  bool advectColdIso = false;
  std::vector<std::string> altSurfNames;
  std::vector<double> altOut;  // [nAlt][nSeed]
  pa_streamalt_params altP{};
  double* daltOut = nullptr;
  if (buildAltSurf) {
    pp.query("advectColdIso", advectColdIso);
    std::vector<long long> cnt((size_t)nSeed, 0);
    bool once = nlines == nSeed;
    for (int32_t id : ids) ++cnt[(size_t)id - 1];
    for (long long c : cnt) once = once && c == 1;
    if (!once)
      pa::Abort("buildAltSurf: " + std::to_string(nlines) + " lines for " + std::to_string(nSeed) + " nodes of the surface: every node must carry exactly one line");
    altP.isoComp = isoCompStr;
    altP.altVal = altVal;
    if (advectColdIso) for (int d = 0; d < 3; ++d) altP.carry[altP.ncarry++] = vCompStr + d;
    altP.carry[altP.ncarry++] = isoCompStr;
    altP.thickComp = thickComp;
    altP.thickLo = thickLo;
    altP.thickHi = thickHi;
    altP.TComp = TComp;
    altP.strainComp = strainComp;
    altP.TVal = TVal;
    altP.addAngle = addAngle ? 1 : 0;
    for (int d = 0; d < 3; ++d) altSurfNames.push_back(strNames[(size_t)d]);
    for (int k = 0; k < altP.ncarry; ++k) altSurfNames.push_back(strNames[(size_t)altP.carry[k]]);
    altSurfNames.push_back(distanceVarName);
    if (thickComp >= 0) altSurfNames.push_back(advectColdIso ? "thermalThickness" : "thermalThickness_notAdv");
    if (TComp >= 0) altSurfNames.push_back("coldStrain");
    if (addAngle) altSurfNames.push_back("angleWRTvert");
    altOut.resize(altSurfNames.size() * (size_t)nSeed);
  }
  {
    pa::Ctx ctx;
    std::vector<std::unique_ptr<pa::DevLevel>> dl;
    std::vector<std::unique_ptr<pa::DevMF>> dm;
    std::vector<pa_mf*> st;
    const int per[3] = {is_per[0], is_per[1], is_per[2]};
    for (int lev = 0; lev < Nlev; ++lev) {
      dl.emplace_back(new pa::DevLevel(ctx, H.lev[lev].boxes, H.lev[lev].domain, per, H.prob_lo, H.prob_hi));
      dm.emplace_back(new pa::DevMF(ctx, *dl.back(), nCompSt, nGrow));
      ctx.check(pa_mf_upload(ctx.h, dm.back()->h, hs[(size_t)lev].data.data()));
      st.push_back(dm.back()->h);
    }
    ctx.check(pa_streamgrad_prepare(ctx.h, Nlev, st.data()));
    double* dnodes = nullptr;
    int32_t* dids = nullptr;
    double* dstrm = nullptr;
    if (nlines > 0) {
      dnodes = (double*)pa_device_malloc(ctx.h, (int64_t)nodes.size() * 8);
      dids = (int32_t*)pa_device_malloc(ctx.h, (int64_t)ids.size() * 4);
      dstrm = (double*)pa_device_malloc(ctx.h, (int64_t)strm.size() * 8);
      if (!dnodes || !dids || !dstrm) pa::Abort(pa_last_error(ctx.h));
      ctx.check(pa_memcpy_h2d(ctx.h, dnodes, nodes.data(), (int64_t)nodes.size() * 8));
      ctx.check(pa_memcpy_h2d(ctx.h, dids, ids.data(), (int64_t)ids.size() * 4));
    }
    if (buildAltSurf) {
      daltOut = (double*)pa_device_malloc(ctx.h, (int64_t)altOut.size() * 8);
      if (!daltOut) pa::Abort(pa_last_error(ctx.h));
    }
    ctx.check(pa_streamgrad_trace(ctx.h, Nlev, st.data(), traceAlongV ? 1 : -1, nSeed, dnodes, box_start.data(), dids, nRKsteps, hRK, dstrm, box_flag.data()));
    if (buildAltSurf) {  // every quantity of the new surface from the lines in device memory, node-ordered
      ctx.check(pa_streamalt_run(ctx.h, (int32_t)(box_start.size() - 1), box_start.data(), dids, dstrm, nCompStr, nRKsteps, nSeed, &altP, daltOut, nullptr));
      ctx.check(pa_memcpy_d2h(ctx.h, altOut.data(), daltOut, (int64_t)altOut.size() * 8));
      pa_device_free(ctx.h, daltOut);
    }
    if (nlines > 0) {
      ctx.check(pa_memcpy_d2h(ctx.h, strm.data(), dstrm, (int64_t)strm.size() * 8));
      pa_device_free(ctx.h, dnodes);
      pa_device_free(ctx.h, dids);
      pa_device_free(ctx.h, dstrm);
    }
    dm.clear();
    dl.clear();
  }
  bool cutLo = false, cutHi = false;
  for (int32_t f : box_flag) {
    if (f == 1) pa::Abort("Problem with interpolation");
    cutLo = cutLo || f == 2;
    cutHi = cutHi || f == 4;
  }
  for (int lev = 0; lev < Nlev; ++lev) std::cout << "Streamlines computed on level " << lev << std::endl;
  if (cutLo) std::cerr << "Lines cut short on low end" << std::endl;
  if (cutHi) std::cerr << "Lines cut short on high end" << std::endl;

  // the Str FABs, level by level (stream.cpp:752-761): box (0,-nRKh,0)..(n-1,nRKsteps-1-nRKh,0), or the null box of zeros
  std::vector<std::vector<pa::StrFab>> fabs((size_t)Nlev);
  std::vector<std::vector<std::vector<int32_t>>> inside((size_t)Nlev);
  std::vector<double> zbuf((size_t)nCompStr, 0.0);
  {
    size_t g = 0;
    for (int lev = 0; lev < Nlev; ++lev)
      for (size_t b = 0; b < H.lev[lev].boxes.size(); ++b, ++g) {
        const long long n = box_start[g + 1] - box_start[g];
        inside[(size_t)lev].emplace_back(ids.begin() + box_start[g], ids.begin() + box_start[g + 1]);
        if (n == 0) fabs[(size_t)lev].push_back({pa::Box3{{0, 0, 0}, {0, 0, 0}}, zbuf.data(), 1});
        else fabs[(size_t)lev].push_back({pa::Box3{{0, -nRKh, 0}, {(int)n - 1, nRKsteps - 1 - nRKh, 0}}, strm.data() + (size_t)box_start[g] * nRKsteps * nCompStr, n * nRKsteps});
      }
  }

  const int nst = pp.countval("streamFile"), no = pp.countval("outFile");
  if (!((nst > 0) ^ (no > 0))) pa::Abort("Assertion `nst>0 ^ no>0' failed: give exactly one of streamFile / outFile");
  if (nst > 0) {  // write_ml_streamline_data (stream.cpp:2091-2226), OLDFORMAT
    std::string dir;
    pp.get("streamFile", dir);
    std::cerr << "Writing the streamline data " << std::endl;
    pa::write_stream_dir(dir, strNames, nElts, faceData, inside, fabs);
    std::cerr << "...done writing the streamline data " << std::endl;
  } else {  // dump_ml_streamline_data (stream.cpp:2228-2302), one process
    std::string dir;
    pp.get("outFile", dir);
    ::mkdir(dir.c_str(), 0755);
    bool will_write = false;
    for (auto& L : fabs)
      for (const pa::StrFab& F : L) will_write = will_write || F.box.lo[1] != 0 || F.box.hi[0] != 0 || F.box.hi[1] != 0;
    if (will_write) {
      std::ofstream o(dir + "/str_00000.dat");
      if (!o) pa::Abort("Unable to create " + dir + "/str_00000.dat");
      o << "VARIABLES = ";
      for (auto& n : strNames) o << n << " ";
      o << '\n';
      for (auto& L : fabs)
        for (const pa::StrFab& F : L) {
          if (F.box.lo[1] == 0 && F.box.hi[0] == 0 && F.box.hi[1] == 0) continue;  // equals the null box
          const int n = F.box.hi[0] + 1, J = F.box.hi[1] - F.box.lo[1] + 1;
          for (int i = 0; i < n; ++i) {
            o << "ZONE I=1 J=" << J << " k=1 FORMAT=POINT\n";
            for (int L2 = 0; L2 < J; ++L2) {
              for (int c = 0; c < nCompStr; ++c) o << F.data[((size_t)c * J + L2) * n + i] << " ";  // operator<<, default precision
              o << '\n';
            }
          }
        }
    }
  }

  if (buildAltSurf) {  // stream.cpp:973-1107; the messages of build_surface_at_isoVal and the add_* functions in their order
    if (verbose > 0) std::cout << "building new surface where " << strNames[(size_t)isoCompStr] << " = " << altVal << std::endl;
    for (int lev = 0; lev < Nlev; ++lev) std::cerr << "building new surface at level: " << lev << std::endl;
    std::cerr << "New surface built, communicating info to ioproc " << std::endl;
    std::cerr << "Data sent, building new iso" << std::endl;
    std::cerr << "New iso built on ioproc " << std::endl;
    if (thickComp >= 0) std::cerr << "Thermal thickness computed, communicating info to ioproc " << std::endl << "New surface data added on ioproc " << std::endl;
    if (TComp >= 0) std::cerr << "Cold Strain computed, communicating info to ioproc " << std::endl << "New surface data added on ioproc " << std::endl;
    if (addAngle) std::cerr << "Angle computed, communicating info to ioproc " << std::endl << "New surface data added on ioproc " << std::endl;
    const size_t nAlt = altSurfNames.size(), N = (size_t)nSeed;
    if (addAngle) {  // the kernel leaves the cosine (add_angle_to_surf :1265)
      double* a = altOut.data() + (nAlt - 1) * N;
      for (size_t i = 0; i < N; ++i) a[i] = std::acos(a[i]);
    }
    if (!advectColdIso) {  // :1041-1060: the input surface's distance is ADDED to the new one, which is renamed in any case
      const size_t dCompAlt = 3 + (size_t)altP.ncarry;
      if (!isoDist.empty())
        for (size_t i = 0; i < N; ++i) altOut[dCompAlt * N + i] += isoDist[i];
      altSurfNames[dCompAlt] = "delta";
    } else {  // :1061-1084: X += v * dt, the velocities are the first carried components
      for (size_t i = 0; i < N; ++i)
        for (size_t d = 0; d < 3; ++d) altOut[d * N + i] += altOut[(3 + d) * N + i] * dt;
    }
    std::string altIsoFile = advectColdIso ? "surf_alt.mef" : "surf_new_flame.mef";
    const std::string label = advectColdIso ? "advected alt surface" : "new flame surface from advected alt";
    pp.query("altIsoFile", altIsoFile);
    std::vector<double> tn(nAlt * N);  // write_iso (:1166-1209): component fastest
    for (size_t i = 0; i < N; ++i)
      for (size_t c = 0; c < nAlt; ++c) tn[i * nAlt + c] = altOut[c * N + i];
    std::vector<int32_t> elts0(faceData.size());
    for (size_t q = 0; q < faceData.size(); ++q) elts0[q] = faceData[q] - 1;
    pa::write_mef(altIsoFile, label, altSurfNames, tn, elts0);
    std::cerr << "Finished writing streamline data " << std::endl;
  }
  return 0;
}
