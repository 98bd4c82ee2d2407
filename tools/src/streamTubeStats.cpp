// streamTubeStats3d -- drop-in for PeleAnalysis Src/streamTubeStats.cpp (stream-tube integrals over the wedges between the three lines
// of every surface triangle, node averages, per-line peak values and peak gradients, as element-centred data in <root>_volInt.mef) on
// MI355X.
//   streamTubeStats3d.ex infile=<streamSampleFile dir> [intComps="c ..."] [avgComps="c ..."] [peakComp="c ..."] [gradComps="c ..."]
//       [FCRComp=<c> compsAtPeakFCR="c ..." namesAtPeakFCR="n ..."] [aux_mef=<file> aux_mef_comps="c ..."] [jlo=<j>] [nSmooth=<n>]
//       [write_tec=0] [write_mef=1] [verbose=0] [grad_use_eps=0] [nCompsPerPass=<n>]
// Host side (this file): the keys and the component bookkeeping of main (:309-541) with its quirks kept, the stream directory
// (read_stream_dir), build_nodeMap (:1256-1281), the passes over the integrated components, the totals and the writers
// (write_binary_mef_file :1610-1704, write_ascii_tec_file :1542-1607).  Device side (pa_tubestats.hip): the wedges of every triangle,
// the lines of every node, the node-to-element means, the element neighbours and the smoothing passes.
// Deviations and kept quirks, all stated in INTEGRATION.md: indices the reference only asserts in debug builds abort here (node ids,
// components, a box that does not hold the swept j range, a missing X / Y / Z); ngpus > 1 and 2-D (nodesPerElt == 2) abort; write_tec
// writes the ASCII .dat (the TECIO binary writer is a compile-time option of the reference and is not built); smoothedInt is 0 when
// there is no output component 4 (the reference reads past the end); max_grad walks the line's own segments in both passes;
// grad_use_eps and nCompsPerPass are keys of our own (nCompsPerPass bounds memory only).
#include "../common/pa_device.h"

using pa::DBuf;

namespace {

// :314-317 (Tokenize skips empty tokens) where the directory part has no '.'; otherwise only a final .ext of the last path component goes
std::string out_root(const std::string& infile) {
  const size_t sl = infile.rfind('/');
  const std::string dir = sl == std::string::npos ? "" : infile.substr(0, sl), base = sl == std::string::npos ? infile : infile.substr(sl + 1);
  if (dir.find('.') == std::string::npos) {
    std::vector<std::string> t;
    std::string cur;
    for (char ch : infile) {
      if (ch == '.') { if (!cur.empty()) t.push_back(cur); cur.clear(); }
      else cur.push_back(ch);
    }
    if (!cur.empty()) t.push_back(cur);
    if (t.empty()) pa::Abort("infile has no name");
    std::string r = t[0];
    for (size_t i = 1; i + 1 < t.size(); ++i) r += "." + t[i];
    return r;
  }
  const size_t p = base.rfind('.');
  return (p == std::string::npos || p == 0) ? infile : infile.substr(0, infile.size() - (base.size() - p));
}

std::vector<int> int_list(const pa::ParmParse& pp, const char* key) {
  std::vector<int> v;
  if (const int nc = pp.countval(key)) pp.queryarr(key, v, 0, nc);
  return v;
}

}  // namespace

int main(int argc, char** argv) {
  pa::ParmParse pp(argc, argv);
  int ngpus = 1;
  pp.query("ngpus", ngpus);
  if (ngpus > 1) pa::Abort("ngpus > 1 is not supported by streamTubeStats3d (one GPU; the reference: \"Code is not yet parallel safe\")");

  std::string infile;
  pp.get("infile", infile);
  const std::string outfile = out_root(infile);
  int verbose = 0;
  pp.query("verbose", verbose);

  int FCRComp = -1;
  pp.query("FCRComp", FCRComp);
  std::vector<int> compsAtPeakFCR;
  std::vector<std::string> namesAtPeakFCR;
  if (FCRComp >= 0) {
    if (const int nc = pp.countval("compsAtPeakFCR")) {
      pp.queryarr("compsAtPeakFCR", compsAtPeakFCR, 0, nc);
      if (!pp.queryarr("namesAtPeakFCR", namesAtPeakFCR, 0, nc)) pa::Abort("ParmParse::getarr(): namesAtPeakFCR not found in table");
    }
  }
  if (verbose) std::cerr << "Reading stream file...\n";
  const std::vector<int> intComps = int_list(pp, "intComps"), avgComps = int_list(pp, "avgComps"), peakComps = int_list(pp, "peakComp") /* no s, as the reference */,
                         gradComps = int_list(pp, "gradComps");

  // the auxiliary MEF (:377-402): read for its names and the range check; its averages are multiplied by the integer 1 / nodesPerElt
  std::string aux_mef = "null";
  pp.query("aux_mef", aux_mef);
  pa::MefSurface aux;
  std::vector<int> aux_mef_comps;
  std::vector<std::string> auxNames;
  if (aux_mef != "null") {
    const int nc = pp.countval("aux_mef_comps");
    if (nc == 0 || !pp.queryarr("aux_mef_comps", aux_mef_comps, 0, nc)) pa::Abort("ParmParse::getarr(): aux_mef_comps not found in table");
    aux = pa::read_mef(aux_mef);
    for (int c : aux_mef_comps) {
      if (c < 0 || c >= (int)aux.names.size()) pa::Abort("aux_mef_comps: component " + std::to_string(c) + " out of range (the file has " + std::to_string(aux.names.size()) + ")");
      auxNames.push_back(aux.names[(size_t)c]);
      if (verbose) std::cerr << "Getting " << auxNames.back() << " from auxiliary mef file...\n";
    }
  }

  // components in memory (:406-430): int, avg, PEAK, GRAD, then FCR and the ones sampled at its peak
  std::vector<int> strComps;
  for (auto* v : {&intComps, &avgComps, &peakComps, &gradComps}) strComps.insert(strComps.end(), v->begin(), v->end());
  int idPFCR = -1;
  if (FCRComp >= 0) {
    idPFCR = (int)strComps.size();
    strComps.push_back(FCRComp);
    strComps.insert(strComps.end(), compsAtPeakFCR.begin(), compsAtPeakFCR.end());
  }
  const int cnt = (int)strComps.size();

  const pa::StreamDir P = pa::read_stream_dir(infile);
  const int Nlev = (int)P.boxes.size(), nCompPath = (int)P.names.size();
  std::cout << "NlevPath:  " << Nlev << '\n' << "nCompPath: " << nCompPath << '\n';  // read_ml_streamline_names (:1344-1345)
  int readXYZ[3] = {-1, -1, -1};
  for (int i = 0; i < nCompPath; ++i)
    for (int d = 0; d < 3; ++d)
      if (P.names[(size_t)i] == std::string(1, "XYZ"[d])) readXYZ[d] = i;
  for (int d = 0; d < 3; ++d)
    if (readXYZ[d] < 0) pa::Abort(std::string("the stream file has no component named ") + "XYZ"[d]);
  for (int c : strComps)
    if (c < 0 || c >= nCompPath) pa::Abort("component " + std::to_string(c) + " out of range (the stream file has " + std::to_string(nCompPath) + ")");
  std::vector<std::string> names = {"X", "Y", "Z"};
  std::vector<int> mem = {readXYZ[0], readXYZ[1], readXYZ[2]};  // file component of every component in memory
  for (int c : strComps) { names.push_back(P.names[(size_t)c]); mem.push_back(c); }
  if (verbose) {
    std::cerr << "...will read the following components: ";
    for (auto& n : names) std::cerr << n << ' ';
    std::cerr << '\n';
  }
  int idX[3] = {-1, -1, -1};  // :461-469: the LAST component in memory with the name
  for (size_t i = 0; i < names.size(); ++i)
    for (int d = 0; d < 3; ++d)
      if (names[i] == std::string(1, "XYZ"[d])) idX[d] = (int)i;

  // output components (:472-526)
  const int nPFCR = idPFCR >= 0 ? (int)compsAtPeakFCR.size() : 0;
  const int nInt = (int)intComps.size(), nAvg = (int)avgComps.size(), nAux = (int)auxNames.size(), nPeak = (int)peakComps.size(), nGrad = (int)gradComps.size();
  const int nCompOut = 4 + nInt + nAvg + nAux + nGrad + 2 * nPeak + nPFCR;
  const int oVol = 0, oArea = 1, oWA = 2, oSmInt = 3, oFirstInt = 4, oFirstAvg = oFirstInt + nInt, oFirstAux = oFirstAvg + nAvg, oFirstGr = oFirstAux + nAux,
            oFirstPk = oFirstGr + nGrad, oFirstPkAtFCR = oFirstPk + 2 * nPeak;
  std::vector<std::string> outNames((size_t)nCompOut);
  outNames[0] = "volume"; outNames[1] = "area"; outNames[2] = "area_wtAvg"; outNames[3] = "smoothedInt";
  int namescnt = 3;
  const int sCompInt = namescnt;
  for (int i = 0; i < nInt; ++i) outNames[(size_t)(oFirstInt + i)] = names[(size_t)namescnt++] + "_int";
  const int sCompAvg = namescnt;
  for (int i = 0; i < nAvg; ++i) outNames[(size_t)(oFirstAvg + i)] = names[(size_t)namescnt++] + "_avg";
  for (int i = 0; i < nAux; ++i) outNames[(size_t)(oFirstAux + i)] = auxNames[(size_t)i] + "_avg";
  const int sCompGr = namescnt;  // counted int, avg, GRAD, PEAK: crossed with the order in memory, kept
  for (int i = 0; i < nGrad; ++i) outNames[(size_t)(oFirstGr + i)] = names[(size_t)namescnt++] + "_gradMax";
  const int sCompPk = namescnt;
  for (int i = 0; i < nPeak; ++i) {
    outNames[(size_t)(oFirstPk + i)] = names[(size_t)namescnt++] + "_peak";
    outNames[(size_t)(oFirstPk + nPeak + i)] = outNames[(size_t)(oFirstPk + i)] + "OK";
  }
  const int sCompFCR = namescnt;
  for (int i = 0; i < nPFCR; ++i) outNames[(size_t)(oFirstPkAtFCR + i)] = namesAtPeakFCR[(size_t)i] + "_at_peakFCR";
  std::cout << "outNames: ";
  for (auto& n : outNames) std::cout << n << " ";
  std::cout << std::endl;
  if (nInt) std::cout << "sCompInt: " << sCompInt << std::endl;
  if (nAvg) std::cout << "sCompAvg: " << sCompAvg << std::endl;
  if (nPeak) std::cout << "sCompPk: " << sCompPk << std::endl;
  if (nGrad) std::cout << "sCompGr: " << sCompGr << std::endl;
  if (nPFCR) std::cout << "sCompFCR: " << sCompFCR << std::endl;

  if (verbose) std::cerr << "Reading stream file data: " << infile << "...\n";
  std::cout << "NlevPath:  " << Nlev << '\n' << "nCompPath: " << nCompPath << '\n';  // read_ml_streamline_data (:1386-1387)
  for (int l = 0; l < Nlev; ++l) std::cout << "Calling ReadMF() at lev: " << l << " ...\n";
  if (verbose) {
    std::cerr << "...finished reading stream file \n" << "   got the following components: ";
    for (auto& n : names) std::cerr << n << ' ';
    std::cerr << '\n' << "nElts: " << P.nElts << '\n';
  }
  const long long nElts = P.nElts;
  if (nElts < 1) pa::Abort("the stream file has no elements");
  if (P.nodesPerElt != 3) pa::Abort("nodesPerElt = " + std::to_string(P.nodesPerElt) + " is not supported by streamTubeStats3d (triangles only)");
  if (P.boxes[0].empty()) pa::Abort("level 0 of the stream file has no Str box");

  // the flat box table, get_nPts / get_jlo (:830-848, placeholders included) and build_nodeMap (:1256-1281)
  std::vector<int64_t> box_desc;
  std::vector<const double*> fab;
  long long npts = 0, num_nodes = 0;
  int nPtsOnStr_max = 0, jlo = P.boxes[0][0].lo[1];
  for (int l = 0; l < Nlev; ++l)
    for (size_t b = 0; b < P.boxes[(size_t)l].size(); ++b) {
      const pa::Box3& B = P.boxes[(size_t)l][b];
      if (B.lo[0] != 0 || B.lo[2] != 0 || B.hi[2] != 0) pa::Abort("Str box " + pa::box_str(B) + " of level " + std::to_string(l) + " is not (0,jlo,0)..(n-1,jhi,0)");
      const long long ni = B.hi[0] + 1, nj = B.hi[1] - B.lo[1] + 1;
      box_desc.insert(box_desc.end(), {(int64_t)ni, (int64_t)nj, (int64_t)B.lo[1], (int64_t)npts});
      fab.push_back(P.data[(size_t)l][b].data());
      npts += ni * nj;
      nPtsOnStr_max = std::max<int>(nPtsOnStr_max, (int)nj);
      jlo = std::min(jlo, B.lo[1]);
      num_nodes += (long long)P.inside[(size_t)l][b].size();
    }
  const int nbt = (int)fab.size();
  pp.query("jlo", jlo);
  const int nPtsOnStr = std::min(nPtsOnStr_max, -2 * jlo + 1);
  if (verbose)
    std::cerr << "nodesPerElt:   " << P.nodesPerElt << '\n' << "nCompStr:      " << names.size() << '\n' << "nPtsOnStr_max: " << nPtsOnStr_max << '\n'
              << "jlo:           " << jlo << '\n' << "nPtsOnStr:     " << nPtsOnStr << '\n';
  std::vector<int32_t> node_table(2 * (size_t)num_nodes, -1);
  {
    int g = 0;
    for (int l = 0; l < Nlev; ++l)
      for (size_t b = 0; b < P.boxes[(size_t)l].size(); ++b, ++g) {
        const auto& ids = P.inside[(size_t)l][b];
        if ((long long)ids.size() > box_desc[4 * (size_t)g]) pa::Abort("Str box " + std::to_string(b) + " of level " + std::to_string(l) + " has more inside_nodes than lines");
        for (size_t k = 0; k < ids.size(); ++k) {
          if (ids[k] < 1 || ids[k] > num_nodes) pa::Abort("inside_nodes id " + std::to_string(ids[k]) + " outside 1 .. " + std::to_string(num_nodes));
          node_table[2 * (size_t)(ids[k] - 1)] = g;
          node_table[2 * (size_t)(ids[k] - 1) + 1] = (int32_t)k;
        }
      }
  }
  for (long long n = 0; n < num_nodes; ++n)
    if (node_table[2 * (size_t)n] < 0) pa::Abort("node " + std::to_string(n + 1) + " has no inside_nodes entry");
  for (int32_t v : P.faceData)
    if (v < 1 || v > num_nodes) pa::Abort("Elements: node id " + std::to_string(v) + " outside 1 .. " + std::to_string(num_nodes));
  for (int g = 0; g < nbt; ++g) {  // every box with lines holds j = 0 and the swept range (the reference indexes without a check)
    int l = 0, b = g;
    while (b >= (int)P.boxes[(size_t)l].size()) b -= (int)P.boxes[(size_t)l++].size();
    if (P.inside[(size_t)l][(size_t)b].empty()) continue;
    const long long bj = box_desc[4 * (size_t)g + 2], bh = bj + box_desc[4 * (size_t)g + 1] - 1;
    if (bj > 0 || bh < 0 || (nPtsOnStr >= 2 && (bj > jlo || bh < (long long)jlo + nPtsOnStr - 1)))
      pa::Abort("Str box " + std::to_string(b) + " of level " + std::to_string(l) + " (j = " + std::to_string(bj) + " .. " + std::to_string(bh) + ") does not hold j = 0 and j = " +
                std::to_string(jlo) + " .. " + std::to_string((long long)jlo + nPtsOnStr - 1));
  }
  if (nPFCR > 32) pa::Abort("more than 32 compsAtPeakFCR");
  for (int j = 0; j < nAux; ++j)
    for (int32_t v : P.faceData)
      if (v > aux.nNodes) pa::Abort("aux_mef has fewer nodes than the stream file");

  // components `m` (in memory) of every box, flat: box g at m.size() * off_g, component-major
  auto gather = [&](const std::vector<int>& m) {
    std::vector<double> v((size_t)((long long)m.size() * npts));
    for (int g = 0; g < nbt; ++g) {
      const long long np = box_desc[4 * (size_t)g] * box_desc[4 * (size_t)g + 1], off = box_desc[4 * (size_t)g + 3];
      for (size_t c = 0; c < m.size(); ++c) std::copy(fab[(size_t)g] + (size_t)mem[(size_t)m[c]] * np, fab[(size_t)g] + (size_t)(mem[(size_t)m[c]] + 1) * np, v.begin() + (size_t)((long long)m.size() * off + (long long)c * np));
    }
    return v;
  };

  std::vector<double> integrals((size_t)(nElts * nCompOut), 0.0);  // [nElts][nCompOut]
  auto put = [&](int o, const std::vector<double>& col, size_t from = 0) {
    for (long long i = 0; i < nElts; ++i) integrals[(size_t)(i * nCompOut + o)] = col[from + (size_t)i];
  };
  std::vector<double> totalIntegral((size_t)nInt, 0.0);
  const size_t eb = sizeof(double) * (size_t)nElts, nb8 = sizeof(double) * (size_t)num_nodes;
  {
    pa::Ctx ctx;
    pa_tube* tube = pa_tube_create(ctx.h, nbt, box_desc.data(), num_nodes, node_table.data(), nElts, P.faceData.data());
    if (!tube) pa::Abort(pa_last_error(ctx.h));
    const std::vector<double> hxyz = gather({idX[0], idX[1], idX[2]});
    DBuf dxyz(ctx, hxyz.size() * 8);
    dxyz.up(hxyz.data(), hxyz.size() * 8);
    std::vector<double> col((size_t)nElts);
    auto up_comps = [&](const std::vector<int>& m) {
      const std::vector<double> h = gather(m);
      std::unique_ptr<DBuf> d(new DBuf(ctx, h.size() * 8));
      d->up(h.data(), h.size() * 8);
      return d;
    };

    // max_grad of every node (:581-589), then the element means (:724-730)
    int use_eps = 0;
    pp.query("grad_use_eps", use_eps);
    DBuf dnode(ctx, nb8 * (size_t)std::max(1, std::max(nGrad, std::max(nPeak ? 1 : 0, nPFCR)))), delt(ctx, eb * (size_t)std::max(1, std::max(nGrad, nPFCR)));
    DBuf dok(ctx, sizeof(int32_t) * (size_t)num_nodes);
    std::vector<int32_t> ok((size_t)num_nodes);
    std::vector<double> cols;
    for (int j = 0; j < nGrad; ++j) {
      auto d = up_comps({sCompGr + j});
      ctx.check(pa_tube_lines(ctx.h, tube, dxyz.d(), d->d(), 1, 0, use_eps, dnode.d() + (size_t)j * (size_t)num_nodes));
    }
    if (nGrad) {
      ctx.check(pa_tube_node_means(ctx.h, tube, nGrad, dnode.d(), delt.d()));
      cols.resize((size_t)(nGrad * nElts));
      delt.down(cols.data(), eb * (size_t)nGrad);
      for (int j = 0; j < nGrad; ++j) put(oFirstGr + j, cols, (size_t)(j * nElts));
    }
    auto count_bad = [&]() {  // peak_val's stderr line, once per node (:991-996)
      dok.down(ok.data(), sizeof(int32_t) * ok.size());
      for (int32_t v : ok)
        if (!v) std::cerr << "peakVal on end of line!" << std::endl;
    };
    for (int j = 0; j < nPeak; ++j) {  // :591-606, :732-743
      auto d = up_comps({sCompPk + j});
      const int32_t s0 = 0;
      ctx.check(pa_tube_peaks(ctx.h, tube, d->d(), 1, 0, 1, &s0, dnode.d(), (int32_t*)dok.p));
      count_bad();
      ctx.check(pa_tube_node_means(ctx.h, tube, 1, dnode.d(), delt.d()));
      delt.down(col.data(), eb);
      put(oFirstPk + j, col);
      ctx.check(pa_tube_node_all(ctx.h, tube, (const int32_t*)dok.p, delt.d()));
      delt.down(col.data(), eb);
      put(oFirstPk + nPeak + j, col);
    }
    if (idPFCR >= 0) {  // :608-627, :744-753: the samples start AT the FCR component (compsAtPeakFCR[i] = sCompFCR + i = idPFCR + 3 + i)
      std::vector<int> m = {idPFCR + 3};
      std::vector<int32_t> sc;
      for (int i = 0; i < nPFCR; ++i) {
        const int want = sCompFCR + i;
        size_t at = 0;
        while (at < m.size() && m[at] != want) ++at;
        if (at == m.size()) m.push_back(want);
        sc.push_back((int32_t)at);
      }
      auto d = up_comps(m);
      ctx.check(pa_tube_peaks(ctx.h, tube, d->d(), (int32_t)m.size(), 0, nPFCR, sc.data(), dnode.d(), (int32_t*)dok.p));
      count_bad();
      if (nPFCR) {
        ctx.check(pa_tube_node_means(ctx.h, tube, nPFCR, dnode.d(), delt.d()));
        cols.resize((size_t)(nPFCR * nElts));
        delt.down(cols.data(), eb * (size_t)nPFCR);
        for (int j = 0; j < nPFCR; ++j) put(oFirstPkAtFCR + j, cols, (size_t)(j * nElts));
      }
    }
    if (verbose) {
      std::cout << "cnt: " << cnt << '\n';
      for (size_t i = 0; i < outNames.size(); i++) std::cout << "outNames[" << i << "]: " << outNames[i] << '\n';
      std::cout << '\n' << "Integrating paths ..." << std::endl;
    }

    // the integrals (:650-699): the coordinates stay resident, the integrated components pass through in groups
    int nCompsPerPass = -1;
    const bool perPassGiven = pp.query("nCompsPerPass", nCompsPerPass);
    if (perPassGiven && nCompsPerPass <= 0) pa::Abort("nCompsPerPass must be positive");
    if (!perPassGiven) {  // as many components as fit in 3/4 of the free device memory
      int64_t fr = 0, tot = 0;
      ctx.check(pa_device_mem_info(ctx.h, &fr, &tot));
      nCompsPerPass = (int)std::max<long long>(1, std::min<long long>(std::max(nInt, 1), (fr / 4 * 3) / std::max(1LL, 8 * npts + 16 * nElts)));
    }
    DBuf dvol(ctx, eb), darea(ctx, eb), dwa(ctx, eb);
    for (int i = 0; i < nInt || i == 0; i += nCompsPerPass) {
      const int kw = std::max(0, std::min(nCompsPerPass, nInt - i));
      std::vector<int> m;
      for (int k = 0; k < kw; ++k) m.push_back(sCompInt + i + k);
      auto d = up_comps(m);
      DBuf draw(ctx, eb * (size_t)kw), dper(ctx, eb * (size_t)kw);
      ctx.check(pa_tube_wedges(ctx.h, tube, dxyz.d(), d->d(), kw, jlo, nPtsOnStr, i == 0, dvol.d(), darea.d(), dwa.d(), draw.d(), dper.d()));
      cols.resize((size_t)(kw * nElts));
      draw.down(cols.data(), eb * (size_t)kw);
      for (int k = 0; k < kw; ++k)  // :693-694: a plain sum in element order, before the division by the area
        for (long long e = 0; e < nElts; ++e) totalIntegral[(size_t)(i + k)] += cols[(size_t)(k * nElts + e)];
      dper.down(cols.data(), eb * (size_t)kw);
      for (int k = 0; k < kw; ++k) put(oFirstInt + i + k, cols, (size_t)(k * nElts));
    }
    dvol.down(col.data(), eb);
    put(oVol, col);
    dwa.down(col.data(), eb);
    put(oWA, col);
    darea.down(col.data(), eb);
    put(oArea, col);
    for (int j = 0; j < nAvg; ++j) {  // :703-713
      auto d = up_comps({sCompAvg + j});
      ctx.check(pa_tube_node_avg(ctx.h, tube, d->d(), 1, 0, delt.d()));
      delt.down(col.data(), eb);
      put(oFirstAvg + j, col);
    }
    for (int j = 0; j < nAux; ++j)  // :716-722: the sum, then *= 1/nodesPerElt in integer arithmetic
      for (long long e = 0; e < nElts; ++e) {
        double s = 0;
        for (int k = 0; k < 3; ++k) s += aux.nodes[(size_t)(P.faceData[(size_t)(3 * e + k)] - 1) * aux.names.size() + (size_t)aux_mef_comps[(size_t)j]];
        integrals[(size_t)(e * nCompOut + oFirstAux + j)] = s * (double)(1 / (int)P.nodesPerElt);
      }

    int nSmooth = 0;  // :757-791
    pp.query("nSmooth", nSmooth);
    for (long long e = 0; e < nElts; ++e) integrals[(size_t)(e * nCompOut + oSmInt)] = nCompOut > oFirstInt ? integrals[(size_t)(e * nCompOut + oFirstInt)] : 0.0;
    if (nSmooth > 0) {
      if (verbose) std::cerr << "Computing element neighbors for smoothing...\n" << "Smoothing...\n";
      for (long long e = 0; e < nElts; ++e) col[(size_t)e] = integrals[(size_t)(e * nCompOut + oSmInt)];
      DBuf dvals(ctx, eb);
      dvals.up(col.data(), eb);
      ctx.check(pa_tube_smooth(ctx.h, tube, dvals.d(), darea.d(), nSmooth, delt.d()));
      delt.down(col.data(), eb);
      put(oSmInt, col);
    }
    pa_tube_destroy(tube);
  }

  if (verbose) std::cerr << "Writing output...\n";
  int write_tec = 0, write_mef = 1;
  pp.query("write_tec", write_tec);
  pp.query("write_mef", write_mef);
  // the multiply defined nodes of the writers (:1638-1665): each triangle's three corners at line point 0 carry the triangle's values
  const int nc = 3 + nCompOut;
  const long long nPts = 3 * nElts;
  std::vector<double> fake;
  std::vector<int32_t> conn0((size_t)nPts);
  auto build_fake = [&]() {
    std::cout << "Building new node data" << std::endl;
    if (!fake.empty()) return;
    fake.resize((size_t)(nPts * nc));
    for (long long q = 0; q < nPts; ++q) {
      const int32_t id = P.faceData[(size_t)q] - 1, g = node_table[2 * (size_t)id], k = node_table[2 * (size_t)id + 1];
      const long long ni = box_desc[4 * (size_t)g], np = ni * box_desc[4 * (size_t)g + 1], at = (0 - box_desc[4 * (size_t)g + 2]) * ni + k;
      for (int d = 0; d < 3; ++d) fake[(size_t)(q * nc + d)] = fab[(size_t)g][(size_t)mem[(size_t)idX[d]] * (size_t)np + (size_t)at];
      std::copy(integrals.begin() + (q / 3) * nCompOut, integrals.begin() + (q / 3 + 1) * nCompOut, fake.begin() + q * nc + 3);
      conn0[(size_t)q] = (int32_t)q;
    }
  };
  std::vector<std::string> vars = {"X", "Y", "Z"};
  vars.insert(vars.end(), outNames.begin(), outNames.end());
  const std::string label = "Volume integrals";
  if (write_tec) {
    build_fake();
    const std::string thisOut = outfile + "_volInt.dat";
    std::ofstream os(thisOut);
    if (!os) pa::Abort("Unable to create " + thisOut);
    os << "VARIABLES =";
    for (auto& v : vars) os << " " << v;
    os << std::endl;
    os << "ZONE T=\"" << label << "\" N=" << nPts << " E=" << nElts << " F=FEBLOCK ET=TRIANGLE" << std::endl;
    for (int k = 0; k < nc; ++k) {
      for (long long i = 0; i < nPts; ++i) os << fake[(size_t)(i * nc + k)] << (i % 5 == 4 ? "\n" : " ");  // operator<<, default precision
      os << std::endl;
    }
    for (long long i = 0; i < nElts; ++i) os << 3 * i + 1 << " " << 3 * i + 2 << " " << 3 * i + 3 << " " << std::endl;
  }
  if (write_mef) {
    build_fake();
    pa::write_mef(outfile + "_volInt.mef", label, vars, fake, conn0);
  }
  std::cout << "Total integrals: " << std::endl;
  for (int j = 0; j < nInt; ++j) std::cout << "  " << names[(size_t)(3 + j)] << ": " << totalIntegral[(size_t)j] << std::endl;
  return 0;
}
