// trimMEFgen3d -- drop-in for PeleAnalysis Src/trimMEFgen.cpp: cut parts of a MEF surface away by conditions on its node fields, on
// MI355X (pa_surfcut.hip: flags, scans and order-preserving gathers).
//   trimMEFgen3d.ex infile=<in.mef> outfile=<out.mef> [comps="c ..." signs="lt|le|gt|ge|eq ..." vals="v ..."] [RXY=<r> sign_RXY=<sign>]
//                   [remComps="c ..."] [do_area_stats=0]
// A node is removed where ANY condition value[comps[i]] <signs[i]> vals[i] holds (trim_surface, :90-192) or, with RXY >= 0, where
// sqrt(x*x + y*y) <sign_RXY> RXY holds (trim_surface_RXY, :195-294; the two passes compose to one OR because both keep the order); an
// element survives only if all three of its nodes do; nodes no surviving element uses are removed (:297-372).  stdout as the
// reference's: "Surface area before: ", "Surface area after: ", with do_area_stats "  Triangle area min, max: <a> , <b>", and
// "Removed <n> unusued nodes" when n > 0.  remComps drops node components when the file is written (:464-497).  An unknown sign aborts
// with the reference's message (after its line on stdout).
// Deviations: the two area totals are exactly rounded fixed-point sums (the reference adds serially); a trim that
// removes everything aborts before outfile is touched (the reference builds an invalid box); elements that are not triangles abort;
// the triangle areas are those of the first three components of the FILE, also where remComps names one of them.  One GPU.
#include "../common/pa_device.h"

static int sign_of(const std::string& s) {
  static const char* names[5] = {"lt", "le", "gt", "ge", "eq"};
  for (int i = 0; i < 5; ++i)
    if (s == names[i]) return i;
  return -1;
}

int main(int argc, char** argv) {
  pa::ParmParse pp(argc, argv);
  std::string infile, outfile;
  pp.get("infile", infile);
  pp.get("outfile", outfile);
  pa::AsyncCtx actx;  // the device comes up while the file is read
  const pa::MefSurface S = pa::read_mef(infile);
  const int nComp = (int)S.names.size();
  if (S.nodesPerElt != 3) pa::Abort("trimMEFgen3d needs 3 nodes per element, " + infile + " has " + std::to_string(S.nodesPerElt));
  if (nComp < 3) pa::Abort("trimMEFgen3d needs the node coordinates x, y, z as the first three components");

  pa::Ctx& ctx = actx.get();
  pa_surf* sf = pa_surf_create(ctx.h, S.nNodes, nComp, S.nodes.data(), S.nElts, S.conn.data());
  if (!sf) pa::Abort(pa_last_error(ctx.h));
  double area = 0, amin = 0, amax = 0;
  ctx.check(pa_surf_area(ctx.h, sf, &area, nullptr, nullptr));
  std::cout << "Surface area before: " << area << '\n';

  std::vector<int> comps;
  std::vector<int32_t> ops;
  std::vector<double> vals;
  const int nc = pp.countval("comps");
  if (nc > 0) {
    pp.getarr("comps", comps);
    std::vector<std::string> signs;
    if (pp.countval("signs") != nc || pp.countval("vals") != nc) pa::Abort("signs and vals need one value per entry of comps");
    pp.getarr("signs", signs);
    pp.getarr("vals", vals);
    for (int i = 0; i < nc; ++i) {
      if (comps[(size_t)i] < 0 || comps[(size_t)i] >= nComp) pa::Abort("comps: " + std::to_string(comps[(size_t)i]) + " is not a node variable of " + infile);
      const int op = sign_of(signs[(size_t)i]);
      if (op < 0) {
        std::cout << "i,signs[i] " << i << "," << signs[(size_t)i] << std::endl;
        pa::Abort("Bad signs data. Use one of [lt,le,gt,ge,eq]");
      }
      ops.push_back(op);
    }
  }
  double RXY = -1;
  pp.query("RXY", RXY);
  int rxy_op = 0;
  if (RXY >= 0) {
    std::string sign_RXY;
    pp.get("sign_RXY", sign_RXY);
    rxy_op = sign_of(sign_RXY);
    if (rxy_op < 0) {
      std::cout << "sign_RXY: " << sign_RXY << std::endl;
      pa::Abort("Bad sign data.  Use one of [lt,le,gt,ge,eq]");
    }
  }
  std::vector<int> remComps;
  if (pp.countval("remComps") > 0) pp.getarr("remComps", remComps);
  bool do_area_stats = false;
  pp.query("do_area_stats", do_area_stats);

  std::vector<int32_t> c32(comps.begin(), comps.end());
  int64_t unused = 0, nNodes = 0, nElts = 0;
  ctx.check(pa_surf_trim(ctx.h, sf, nc, c32.data(), ops.data(), vals.data(), RXY >= 0 ? RXY : -1.0, rxy_op, &unused));
  ctx.check(pa_surf_counts(sf, &nNodes, &nElts, nullptr));
  if (nElts == 0 || nNodes == 0) pa::Abort("trimMEFgen3d: the conditions remove every element of " + infile + ": " + outfile + " is not written");
  ctx.check(pa_surf_area(ctx.h, sf, &area, &amin, &amax));
  std::cout << "Surface area after: " << area << '\n';
  if (do_area_stats) std::cout << "  Triangle area min, max: " << amin << " , " << amax << '\n';
  if (unused > 0) std::cout << "Removed " << unused << " unusued nodes" << std::endl;

  std::vector<double> nodes((size_t)nNodes * (size_t)nComp);
  std::vector<int32_t> elts((size_t)nElts * 3);
  ctx.check(pa_surf_read(ctx.h, sf, nodes.data(), elts.data()));
  pa_surf_destroy(sf);
  std::vector<std::string> names = S.names;
  if (!remComps.empty()) {  // :464-497
    std::vector<int> keep;
    for (int i = 0; i < nComp; ++i) {
      bool k = true;
      for (int r : remComps) if (r == i) k = false;
      if (k) keep.push_back(i);
    }
    if (keep.empty()) pa::Abort("remComps removes every component");
    std::vector<double> nn((size_t)nNodes * keep.size());
    for (size_t i = 0; i < (size_t)nNodes; ++i)
      for (size_t j = 0; j < keep.size(); ++j) nn[i * keep.size() + j] = nodes[i * (size_t)nComp + (size_t)keep[j]];
    nodes.swap(nn);
    names.clear();
    for (int c : keep) names.push_back(S.names[(size_t)c]);
  }
  for (int32_t& e : elts) e -= 1;  // write_mef takes 0-based triples
  pa::write_mef(outfile, S.title, names, nodes, elts);
  pa::Finish();
}
