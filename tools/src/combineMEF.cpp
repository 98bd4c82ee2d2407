// combineMEF3d -- drop-in for PeleAnalysis Src/combineMEF.cpp: a MEF surface whose node fields are chosen components of two files of
// the same surface, on MI355X (pa_surfjoin.hip: column copies on the device handle).
//   combineMEF3d.ex infileL=<l.mef> infileR=<r.mef> outfile=<out.mef> [compsL="c ..." | sCompL=0 nCompL=<all>] [compsR="c ..." | sCompR=0 nCompR=<all>]
// The output holds the chosen components of L, then those of R (:165-179), in the given order, repeats allowed; title and elements are
// L's (:181).  stdout as the reference's: "(L): <name>" per component of L, then "(R): <name>" per component of R.  Files whose
// element counts differ abort with the reference's "MEF files not compible" (:117-120).
// Deviations: files whose NODE counts differ abort (the reference copies over the intersection of the two boxes and
// leaves the rest uninitialised); a component out of range aborts (the reference asserts in debug builds only); elements that are not
// triangles abort.  Everything is checked before outfile is touched.  One GPU.
#include "../common/pa_mefsurf.h"

int main(int argc, char** argv) {
  pa::ParmParse pp(argc, argv);
  std::string infileL, infileR, outfile;
  pp.get("infileL", infileL);
  pp.get("infileR", infileR);
  pp.get("outfile", outfile);
  pa::AsyncCtx actx;  // the device comes up while the files are read
  const pa::MefSurface L = pa::read_mef(infileL), R = pa::read_mef(infileR);
  if (L.nElts != R.nElts) pa::Abort("MEF files not compible");
  const std::vector<int> compsL = pa::comps_of(pp, "compsL", "sCompL", "nCompL", (int)L.names.size(), (int)L.names.size(), infileL);
  const std::vector<int> compsR = pa::comps_of(pp, "compsR", "sCompR", "nCompR", (int)R.names.size(), (int)R.names.size(), infileR);
  if (compsL.empty() && compsR.empty()) pa::Abort("combineMEF3d: no component is chosen");
  if (L.nNodes != R.nNodes) pa::Abort("combineMEF3d: " + infileL + " has " + std::to_string(L.nNodes) + " nodes, " + infileR + " has " + std::to_string(R.nNodes));

  pa::Ctx& ctx = actx.get();
  pa_surf* sl = pa::surf_of_mef(ctx, L, infileL, "combineMEF3d");
  pa_surf* sr = pa::surf_of_mef(ctx, R, infileR, "combineMEF3d");
  std::vector<int32_t> which, comps;
  std::vector<std::string> names;
  for (int c : compsL) { which.push_back(0); comps.push_back(c); names.push_back(L.names[(size_t)c]); }
  for (int c : compsR) { which.push_back(1); comps.push_back(c); names.push_back(R.names[(size_t)c]); }
  pa_surf* out = pa_surfjoin_select(ctx.h, sl, sr, (int)which.size(), which.data(), comps.data());
  if (!out) pa::Abort(pa_last_error(ctx.h));
  pa_surf_destroy(sl);
  pa_surf_destroy(sr);
  for (int c : compsL) std::cout << "(L): " << L.names[(size_t)c] << std::endl;
  for (int c : compsR) std::cout << "(R): " << R.names[(size_t)c] << std::endl;
  pa::write_surf(ctx, out, outfile, L.title, names);
  pa::Finish();
}
