// multMEF3d -- drop-in for PeleAnalysis Src/multMEF.cpp: the product of node fields of a MEF surface as a one-component MEF, on MI355X
// (pa_surfjoin.hip).
//   multMEF3d.ex infile=<in.mef> outfile=<out.mef> [comps="c ..." | sComp=0 nComp=1] [nameOut=product]
// The one component is ((1.0 * value[comps[0]]) * value[comps[1]]) * ... at every node (:139-148), repeats allowed; title and elements
// are the input's.  The reference prints nothing, and neither does this tool.
// Deviations: a component out of range aborts (the reference asserts in debug builds only); at most 32 components;
// elements that are not triangles and files of fewer than three components abort.  Everything is checked before outfile is touched.  One GPU.
#include "../common/pa_mefsurf.h"

int main(int argc, char** argv) {
  pa::ParmParse pp(argc, argv);
  std::string infile, outfile, nameOut = "product";
  pp.get("infile", infile);
  pp.get("outfile", outfile);
  pp.query("nameOut", nameOut);
  pa::AsyncCtx actx;  // the device comes up while the file is read
  const pa::MefSurface S = pa::read_mef(infile);
  if (S.names.size() < 3) pa::Abort("multMEF3d needs the node coordinates x, y, z as the first three components");
  const std::vector<int> comps = pa::comps_of(pp, "comps", "sComp", "nComp", 1, (int)S.names.size(), infile);
  if (comps.empty() || comps.size() > 32) pa::Abort("multMEF3d takes 1 to 32 components");
  pa::Ctx& ctx = actx.get();
  pa_surf* sf = pa::surf_of_mef(ctx, S, infile, "multMEF3d");
  const std::vector<int32_t> c32(comps.begin(), comps.end());
  pa_surf* out = pa_surfjoin_product(ctx.h, sf, (int)c32.size(), c32.data());
  if (!out) pa::Abort(pa_last_error(ctx.h));
  pa_surf_destroy(sf);
  pa::write_surf(ctx, out, outfile, S.title, {nameOut});
  pa::Finish();
}
