// scaleMEF3d -- drop-in for PeleAnalysis Src/scaleMEF.cpp: multiply node fields of a MEF surface by constants, on MI355X
// (pa_surfjoin.hip).
//   scaleMEF3d.ex infile=<in.mef> outfile=<out.mef> [comps="c ..." | sComp=0 nComp=1] vals="v ..." [newNames="n ..." newComps="c ..."]
// value[comps[j]] = value[comps[j]] * vals[j] at every node, for j in list order (:101-108): a component named twice is scaled twice.
// newNames / newComps rename components of the output (:110-125).  The reference prints nothing, and neither does this tool.
// Deviations: vals must have one value per component and newNames one name per entry of newComps (the reference
// asserts in debug builds only); a component or a newComps entry at or past the component count aborts (the reference's assert
// allows newComps one past the end); elements that are not triangles and files of fewer than three components abort.  Everything is checked before outfile is touched.  One GPU.
#include "../common/pa_mefsurf.h"

int main(int argc, char** argv) {
  pa::ParmParse pp(argc, argv);
  std::string infile, outfile;
  pp.get("infile", infile);
  pp.get("outfile", outfile);
  pa::AsyncCtx actx;  // the device comes up while the file is read
  const pa::MefSurface S = pa::read_mef(infile);
  const int nCompMEF = (int)S.names.size();
  if (nCompMEF < 3) pa::Abort("scaleMEF3d needs the node coordinates x, y, z as the first three components");
  const std::vector<int> comps = pa::comps_of(pp, "comps", "sComp", "nComp", 1, nCompMEF, infile);
  std::vector<double> vals;
  if (pp.countval("vals") != (int)comps.size()) pa::Abort("vals needs one value per component (" + std::to_string(comps.size()) + ")");
  if (!comps.empty()) pp.getarr("vals", vals);
  std::vector<std::string> names = S.names;
  if (pp.countval("newNames") > 0) {
    std::vector<std::string> newNames;
    std::vector<int> newComps;
    if (pp.countval("newComps") != pp.countval("newNames")) pa::Abort("newNames and newComps need the same number of entries");
    pp.getarr("newNames", newNames);
    pp.getarr("newComps", newComps);
    for (size_t i = 0; i < newNames.size(); ++i) {
      if (newComps[i] < 0 || newComps[i] >= nCompMEF) pa::Abort("newComps: " + std::to_string(newComps[i]) + " is not a node variable of " + infile);
      names[(size_t)newComps[i]] = newNames[i];
    }
  }
  pa::Ctx& ctx = actx.get();
  pa_surf* sf = pa::surf_of_mef(ctx, S, infile, "scaleMEF3d");
  const std::vector<int32_t> c32(comps.begin(), comps.end());
  ctx.check(pa_surfjoin_scale(ctx.h, sf, (int)c32.size(), c32.data(), vals.data()));
  pa::write_surf(ctx, sf, outfile, S.title, names);
  pa::Finish();
}
