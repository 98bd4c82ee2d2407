// smoothMEF3d -- drop-in for PeleAnalysis Src/smoothMEF.cpp: smooth one node field of a MEF surface over the one-ring of elements,
// on MI355X (pa_surfsmooth.hip).
//   smoothMEF3d.ex infile=<in.mef> outfile=<out.mef> comp=<c> [areaComp=-1] [nSmooth=1]
// The field goes to the elements (the mean of the three node values), is averaged nSmooth times over each element and the elements
// that share a node with it, weighted by area, and comes back to the nodes as the area-weighted mean of the elements at each node.
// The areas are component areaComp (the mean of the three node values) where it names a component of the file, else the triangles'
// own (:221, :231-243).  The title and the names pass through.  The reference prints nothing, and neither does this tool.
// Deviations: the algorithm is the reference's evident intent, not its letter -- its code indexes element areas by
// node id, weights by a running partial sum, divides by the area twice and writes element values over node slots (:241-273); comp
// must name a component and nSmooth must not be negative; elements that are not triangles and, without areaComp, files of fewer
// than three components abort.  Everything is checked before outfile is touched.  One GPU.
#include "../common/pa_mefsurf.h"

int main(int argc, char** argv) {
  pa::ParmParse pp(argc, argv);
  std::string infile, outfile;
  pp.get("infile", infile);
  pp.get("outfile", outfile);
  int comp = -1, areaComp = -1, nSmooth = 1;
  pp.get("comp", comp);
  pp.query("areaComp", areaComp);
  pp.query("nSmooth", nSmooth);
  pa::AsyncCtx actx;  // the device comes up while the file is read
  const pa::MefSurface S = pa::read_mef(infile);
  const int nCompMEF = (int)S.names.size();
  if (S.nodesPerElt != 3) pa::Abort("smoothMEF3d needs 3 nodes per element, " + infile + " has " + std::to_string(S.nodesPerElt));
  if (comp < 0 || comp >= nCompMEF) pa::Abort("comp: " + std::to_string(comp) + " is not a node variable of " + infile);
  if (nSmooth < 0) pa::Abort("nSmooth must not be negative");
  const bool by_comp = areaComp >= 0 && areaComp < nCompMEF;
  if (!by_comp && nCompMEF < 3) pa::Abort("smoothMEF3d needs the node coordinates x, y, z as the first three components, or areaComp");
  pa::Ctx& ctx = actx.get();
  pa_surf* sf = pa::surf_of_mef(ctx, S, infile, "smoothMEF3d");
  ctx.check(pa_surfsmooth_run(ctx.h, sf, comp, by_comp ? areaComp : -1, nSmooth));
  // a file of fewer than three components was uploaded with zero columns behind its own: only its own go out
  int64_t nNodes = 0, nElts = 0;
  int nc = 0;
  ctx.check(pa_surf_counts(sf, &nNodes, &nElts, &nc));
  if (nc == nCompMEF) {
    pa::write_surf(ctx, sf, outfile, S.title, S.names);
  } else {
    std::vector<double> all((size_t)nNodes * (size_t)nc), nodes((size_t)nNodes * (size_t)nCompMEF);
    std::vector<int32_t> elts((size_t)nElts * 3);
    ctx.check(pa_surf_read(ctx.h, sf, all.data(), elts.data()));
    pa_surf_destroy(sf);
    for (size_t i = 0; i < (size_t)nNodes; ++i)
      for (int c = 0; c < nCompMEF; ++c) nodes[i * (size_t)nCompMEF + (size_t)c] = all[i * (size_t)nc + (size_t)c];
    for (int32_t& e : elts) e -= 1;
    pa::write_mef(outfile, S.title, S.names, nodes, elts);
  }
  pa::Finish();
}
