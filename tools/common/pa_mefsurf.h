// pa_mefsurf.h -- a MEF file as a device surface (pa_surf) and back, for the tools that edit node fields (combineMEF3d, scaleMEF3d,
// multMEF3d).  pa_surf_create wants three components in front; the one-component file multMEF3d writes is a legitimate input of
// combineMEF3d, so a file of fewer than three components is uploaded with zero columns behind its own -- combineMEF3d checks every
// component a user names against the FILE's count, so a padding column is never read.  scaleMEF3d and multMEF3d refuse such files.
#pragma once
#include "pa_device.h"

namespace pa {
inline pa_surf* surf_of_mef(Ctx& ctx, const MefSurface& S, const std::string& file, const char* tool) {
  if (S.nodesPerElt != 3) Abort(std::string(tool) + " needs 3 nodes per element, " + file + " has " + std::to_string(S.nodesPerElt));
  const size_t nc = S.names.size(), ncp = std::max<size_t>(nc, 3);
  if (nc == 0) Abort(file + " has no node components");
  pa_surf* sf = nullptr;
  if (ncp == nc) {
    sf = pa_surf_create(ctx.h, S.nNodes, (int)nc, S.nodes.data(), S.nElts, S.conn.data());
  } else {
    std::vector<double> padded((size_t)S.nNodes * ncp, 0.0);
    for (size_t i = 0; i < (size_t)S.nNodes; ++i)
      for (size_t c = 0; c < nc; ++c) padded[i * ncp + c] = S.nodes[i * nc + c];
    sf = pa_surf_create(ctx.h, S.nNodes, (int)ncp, padded.data(), S.nElts, S.conn.data());
  }
  if (!sf) Abort(pa_last_error(ctx.h));
  return sf;
}
// the surface as write_mef takes it; destroys the handle
inline void write_surf(Ctx& ctx, pa_surf* sf, const std::string& outfile, const std::string& title, const std::vector<std::string>& names) {
  int64_t nNodes = 0, nElts = 0;
  int nComp = 0;
  ctx.check(pa_surf_counts(sf, &nNodes, &nElts, &nComp));
  if ((size_t)nComp != names.size()) Abort("write_surf: " + std::to_string(nComp) + " components, " + std::to_string(names.size()) + " names");
  std::vector<double> nodes((size_t)nNodes * (size_t)nComp);
  std::vector<int32_t> elts((size_t)nElts * 3);
  ctx.check(pa_surf_read(ctx.h, sf, nodes.data(), elts.data()));
  pa_surf_destroy(sf);
  for (int32_t& e : elts) e -= 1;  // write_mef takes 0-based triples
  write_mef(outfile, title, names, nodes, elts);
}
// comps= or sComp= nComp= (combineMEF.cpp:127-163, scaleMEF.cpp:77-94, multMEF.cpp:116-133); every entry must name a component of the file
inline std::vector<int> comps_of(const ParmParse& pp, const std::string& list, const std::string& s, const std::string& n, int ndef, int nfile, const std::string& file) {
  std::vector<int> comps;
  if (pp.countval(list) > 0) {
    pp.getarr(list, comps);
  } else {
    int sComp = 0, nComp = ndef;
    pp.query(s, sComp);
    pp.query(n, nComp);
    for (int i = 0; i < nComp; ++i) comps.push_back(sComp + i);
  }
  for (int c : comps)
    if (c < 0 || c >= nfile) Abort(list + ": " + std::to_string(c) + " is not a node variable of " + file);
  return comps;
}
}  // namespace pa
