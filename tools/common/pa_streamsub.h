// pa_streamsub.h -- the host-only pieces of streamSub3d (tools/src/streamSub.cpp): the default output name (streamSub.cpp:88-93), the
// keys -> the element list (:103-118, plus the seed-box keys of our own), the names -> the component selection (:121-147), the flat
// tables with the checks of build_nodeMap (:228-250), and every refusal.  No GPU, no I/O: tools/src/streamSubCheck.cpp runs all of it
// as a stand-alone program, plain and under AddressSanitizer + UBSan.  A function returns false with the message the tool aborts with.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "pa_parmparse.h"

namespace pa {

// :88-93: infile split at '.', the last token dropped when there are several, rejoined with '.', "_new" appended.  Empty tokens are
// kept (AMReX's Tokenize, not in the reference tree, is recalled to drop them: "./a.b" would become "/a_new")
inline std::string streamsub_default_outfile(const std::string& infile) {
  std::vector<std::string> tok(1);
  for (char c : infile) {
    if (c == '.') tok.emplace_back();
    else tok.back() += c;
  }
  std::string out = tok[0];
  for (size_t i = 1; i + 1 < tok.size(); ++i) out += "." + tok[i];
  return out + "_new";
}

struct SubKeys {
  bool hasEltIDs = false, hasSElt = false, hasNElt = false, hasLo = false, hasHi = false;
  std::vector<int> eltIDs;
  int sElt = 0, nElt = 1;
  std::vector<double> seedLo, seedHi;
};
inline void streamsub_read_keys(const ParmParse& pp, SubKeys& K) {
  K.hasEltIDs = pp.countval("eltIDs") > 0;  // :104
  if (K.hasEltIDs) pp.getarr("eltIDs", K.eltIDs);
  K.hasSElt = pp.query("sElt", K.sElt);
  K.hasNElt = pp.query("nElt", K.nElt);
  K.hasLo = pp.contains("seedLo");
  K.hasHi = pp.contains("seedHi");
  if (K.hasLo) pp.getarr("seedLo", K.seedLo);
  if (K.hasHi) pp.getarr("seedHi", K.seedHi);
}
// bySeed: the list comes from the seed points (pa_ssub_select_seedbox); else E holds it (:103-118), checked against 0 .. nElts-1
inline bool streamsub_element_list(const SubKeys& K, long long nElts, bool& bySeed, std::vector<int32_t>& E, std::string& why) {
  bySeed = false;
  E.clear();
  if (K.hasLo || K.hasHi) {
    if (!(K.hasLo && K.hasHi)) { why = "seedLo and seedHi must come together"; return false; }
    if (K.hasEltIDs || K.hasSElt || K.hasNElt) { why = "seedLo / seedHi exclude eltIDs, sElt and nElt"; return false; }
    if (K.seedLo.size() != 3 || K.seedHi.size() != 3) { why = "seedLo and seedHi take three values each"; return false; }
    bySeed = true;
    return true;
  }
  if (K.hasEltIDs) {
    for (int e : K.eltIDs) E.push_back(e);
  } else {
    if (K.nElt <= 0) { why = "nElt = " + std::to_string(K.nElt) + ": no element is selected"; return false; }
    for (int i = 0; i < K.nElt; ++i) {
      const long long e = (long long)K.sElt + i;
      if (e < 0 || e >= nElts) { why = "element id " + std::to_string(e) + " outside 0 .. " + std::to_string(nElts - 1); return false; }
      E.push_back((int32_t)e);
    }
  }
  for (int32_t e : E)
    if (e < 0 || e >= nElts) { why = "element id " + std::to_string(e) + " outside 0 .. " + std::to_string(nElts - 1); return false; }
  return true;
}

// :121-147: without `want` every component; with it the file components whose name is listed, in the FILE's order (a name the file
// holds twice selects both).  A name the file does not hold, or a name given twice, is refused (the reference overruns readComps or
// leaves an entry unset)
inline bool streamsub_components(const std::vector<std::string>& fileNames, const std::vector<std::string>& want, std::vector<int>& comps, std::string& why) {
  comps.clear();
  if (want.empty()) {
    for (size_t i = 0; i < fileNames.size(); ++i) comps.push_back((int)i);
    return true;
  }
  for (size_t j = 0; j < want.size(); ++j) {
    for (size_t k = 0; k < j; ++k)
      if (want[k] == want[j]) { why = "Component given twice: " + want[j]; return false; }
    bool found = false;
    for (const std::string& n : fileNames) found = found || n == want[j];
    if (!found) { why = "Component not found: " + want[j]; return false; }
  }
  for (size_t i = 0; i < fileNames.size(); ++i)
    for (size_t j = 0; j < want.size(); ++j)
      if (fileNames[i] == want[j]) comps.push_back((int)i);
  return true;
}

// one Str box as the tables need it
struct SubBox { long long ni, nj, jlo; };
struct SubTables {
  std::vector<int64_t> box_desc;     // [nbt][4]: ni, nj, jlo, points of the boxes before
  std::vector<int32_t> node_table;   // [num_nodes][2]: flat box, position
  std::vector<int> lev_of, box_of;   // [nbt]
  long long num_nodes = 0, npts = 0;
};
// build_nodeMap (:228-250) over the flat box order (level-major), with the checks the sister tools make, then the element table
// (ids outside 1 .. num_nodes) and, for the seed keys, a box with lines whose j range lacks the seed point
inline bool streamsub_tables(const std::vector<std::vector<SubBox>>& boxes, const std::vector<std::vector<std::vector<int32_t>>>& inside, const std::vector<int32_t>& faceData,
                             bool bySeed, int ncomp, SubTables& T, std::string& why) {
  T = SubTables();
  for (size_t l = 0; l < boxes.size(); ++l)
    for (size_t b = 0; b < boxes[l].size(); ++b) {
      const SubBox& B = boxes[l][b];
      T.box_desc.insert(T.box_desc.end(), {(int64_t)B.ni, (int64_t)B.nj, (int64_t)B.jlo, (int64_t)T.npts});
      T.lev_of.push_back((int)l);
      T.box_of.push_back((int)b);
      T.npts += B.ni * B.nj;
      T.num_nodes += (long long)inside[l][b].size();
    }
  if (T.lev_of.empty()) { why = "the stream file has no Str box"; return false; }
  if (T.num_nodes > 0x7fffffffLL) { why = "more than 2^31 - 1 nodes"; return false; }
  T.node_table.assign(2 * (size_t)T.num_nodes, -1);
  size_t g = 0;
  for (size_t l = 0; l < boxes.size(); ++l)
    for (size_t b = 0; b < boxes[l].size(); ++b, ++g) {
      const auto& ids = inside[l][b];
      if ((long long)ids.size() > boxes[l][b].ni) { why = "Str box " + std::to_string(b) + " of level " + std::to_string(l) + " has more inside_nodes than lines"; return false; }
      for (size_t k = 0; k < ids.size(); ++k) {
        if (ids[k] < 1 || ids[k] > T.num_nodes) { why = "inside_nodes id " + std::to_string(ids[k]) + " outside 1 .. " + std::to_string(T.num_nodes); return false; }
        T.node_table[2 * (size_t)(ids[k] - 1)] = (int32_t)g;
        T.node_table[2 * (size_t)(ids[k] - 1) + 1] = (int32_t)k;
      }
    }
  for (long long n = 0; n < T.num_nodes; ++n)
    if (T.node_table[2 * (size_t)n] < 0) { why = "node " + std::to_string(n + 1) + " has no inside_nodes entry"; return false; }
  for (int32_t v : faceData)
    if (v < 1 || v > T.num_nodes) { why = "Elements names node id " + std::to_string(v) + " outside 1 .. " + std::to_string(T.num_nodes); return false; }
  if (bySeed) {
    if (ncomp < 3) { why = "seedLo / seedHi need the coordinates: the stream file has " + std::to_string(ncomp) + " components"; return false; }
    g = 0;
    for (size_t l = 0; l < boxes.size(); ++l)
      for (size_t b = 0; b < boxes[l].size(); ++b, ++g) {
        const SubBox& B = boxes[l][b];
        if (!inside[l][b].empty() && (B.jlo > 0 || B.jlo + B.nj - 1 < 0)) {
          why = "Str box " + std::to_string(b) + " of level " + std::to_string(l) + " (j = " + std::to_string(B.jlo) + " .. " + std::to_string(B.jlo + B.nj - 1) + ") has lines but no seed point j = 0";
          return false;
        }
      }
  }
  return true;
}

}  // namespace pa
