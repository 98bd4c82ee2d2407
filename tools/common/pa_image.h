// pa_image.h -- the image side of avgToPlane3d and slicePlot3d, host only (no GPU, no library): the palette loader and the PPM / PGM
// writers both reference files carry (LOAD_PALETTE_STR, STORE_PPM_STR, STORE_PGM_STR: avgToPlane.cpp:279-381, slicePlot.cpp:141-243)
// and the tools' keys, read and VALIDATED as a whole before any output exists (avgToPlane.cpp:58-123, :204-223; slicePlot.cpp:28-89).
// Defined where the reference is undefined or silent: a palette file shorter than 768 bytes aborts (the reference
// reads garbage), as do dir / slicedir outside 0..2, a box or sliceloc outside the finest level's domain, components out of range,
// finestLevel out of range, a max_grid_size below 1 and an unknown varname.  tools/src/planeImageCheck.cpp runs this header alone.
#pragma once
#include <array>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "pa_parmparse.h"

namespace pa {

struct Palette {
  unsigned char r[256], g[256], b[256], a[256];
};

// 256 r, 256 g, 256 b bytes and an optional 256 alpha (0 without)
inline Palette load_palette(const std::string& file) {
  FILE* fp = std::fopen(file.c_str(), "rb");
  if (!fp) Abort("cannot open palette file " + file);
  Palette P;
  unsigned char c[1024];
  const size_t n = std::fread(c, 1, sizeof c, fp);
  std::fclose(fp);
  if (n < 768) Abort("palette file " + file + " is shorter than 768 bytes");
  for (int i = 0; i < 256; ++i) {
    P.r[i] = c[i];
    P.g[i] = c[256 + i];
    P.b[i] = c[512 + i];
    P.a[i] = n == 1024 ? c[768 + i] : 0;
  }
  return P;
}

// levels[height][width]: row j' of the array is row j' of the file (no flip); an existing file is overwritten
inline void store_ppm(const std::string& file, int width, int height, const uint8_t* levels, const Palette& P) {
  std::vector<unsigned char> image((size_t)3 * width * height);
  for (size_t i = 0; i < (size_t)width * height; ++i) {
    const int j = levels[i];
    image[3 * i + 0] = P.r[j];
    image[3 * i + 1] = P.g[j];
    image[3 * i + 2] = P.b[j];
  }
  FILE* fp = std::fopen(file.c_str(), "w");
  if (!fp) Abort("cannot open output file " + file);
  std::fprintf(fp, "P6\n%d %d\n%d\n", width, height, 255);
  const size_t w = std::fwrite(image.data(), 1, image.size(), fp);
  if (std::fclose(fp) != 0 || w != image.size()) Abort("short write to " + file);
}

inline void store_pgm(const std::string& file, int width, int height, const uint8_t* levels) {
  FILE* fp = std::fopen(file.c_str(), "w");
  if (!fp) Abort("cannot open output file " + file);
  std::fprintf(fp, "P5\n%d %d\n%d\n", width, height, 255);
  const size_t n = (size_t)width * height, w = std::fwrite(levels, 1, n, fp);
  if (std::fclose(fp) != 0 || w != n) Abort("short write to " + file);
}

// what the keys are checked against: the plotfile's variable names and the index domain (lo0 lo1 lo2 hi0 hi1 hi2) of every level
struct PlaneFileInfo {
  std::vector<std::string> names;
  std::vector<std::array<int, 6>> domains;
};

inline int finest_level_key(const ParmParse& pp, const PlaneFileInfo& I) {
  int finestLevel = (int)I.domains.size() - 1;
  pp.query("finestLevel", finestLevel);
  if (finestLevel < 0 || finestLevel >= (int)I.domains.size()) Abort("finestLevel out of range");
  return finestLevel;
}

struct AvgToPlaneArgs {
  std::vector<int> comps;
  int finestLevel = 0, dir = 0, max_grid_size = 32;
  int box[6];
  bool have_min = false, have_max = false;
  double vmin = 0.0, vmax = 0.0;
  std::string outfile, sumfile;
  Palette palette{};
};

inline AvgToPlaneArgs parse_avgtoplane(const ParmParse& pp, const std::string& infile, const PlaneFileInfo& I) {
  AvgToPlaneArgs A;
  const int ncfile = (int)I.names.size();
  if (const int nc = pp.countval("comps")) {  // :73-89
    A.comps.resize((size_t)nc);
    for (int i = 0; i < nc; ++i) pp.get("comps", A.comps[(size_t)i], i);
  } else {
    int sComp = 0, nComp = ncfile;
    pp.query("sComp", sComp);
    pp.query("nComp", nComp);
    if (nComp < 1) Abort("nComp must be at least 1");
    A.comps.resize((size_t)nComp);
    for (int i = 0; i < nComp; ++i) A.comps[(size_t)i] = sComp + i;
  }
  for (int c : A.comps)
    if (c < 0 || c >= ncfile) Abort("component " + std::to_string(c) + " is not in the plotfile (" + std::to_string(ncfile) + " components)");
  A.finestLevel = finest_level_key(pp, I);  // :91-92
  const std::array<int, 6>& dom = I.domains[(size_t)A.finestLevel];
  for (int q = 0; q < 6; ++q) A.box[q] = dom[(size_t)q];
  if (const int nx = pp.countval("box")) {  // :95-104
    if (nx != 6) Abort("box needs six integers: lo0 lo1 lo2 hi0 hi1 hi2");
    for (int q = 0; q < 6; ++q) pp.get("box", A.box[q], q);
    for (int d = 0; d < 3; ++d)
      if (A.box[d] > A.box[3 + d] || A.box[d] < dom[(size_t)d] || A.box[3 + d] > dom[(size_t)(3 + d)]) Abort("box is empty or not inside the domain of level " + std::to_string(A.finestLevel));
  }
  pp.query("dir", A.dir);  // :118
  if (A.dir < 0 || A.dir > 2) Abort("dir must be 0, 1 or 2");
  pp.query("max_grid_size", A.max_grid_size);  // :122
  if (A.max_grid_size < 1) Abort("max_grid_size must be at least 1");
  A.have_min = pp.query("min", A.vmin);  // :208-209
  A.have_max = pp.query("max", A.vmax);
  std::string palfile;
  pp.get("palette", palfile);  // :218-221
  A.palette = load_palette(palfile);
  A.outfile = getFileRoot(infile) + ".ppm";  // :223
  pp.query("sumfile", A.sumfile);
  return A;
}

struct SlicePlotArgs {
  int finestLevel = 0, slicedir = 0, sliceloc = 0, comp = 0;
  std::string varname, outtype = "image", outfile;
  bool writes = true, have_min = false, have_max = false;
  double vmin = 0.0, vmax = 0.0;
  int box[6];
  Palette palette{};
};

inline SlicePlotArgs parse_sliceplot(const ParmParse& pp, const std::string& file, const PlaneFileInfo& I) {
  SlicePlotArgs A;
  A.finestLevel = finest_level_key(pp, I);  // :39-40
  pp.get("slicedir", A.slicedir);           // :44-46
  pp.get("sliceloc", A.sliceloc);
  pp.get("varname", A.varname);  // :47-49: CanDerive is the plotfile's names
  A.comp = -1;
  for (size_t i = 0; i < I.names.size(); ++i)
    if (I.names[i] == A.varname) { A.comp = (int)i; break; }
  if (A.comp < 0) Abort("varname " + A.varname + " is not a variable of the plotfile");
  if (A.slicedir < 0 || A.slicedir > 2) Abort("slicedir must be 0, 1 or 2");
  const std::array<int, 6>& dom = I.domains[(size_t)A.finestLevel];
  if (A.sliceloc < dom[(size_t)A.slicedir] || A.sliceloc > dom[(size_t)(3 + A.slicedir)]) Abort("sliceloc is outside the domain of level " + std::to_string(A.finestLevel));
  for (int q = 0; q < 6; ++q) A.box[q] = dom[(size_t)q];  // :51-53
  A.box[A.slicedir] = A.box[3 + A.slicedir] = A.sliceloc;
  pp.query("outtype", A.outtype);  // :58-59
  A.writes = A.outtype == "image" || A.outtype == "gray";
  A.have_min = pp.query("min", A.vmin);  // :63-64
  A.have_max = pp.query("max", A.vmax);
  if (A.outtype == "image") {  // :75-81
    std::string palfile;
    pp.get("palette", palfile);
    A.palette = load_palette(palfile);
  }
  A.outfile = getFileRoot(file) + (A.outtype == "image" ? ".ppm" : ".pgm");  // :80-81, :86-87
  pp.query("outfile", A.outfile);
  return A;
}

}  // namespace pa
