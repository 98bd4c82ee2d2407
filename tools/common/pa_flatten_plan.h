// pa_flatten_plan.h -- host arithmetic of flattenAMRFile3d (flattenAMRFile.cpp:77-97): the slabs of output boxes, the rectangles
// (file box) x (output box) that the file's own cells are copied through, and a plotfile writer that does not need the whole
// level in memory.  The first part is arithmetic on boxes only (B: any type with inclusive int lo[3], hi[3]) and includes
// nothing else: pa_flatten.hip builds its overlay table with it (PA_FLATTEN_PLAN_ONLY).  The second part is the writer.
#pragma once
#include <cstddef>
#include <utility>
#include <vector>

namespace pa {

// consecutive boxes b0 .. b1-1 per slab, in order, slab_boxes of them (the last slab: what is left)
inline std::vector<std::pair<int, int>> flat_slabs(int nboxes, int slab_boxes) {
  std::vector<std::pair<int, int>> s;
  if (slab_boxes < 1) slab_boxes = 1;
  for (int b = 0; b < nboxes; b += slab_boxes) s.emplace_back(b, b + slab_boxes < nboxes ? b + slab_boxes : nboxes);
  return s;
}

struct FlatRect {
  int fbox, obox;  // box of the file's level, box of the slab
  int lo[3], hi[3];
  long long numPts() const { return (long long)(hi[0] - lo[0] + 1) * (hi[1] - lo[1] + 1) * (hi[2] - lo[2] + 1); }
};

// (file box) n (slab box) for every pair that meets, file boxes outermost: the file's boxes are disjoint and so are the slab's,
// so the rectangles are disjoint and tile (file n slab) exactly.  take: per slab box, zero = leave it out (null: all);
// covered (may be null): per slab box the cells its rectangles hold
template <typename BF, typename BO>
inline std::vector<FlatRect> flat_rects(const std::vector<BF>& file, const std::vector<BO>& slab, const std::vector<char>* take = nullptr,
                                        std::vector<long long>* covered = nullptr) {
  std::vector<FlatRect> out;
  if (covered) covered->assign(slab.size(), 0);
  if (file.empty() || slab.empty()) return out;
  int blo[3], bhi[3];  // the slab's bounding box: most file boxes miss it
  for (int d = 0; d < 3; ++d) { blo[d] = slab[0].lo[d]; bhi[d] = slab[0].hi[d]; }
  for (const BO& o : slab)
    for (int d = 0; d < 3; ++d) { blo[d] = o.lo[d] < blo[d] ? o.lo[d] : blo[d]; bhi[d] = o.hi[d] > bhi[d] ? o.hi[d] : bhi[d]; }
  for (std::size_t f = 0; f < file.size(); ++f) {
    bool near = true;
    for (int d = 0; d < 3; ++d) near = near && file[f].lo[d] <= bhi[d] && file[f].hi[d] >= blo[d];
    if (!near) continue;
    for (std::size_t o = 0; o < slab.size(); ++o) {
      if (take && !(*take)[o]) continue;
      FlatRect r;
      bool in = true;
      for (int d = 0; d < 3; ++d) {
        r.lo[d] = file[f].lo[d] > slab[o].lo[d] ? file[f].lo[d] : slab[o].lo[d];
        r.hi[d] = file[f].hi[d] < slab[o].hi[d] ? file[f].hi[d] : slab[o].hi[d];
        in = in && r.lo[d] <= r.hi[d];
      }
      if (!in) continue;
      r.fbox = (int)f;
      r.obox = (int)o;
      out.push_back(r);
      if (covered) (*covered)[o] += r.numPts();
    }
  }
  return out;
}

// the file boxes that meet a slab (the ones a slab's pass has to upload), ascending
template <typename BF, typename BO>
inline std::vector<int> flat_file_boxes(const std::vector<BF>& file, const std::vector<BO>& slab) {
  std::vector<char> hit(file.size(), 0);
  for (const FlatRect& r : flat_rects(file, slab)) hit[(std::size_t)r.fbox] = 1;
  std::vector<int> ids;
  for (std::size_t f = 0; f < file.size(); ++f)
    if (hit[f]) ids.push_back((int)f);
  return ids;
}

}  // namespace pa

#ifndef PA_FLATTEN_PLAN_ONLY
#include "pa_plotfile.h"

namespace pa {

// Where every (box, component) block of a single-level plotfile's Cell_D_00000 lies: a FAB is its header line followed by ncomp
// blocks of numPts doubles, FABs in box order -- what a sequential writer (write_fab per box) produces
struct FlatOffsets {
  std::vector<std::string> hdr;
  std::vector<long long> fab;  // offset of the FAB's header line
  long long total = 0;
  FlatOffsets() = default;
  FlatOffsets(const std::vector<Box3>& boxes, int ncomp) {
    for (const Box3& B : boxes) {
      hdr.push_back("FAB ((8, (64 11 52 0 1 12 0 1023)),(8, (8 7 6 5 4 3 2 1)))" + box_str(B) + ' ' + std::to_string(ncomp) + "\n");
      fab.push_back(total);
      total += (long long)hdr.back().size() + 8LL * ncomp * B.numPts();
    }
  }
  long long block(size_t b, int comp, long long npts) const { return fab[b] + (long long)hdr[b].size() + 8LL * comp * npts; }
};

// WriteSingleLevelPlotfile (flattenAMRFile.cpp:97) for data that arrive in pieces: blocks are written with pwrite at their final
// offsets in any order of slabs and component batches, the per-FAB minima / maxima are kept as write_plotfile computes them
// (minmax_run over a whole component of a FAB, from 1e300 / -1e300), and the FAB header lines, Cell_H and Header are written
// last.  The tree is byte-identical to pa::write_plotfile of the same data.
struct FlatWriter {
  std::string path;
  std::vector<std::string> names;
  Box3 domain;
  double prob_lo[3], prob_hi[3], time = 0.0;
  std::vector<Box3> boxes;
  FlatOffsets offs;
  std::vector<std::vector<double>> mins, maxs;
  int fd = -1;
  std::vector<int> bad;

  FlatWriter(const std::string& p, const std::vector<std::string>& n, const Box3& dom, const double plo[3], const double phi[3], const std::vector<Box3>& b, double t)
      : path(p), names(n), domain(dom), time(t), boxes(b), offs(b, (int)n.size()) {
    for (int d = 0; d < 3; ++d) { prob_lo[d] = plo[d]; prob_hi[d] = phi[d]; }
  }
  ~FlatWriter() { if (fd >= 0) ::close(fd); }
  FlatWriter(const FlatWriter&) = delete;

  void open() {  // the first byte written: after every input is validated
    const int ncomp = (int)names.size();
    ::mkdir(path.c_str(), 0755);
    ::mkdir((path + "/Level_0").c_str(), 0755);
    const std::string fname = path + "/Level_0/Cell_D_00000";
    fd = ::open(fname.c_str(), O_CREAT | O_TRUNC | O_WRONLY, 0644);
    if (fd < 0) Abort("Unable to create " + fname);
    mins.assign(boxes.size(), std::vector<double>((size_t)ncomp, 1e300));
    maxs.assign(boxes.size(), std::vector<double>((size_t)ncomp, -1e300));
    bad.assign(boxes.size(), 0);
  }
  void put(size_t b, const char* p, size_t n, long long at) {
    size_t done = 0;
    while (done < n) {
      const ssize_t r = ::pwrite(fd, p + done, n - done, (off_t)(at + (long long)done));
      if (r <= 0) { bad[b] = 1; return; }
      done += (size_t)r;
    }
  }
  // component `comp` of box b: numPts doubles, contiguous.  Every (b, comp) exactly once, from one thread per box at a time
  void put_block(size_t b, int comp, const double* p) {
    const long long npts = boxes[b].numPts();
    minmax_run(p, npts, mins[b][(size_t)comp], maxs[b][(size_t)comp]);
    put(b, (const char*)p, (size_t)npts * 8, offs.block(b, comp, npts));
  }
  // boxes b0 .. b0 + h.boxes.size() - 1, components comp0 .. comp0 + n - 1, from a ghost-free host multifab on those boxes
  void put_slab(int b0, int comp0, int n, HostMF& h) {
    parallel_for(h.boxes.size(), [&](size_t i) {
      const Box3& B = h.boxes[i];
      for (int a = 0; a < n; ++a) put_block((size_t)b0 + i, comp0 + a, h.ptr((int)i, a, B.lo[0], B.lo[1], B.lo[2]));
    });
  }
  // a run that ends without a plotfile: only what open() created is removed -- the data file, then the two directories IF they are
  // empty (an existing directory that is not a plotfile is written into as it is, OldOutput: whatever else it holds stays)
  void abandon() {
    if (fd < 0) return;
    ::close(fd);
    fd = -1;
    ::unlink((path + "/Level_0/Cell_D_00000").c_str());
    ::rmdir((path + "/Level_0").c_str());
    ::rmdir(path.c_str());
  }
  void finish() {
    const int ncomp = (int)names.size();
    for (size_t b = 0; b < boxes.size(); ++b) put(b, offs.hdr[b].data(), offs.hdr[b].size(), offs.fab[b]);
    ::close(fd);
    fd = -1;
    for (int x : bad)
      if (x) Abort("short write to " + path + "/Level_0/Cell_D_00000");
    std::vector<std::string> bs;
    for (const Box3& B : boxes) bs.push_back(box_str(B));
    write_vismf_header(path + "/Level_0/Cell_H", "Cell_D_00000", ncomp, bs, offs.fab, mins, maxs);
    write_plotfile_header(path, names, {domain}, prob_lo, prob_hi, {&boxes}, time, {0});  // one 3-D level at step 0
  }
};

}  // namespace pa
#endif
