// pa_streamsel.h -- the tables of one stream directory as pa_streamsel.hip (selection) and pa_streamsub.hip (subsetting) share them
#pragma once
#include "pa_internal.h"

struct pa_ssel {
  pa_ctx* ctx = nullptr;
  int nbt = 0;
  long long nNodes = 0;
  std::vector<long long> box;  // [nbt][4]: ni, nj, jlo, off (points of the boxes before)
  std::vector<int> node;       // [nNodes][2]: box, i
  long long* d_box = nullptr;
  int* d_node = nullptr;
  int* d_order = nullptr;      // node ids sorted by (box, i): consecutive threads of the peak kernel read consecutive i of one box
  int* d_bsum = nullptr;       // kept nodes of every block of SS_BLOCK node ids
  long long* d_boff = nullptr; // their exclusive scan, [nblocks + 1]
  int* d_err = nullptr;        // set by a kernel that was handed a j outside its box
  // pa_streamsub.hip, built at the first pa_ssub_* call on the handle and kept with it
  int sub_state = 0;               // 0 not built, 1 good, -1 refused (sub_why)
  std::string sub_why;
  std::vector<long long> nline;    // [nbt]: node ids listed by box g (its inside_nodes list); they sit on lines 0 .. nline - 1
  long long* d_nline = nullptr;
};
