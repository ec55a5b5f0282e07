// walk_map.h -- what map.hip keeps for the pose graph's walks (map_walk.inc): the strength-ordered adjacency of the keyframes, built on the device from the edge
// records, and the work space of the breadth-first searches.  map.hip holds one MapWalkState and includes map_walk.inc behind map_edges.inc; nothing else
// sees either.
#pragma once
#include "common.h"
#include "owned.h"

enum { WALK_WINDOW = 0, WALK_NEIGHBORHOOD = 1, WALK_ABSOLUTE = 2, WALK_REINIT = 3 };

// rows of the work space of one request, each `stride` int32 long
enum { WALK_ROW_KEY = 0,      // best claim of a keyframe: ((visit index of the claimer + 1) << 14) | rank in the claimer's row; 0 the root, ~0 unclaimed
       WALK_ROW_ORDER,        // the keyframes in visit order
       WALK_ROW_PARENT,       // by keyframe: the claimer
       WALK_ROW_PEDGE,        // by keyframe: the slot of the edge to the claimer
       WALK_ROW_CNT,          // by position in the level: winners of that keyframe's row, then their exclusive prefix
       WALK_ROW_FLAG,         // by keyframe: bit 0 reinitializePoses' mark_reinitialize, bit 1 its pose was rewritten
       WALK_ROWS };

struct MapWalkState {
  // CSR over keyframe ids: row v = v's neighbours in descending (strength, edge slot), the edge slot beside each
  DevBuf<int32_t> d_begin, d_cur, d_nb, d_slot, d_tmp_nb;
  DevBuf<unsigned long long> d_tmp_key;
  int built_edges = -1, built_kf_hi = -1;      // what the rows were built from
  DevBuf<int32_t> d_work; int work_rows = 0, work_stride = 0;
  DevBuf<int32_t> d_pairs;                     // svs_map_prepare_window_from_root: W0's ids | types | INNER ids | pairs
};
