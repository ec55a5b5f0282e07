// nbh_map.h -- what frontend.hip and map.hip share: the request by which a front-end stream asks the device-resident map (map.hip: map_nbh.inc) for its neighbourhood list
// (Backend::computeNeighborhood from the vertex list onwards, backend.cpp:311-386), and the places of the front end's own tables the map's walk writes.
// Neither translation unit reaches into the other's handle.
#pragma once
#include "common.h"

constexpr int NBH_MAX_GROUPS = 64;      // = the front end's MAX_GROUPS: rows of its group-end table

// one request as it is staged: the id lists of all requests lie in one int32 array (vertex list, slot table), the head records of all requests in one record array
struct nbh_req {
  int32_t stream, n_vertex, n_head, n_groups;       // n_groups: the head's groups + 1
  int32_t vertex_off, slot_off, head_off, prev_len;   // prev_len: records of the stream's list before the call (the tail up to it becomes 0xff)
  int32_t group_end[NBH_MAX_GROUPS];                  // the head's group ends, then zeros (the kernel puts the total behind them)
};

// where the walk reads its requests and writes (all DEVICE).  The front end's tables: rows of max_points / NBH_MAX_GROUPS / max_keyframes entries per STREAM;
// the outputs: rows per REQUEST
struct MapNbhDst {
  const nbh_req *req; const int32_t *ids; const svs_candidate_point *head;
  svs_candidate_point *pts; int max_points;
  int32_t *group_end, *n_groups, *n_new;
  svs_keyframe *kfs; int max_keyframes;
  int refresh;                    // rule 5: slots whose id is in the map take the map's pose
  svs_nbh_result *res;            // [R]
  double *slot_T;                 // [R][max_keyframes][12]: the poses written by the refresh (zeros for the other slots), for the front end's host mirror
  int32_t *vertex_id; double *vertex_T; int VB;      // [R][VB], [R][VB][12]
  int32_t *point_id;              // [R][max_points]: the point id of every record of the built list, -1 behind it.  Also the walk's work space
};

svs_ctx *svs_map_ctx(svs_map *map);
bool svs_map_has_keyframe(const svs_map *map, int32_t id);
// rebuilds the CSR views when the log has grown, then one workgroup per request; asynchronous on the context's stream.  The host has checked: every id of a
// vertex list is a keyframe of the map, every slot id is one or -1, streams are distinct, the heads fit
int svs_map_build_neighborhoods(svs_map *map, int n_requests, const MapNbhDst &dst);
