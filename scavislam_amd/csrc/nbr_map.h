// nbr_map.h -- what frontend.hip and map.hip share for svs_frontend_set_neighborhood_from_root: the request by which a front-end stream asks the device-resident
// map (map.hip: map_nbh.inc) for its whole neighbourhood from a root id (Backend::computeNeighborhood, backend.cpp:244-386), and the places of the front end's own tables the
// map's kernels write -- the candidate list and keyframe slots as in nbh_map.h, and the resident vertex table of the keyframe decision (keyframe.h).
// Neither translation unit reaches into the other's handle.
#pragma once
#include "nbh_map.h"

enum { NBR_OK = 0, NBR_ROOT_OUTSIDE = 1, NBR_OVER = 2 };

// one request as it is staged: the slot tables of all requests lie in one int32 array (per request: the slots that name a keyframe of the map, -1 elsewhere;
// then the caller's table as it came), the head records of all requests in one record array
struct nbr_req {
  int32_t stream, root, act, max_nn;
  int32_t n_head, n_groups, n_fixed, prev_len;        // n_groups: the head's groups; prev_len: records of the stream's list before the call
  int32_t slot_off, slot_raw_off, head_off;
  int32_t fixed_at;                                   // 0: the n_fixed leading groups are the fixed ones; 1 + f (the head is a stream's store, n_fixed = 1): group f alone is fixed
  int32_t group_end[NBH_MAX_GROUPS];                  // the head's group ends, then zeros
  int32_t group_kf[NBH_MAX_GROUPS];                   // the key of every group behind the fixed ones (with fixed_at: of every group)
};

// what the first launch leaves for the later ones, per request
struct nbr_mid {
  int32_t status;                                     // NBR_*
  int32_t n_given, n_vert, n_map, n_no_slot, n_walk;  // rule 1's list (root included), the vertex set, the map's points, records without a slot, vertices outside the window
  int32_t pad_[2];
};

struct MapNbrDst {
  const nbr_req *req; const int32_t *ids; const svs_candidate_point *head;      // staged
  int head_stride, from_store;    // the head of request Q lies at head + Q.stream * head_stride + Q.head_off; from the front end's new-point store (newpoints.h):
                                  // head = its record rows, head_stride = record_cap, and a head record's kf_index is written as the slot of its group's key
  int R, VB;
  // the front end's tables: rows per STREAM
  svs_candidate_point *pts; int max_points;
  int32_t *group_end, *n_groups, *n_new;
  svs_keyframe *kfs; int max_keyframes;
  svs_kf_table *vt_tab; svs_kf_vertex *vt_vtx; int32_t *vt_slot;                // [B], [B][SVS_KF_MAX_VERTICES], [B][max_keyframes]
  int refresh;
  // outputs: rows per REQUEST
  svs_nbr_result *res;            // [R]
  double *slot_T;                 // [R][max_keyframes][12]
  int32_t *vertex_id; double *vertex_T;      // [R][VB], [R][VB][12]
  int32_t *act_nb;                // [R][VB]
  int32_t *strength;              // [R][VB][VB]
  int32_t *point_id;              // [R][max_points]
  // work space, all [R]-rowed
  nbr_mid *mid;                   // [R]
  int32_t *map_pid;               // [R][max_points]: the map's points of the request, ascending
  int32_t *walk_v;                // [R][VB]: the vertices outside the window, ascending index
  int32_t *walk_off;              // [R + 1]: their exclusive prefix over the requests; [R] = the length of the list
  int2 *walk_list;                // [R * VB]: (request, vertex index)
  int4 *walk_hdr;                 // [R * VB]: (status, path length, 0, 0) by r * VB + v
};

// rebuilds the CSR views and the adjacency when the logs have grown, then the four launches; asynchronous on the context's stream.  The host has checked: root
// and act are keyframes of the map, every staged slot id is one or -1, every key is one, streams are distinct, the heads are well formed
int svs_map_build_root_neighborhoods(svs_map *map, const MapNbrDst &dst);
