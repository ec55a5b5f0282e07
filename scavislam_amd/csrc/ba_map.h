// ba_map.h -- what ba.hip and map.hip share: the window svs_map_prepare_window leaves in the device-resident map (map.hip: map_window.inc), as svs_ba_window_from_map /
// svs_ba_store_to_map (ba_window.inc) read and write it.  Neither translation unit reaches into the other's handle.
#pragma once
#include "common.h"
#include <vector>

// the prepared window (device pointers but for h_window_ids): the pieces of the block win_unpack_kernel reads
struct MapWindowView {
  int P, L;                            // final window, active points
  const int32_t *window_ids;           // [P]  W0 in the caller's order, then the extension ascending
  const int32_t *h_window_ids;         // the same on the host (the constraints come by frame id)
  const int32_t *active_ids;           // [L]  ascending
  const int32_t *anchor_ids;           // [L]  keyframe ids
  const double *poses, *psi;           // [P][12], [L][3]: filled by svs_map_window_view's launch
  const svs_ba_edge *store; size_t n_store;      // the measured store: ids in .point / .pose, log order
  int kf_hi, pt_hi;                    // every id of the store is below these
  uint64_t serial;                     // of this prepare (no two prepares of a process share one)
  const int32_t *h_window_types;       // [P] on the host: 0 INNER / 1 OUTER (the extension is OUTER)
  const svs_map_edge *edges;           // the edge table's records by slot (nullptr without svs_map_reserve_edges)
};

// copyContraintsToG2o's list for the prepared window from the host's mirror of the edge table, in the order the header states: (i, j, slot, T_21 is the inverse of
// the stored T_lo_from_hi) per constraint.  SVS_ERR_INVALID (nothing enqueued) without a valid prepared window or where an edge of the list is not marginalised
int svs_map_window_constraint_list(svs_map *map, std::vector<int4> *out);
// one launch, asynchronous: record c of d_out = (T_21, info, pose1 = i, pose2 = j) of d_list[c] from the edge table (pose_inv where the list says so; built in
// map.hip (map_edges.inc): no contraction, so the inverse is the one svs_map_set_constraints and the NumPy model form)
int svs_map_gather_constraints(svs_map *map, const int4 *d_list, int C, svs_ba_constraint *d_out);

svs_ctx *svs_map_ctx(svs_map *map);
// SVS_ERR_INVALID without a valid prepared window (nothing enqueued); else one launch on the context's stream re-reads the window's poses and psi = (x / z,
// y / z, 1 / z) from the map into the block
int svs_map_window_view(svs_map *map, MapWindowView *out);
// is `serial` the map's valid prepared window
bool svs_map_window_is(const svs_map *map, uint64_t serial);
// one launch, asynchronous: d_poses [P][12] to the keyframes of the prepared window, invert_depth(d_psi [L][3]) to its points
int svs_map_window_store(svs_map *map, const double *d_poses, const double *d_psi);
