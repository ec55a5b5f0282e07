// keyframe.h -- internal interface of keyframe.hip for frontend.hip.
#pragma once
#include "common.h"
// the front end's device state as the source of tracking_ok (svs_frontend_decide_keyframes): what fill_result derives on the host -- the refinement's observation
// count against matchAndTrack's minimum, and a tracker whose workgroups met.  NULL for svs_keyframe_decide, which reads d_tracking_ok
struct KfdFrontendSrc {
  const svs_pose_opt_stats *pstats; const int32_t *passes;      // [streams]
  int min_matches;
};
int svs_keyframe_decide_launch(svs_ctx *ctx, const svs_keyframe_decide_args *a, const svs_keyframe_decide_params *prm, const KfdFrontendSrc *fs,
                               svs_keyframe_decision *d_dec, svs_map_new_point *d_new, svs_map_track_point *d_track, int32_t *d_new_rec, int32_t *d_track_rec, int cap);

// svs_frontend_set_vertex_table: the staged requests and the stream-indexed resident tables they are scattered into (one workgroup per request, word copies)
struct kfd_up { int32_t stream, n_ids, ids_off, pad_; };      // ids_off: into the staged id array
struct KfdScatter {
  const kfd_up *up; const svs_kf_table *tab; const svs_kf_vertex *vtx; const int32_t *slot; const int32_t *ids;      // staged: [R], [R], [R][MAX_VERTICES], [R][S], packed
  svs_kf_table *d_tab; svs_kf_vertex *d_vtx; int32_t *d_slot; int32_t *d_ids;                                         // resident: [B], [B][MAX_VERTICES], [B][S], [B][set_cap]
  int S, set_cap;
};
int svs_keyframe_scatter_tables(svs_ctx *ctx, int n_requests, const KfdScatter &s);
