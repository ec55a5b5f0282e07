// newpoints.h -- internal interface of newpoints.hip for frontend.hip (the front end's resident newpoint_map).
#pragma once
#include "common.h"

// a stream's store rebuilt from segments (put, seed, drop): one workgroup per stream named.  The new content is the segments in order -- a segment belongs to
// group `group` of the NEW table, and the segments of a group follow each other -- gathered into the scratch row and copied back.
enum { NP_SEG_STORE = 0,       // off: record offset in the stream's own row, as it lies before the call
       NP_SEG_STAGED = 1,      // off: record offset in the staged records
       NP_SEG_SEED = 2 };      // off: the seed request r -- its records at seed_out + r * seed_cap, their number the sum of seed_cnt[3 r .. 3 r + 3)
struct np_seg { int32_t kind, off, len, group; };
struct np_op {
  int32_t stream, n_seg, seg_off, n_groups;
  int32_t key[SVS_NEWPOINTS_MAX_GROUPS];
};
struct NpCompose {
  const np_op *ops; const np_seg *segs; const svs_candidate_point *staged;                    // staged: [n_ops], packed, packed
  const svs_candidate_point *seed_out; const int32_t *seed_cnt; int seed_cap;                 // the seed kernel's outputs (NP_SEG_SEED)
  svs_candidate_point *rec, *tmp; int32_t *key, *cnt, *ng; int record_cap;                    // resident: [B][record_cap] x 2, [B][64] x 2, [B]
};
int svs_newpoints_compose(svs_ctx *ctx, int n_ops, const NpCompose &c);

// the hand-over: a stream's candidate list gathered from its store and the staged tail; one workgroup per request
struct np_list_seg { int32_t kind, off, len, kf_index; };      // NP_SEG_STORE (kf_index is written into every record) or NP_SEG_STAGED (records as given)
struct np_list_req {
  int32_t stream, n_seg, prev_len, pad_;       // n_seg = the groups of the list
  np_list_seg seg[SVS_NEWPOINTS_MAX_GROUPS];
};
struct NpList {
  const np_list_req *req; const svs_candidate_point *staged;
  const svs_candidate_point *rec; int record_cap;
  svs_candidate_point *pts; int max_points; int32_t *group_end, *n_groups, *n_new;           // the front end's list: [B][max_points], [B][64], [B], [B]
};
int svs_newpoints_list(svs_ctx *ctx, int n_requests, const NpList &l);
