/*
 * ransac_hip_diag.h -- entry points that exist in the DIAG build only (libransac_hip_diag.so, -DRH_DIAG): audits of the
 * score kernel's binary32 classifier and box tests against the exact test, a host-side self-check of the octree
 * sampler's search routines, and one window of the device sampler with everything it made.  Test infrastructure: the
 * product library (libransac_hip.so) does not export them, reads no environment variable and knows none of the A/B
 * switches (ransac.jl_amd/csrc/options.cpp lists them).
 */
#ifndef RANSAC_HIP_DIAG_H
#define RANSAC_HIP_DIAG_H

#include "ransac_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The batched score decides most (candidate, point) pairs with a binary32 evaluation of the reference's
 * compatibles* quantities (plane.jl:114-130, sphere.jl:144-172, cylinder.jl:194-221) and keeps the binary64
 * test for the pairs within a rounding margin of a threshold (csrc/score4_device.h).  This runs every
 * candidate of `shapes` against every point of subset 1 and returns the worst binary32 error in units of
 * the margin width: out[2k], out[2k+1] = max |a32 - a64|, |b32 - b64| for kind k (plane, sphere, cylinder, cone;
 * sound below 1/2), out[8+k] = pairs looked at.  Host shapes, synchronous. */
int rh_dbg_cls_audit(rh_cloud *c, const rh_shape *shapes, int32_t b, const rh_params *p, double *out /* [12] */);
/* diagnostics: the DECISIONS of the score kernel's culling box test and binary32 classifier against the exact test, over
 * every (candidate, point) of shapes x subset 1: per kind k (plane, sphere, cylinder, cone) out[10 k + ...] = 0 pairs
 * (candidate, 64-point group), 1 pairs the box test skips, 2 skipped pairs that hold an exact inlier (must be 0), 3 points,
 * 4 classified surely-in, 5 surely-out, 6 surely-in that the exact test rejects (must be 0), 7 surely-out that it accepts
 * (must be 0), 8 exact inliers, 9 candidates whose classifier takes the all-zero point (a disabled point as staged) for an
 * inlier (must be 0).  The soundness the bit-exact counts rest on, as a count (score4_device.h).  out[40 + k]: pairs whose
 * group holds a BAND point (one whose distance half alone is not surely failed: no test on the group's position box can
 * decide such a pair -- the floor of the necessary pair work, bench.py's frac_necessary); out[44 + k]: pairs with an exact inlier;
 * out[48 + k]: pairs whose SUPER-TILE's box (16 groups: the lists of st_cull) rules the candidate out, out[52 + k]: VIOLATION: such
 * a pair with an exact inlier (must be 0). */
int rh_dbg_cls_soundness(rh_cloud *c, const rh_shape *shapes, int32_t b, const rh_params *p, uint64_t *out /* [56] */);
/* the same census at the level of the TILES (4 groups: what candidate lists per tile would skip): out[k] = pairs
 * (candidate, group) whose tile's box rules the candidate out, out[4 + k] = VIOLATION: such a pair with an exact inlier
 * (must be 0). */
int rh_dbg_cls_soundness_tiles(rh_cloud *c, const rh_shape *shapes, int32_t b, const rh_params *p, uint64_t *out /* [8] */);
/* the same census for the normal-cell masks of the plane pairs (csrc/score4_device.h): out[0] = pairs (candidate, group) that the
 * GROUP's mask rules out, out[1] = VIOLATION: such a pair with an exact inlier (must be 0), out[2], out[3] = the same for the
 * SUPER-TILE's mask (what the list launch applies). */
int rh_dbg_cls_soundness_nsig(rh_cloud *c, const rh_shape *shapes, int32_t b, const rh_params *p, uint64_t *out /* [4] */);
/* The normal-cell mask of a plane candidate as the host builds it (cls_make on the host's record; M, Nm, Ln: max |coordinate|,
 * max |normal component| and largest normal length of the point set, Ln = 0: not known; f32: a Float32 cloud's margins) into
 * mask_out[3] (shape = NULL: skipped), and the cell (0..95) of each of the ndirs directions dirs[3 i ..] into cells_out[i]
 * (-1: a zero vector or a NaN, which set no bit; -2: an infinite component, which sets all).  Needs no GPU. */
int rh_dbg_nsig(const rh_shape *shape, const rh_params *p, double M, double Nm, double Ln, int f32, uint32_t *mask_out /* [3] */,
                const double *dirs, int64_t ndirs, int32_t *cells_out);
/* The binary64 boxes of the 64-point groups of subset 1 in the library's own (k-d leaf) order: out[6 g ..] = centre and half
 * extents of group g; *ngroups_out: their number (out = NULL or cap < that number: only the number is returned). */
int rh_dbg_group_boxes(rh_cloud *c, double *out, int64_t cap, int64_t *ngroups_out);
/* The shape of the position k-d tree of a subset of s points (1 .. 2^31 - 1), as the library's one statement of it
 * (kd_left_count, csrc/rh_internal.h) makes it for the device order, the host order and the plane order's blocks alike.
 * aligned: 0 = a node of cnt > 64 points gives its left child ((cnt / 64 + 1) / 2) * 64 of them; 1 = a node of more than 1024
 * points gives it ((ceil(cnt / 1024) + 1) / 2) * 1024 instead; -1 = what a cloud of s subset points created now would take
 * (the process-wide "kd_align").  info_out[5]: the number of nodes of at most 1024 points (the first such node on every way
 * down from [0, s)), of nodes of more than 1024 points, of leaves (nodes of at most 64 points; 0 unless leaves_out is given),
 * the tree's height over its leaves (the levels the device order sorts), 1 if the shape is the aligned one.
 * nodes_out [2 node_cap]: lo, hi of the nodes of at most 1024 points in position order; splits_out [3 split_cap]: lo, mid, hi of
 * the larger nodes, parents first; leaves_out [2 leaf_cap]: lo, hi of the leaves in position order.  Each may be NULL; entries
 * beyond a capacity are counted and not written.  Needs no GPU. */
int rh_dbg_kd_shape(int64_t s, int aligned, int64_t *info_out /* [5] */, int64_t *nodes_out, int64_t node_cap, int64_t *splits_out,
                    int64_t split_cap, int64_t *leaves_out, int64_t leaf_cap);
/* The plane order of subset 1 (csrc/kdorder.hip: inside every node of the position k-d tree with at most 1024 points the same
 * points, ordered by a k-d tree on their normals; what plane candidates of counts-only score launches walk) as the cloud holds it.
 * The nodes: those of rh_dbg_kd_shape below, in the shape the cloud was created with ("kd_align").
 * info_out[4]: s, the number of 64-point groups, the number of super-tiles, 1 if the cloud has a plane order (else nothing more
 * is written).  Every other pointer may be NULL.  sub_out / pl_out [6 s]: the subset in leaf order / in plane order, planes
 * x y z nx ny nz, s apart; src_out [s]: plane-order position i holds the point of leaf-order position src_out[i];
 * gb32_out [8 groups]: the plane-order groups' binary32 boxes (cx cy cz hx hy hz hr 0); gm32_out [4 groups]: their normal-cell
 * masks; en_out [2 ceil(s / 64)]: the enabled words in leaf order, then in plane order.  Synchronous. */
int rh_dbg_plane_order(rh_cloud *c, int64_t *info_out /* [4] */, double *sub_out, double *pl_out, int32_t *src_out, float *gb32_out,
                       uint32_t *gm32_out, uint64_t *en_out);
/* The box test of a cylinder candidate as the score kernel's stage 1 runs it, on the host (csrc/score4_device.h: cls_make on the
 * host's record, box_to_f32, cyl_box_skip32 -- the very code of the kernel).  boxes[6 i ..]: centre and half extents of the n
 * binary64 boxes; skip_out[i]: 1 = the box is skipped for the candidate; ball_out[i]: the same by the two clauses alone that
 * bound the box by its half diagonal (the test without the support clause); fields_out (may be NULL): the RH_BOX_FIELDS = 11
 * fields of the culling record (field 6: (R + eps) + slack, field 9: A^2 of the support clause; NaN: never skip).
 * Needs no GPU. */
int rh_dbg_cylbox(const rh_shape *shape, const rh_params *p, double M, double Nm, int f32, const double *boxes, int64_t n,
                  uint8_t *skip_out, uint8_t *ball_out, float *fields_out /* [11] */);
/* The classifier of a sphere or cylinder candidate as the score kernel runs it, on the host (csrc/score4_device.h: cls_make on
 * the host's record, then the kernel's own cls_round_ab on the n points xyz[3 i ..] with normals nrm[3 i ..], converted to
 * binary32 as the kernel's staging converts them).  ua_out[i], ub_out[i]: the scaled values of the distance and the normal half
 * (u = max of the two: u < 0 surely an inlier, u > 1 surely not, else undecided); rec_out: the 16 fields of the classifier
 * record (field 15 NaN: the candidate is exact-only and the kernel does not read ua / ub); dbg4_out: the margins and widths of
 * the squared form, m2, W2 = 2 m2, mv, Wv = 2 mv (zeros for an exact-only candidate).  M, Nm: max |coordinate| and max |normal
 * component| of the point set the margins are made for; f32: a Float32 cloud's margins.  Needs no GPU. */
int rh_dbg_cls_round(const rh_shape *shape, const rh_params *p, double M, double Nm, int f32, int64_t n, const double *xyz,
                     const double *nrm, float *ua_out, float *ub_out, float *rec_out /* [16] */, double *dbg4_out /* [4] */);
/* The two-bit books of the score kernel's point loops (csrc/score4_device.h, "Two-bit books") as the host runs them, through the
 * very functions of the kernel.  u2[64 s ..]: the 64 values u' = 2 u of sequence s in point order.  sure_count_out[s]: points
 * with the sign bit set; sure_word_out[s] / und_word_out[s]: bit p = point p is surely in / undecided (sign clear and u' < 2,
 * i.e. bit 30 clear; a NaN with a clear sign is "out"); any_und_out[s]: 1 = some point is undecided.  Needs no GPU. */
int rh_dbg_books2(const float *u2, int64_t nseq, int32_t *sure_count_out, uint64_t *sure_word_out, uint64_t *und_word_out,
                  uint8_t *any_und_out);
/* The undecided word of a pair as the counts-only launches read it off the books IN PLACE (csrc/score4_device.h, "Books in
 * place"), on the host, by the very functions of the kernel.  u2: as for rh_dbg_books2.  packed_out[s]: the undecided points of
 * sequence s in the books' own bit order; pi_out[L], L = 0 .. 63: the point that bit L of such a word stands for (a permutation
 * of 0 .. 63).  point_words / deposit_out (both or neither NULL): deposit_out[s] = the point-ordered word point_words[s] brought
 * into the books' order (the pairs that ignore their books queue their group's enabled word so).  Needs no GPU. */
int rh_dbg_books2_inplace(const float *u2, int64_t nseq, uint64_t *packed_out, int32_t *pi_out /* [64] */, const uint64_t *point_words,
                          uint64_t *deposit_out);
/* u and u' of a plane, sphere or cylinder candidate on the n points xyz[3 i ..] with normals nrm[3 i ..] (converted to binary32
 * as the kernel's staging converts them), on the host: u_out[i] = max(ua, ub) from the record cls_make builds, by the functions
 * the audits use; u2_out[i] = what the kernel's point loops compute, from that record doubled in registers (cls_double) with
 * the inline 1/2 of the round kinds as 1.  bits(u2) == bits(2 u) away from the subnormal range.  rec_out (may be NULL): the
 * 16 fields of the undoubled record.  M, Nm, f32: as for rh_dbg_cls_round.  Needs no GPU. */
int rh_dbg_cls_u2(const rh_shape *shape, const rh_params *p, double M, double Nm, int f32, int64_t n, const double *xyz,
                  const double *nrm, float *u_out, float *u2_out, float *rec_out /* [16] or NULL */);
/* The box test of a cone candidate as the score kernel's stage 1 runs it, on the host (csrc/score4_device.h: cls_make on the
 * host's record, box_to_f32, cone_box_skip32 -- the very code of the kernel).  boxes[6 i ..]: centre and half extents of the n
 * binary64 boxes; skip_out[i]: 1 = the box is skipped for the candidate; fields_out (may be NULL): the RH_BOX_FIELDS = 11 fields
 * of the culling record (0-2 apex, 3-5 unit axis, 6 k = tan(opang / 2), 7 1 / cn, 8 (eps + slack) / cn, 9 beta and 10 alpha of
 * the axis guard; NaN: never skip).  M, Nm, f32: as for rh_dbg_cylbox.  Needs no GPU. */
int rh_dbg_conebox(const rh_shape *shape, const rh_params *p, double M, double Nm, int f32, const double *boxes, int64_t n,
                   uint8_t *skip_out, float *fields_out /* [11] */);
/* The classifier of a cone candidate as the score kernel runs it (csrc/score4_device.h: cls_make on the host's record, then the
 * kernel's own cls_cone_ab -- device code: its rho goes through the hardware's reciprocal root -- in a kernel of its own on
 * `device`, on the n points xyz[3 i ..] with normals nrm[3 i ..], converted to binary32 as the kernel's staging converts them).
 * ua_out[i], ub_out[i]: the scaled values of the distance and the normal half; near_out[i]: 1 = the point lies inside the axis
 * guard (n2 <= alpha |w|^2 + beta, or a NaN), where the kernel takes u = 1/2 -- undecided -- whatever ua and ub are (elsewhere
 * u = max of the two: u < 0 surely an inlier, u > 1 surely not, else undecided).  rec_out: the 16 fields of the classifier
 * record (field 15 NaN: the candidate is exact-only and the kernel reads none of the three); dbg4_out: 0, wL, eD_lo, wD -- the
 * width of the normal half (infinite on a Float32 cloud, which never decides it), the lower threshold and the width of the
 * distance half (zeros for a candidate without a record).  M, Nm, f32: as for rh_dbg_cls_round.  Synchronous; with n = 0 only
 * the record and its widths are made, on the host: no GPU is touched. */
int rh_dbg_cls_cone(const rh_shape *shape, const rh_params *p, double M, double Nm, int f32, int64_t n, const double *xyz,
                    const double *nrm, int device, float *ua_out, float *ub_out, uint8_t *near_out, float *rec_out /* [16] */,
                    double *dbg4_out /* [4] */);
/* The device's octree sampler finds a point's cell and the r-th enabled point of a cell with a cell directory and
 * bracketed 8-ary searches (csrc/fit_shared.h: cell_bounds_code, lower_bound_in, select_in, select_in_many, select_bit)
 * where the host form uses plain binary searches.  Host-only self-check of those routines against the plain ones on a
 * synthetic Morton order of n points (duplicate codes, random enabled bits, every level): *mismatches = the number of
 * disagreements over `queries` random queries.  Needs no GPU. */
int rh_dbg_oct_search_selftest(int64_t n, uint64_t seed, int64_t queries, int64_t *mismatches);

/* The protocol of the enabled bits (csrc/enabled_state.h) on its own, host code only: nseq sequences of len events each,
 * every sequence on a fresh state; answers[q * len + t] = what the state's queries say after event t of sequence q.
 * Events: 0 / 1 bits_replaced(mirror copied: no / yes), 2 / 3 bits_cleared_by_list(mirror updated: no / yes), 4 .. 7
 * scan_started(culled = bit 1, apply = bit 0 of event - 4), 8 / 9 scan_folded(has blocks: yes / no), 10 scratch_taken,
 * 11 directory_built, 12 list_built, 13 records_built, 14 mirror_built, 15 / 16 long_window(very long: no / yes), 17 nothing
 * (scoring, reads).  Answer bits: 1 has_directory, 2 has_list, 4 has_records, 8 has_mirror, 16 has_block_sums,
 * 32 scan_left_sums, 64 what long_window returned (events 15 / 16), bits 8 and up long_windows().  Needs no GPU. */
int rh_dbg_enabled_events(const uint8_t *events, int64_t nseq, int32_t len, uint16_t *answers);

/* Event counters of the culled score kernel's launches on cloud c (csrc/score4.hip, S4_STAT: chunk visits, box-tested
 * candidates, surviving pairs, batches, pairs of the second pass, undecided points, ring drains, ... per kind; blocks and
 * stagings): what tools/isa_account.py multiplies with the static instruction histogram of the kernel's regions.
 * mode 1: switch on + zero, 0: read into out[128], 2: switch off. */
int rh_dbg_s4_stats(rh_cloud *c, int mode, uint64_t *out /* [128] or NULL */);

/* One window of the device sampler (csrc/sampler.hip, rhk_sample_fit: the call rh_ransac's windows make) on cloud c as it
 * is -- the enabled count, the select structures and, with P, the linear octree prepared the way the driver prepares them
 * before its first window, the status block zeroed, no chained-window state -- and everything it made: the minimal sets of
 * the iterations k0 .. k0 + n_iters - 1 of a run whose generator state starts with `seed`, fitted to every type of
 * p->shape_types.  P = NULL: root-cell sampling; else n_iters x depth level distributions (host) for octree sampling
 * (depth: info_out[0] of an earlier call, or the oracle's).  rank / world: the share of every iteration's sets this call draws
 * (set j belongs to rank j % world, rh_ransac_mp); 0, 1 = all of them; the cloud's own share is put back afterwards.
 * out[cap]: the fitted candidates sorted by slot = ((it * minsubsetN) + set) * n_shape_types + type position, it = 0 for
 * iteration k0; *n_out: how many were fitted -- when that exceeds cap only cap of them come back, which ones is not
 * determined.  draws_out[n_iters]: rand() calls per iteration; *gave_up_out: a set ran into the limit of rejected draws.
 * info_out[8]: 0 octree depth, 1 level of the cell directory (both 0 without P), 2 the kernels that ran (1 fused rank-space,
 * 2 fused octree, 3 sampler + fit kernels), 3 their drawN instantiation (3, or 0 = generic), 4 fit kernel with cones,
 * 5 the flat select list was handed over, 6 the compact records, 7 the cell directory.  RH_E_INVALID for a cloud with no
 * enabled point.  Synchronous. */
typedef struct { int64_t slot; int32_t level; int32_t pad; rh_shape shape; } rh_dbg_cand;
int rh_dbg_sample_fit(rh_cloud *c, const rh_params *p, uint64_t seed, int64_t k0, int32_t n_iters, const double *P_or_null,
                      int32_t rank, int32_t world, rh_dbg_cand *out, int32_t cap, int32_t *n_out, uint64_t *draws_out,
                      int32_t *gave_up_out, int32_t *info_out /* [8] */);

/* wave_each_key (csrc/wave_keys.h: one action per distinct key of a wave) in a kernel of its own: one block of 256 threads,
 * thread i holds keys[i] (u32 = 0: as int32_t, 1: as uint32_t) and counts as active when i < n and act[i] != 0; an inactive
 * thread below n keeps its key all the same.  slot[i] (0 .. nslots - 1): where thread i's key is tallied -- the caller numbers
 * the distinct keys.  Every time the helper calls its function, the leader adds popcount(same) to sum_out[its slot], lowers
 * minlead_out[its slot] to its thread index (0x7F7F7F7F: the slot never had a leader) and adds 1 to scal_out[0]; scal_out[1]
 * counts violations (must be 0): a lane that did not see all 64 lanes of its wave inside the function, or whose bit of `same`
 * is not "active and my key is the leader's".  n <= 256. */
int rh_dbg_wave_keys(const uint32_t *keys, const uint8_t *act, const int32_t *slot, int32_t n, int32_t nslots, int u32, int device,
                     int32_t *sum_out /* [nslots] */, int32_t *minlead_out /* [nslots] */, int32_t *scal_out /* [2] */);

#ifdef __cplusplus
}
#endif
#endif
